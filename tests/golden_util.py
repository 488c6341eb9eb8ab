"""Weights of the golden fixtures (tests/golden/): regenerated from oracle.encoder_ref.det_state_dict -- a counter-based
generator written out in the oracle, independent of any torch / NumPy random stream -- and checked against the sha256 the
generating script recorded.  A mismatch is a failure, never a skip: these fixtures are the only evidence pinned to the
reference's own classes.  A manifest entry with a ``trained`` field (tests/golden/trained_manifest.json) holds the arguments of
oracle.encoder_ref.trained_like_state_dict: the same generator with the trained-like edits on top."""
from oracle import encoder_ref


def golden_weights(meta, **kw):
    assert meta.get("gen") == "det", "fixture predates the deterministic weight generator: run tests/golden/make_golden.py"
    if "trained" in meta:
        t = meta["trained"]
        sd = encoder_ref.trained_like_state_dict(meta["n_layers"], ffn_drive=t["ffn_drive"], emb_scale=t["emb_scale"],
                                                 outliers=tuple((int(d), float(f)) for d, f in t["outliers"]), seed=meta["seed"],
                                                 ln_jitter=meta["ln_jitter"], **kw)
    else:
        sd = encoder_ref.det_state_dict(seed=meta["seed"], n_layers=meta["n_layers"], ln_jitter=meta["ln_jitter"], **kw)
    got = encoder_ref.state_dict_sha256(sd)
    assert got == meta["checksum"], "deterministic weights differ from the ones the golden vectors were made with: %s" % got
    return sd
