"""SEED-Encoder fixtures (tests/golden/make_golden_seed.py, tests/test_seed_model.py, tests/test_gpu_seed.py): the deterministic
weights of oracle.encoder_ref.det_state_dict under the reference's SEEDEncoderDot_NLL_LN names, and MS MARCO-shaped toy data
inside SEED's 32,769-token vocabulary."""
import os

import numpy as np

from oracle import encoder_ref, synth

SEED_VOCAB = 32769
SRC = "seed_encoder.encoder.sentence_encoder."
_LAYER = (("attention.self.query", "self_attn.q_proj"), ("attention.self.key", "self_attn.k_proj"),
          ("attention.self.value", "self_attn.v_proj"), ("attention.output.dense", "self_attn.out_proj"),
          ("attention.output.LayerNorm", "self_attn_layer_norm"), ("intermediate.dense", "fc1"), ("output.dense", "fc2"),
          ("output.LayerNorm", "final_layer_norm"))


def to_seed_names(sd, prefix="roberta."):
    """HF RoBERTa names -> SEEDEncoderDot_NLL_LN names; the token-type table is dropped (SEED has none)."""
    e = prefix + "embeddings."
    out = {SRC + "embed_tokens.weight": sd[e + "word_embeddings.weight"],
           SRC + "embed_positions.weight": sd[e + "position_embeddings.weight"],
           SRC + "emb_layer_norm.weight": sd[e + "LayerNorm.weight"], SRC + "emb_layer_norm.bias": sd[e + "LayerNorm.bias"]}
    i = 0
    while "%sencoder.layer.%d.output.dense.weight" % (prefix, i) in sd:
        for hf, fs in _LAYER:
            for t in ("weight", "bias"):
                out["%slayers.%d.%s.%s" % (SRC, i, fs, t)] = sd["%sencoder.layer.%d.%s.%s" % (prefix, i, hf, t)]
        i += 1
    for k in ("embeddingHead.weight", "embeddingHead.bias", "norm.weight", "norm.bias"):
        out[k] = sd[k]
    return out


def det_seed_state_dict(seed, n_layers, ln_jitter):
    return to_seed_names(encoder_ref.det_state_dict(seed=seed, n_layers=n_layers, ln_jitter=ln_jitter, vocab=SEED_VOCAB,
                                                    max_pos=514))


def seed_golden_weights(meta):
    assert meta.get("gen") == "det_seed", meta
    sd = det_seed_state_dict(meta["seed"], meta["n_layers"], meta["ln_jitter"])
    got = encoder_ref.state_dict_sha256(sd)
    assert got == meta["checksum"], "deterministic SEED weights differ from the ones the golden vectors were made with: %s" % got
    return sd


def into_seed_vocab(ids):
    """Token ids of oracle.synth (RoBERTa's 50,265) folded into [3, 32769); 0 / 1 / 2 ([CLS] / pad / [SEP]) unchanged."""
    ids = np.asarray(ids).astype(np.int64)
    return np.where(ids >= SEED_VOCAB, 3 + (ids - 3) % (SEED_VOCAB - 3), ids).astype(np.int32)


def interior_pads(rng, ids, lens, frac):
    """Sets about ``frac`` of the tokens strictly inside [1, len - 1) of every record to the pad id 1."""
    ids = ids.copy()
    pos = np.arange(ids.shape[1])[None, :]
    hit = (rng.random(ids.shape) < frac) & (pos >= 1) & (pos < (np.asarray(lens)[:, None] - 1))
    ids[hit] = synth.PAD
    return ids


def make_seed_msmarco_like(out_dir, pad_frac=0.05, **dargs):
    """oracle.synth.make_msmarco_like, then every cache rewritten in SEED's vocabulary with interior pad ids planted in the
    passages (the SEED encoder masks those by id)."""
    from oracle import ann_ref
    synth.make_msmarco_like(out_dir, **dargs)
    rng = np.random.default_rng(int(dargs.get("seed", 0)) + 1)
    for name in ("passages", "train-query", "dev-query"):
        path = os.path.join(out_dir, name)
        lens, ids = ann_ref.read_cache(path)
        ids = into_seed_vocab(ids)
        if name == "passages":
            ids = interior_pads(rng, ids, lens, pad_frac)
        synth.write_cache(path, ids, np.asarray(lens))
