"""Generates tests/golden/embeddings.npz (the rdot tower), embeddings_bert.npz (the bert tower) and embeddings.json by running the
REAL reference (imported through oracle/ref_harness.py) on the CPU in the build container:

    python tests/golden/make_golden_embeddings.py

The two shallow towers, triplets and losses of make_golden_attention_train.py (its CASES, weights and ids), in eval mode, once in
fp32 and once after model.double().  A forward hook on tower.embeddings captures, per tower call, input_ids, token_type_ids (None in
both towers: zeros), the output y and the gradient arriving at y; after the backward, the .grad of the five embedding parameters,
which the three tower calls of the triplet accumulate -- so they are sums over the rows of all three calls, the three sequences of
one [3, L] batch.
Committed (fp32): ids, type ids, y and dy of every row (pad rows included), dgamma, dbeta, the whole token-type gradient, rows
0 .. L + 1 of the position table's gradient and, of the word table's, the rows of the ids that occur (word_rows); every other row of
both is asserted zero here.  The weights are NOT stored: they come from oracle.encoder_ref.det_state_dict by seed (the JSON has the
sha256 of the whole state dict and of its five embedding tensors).  The JSON records per tensor ref_err (max |fp32 run - fp64 run|),
same_inputs (the distance of tests/embeddings_util.py's eager fp32 expression from its fp64 restatement on the committed inputs) and
fp64_restatement_rel (the restatement on the fp64 run's inputs against the fp64 run's own tensors, asserted <= 1e-12 relative here)."""
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, OUT)

from oracle import encoder_ref, ref_harness  # noqa: E402
import embeddings_util as U  # noqa: E402
import make_golden_attention_train as M  # noqa: E402

FILES = U.GOLDEN_FILES


def run(ref, spec, dtype):
    """make_golden_attention_train.run with a hook on the embeddings instead."""
    lens, L = spec["lens"], spec["L"]
    rng = np.random.default_rng(spec["seed"])
    if spec["kind"] == "bert":
        sd = encoder_ref.det_state_dict(kind="bert", seed=spec["seed"], n_layers=2, vocab=30522, max_pos=512, head=False,
                                        prefixes=("",), ln_jitter=spec["ln_jitter"])
        tower = ref_harness.build_reference_model("bert", n_layers=2, seed=0)
        M.load_into(tower, sd)
        ids = rng.integers(1000, 30522, size=(3, L))
        ids[:, 0] = 101
        ids = np.where(np.arange(L)[None, :] < np.asarray(lens)[:, None], ids, 0)
        model = types.SimpleNamespace(query_emb=lambda i, m: tower(i, m)[1], body_emb=lambda i, m: tower(i, m)[1])
        forward, emb, cfg, prefix = ref.models.BiEncoder.forward, tower.embeddings, tower.config, "embeddings."
    else:
        sd = encoder_ref.det_state_dict(seed=spec["seed"], n_layers=2, ln_jitter=spec["ln_jitter"])
        tower = ref_harness.build_reference_model("rdot_nll", n_layers=2, seed=0)
        M.load_into(tower, sd)
        ids = rng.integers(3, 50265, size=(3, L))
        ids[:, 0] = 0
        if spec.get("negative_edits_positive"):
            ids[2] = ids[1]
            ids[2, lens[2] - 2] = 777
        ids = np.where(np.arange(L)[None, :] < np.asarray(lens)[:, None], ids, 1)
        model, forward, emb, cfg, prefix = tower, ref.models.NLL.forward, tower.roberta.embeddings, tower.roberta.config, "roberta.embeddings."
    tower.eval()
    if dtype == torch.float64:
        tower.double()
    store = dict(ids=[], types=[], y=[], dy={})

    def hook(_m, args, kwargs, out):
        i = len(store["y"])
        got = kwargs.get("input_ids", args[0] if args else None)
        tt = kwargs.get("token_type_ids", args[1] if len(args) > 1 else None)
        store["ids"].append(got.detach().clone())
        store["types"].append(torch.zeros_like(got) if tt is None else tt.detach().clone())
        store["y"].append(out.detach().clone())
        out.register_hook(lambda g: store["dy"].__setitem__(i, g.detach().clone()))

    handle = emb.register_forward_hook(hook, with_kwargs=True)
    t = torch.from_numpy(ids).long()
    mask = encoder_ref.mask_from_lengths(np.asarray(lens, np.int32), L)
    (loss,) = forward(model, t[0:1], mask[0:1], t[1:2], mask[1:2], t[2:3], mask[2:3])
    loss.backward()
    handle.remove()
    assert len(store["y"]) == 3 and sorted(store["dy"]) == [0, 1, 2]
    H = cfg.hidden_size
    out = dict(ids=torch.cat(store["ids"], 0).numpy(), types=torch.cat(store["types"], 0).numpy(),
               y=torch.cat(store["y"], 0).numpy().reshape(3 * L, H), dy=torch.cat([store["dy"][i] for i in range(3)], 0).numpy().reshape(3 * L, H))
    assert np.array_equal(out["ids"], ids)
    params = dict(emb.named_parameters())
    assert sorted(params) == sorted(U.PARAMS), sorted(params)
    assert sorted(emb.state_dict().keys()) == sorted(U.PARAMS), sorted(emb.state_dict().keys())   # the buffers are not persistent
    for name in U.PARAMS:
        out[name] = params[name].detach().numpy().copy()
        out[U.GRAD_OF[name]] = params[name].grad.numpy().copy()
    emb_sd = {k: v for k, v in sd.items() if k.startswith(prefix)}
    info = dict(eps=float(cfg.layer_norm_eps), pad=int(cfg.pad_token_id), loss=float(loss), weights_sha256=encoder_ref.state_dict_sha256(sd),
                embeddings_sha256=encoder_ref.state_dict_sha256(emb_sd))
    return out, info


def restate(r, fn, mode, pad, eps):
    return fn(r["ids"], r["types"], *(r[n] for n in U.PARAMS), eps, r["dy"], mode, pad)


def main():
    ref = ref_harness.load_reference()
    meta = dict(generator="tests/golden/make_golden_embeddings.py", torch=torch.__version__, files=FILES)
    for case, spec in M.CASES.items():
        r32, info = run(ref, spec, torch.float32)
        r64, info64 = run(ref, spec, torch.float64)
        L = spec["L"]
        mode = "absolute" if spec["kind"] == "bert" else "roberta"
        pad, eps = info["pad"], info["eps"]
        rows = np.unique(r32["ids"])
        for r in (r32, r64):   # what is not stored is zero: the word rows that do not occur, the position rows past L + 1
            rest = np.ones(r["dword"].shape[0], bool)
            rest[rows] = False
            assert np.abs(r["dword"][rest]).max() == 0.0 and np.abs(r["dpos"][L + 2:]).max() == 0.0
            r["dword"], r["dpos"] = r["dword"][rows], r["dpos"][:L + 2]
        # the fp64 restatement on the fp64 run's inputs reproduces the fp64 run
        want64 = restate(r64, U.embed_fp64, mode, pad, eps)
        assert np.array_equal(want64["word_rows"], rows)
        want64["dpos"] = want64["dpos"][:L + 2]
        restated = {}
        for n in U.NAMES:
            d = float(np.abs(want64[n] - r64[n]).max() / np.abs(r64[n]).max())
            assert d <= 1e-12, (case, n, d)
            restated[n] = d
        ref_err = {n: float(np.abs(r32[n].astype(np.float64) - r64[n]).max()) for n in U.NAMES}
        w32, e32 = restate(r32, U.embed_fp64, mode, pad, eps), restate(r32, U.embed_eager_fp32, mode, pad, eps)
        for d in (w32, e32):
            d["dpos"] = d["dpos"][:L + 2]
        same_inputs = U.distances(e32, w32)
        arrays = dict(ids=r32["ids"].astype(np.int32), types=r32["types"].astype(np.int32), word_rows=rows.astype(np.int32))
        for n in U.NAMES + ("dy",):
            assert r32[n].dtype == np.float32, (n, r32[n].dtype)
            arrays[n] = r32[n]
        path = os.path.join(OUT, FILES[case])
        np.savez_compressed(path, **arrays)
        assert os.path.getsize(path) < (1 << 20), os.path.getsize(path)
        meta[case] = dict(kind=spec["kind"], seed=spec["seed"], ln_jitter=spec["ln_jitter"], lens=list(spec["lens"]), L=L, n_rows=3 * L,
                          position_mode=mode, padding_idx=pad, eps=eps, loss=info["loss"], loss_fp64=info64["loss"],
                          weights_sha256=info["weights_sha256"], embeddings_sha256=info["embeddings_sha256"],
                          param_names=list(U.PARAMS), ref_err=ref_err, same_inputs=same_inputs, fp64_restatement_rel=restated,
                          scale={n: float(np.abs(w32[n]).max()) for n in U.NAMES})
        print("%s %d B" % (FILES[case], os.path.getsize(path)))
    with open(os.path.join(OUT, "embeddings.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
    print(json.dumps(meta, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
