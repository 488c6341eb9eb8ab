"""Generates tests/golden/layer_tail.npz (the rdot tower), layer_tail_bert.npz (the bert tower) and layer_tail.json by running the
REAL reference (imported through oracle/ref_harness.py) on the CPU in the build container:

    python tests/golden/make_golden_layer_tail.py

The two shallow towers, triplets and losses of make_golden_attention_train.py (its CASES and its run(), with other hooks), in eval
mode, once in fp32 and once after model.double().  In layer 0 of each tower, for the three row-wise seams
  attention.output   BertSelfOutput.forward   LayerNorm(dropout(dense(x)) + input_tensor)
  output             BertOutput.forward       the same
  intermediate       BertIntermediate.forward gelu(dense(x))
hooks capture: the dense module's output minus its bias (x), input_tensor (res), the module's output (y), the gradient arriving at the
output (dy) and the one leaving through the dense output (dx); after the backward, the .grad of the seam's parameters (dbias of the
dense, dgamma / dbeta of the LayerNorm), which the three tower calls of the triplet accumulate -- so they are the column sums over
the rows of all three calls.  In eval mode the dropout is the identity and the gradient leaving through input_tensor (dres) is the
one leaving through the dense output, bit for bit: dres is not stored, the tests compare against dx.
Committed (fp32): every row, pad rows included, of both tails; the `output` tail's input_tensor is the `attention.output` tail's y
and is stored once; of the intermediate as many leading rows as keep the file under 1 MiB, with dbias restated as the fp32 sum of
the reference's dx over those rows.  The JSON records per tensor ref_err (max |fp32 run - fp64 run|), same_inputs (the distance of
tests/layer_tail_util.py's eager fp32 expression from its fp64 restatement on the committed inputs), fp64_restatement_rel (the
restatement on the fp64 run's inputs against the fp64 run's own tensors, asserted <= 1e-12 relative here), the weights' sha256 and
the parameter names of the reference's BertLayer."""
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
import layer_tail_util as U  # noqa: E402
import make_golden_attention_train as M  # noqa: E402

FILES = {"rdot": "layer_tail.npz", "bert": "layer_tail_bert.npz"}
RAW_BUDGET = 1250000   # bytes of raw fp32 per file: compressed (about 0.73 of raw) the file stays under 1 MiB
TAILS = ("attention.output", "output")


def capture(layer, store):
    """Hooks on one BertLayer's three seams: per tower call, x / res / y and the gradients dy / dx."""
    handles = []

    def keep(name, t):
        store.setdefault(name, []).append(t.detach().clone())
        i = len(store[name]) - 1
        return lambda g: store.setdefault("d" + name, {}).__setitem__(i, g.detach().clone())

    for seam, mod in (("attention.output", layer.attention.output), ("output", layer.output), ("intermediate", layer.intermediate)):
        def dense_hook(m, _inp, out, seam=seam):
            out.register_hook(keep(seam + ".x", out - m.bias))       # d(loss) / dx is the gradient at the dense output
        handles.append(mod.dense.register_forward_hook(dense_hook))

        def out_hook(_m, inp, out, seam=seam):
            if len(inp) > 1:
                store.setdefault(seam + ".res", []).append(inp[1].detach().clone())
            out.register_hook(keep(seam + ".y", out))
        handles.append(mod.register_forward_hook(out_hook))
    return handles


def run(ref, spec, dtype):
    """make_golden_attention_train.run with this file's hooks; also the seams' parameter gradients and the layer's parameter names."""
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
        forward, layer, eps = ref.models.BiEncoder.forward, tower.encoder.layer[0], tower.config.layer_norm_eps
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
        model, forward, layer, eps = tower, ref.models.NLL.forward, tower.roberta.encoder.layer[0], tower.roberta.config.layer_norm_eps
    tower.eval()
    if dtype == torch.float64:
        tower.double()
    store = {}
    handles = capture(layer, store)
    t = torch.from_numpy(ids).long()
    mask = encoder_ref.mask_from_lengths(np.asarray(lens, np.int32), L)
    (loss,) = forward(model, t[0:1], mask[0:1], t[1:2], mask[1:2], t[2:3], mask[2:3])
    loss.backward()
    for h in handles:
        h.remove()
    out = {}
    for seam in U.SEAMS:
        for n in ("x", "y"):
            key = "%s.%s" % (seam, n)
            assert len(store[key]) == 3, (key, len(store[key]))
            out[key] = torch.cat(store[key], 0).numpy().reshape(3 * L, -1)
            out["%s.d%s" % (seam, n)] = torch.cat([store["d" + key][i] for i in range(3)], 0).numpy().reshape(3 * L, -1)
        mod = layer.attention.output if seam == "attention.output" else getattr(layer, seam)
        out[seam + ".bias"] = mod.dense.bias.detach().numpy().copy()
        out[seam + ".dbias"] = mod.dense.bias.grad.numpy().copy()
        if seam in TAILS:
            out[seam + ".res"] = torch.cat(store[seam + ".res"], 0).numpy().reshape(3 * L, -1)
            for n, p in (("gamma", mod.LayerNorm.weight), ("beta", mod.LayerNorm.bias)):
                out["%s.%s" % (seam, n)] = p.detach().numpy().copy()
                out["%s.d%s" % (seam, n)] = p.grad.numpy().copy()
    return out, float(eps), list(layer.state_dict().keys()), encoder_ref.state_dict_sha256(sd)


def seam_results(r, seam, eps, fn_tail, fn_gelu, rows=None):
    """The util's restatement (fp64 or eager fp32) of one seam on the tensors of run r, over the leading `rows` rows."""
    s = slice(None, rows)
    if seam in TAILS:
        return fn_tail(r[seam + ".x"][s], r[seam + ".bias"], r[seam + ".res"][s], r[seam + ".gamma"], r[seam + ".beta"], eps, r[seam + ".dy"][s])
    return fn_gelu(r[seam + ".x"][s], r[seam + ".bias"], r[seam + ".dy"][s])


def names_of(seam):
    return ("y", "dx", "dgamma", "dbeta", "dbias") if seam in TAILS else ("y", "dx", "dbias")


def main():
    ref = ref_harness.load_reference()
    meta = dict(generator="tests/golden/make_golden_layer_tail.py", torch=torch.__version__, files=FILES)
    for case, spec in M.CASES.items():
        r32, eps, names, sha = run(ref, spec, torch.float32)
        r64, _, _, _ = run(ref, spec, torch.float64)
        n_rows = 3 * spec["L"]
        assert np.array_equal(r32["output.res"], r32["attention.output.y"])   # stored once
        arrays, seams = {}, {}
        tail_bytes = 0
        for seam in U.SEAMS:
            width = r32[seam + ".x"].shape[1]
            if seam in TAILS:
                rows = n_rows
            else:
                rows = min(n_rows, (RAW_BUDGET - tail_bytes) // (4 * 4 * width))
                assert rows >= 4, rows
            # the fp64 restatement on the fp64 run's inputs reproduces the fp64 run (all rows: the parameter gradients are over all)
            want64 = seam_results(r64, seam, eps, U.tail_fp64, U.gelu_fp64)
            restated = {}
            for n in names_of(seam):
                own = r64["%s.%s" % (seam, n)]
                d = float(np.abs(want64[n] - own).max() / np.abs(own).max())
                assert d <= 1e-12, (case, seam, n, d)
                restated[n] = d
            committed = {n: r32["%s.%s" % (seam, n)][:rows] for n in ("x", "y", "dy", "dx")}
            own64 = {n: r64["%s.%s" % (seam, n)][:rows] for n in ("y", "dx")}
            for n in names_of(seam)[2:]:
                if rows == n_rows:
                    committed[n], own64[n] = r32["%s.%s" % (seam, n)], r64["%s.%s" % (seam, n)]
                else:   # the intermediate's dbias over the committed rows only
                    committed[n] = torch.from_numpy(r32[seam + ".dx"][:rows]).sum(0).numpy()
                    own64[n] = r64[seam + ".dx"][:rows].sum(0)
            ref_err = {n: float(np.abs(committed[n].astype(np.float64) - own64[n]).max()) for n in names_of(seam)}
            w32 = seam_results(r32, seam, eps, U.tail_fp64, U.gelu_fp64, rows)
            e32 = seam_results(r32, seam, eps, U.tail_eager_fp32, U.gelu_eager_fp32, rows)
            same_inputs = U.distances(e32, w32, names_of(seam))
            committed["bias"] = r32[seam + ".bias"]
            if seam in TAILS:
                committed["gamma"], committed["beta"] = r32[seam + ".gamma"], r32[seam + ".beta"]
                if seam == "attention.output":
                    committed["res"] = r32[seam + ".res"]
            for n, a in committed.items():
                assert a.dtype == np.float32, (seam, n, a.dtype)
                arrays["%s.%s" % (seam, n)] = a
                if seam in TAILS:
                    tail_bytes += a.nbytes
            seams[seam] = dict(rows=int(rows), width=int(width), ref_err=ref_err, same_inputs=same_inputs, fp64_restatement_rel=restated,
                               scale={n: float(np.abs(w32[n]).max()) for n in names_of(seam)})
        path = os.path.join(OUT, FILES[case])
        np.savez_compressed(path, **arrays)
        assert os.path.getsize(path) < (1 << 20), os.path.getsize(path)
        meta[case] = dict(lens=list(spec["lens"]), L=spec["L"], n_rows=n_rows, eps=eps, weights_sha256=sha, layer_param_names=names,
                          seams=seams)
        print("%s %d B" % (FILES[case], os.path.getsize(path)))
    with open(os.path.join(OUT, "layer_tail.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
    print(json.dumps(meta, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
