"""Generates tests/golden/attention_train.npz and attention_train.json by running the REAL reference (imported through
oracle/ref_harness.py) on the CPU in the build container:

    python tests/golden/make_golden_attention_train.py

Two shallow towers of the reference's own classes in eval mode, weights from oracle.encoder_ref.det_state_dict, one backward of the
reference's own NLL loss over one triplet (the query, the positive and the negative passage padded to one length, so the three tower
calls are the three sequences of one padded batch):
  rdot   RobertaDot_NLL_LN (model/models.py:137-157), 2 layers, NLL.forward (:58-81)
  bert   HFBertEncoder (:223-244), 2 layers, as both towers of BiEncoder.forward's triplet branch (:260-271)
In layer 0 of each tower, forward hooks on attention.self.query / key / value capture q, k, v [1, L, 768]; a forward pre-hook on
attention.output.dense captures context_layer; tensor hooks on the four capture their gradients.  (Layer 0 of two: the gradient
that reaches its context_layer is dense over the valid rows and exactly zero at pad rows -- layer 1's pad keys are masked.)  The
whole run is made twice, in fp32 and after model.double().
Committed: the VALID rows of the fp32 q, k, v, dctx (inputs) and of the reference's fp32 ctx, dq, dk, dv (results); in the JSON,
per tensor, max |delta| between the reference's fp32 and fp64 runs over those rows (ref_err; for lse, which the reference never
forms, that of tests/attention_train_util.py's eager fp32 expression against fp64), the distance between the util's fp64 restatement
on the fp64 run's inputs and the fp64 run's own tensors (asserted <= 1e-12 relative here), and the sha256 of the weights."""
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from oracle import encoder_ref, ref_harness  # noqa: E402
import attention_train_util as A  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
N_HEADS = 12
CASES = {
    # lens = (query, positive, negative); L = the padded length of all three
    # rdot: the negative is the positive with one token changed -- the layer-normed embeddings have norm ~ 28, and two unrelated
    # passages saturate the two-way softmax (loss 0.0 in fp32, gradients of 1e-11)
    "rdot": dict(kind="rdot_nll", lens=(4, 7, 7), L=9, seed=41, ln_jitter=0.1, negative_edits_positive=True),
    "bert": dict(kind="bert", lens=(3, 6, 2), L=8, seed=42, ln_jitter=0.1),
}


def load_into(model, sd):
    missing, unexpected = model.load_state_dict(sd, strict=False)
    bad = [k for k in missing if not (k.startswith("classifier.") or "pooler" in k or "position_ids" in k)]
    assert not bad and not unexpected, (bad, unexpected)


def capture(layer, store):
    """Hooks on one BertLayer's attention: appends (q, k, v, ctx) per tower call and their gradients."""
    att = layer.attention
    handles = []

    def grab(name):
        def hook(_m, _inp, out):
            store.setdefault(name, []).append(out.detach().clone())
            i = len(store[name]) - 1
            out.register_hook(lambda g: store.setdefault("d" + name, {}).__setitem__(i, g.detach().clone()))
        return hook

    for name, mod in (("q", att.self.query), ("k", att.self.key), ("v", att.self.value)):
        handles.append(mod.register_forward_hook(grab(name)))

    def pre(_m, inp):
        x = inp[0]
        store.setdefault("ctx", []).append(x.detach().clone())
        i = len(store["ctx"]) - 1
        x.register_hook(lambda g: store.setdefault("dctx", {}).__setitem__(i, g.detach().clone()))
    handles.append(att.output.dense.register_forward_pre_hook(pre))
    return handles


def run(ref, spec, dtype):
    lens, L = spec["lens"], spec["L"]
    rng = np.random.default_rng(spec["seed"])
    if spec["kind"] == "bert":
        sd = encoder_ref.det_state_dict(kind="bert", seed=spec["seed"], n_layers=2, vocab=30522, max_pos=512, head=False,
                                        prefixes=("",), ln_jitter=spec["ln_jitter"])
        tower = ref_harness.build_reference_model("bert", n_layers=2, seed=0)
        load_into(tower, sd)
        ids = rng.integers(1000, 30522, size=(3, L))
        ids[:, 0] = 101
        ids = np.where(np.arange(L)[None, :] < np.asarray(lens)[:, None], ids, 0)
        model = types.SimpleNamespace(query_emb=lambda i, m: tower(i, m)[1], body_emb=lambda i, m: tower(i, m)[1])
        forward, layer = ref.models.BiEncoder.forward, tower.encoder.layer[0]
    else:
        sd = encoder_ref.det_state_dict(seed=spec["seed"], n_layers=2, ln_jitter=spec["ln_jitter"])
        tower = ref_harness.build_reference_model("rdot_nll", n_layers=2, seed=0)
        load_into(tower, sd)
        ids = rng.integers(3, 50265, size=(3, L))
        ids[:, 0] = 0
        if spec.get("negative_edits_positive"):
            ids[2] = ids[1]
            ids[2, lens[2] - 2] = 777
        ids = np.where(np.arange(L)[None, :] < np.asarray(lens)[:, None], ids, 1)
        model, forward, layer = tower, ref.models.NLL.forward, tower.roberta.encoder.layer[0]
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
    for name in ("q", "k", "v", "ctx"):
        assert len(store[name]) == 3, (name, len(store[name]))
        out[name] = torch.cat(store[name], 0).numpy()
        out["d" + name] = torch.cat([store["d" + name][i] for i in range(3)], 0).numpy()
    return out, float(loss), encoder_ref.state_dict_sha256(sd)


def main():
    ref = ref_harness.load_reference()
    arrays, meta = {}, dict(generator="tests/golden/make_golden_attention_train.py", torch=torch.__version__, n_heads=N_HEADS)
    for case, spec in CASES.items():
        lens, L = np.asarray(spec["lens"], np.int32), spec["L"]
        r32, loss32, sha = run(ref, spec, torch.float32)
        r64, loss64, _ = run(ref, spec, torch.float64)
        rows = np.arange(L)[None, :] < lens[:, None]
        for n in ("dq", "dk", "dv", "dctx"):   # what the contract relies on: the reference's gradients are zero at pad rows
            assert np.abs(r64[n][~rows]).max() == 0.0 and np.abs(r32[n][~rows]).max() == 0.0, n
        # the util's fp64 restatement on the fp64 run's inputs reproduces the fp64 run
        want = A.attention_fp64(r64["q"], r64["k"], r64["v"], r64["dctx"], lens, N_HEADS)
        restated = {}
        for n in ("ctx", "dq", "dk", "dv"):
            d = float(np.abs(want[n][rows] - r64[n][rows]).max() / np.abs(r64[n][rows]).max())
            assert d <= 1e-12, (case, n, d)
            restated[n] = d
        ref_err = {n: float(np.abs(r32[n][rows].astype(np.float64) - r64[n][rows]).max()) for n in ("ctx", "dq", "dk", "dv")}
        w32 = A.attention_fp64(r32["q"], r32["k"], r32["v"], r32["dctx"], lens, N_HEADS)
        ref_err["lse"] = A.distances(A.eager_fp32(r32["q"], r32["k"], r32["v"], r32["dctx"], lens, N_HEADS), w32)["lse"]
        # the same fp32 results against fp64 on the SAME fp32 inputs: recorded for the reader, not used as a bound
        same_inputs = {n: float(np.abs(r32[n][rows].astype(np.float64) - w32[n][rows]).max()) for n in ("ctx", "dq", "dk", "dv")}
        for n in ("q", "k", "v", "dctx", "ctx", "dq", "dk", "dv"):
            assert r32[n].dtype == np.float32
            arrays["%s.%s" % (case, n)] = A.pack(r32[n], lens)[0]
        meta[case] = dict(lens=[int(x) for x in lens], L=L, weights_sha256=sha, loss=loss32, loss_fp64=loss64, ref_err=ref_err,
                          ref_fp32_vs_fp64_on_same_inputs=same_inputs, fp64_restatement_rel=restated,
                          scale={n: float(np.abs(w32[n]).max()) for n in A.NAMES})
    np.savez_compressed(os.path.join(OUT, "attention_train.npz"), **arrays)
    with open(os.path.join(OUT, "attention_train.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
    print("attention_train.npz %d B" % os.path.getsize(os.path.join(OUT, "attention_train.npz")))
    print(json.dumps(meta, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
