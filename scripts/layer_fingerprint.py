#!/usr/bin/env python
"""SHA-256 fingerprints of everything the BertLayer seams, the layers and the models built on them compute (ance_amd.layers ->
csrc/layer_tail_kernels.h behind layer_tail_common.h; ance_amd.model): the check that a restructuring of the Python front end, of the
host front end or of the kernels moved no bit.  Both the library and the Python may change, so whole trees are compared:

    python scripts/layer_fingerprint.py                                   # the tree this script is in
    python scripts/layer_fingerprint.py --trees PARENT_DIR NEW_DIR --out F  # one fresh child process per tree; exit 1 unless they agree

A tree is a checkout with its own built ``ance_amd/libance_amd.so``; its child process has that tree first on ``sys.path``.  Only names
that both trees have are used: dropout_add_layer_norm, bias_gelu, the four BertLayer methods, SeedLayer, BertEmbeddings.pack, the model
classes, manual_seed, dropout_state.  A hash is taken over the raw bytes of every tensor of a case, in a fixed order, each under its
name; a NaN in any of them fails the run (the models' embeddings excepted where a dropped sequence is the point: none is here).
Cases (inputs from numpy.random.RandomState with fixed seeds):
  seams    dropout_add_layer_norm: y (y16), dx, dres, dgamma, dbeta, dbias; bias_gelu: y, dx, dbias.  fp32 / fp16 / bf16; H 768 and
           1024, N 3072 and 4096; x contiguous and as a strided view (row stride W + 4 in fp32, W + 8 in 16 bits); bias present and None
           (tail); the residual contiguous and as the [:, 0] view of [rows, 3, H]; 16-bit tail: return_half off, and on with the gradient
           arriving through y only, y16 only and both; dropout off, p = 0.1 under the host pair, p = 0.1 under the device stream.  One hash
           per such case covers rows 1, 15, 16, 17, 65 (the 4-rows-per-wave and 16-rows-per-workgroup edges) and two calls each, so that
           the offset moves.
  layers   BertLayer and SeedLayer, 768 / 12 / 3072: B = 4, L = 40, lengths (40, 17, 1, 0), the packed forms with the same lengths in
           64 rows (6 that no sequence covers); forward, forward_first_rows, forward_packed, forward_first_rows_packed; fp32, half under
           fp16 and bf16 autocast, and attention_precision="half" with fp32 seams (BertLayer); training with p = 0.1 (host pair, device
           stream) and eval: the output, the input gradient and the 16 parameter gradients.  BertLayer 1024 / 16 / 4096: forward only.
  models   two layers, vocabulary 64, 48 positions: RobertaDot_NLL_LN padded and with set_packed_rows(query=64, body=160), BiEncoder,
           SEEDEncoderDot_NLL_LN; fp32 and fp16 autocast, p = 0.1: the loss, the three embeddings and every parameter gradient of one
           step, and packed_dropped.  (RobertaDot_CLF_ANN_NLL_MultiChunk is left out: its 512-token chunks run the same tower code.)"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import types

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P_DROP = 0.1
SEED = 20241
ROWS = (1, 15, 16, 17, 65)
LENS, L_PAD, PACK_ROWS = (40, 17, 1, 0), 40, 64


def fingerprints(tree):
    sys.path.insert(0, tree)
    os.environ.pop("ANCE_AMD_LIB", None)   # the tree's own library
    import numpy as np
    import torch
    import ance_amd
    from ance_amd import attention as A
    from ance_amd import layers as Ly
    from ance_amd import model as M
    from ance_amd.embeddings import BertEmbeddings
    assert os.path.abspath(ance_amd.__file__).startswith(os.path.abspath(tree) + os.sep), ance_amd.__file__

    dev = torch.device("cuda", 0)
    dtypes = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}
    out = {}

    class Case(object):
        """One hash over the named tensors added to it, in order."""

        def __init__(self, name):
            self.name, self.h, self.n = name, hashlib.sha256(), 0

        def add(self, what, t, nan_ok=False):
            if t is None:
                self.h.update(("%s=None;" % what).encode())
                return
            t = t.detach()
            assert nan_ok or not bool(torch.isnan(t.float()).any()), "%s/%s: NaN" % (self.name, what)
            self.h.update(("%s:%s:%r;" % (what, t.dtype, tuple(t.shape))).encode())
            self.h.update(t.contiguous().reshape(-1).view(torch.uint8).cpu().numpy().tobytes())
            self.n += 1

        def close(self):
            assert self.name not in out and self.n > 0, self.name
            out[self.name] = self.h.hexdigest()

    def normal(seed, shape, std=1.0, dtype=torch.float32):
        return torch.from_numpy((np.random.RandomState(seed).standard_normal(shape) * std).astype(np.float32)).to(dev).to(dtype)

    def with_dropout(mode, body, calls=2):
        """body(p, call) under one mode: off, the host pair, or the device stream."""
        A.manual_seed(SEED)
        if mode == "device":
            A.dropout_state.to_device(dev)
        for call in range(calls):
            body(0.0 if mode == "off" else P_DROP, call)
        if mode == "device":
            A.dropout_state.to_host(dev)

    def strided(t, pad):
        """t's values in a leaf whose rows are pad elements further apart: (leaf, view)."""
        wide = torch.cat([t, torch.full(t.shape[:-1] + (pad,), float("nan"), dtype=t.dtype, device=dev)], dim=-1).requires_grad_()
        return wide, wide[..., :t.shape[-1]]

    # ------------------------------------------------------------------------------------------------------------ seams
    for pname, dtype in dtypes.items():
        half = dtype != torch.float32
        prec = dict(precision="half") if half else {}
        pad = 8 if half else 4
        for H in (768, 1024):
            for layout in ("contiguous", "strided"):
                for use_bias in (True, False):
                    for res_form in ("contiguous", "view"):
                        for ret in (("y", "y16", "both", "off") if half else ("off",)):
                            for mode in ("off", "host", "device"):
                                case = Case("tail/%s/H%d/x-%s/%s/res-%s/half-%s/%s" % (pname, H, layout, "bias" if use_bias else "nobias",
                                                                                       res_form, ret, mode))

                                def body(p, call):
                                    for n in ROWS:
                                        x = normal(1000 + n + call, (n, H), 1.0, dtype)
                                        xl, xv = strided(x, pad) if layout == "strided" else (x.requires_grad_(), x)
                                        r = normal(2000 + n + call, (n, H))
                                        if res_form == "view":
                                            rl = torch.stack([r, r + 1, r + 2], dim=1).requires_grad_()
                                            rv = rl[:, 0]
                                        else:
                                            rl = rv = r.requires_grad_()
                                        b = normal(3000 + H, (H,), 0.1).requires_grad_() if use_bias else None
                                        g, be = (1.0 + normal(3001 + H, (H,), 0.1)).requires_grad_(), normal(3002 + H, (H,), 0.1).requires_grad_()
                                        y = Ly.dropout_add_layer_norm(xv, b, rv, g, be, 1e-5, p, True, return_half=ret != "off", **prec)
                                        y, y16 = y if ret != "off" else (y, None)
                                        outs, gouts = [], []
                                        if ret in ("off", "y", "both"):
                                            outs.append(y)
                                            gouts.append(normal(4000 + n + call, (n, H), 0.1))
                                        if ret in ("y16", "both"):
                                            outs.append(y16)
                                            gouts.append(normal(4100 + n + call, (n, H), 0.1, dtype))
                                        ins = [xl, rl, g, be] + ([b] if use_bias else [])
                                        grads = torch.autograd.grad(outs, ins, gouts)
                                        tag = "n%d/call%d/" % (n, call)
                                        case.add(tag + "y", y)
                                        case.add(tag + "y16", y16)
                                        dx = grads[0][..., :H] if layout == "strided" else grads[0]
                                        dres = grads[1][:, 0] if res_form == "view" else grads[1]
                                        for what, t in zip(("dx", "dres", "dgamma", "dbeta", "dbias"), [dx, dres] + list(grads[2:])):
                                            case.add(tag + what, t)
                                with_dropout(mode, body)
                                case.close()
        for N in (3072, 4096):
            for layout in ("contiguous", "strided"):
                case = Case("gelu/%s/N%d/x-%s" % (pname, N, layout))
                for call in range(2):
                    for n in ROWS:
                        x = normal(5000 + n + call, (n, N), 1.5, dtype)
                        xl, xv = strided(x, pad) if layout == "strided" else (x.requires_grad_(), x)
                        b = normal(5100 + N, (N,), 0.1).requires_grad_()
                        y = Ly.bias_gelu(xv, b, **prec)
                        dx, db = torch.autograd.grad(y, [xl, b], normal(5200 + n + call, (n, N), 0.1, dtype))
                        tag = "n%d/call%d/" % (n, call)
                        case.add(tag + "y", y)
                        case.add(tag + "dx", dx[..., :N] if layout == "strided" else dx)
                        case.add(tag + "dbias", db)
                case.close()

    # ----------------------------------------------------------------------------------------------------------- layers
    def fill(module, seed):
        """Every parameter from its own seeded draw: weights N(0, 0.02), vectors N(0, 0.1), LayerNorm weights around 1."""
        with torch.no_grad():
            for i, (name, p) in enumerate(module.named_parameters()):
                v = normal(seed + i, tuple(p.shape), 0.02 if p.dim() == 2 else 0.1)
                if p.dim() == 1 and (name.endswith("LayerNorm.weight") or name.endswith("norm.weight")):
                    v = v + 1.0
                p.copy_(v)
        return module

    B = len(LENS)
    d_lens = torch.tensor(LENS, dtype=torch.int32, device=dev)
    ids = torch.from_numpy(np.random.RandomState(7).randint(2, 64, size=(B, L_PAD))).to(dev)
    packed = BertEmbeddings(64, 768, 48, 1, 1e-5, 0.1, 1, "roberta").to(dev).pack(ids, d_lens, PACK_ROWS)

    def layer_case(name, layer, hidden, methods, autocast):
        for method in methods:
            for mode in ("host", "device", "eval"):   # the layer's own p = 0.1 in training; eval draws nothing
                case = Case("%s/%s/%s" % (name, method, mode))
                layer.train(mode != "eval")

                def body(_p, call):
                    shape = (PACK_ROWS, hidden) if "packed" in method else (B, L_PAD, hidden)
                    hs = normal(6000 + call, shape).requires_grad_()
                    where = packed if "packed" in method else d_lens
                    with torch.autocast("cuda", dtype=autocast, enabled=autocast is not None):
                        y = getattr(layer, method)(hs, where)
                    params = [p_ for _, p_ in layer.named_parameters()]
                    grads = torch.autograd.grad(y, [hs] + params, normal(6100 + call, tuple(y.shape), 0.1), allow_unused=True)
                    case.add("call%d/out" % call, y)
                    case.add("call%d/dhidden" % call, grads[0])
                    for (pn, _), g in zip(layer.named_parameters(), grads[1:]):
                        case.add("call%d/d.%s" % (call, pn), g)
                with_dropout("off" if mode == "eval" else mode, body)
                case.close()

    four = ("forward", "forward_first_rows", "forward_packed", "forward_first_rows_packed")
    variants = (("fp32", dict(), None), ("half-fp16", dict(precision="half"), torch.float16), ("half-bf16", dict(precision="half"), torch.bfloat16),
                ("att-half-fp16", dict(attention_precision="half"), torch.float16))
    for vname, kw, autocast in variants:
        layer = fill(Ly.BertLayer(768, 12, 3072, 1e-12, P_DROP, P_DROP, **kw).to(dev), 7000)
        layer_case("BertLayer768/" + vname, layer, 768, four, autocast)
        if "attention_precision" not in kw:
            seed_layer = fill(Ly.SeedLayer(768, 12, 3072, 1e-5, P_DROP, P_DROP, **kw).to(dev), 7100)
            layer_case("SeedLayer768/" + vname, seed_layer, 768, four, autocast)
        wide = fill(Ly.BertLayer(1024, 16, 4096, 1e-12, P_DROP, P_DROP, **kw).to(dev), 7200)
        layer_case("BertLayer1024/" + vname, wide, 1024, ("forward",), autocast)

    # ----------------------------------------------------------------------------------------------------------- models
    def batch(seed, lens, L, pad_id, low):
        lens = np.asarray(lens)
        ids = np.random.RandomState(seed).randint(low, 64, size=(len(lens), L))
        mask = (np.arange(L)[None, :] < lens[:, None]).astype(np.int64)
        ids = np.where(mask != 0, ids, pad_id)
        return torch.from_numpy(ids).to(dev), torch.from_numpy(mask).to(dev)

    def model_case(name, model, pad_id, autocast):
        model = fill(model.to(dev), 8000).train()
        q = batch(81, (16, 5, 1, 9), 16, pad_id, 2)
        a = batch(82, (40, 17, 3, 28), 40, pad_id, 2)
        b = batch(83, (2, 40, 31, 8), 40, pad_id, 2)
        case = Case(name)
        A.manual_seed(SEED)
        with torch.autocast("cuda", dtype=autocast, enabled=autocast is not None):
            loss = model(q[0], q[1], a[0], a[1], b[0], b[1])[0]
        loss.backward()
        case.add("loss", loss)
        for pn, p in model.named_parameters():
            case.add("d." + pn, p.grad)
        with torch.autocast("cuda", dtype=autocast, enabled=autocast is not None):
            case.add("query_emb", model.query_emb(q[0], q[1]))
            case.add("body_emb_a", model.body_emb(a[0], a[1]))
            case.add("body_emb_b", model.body_emb(b[0], b[1]))
        case.add("packed_dropped", getattr(model, "packed_dropped", None))
        case.close()

    def tower_config(type_vocab, eps, pad_id):
        return M.TowerConfig(64, 768, 2, 3072, 48, type_vocab, eps, pad_id, P_DROP, P_DROP)

    seed_config = types.SimpleNamespace(pad_token_id=1, vocab_size=64, encoder_layers=2, encoder_embed_dim=768, encoder_ffn_embed_dim=3072,
                                        encoder_attention_heads=12, dropout=P_DROP, attention_dropout=P_DROP, activation_dropout=0.0,
                                        encoder_layerdrop=0.0, max_positions=46, activation_fn="gelu", quant_noise_pq=0.0)
    for pname, kw, autocast in (("fp32", dict(), None), ("fp16", dict(precision="half"), torch.float16)):
        model_case("RobertaDot_NLL_LN/padded/" + pname, M.RobertaDot_NLL_LN(tower_config(1, 1e-5, 1), **kw), 1, autocast)
        model_case("RobertaDot_NLL_LN/packed/" + pname,
                   M.RobertaDot_NLL_LN(tower_config(1, 1e-5, 1), **kw).to(dev).set_packed_rows(query=64, body=160), 1, autocast)
        model_case("BiEncoder/padded/" + pname, M.BiEncoder(tower_config(2, 1e-12, 0), **kw), 0, autocast)
        model_case("SEEDEncoderDot_NLL_LN/" + pname, M.SEEDEncoderDot_NLL_LN(seed_config, **kw), 1, autocast)
    torch.cuda.synchronize()
    return dict(hashes=out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--trees", nargs="+", help="PARENT_DIR NEW_DIR ...: one fresh child process each, with its own built library")
    ap.add_argument("--child", help=argparse.SUPPRESS)
    ap.add_argument("--out", help="write the result as JSON")
    ap.add_argument("--timeout", type=int, default=420, help="seconds each child process may take")
    a = ap.parse_args()
    if not a.trees:
        res = fingerprints(os.path.abspath(a.child or HERE))
    else:
        got = {}
        for tree in a.trees:
            p = subprocess.run(["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child", os.path.abspath(tree)],
                               stdout=subprocess.PIPE, text=True, cwd=os.path.abspath(tree))
            if p.returncode != 0:
                sys.exit("fingerprint run of %s failed (%d)" % (tree, p.returncode))   # nothing more is started after a failure
            got[tree] = json.loads(p.stdout.strip().splitlines()[-1])
        first = got[a.trees[0]]
        # the first tree's hashes in full; of the others only what differs
        res = dict(trees=a.trees, n_hashes=len(first["hashes"]), hashes=first["hashes"])
        res["unequal"] = {tree: {k: got[tree]["hashes"].get(k) for k in sorted(set(first["hashes"]) | set(got[tree]["hashes"]))
                                 if first["hashes"].get(k) != got[tree]["hashes"].get(k)} for tree in a.trees[1:]}
    text = json.dumps(res, indent=1, sort_keys=True) if a.out else json.dumps(res, sort_keys=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text if not a.out else "%d hashes; unequal: %s" % (len(res["hashes"]), res.get("unequal")))
    if a.trees and any(res["unequal"].values()):
        sys.exit(1)


if __name__ == "__main__":
    main()
