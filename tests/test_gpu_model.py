"""ance_amd/model.py on the GPU: the reference's classes assembled from the differentiable pieces, with a first-rows-only last layer.

  eval-mode pins      the reference's own outputs in the existing fixtures (nll.npz, encoder_firstp12 / bert12 / large24.npz): 2e-5, the
                      project's stated fp32 tolerance (test_gpu_encoder.py); the large tower max(2e-5, 4 x its fp32-vs-fp64 distance)
                      (test_gpu_large.py); the losses 1e-4 (test_nll.py)
  gradients           tests/golden/model_step.npz: the reference's own forward + backward in fp64; loss and every stored gradient within
                      max(4 x ref_err, 16 ulp32) (train_step_util.compare), ref_err the reference's own fp32 run's distance
  training mode       dropout 0.1 against the fp64 restatement with the restated masks (model_util.first_row_masks), same bound with
                      ref_err the eager fp32 restatement's distance
  precision="half"    under autocast against the fp32 model: max(4 x D, 16 ulp32), D the eager autocast tower's own distance
  replay              three captured-and-replayed steps equal the eager host-mode steps bit for bit
  hand-off            Encoder(model.reference_state_dict()) against model.eval(): 4e-5 (both are held to the reference within 2e-5)
"""
import functools
import json
import os

import numpy as np
import pytest
import torch

import attention_train_util as A
import lamb_util as U
import model_util as M
import train_step_util as S
from golden_util import golden_weights

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SEED = S.SEED
ROBERTA_BASE = dict(S.BASE, mode="roberta", n_types=1, pad=1)   # BASE's shapes as a RoBERTa tower: what RobertaDot_NLL_LN runs


@pytest.fixture(autouse=True)
def _host_mode_afterwards():
    from ance_amd import attention as T
    yield
    T.dropout_state.to_host(0)
    T.manual_seed(SEED)


def _np(t):
    return t.detach().float().cpu().numpy()


def _ids(x):
    return torch.from_numpy(np.ascontiguousarray(x)).long().to(DEV)


def _mask(lens, L):
    return (torch.arange(L)[None, :] < torch.as_tensor(np.asarray(lens))[:, None]).long().to(DEV)


def _json(golden_dir, name):
    with open(os.path.join(golden_dir, name)) as f:
        return json.load(f)


def _config(cfg, p):
    from ance_amd.model import TowerConfig
    return TowerConfig(S.VOCAB, cfg["H"], cfg["N"], cfg["inter"], S.MAX_POS, cfg["n_types"], cfg["eps"], cfg["pad"], p, p, cfg["heads"])


def _load(model, sd):
    return model.to(DEV).load_reference_state_dict({k: torch.from_numpy(np.ascontiguousarray(v, np.float32)) for k, v in sd.items()})


def _bits_equal(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.reshape(-1).contiguous().view(torch.uint8),
                                                                           b.reshape(-1).contiguous().view(torch.uint8))


# ---------------------------------------------------------------------------------------------------------------- 3. eval-mode pins
@functools.lru_cache(maxsize=None)
def _nll_models(golden_dir):
    from ance_amd import model
    j = _json(golden_dir, "nll.json")
    first = model.RobertaDot_NLL_LN.from_state_dict(golden_weights(j["firstp"]["weights"])).to(DEV).eval()
    maxp = model.RobertaDot_CLF_ANN_NLL_MultiChunk.from_state_dict(golden_weights(j["maxp"]["weights"])).to(DEV).eval()
    return j, np.load(os.path.join(golden_dir, "nll.npz")), first, maxp


def test_eval_firstp_embeddings_and_loss_of_the_reference(golden_dir):
    j, g, m, _ = _nll_models(golden_dir)
    args = []
    for n, L in (("q", 32), ("a", 64), ("b", 64)):
        args += [_ids(g["f_%s_ids" % n]), _mask(g["f_%s_len" % n], L)]
    with torch.no_grad():
        embs = [m(args[0], args[1]), m(args[2], args[3], is_query=False), m.body_emb(args[4], args[5])]
        loss = m(*args)[0]
    for n, e in zip("qab", embs):
        d = float(np.abs(_np(e) - g["f_" + n]).max())
        print("firstp emb %s max|d| %.3e" % (n, d))
        assert tuple(e.shape) == g["f_" + n].shape and d <= 2e-5, (n, d)
    print("firstp loss %.7f reference %.7f" % (float(loss.detach()), j["firstp"]["loss"]))
    assert abs(float(loss.detach()) - j["firstp"]["loss"]) <= 1e-4


def test_eval_maxp_valid_chunks_and_loss_of_the_reference(golden_dir):
    j, g, _, m = _nll_models(golden_dir)
    args = [_ids(g["m_q_ids"]), _mask(g["m_q_len"], 32)]
    for n in "ab":
        args += [_ids(g["m_%s_ids" % n]), _mask(g["m_%s_len" % n], 2048)]
    with torch.no_grad():
        q, a, b = m.query_emb(args[0], args[1]), m.body_emb(args[2], args[3]), m.body_emb(args[4], args[5])
        loss = m(*args)[0]
    assert float(np.abs(_np(q) - g["m_q"]).max()) <= 2e-5
    some_pad = 0
    for n, e in (("a", a), ("b", b)):
        valid = np.asarray(g["m_%s_len" % n])[:, None] > np.arange(4)[None, :] * 512
        some_pad += int((~valid).sum())
        e = _np(e)
        assert e.shape == (6, 4, 768) and np.isfinite(e).all(), n   # every all-pad chunk's embedding is finite
        d = float(np.abs(e - g["m_" + n])[valid].max())
        print("maxp emb %s valid chunks max|d| %.3e" % (n, d))
        assert d <= 2e-5, (n, d)
    assert some_pad > 0
    print("maxp loss %.7f reference %.7f" % (float(loss.detach()), j["maxp"]["loss"]))
    assert abs(float(loss.detach()) - j["maxp"]["loss"]) <= 1e-4


def test_eval_twelve_layers_of_the_reference(golden_dir):
    from ance_amd import model
    g = np.load(os.path.join(golden_dir, "encoder_firstp12.npz"))
    m = model.RobertaDot_NLL_LN.from_state_dict(golden_weights(_json(golden_dir, "manifest.json")["encoder"]["firstp12"])).to(DEV).eval()
    with torch.no_grad():
        e = _np(m.body_emb(_ids(g["ids"]), _mask(g["lens"], g["ids"].shape[1])))
    d = float(np.abs(e - g["emb"]).max())
    print("firstp12 max|d| %.3e" % d)
    assert d <= 2e-5, d


def test_eval_bert_tower_without_a_head(golden_dir):
    from ance_amd import model
    g = np.load(os.path.join(golden_dir, "encoder_bert12.npz"))
    sd = golden_weights(_json(golden_dir, "manifest.json")["encoder12"]["bert12"], kind="bert", vocab=30522, max_pos=512, head=False,
                        prefixes=("ctx_model.",))
    sd.update({"question_model." + k[len("ctx_model."):]: v for k, v in list(sd.items())})
    m = model.BiEncoder.from_state_dict(sd).to(DEV).eval()
    ids = _ids(g["ids"])
    with torch.no_grad():
        e = _np(m.body_emb(ids, (ids != 0).long()))
        q = _np(m.query_emb(ids, (ids != 0).long()))
    d = float(np.abs(e - g["emb"]).max())
    print("bert12 max|d| %.3e" % d)
    assert e.shape == g["emb"].shape and d <= 2e-5, d
    assert np.array_equal(e, q)   # the same weights in both towers


def test_eval_large_tower_head_1024_to_768(golden_dir):
    from ance_amd import model
    meta = _json(golden_dir, "large_manifest.json")["encoder"]["large24"]
    g = np.load(os.path.join(golden_dir, "encoder_large24.npz"))
    m = model.RobertaDot_NLL_LN.from_state_dict(golden_weights(meta, hidden=1024, inter=4096)).to(DEV).eval()
    assert m.roberta.encoder.layer[0].num_attention_heads == 16 and tuple(m.embeddingHead.weight.shape) == (768, 1024)
    with torch.no_grad():
        e = _np(m.body_emb(_ids(g["ids"]), _mask(g["lens"], g["ids"].shape[1])))
    d, tol = float(np.abs(e - g["emb"]).max()), max(2e-5, 4.0 * meta["fp32_vs_fp64"])
    print("large24 max|d| %.3e tolerance %.3e" % (d, tol))
    assert d <= tol, (d, tol)


# ---------------------------------------------------------------------------------------------------------------- 4. the reference's gradients
@pytest.mark.parametrize("case", ["firstp", "maxp", "biencoder"])
def test_gradients_of_the_reference_step(golden_dir, case):
    """Loss and every stored fp64 gradient of the reference's own step within max(4 x ref_err, 16 ulp32); key.bias exactly zero."""
    from ance_amd import model
    from oracle import encoder_ref
    meta, g = _json(golden_dir, "model_step.json")[case], np.load(os.path.join(golden_dir, "model_step.npz"))
    w = {k: (tuple(v) if isinstance(v, list) else v) for k, v in meta["weights"].items() if k not in ("gen", "checksum")}
    sd = encoder_ref.det_state_dict(**w)
    assert encoder_ref.state_dict_sha256(sd) == meta["weights"]["checksum"]
    cls = dict(firstp=model.RobertaDot_NLL_LN, maxp=model.RobertaDot_CLF_ANN_NLL_MultiChunk, biencoder=model.BiEncoder)[case]
    m = cls.from_state_dict(sd).to(DEV).eval()
    args = []
    for n in "qab":
        ids = g["%s.%s_ids" % (case, n)]
        args += [_ids(ids), _mask(g["%s.%s_len" % (case, n)], ids.shape[1])]
    loss = m(*args)[0]
    loss.backward()
    with torch.no_grad():
        embs = [m.query_emb(args[0], args[1]), m.body_emb(args[2], args[3]), m.body_emb(args[4], args[5])]
    for n, e in zip("qab", embs):
        want = g["%s.emb.%s" % (case, n)]
        valid = np.ones(want.shape[:-1], bool)
        if want.ndim == 3:
            valid = np.asarray(g["%s.%s_len" % (case, n)])[:, None] > np.arange(want.shape[1])[None, :] * 512
        assert float(np.abs(_np(e) - want)[valid].max()) <= 2e-5, n
    got, want = {"loss": float(loss.detach())}, {"loss": meta["loss"]}
    params = dict(m.named_parameters())
    assert sorted(params) == meta["params"]
    for n, p in params.items():
        rows = g["%s.rows.%s" % (case, n)] if n.endswith("word_embeddings.weight") else None
        got[n] = M.golden_view(n, _np(p.grad).astype(np.float64), rows)
        want[n] = g["%s.grad.%s" % (case, n)]
        assert got[n].shape == want[n].shape, n
        if n.endswith("attention.self.key.bias"):
            assert not p.grad.any(), n
    bad, worst = S.compare("reference step " + case, got, want, meta["ref_err"])
    print("reference step %s largest d / bound %.3f" % (case, worst))
    assert not bad, bad
    assert sum(float(np.abs(want[n]).max()) > 1e-6 for n in params) > len(params) // 2   # not a comparison of zeros


# ---------------------------------------------------------------------------------------------------------------- 5. training mode
# The embeddings are LayerNorm outputs: the logits are in the hundreds and the objective saturated, so a triplet whose positive leads
# sends a rounded zero into its three sequences (train_step_util.TRIPLET_SEEDS).  These seeds of train_step_util.batches are the
# first at which, with these models' parameters (model_util.model_state: the head is H -> 768, BiEncoder has none), every triplet's
# negative leads -- searched on the CPU with the restatement, dropout as in the test that uses them; the tests assert it.
BATCH_SEEDS = dict(large_roberta_dot=11, base_biencoder=4, roberta_base_no_dropout=0)


def _negative_weights(embs):
    q, a, b = (np.asarray(e, np.float64) for e in embs)
    la, lb = (q * a).sum(-1), (q * b).sum(-1)
    return 1.0 / (1.0 + np.exp(la - lb))


def _call_args(calls, pad):
    out = []
    for c in calls:
        out += [_ids(c["ids"]), _mask(c["lens"], c["ids"].shape[1])]
    return out


@functools.lru_cache(maxsize=None)
def _training_case(which):
    """(cfg, state, prefixes, head, calls, masks, want fp64, ref_err) of one dropout-0.1 step; the reference is computed once."""
    p = 0.1
    if which == "large_roberta_dot":
        cfg, prefixes, head = S.LARGE, ("roberta.",) * 3, True
        sd = M.model_state(cfg)
    else:
        cfg, prefixes, head = S.BASE, ("question_model.", "ctx_model.", "ctx_model."), False
        sd = {}
        for pre, seed in (("question_model.", 73), ("ctx_model.", 74)):
            sd.update({k: v for k, v in M.model_state(cfg, seed, prefix=pre).items() if k.startswith(pre)})
    calls = [dict(c, types=None) for c in S.batches(cfg, 0, BATCH_SEEDS[which])]   # the models pass no token types: type 0
    masks = M.calls_first_row_masks(p, SEED, 0, cfg, calls)
    want = M.reference_step(sd, prefixes, calls, cfg, "triplet", masks, p, "float64", head)
    assert _negative_weights(want["embs"]).min() > 0.5   # every sequence of every call carries a full gradient
    ref32 = M.reference_step(sd, prefixes, calls, cfg, "triplet", masks, p, "float32", head)
    ref_err = S.distances(ref32["grads"], want["grads"])
    ref_err["loss"] = abs(ref32["loss"] - want["loss"])
    for i in range(3):
        ref_err["emb%d" % i] = float(np.abs(ref32["embs"][i].astype(np.float64) - want["embs"][i]).max())
    return cfg, sd, head, calls, want, ref_err


@pytest.mark.parametrize("which", ["base_biencoder", "large_roberta_dot"])
def test_training_step_with_dropout_against_fp64(which):
    """BASE (N = 2, absolute positions, no head: BiEncoder, towers of different weights) and LARGE (N = 1, RoBERTa positions, head
    1024 -> 768: RobertaDot_NLL_LN) at train_step_util.SHAPES, dropout 0.1: the embeddings, the loss and every parameter gradient
    against the fp64 restatement under the restated masks -- the last layer's tails draw the masks of a B-row call."""
    from ance_amd import attention as T
    from ance_amd import model
    cfg, sd, head, calls, want, ref_err = _training_case(which)
    m = model.RobertaDot_NLL_LN(_config(cfg, 0.1)) if head else model.BiEncoder(_config(cfg, 0.1))
    m = _load(m, sd).train()
    T.manual_seed(SEED)
    args = _call_args(calls, cfg["pad"])
    tower_q, tower_c = (m.roberta, m.roberta) if head else (m.question_model, m.ctx_model)
    loss = m(*args)[0]
    assert T.dropout_state.offsets[0] == 3 * S.draws_per_call(cfg)
    loss.backward()
    T.manual_seed(SEED)
    with torch.no_grad():
        embs = [m.query_emb(args[0], args[1]), m.body_emb(args[2], args[3]), m.body_emb(args[4], args[5])]
    got = {n: _np(p.grad) for n, p in m.named_parameters()}
    assert sorted(got) == sorted(want["grads"])
    got["loss"] = float(loss.detach())
    w = dict(want["grads"], loss=want["loss"])
    for i in range(3):
        got["emb%d" % i], w["emb%d" % i] = _np(embs[i]), want["embs"][i]
    bad, worst = S.compare("training step " + which, got, w, ref_err)
    print("training step %s largest d / bound %.3f" % (which, worst))
    assert not bad, bad
    for n, p in m.named_parameters():
        if n.endswith("attention.self.key.bias"):
            assert not p.grad.any(), n
    assert tower_q is not None and tower_c is not None


# ---------------------------------------------------------------------------------------------------------------- 6. precision="half"
@pytest.mark.parametrize("dt", ["fp16", "bf16"])
def test_half_precision_model_under_autocast(dt):
    """RobertaDot_NLL_LN(precision="half"), N = 2, under torch.autocast against the fp32 model outside it, dropout off: the
    embeddings, the loss and every parameter gradient within max(4 x D, 16 ulp32), D = |eager autocast tower - fp32 model| per tensor
    (embeddings_util.embed_torch_forward, layer_half_util.eager_layer and the torch head under the same autocast)."""
    import embeddings_util as E
    import layer_half_util as HL
    import layer_tail_util as LT
    from ance_amd import model
    dtype = torch.float16 if dt == "fp16" else torch.bfloat16
    cfg = ROBERTA_BASE
    sd = M.model_state(cfg)
    calls = S.batches(cfg, 0, BATCH_SEEDS["roberta_base_no_dropout"])
    args = _call_args(calls, cfg["pad"])

    def run(precision, autocast):
        m = _load(model.RobertaDot_NLL_LN(_config(cfg, 0.0), precision=precision), sd).train()
        with torch.autocast("cuda", dtype=dtype, enabled=autocast):
            embs = [m.query_emb(args[0], args[1]), m.body_emb(args[2], args[3]), m.body_emb(args[4], args[5])]
            from ance_amd.loss import nll_loss
            loss = nll_loss(*embs)
        loss.backward()
        out = {n: _np(p.grad) for n, p in m.named_parameters()}
        assert all(p.grad.dtype == torch.float32 for p in m.parameters()) and all(e.dtype == torch.float32 for e in embs)
        out["loss"] = np.float64(float(loss.detach()))
        out.update({"emb%d" % i: _np(e) for i, e in enumerate(embs)})
        return out

    base = run("fp32", False)
    assert _negative_weights([base["emb%d" % i] for i in range(3)]).min() > 0.5
    got = run("half", True)
    W = {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV).requires_grad_(True) for k, v in sd.items()}
    F = torch.nn.functional
    with torch.autocast("cuda", dtype=dtype):
        embs = []
        for c in calls:
            h = E.embed_torch_forward(c["ids"], None, *(W["roberta." + n] for n in S.EMB), cfg["eps"], cfg["mode"], cfg["pad"])
            rows = torch.from_numpy(A._valid(c["lens"], c["ids"].shape[1])).to(DEV)
            for i in range(cfg["N"]):
                pre = "roberta." + S.layer_prefix(i)
                h = HL.eager_layer(h, rows, {n: W[pre + n] for n in LT.LAYER_PARAMS}, cfg["heads"], cfg["eps"])
            e = F.linear(h[:, 0], W["embeddingHead.weight"], W["embeddingHead.bias"])
            embs.append(F.layer_norm(e.float(), (768,), W["norm.weight"], W["norm.bias"], S.HEAD_EPS))
        loss = S.loss_torch("triplet", [e.float() for e in embs])
    loss.backward()
    eager = {k: _np(w.grad) for k, w in W.items()}
    eager["loss"] = np.float64(float(loss.detach()))
    eager.update({"emb%d" % i: _np(e) for i, e in enumerate(embs)})
    def logits(r):
        q, a, b = (np.asarray(r["emb%d" % i], np.float64) for i in range(3))
        return np.stack([(q * a).sum(-1), (q * b).sum(-1)], 1)

    bad, worst = [], 0.0
    for n in sorted(base):
        D = float(np.abs(np.asarray(eager[n], np.float64) - base[n]).max())
        if n == "loss":
            # One scalar: the eager tower's realised loss difference is a single draw, not a scale (measured fp16: 1.2e-3 beside
            # 1.0e-2 here, while each of the 47 tensors has a ratio of 0.4 - 1.3).  Its scale is what its own logit errors can move
            # the loss by: the objective is mean softplus(lb - la), of slope <= 1 in either logit, so |d loss| <= mean(|d la| + |d lb|).
            print("model precision=half %s loss: the eager tower's own |d loss| %.3e" % (dt, D))
            D = float(np.abs(logits(eager) - logits(base)).sum(1).mean())
        d = float(np.abs(np.asarray(got[n], np.float64) - base[n]).max())
        bound = max(4.0 * D, 16.0 * A.ulp32(np.abs(base[n]).max()))
        worst = max(worst, d / bound)
        print("model precision=half %s %-58s |half - fp32| %.3e  D %.3e  ratio %6.2f  bound %.3e%s"
              % (dt, n, d, D, d / D if D > 0 else float("nan"), bound, "" if d <= bound else "  BEYOND ITS BOUND"))
        if not d <= bound:
            bad.append((n, d, D, bound))
    print("model precision=half %s largest d / bound %.3f" % (dt, worst))
    assert not bad, bad


# ---------------------------------------------------------------------------------------------------------------- 7. replay
def _step_inputs(cfg, t):
    return _call_args(S.batches(cfg, t, S.TRIPLET_SEEDS[t % len(S.TRIPLET_SEEDS)]), cfg["pad"])


def _model_and_optimizer(cfg):
    from ance_amd import model, optim
    m = _load(model.RobertaDot_NLL_LN(_config(cfg, 0.1)), M.model_state(cfg)).train()
    named = list(m.named_parameters())
    groups = [dict(params=[q for n, q in named if S.group_of(n.replace("roberta.", "")) == k], lr=U.GROUPS[k]["lr"],
                   weight_decay=U.GROUPS[k]["weight_decay"]) for k in range(len(U.GROUPS))]
    return m, optim.Lamb(groups, lr=1e-3, betas=U.BETAS, eps=U.EPS, max_grad_norm=1.0)


def _snapshot(m, opt):
    return [(q.detach().clone(), opt.state[q]["exp_avg"].clone(), opt.state[q]["exp_avg_sq"].clone()) for q in m.parameters()]


def test_three_replayed_steps_equal_the_eager_host_steps():
    """RobertaDot_NLL_LN + Lamb(max_grad_norm=1.0), N = 2, dropout 0.1, by the capture recipe of INTEGRATION.md: after
    dropout_state.to_device() three replays, fed by copy_, equal three eager host-mode steps in every parameter and both moments, bit
    for bit."""
    from ance_amd import attention as T
    cfg, steps = ROBERTA_BASE, 3
    m, opt = _model_and_optimizer(cfg)
    T.dropout_state.to_host(0)
    T.manual_seed(SEED)
    want = []
    for t in range(steps):
        m(*_step_inputs(cfg, t))[0].backward()
        opt.step()
        want.append(_snapshot(m, opt))
        opt.zero_grad(set_to_none=True)

    m, opt = _model_and_optimizer(cfg)
    T.dropout_state.to_host(0)
    T.manual_seed(SEED)
    T.dropout_state.to_device(0)
    static = _step_inputs(cfg, 0)
    start = [q.detach().clone() for q in m.parameters()]

    def step():
        m(*static)[0].backward()
        opt.step()
        T.dropout_state.advance(0)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
            opt.zero_grad(set_to_none=True)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    with torch.no_grad():   # back to step 0, in place: no pointer the plan or the graph holds changes
        for q, q0 in zip(m.parameters(), start):
            q.copy_(q0)
            st = opt.state[q]
            st["exp_avg"].zero_()
            st["exp_avg_sq"].zero_()
            if isinstance(st.get("step"), torch.Tensor):
                st["step"].zero_()
    T.manual_seed(SEED)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    for t in range(steps):
        for dst, src in zip(static, _step_inputs(cfg, t)):
            dst.copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        got = _snapshot(m, opt)
        for (n, _), a, b in zip(m.named_parameters(), want[t], got):
            for k, (x, y) in enumerate(zip(a, b)):
                assert _bits_equal(x, y), "step %d %s %s: max |d| %.3e" % (t, n, "pmv"[k], float((x.double() - y.double()).abs().max()))
    assert T.dropout_state.to_host(0) == (SEED, steps * 3 * S.draws_per_call(cfg))
    assert not _bits_equal(want[0][0][0], want[1][0][0])


# ---------------------------------------------------------------------------------------------------------------- 8. hand-off
def test_encoder_builds_from_the_models_state_dict(golden_dir):
    """The refresh side: Encoder(model.reference_state_dict(), precision="fp32") with no renaming, against model.eval() on the same
    ids: 4e-5, both being held to the reference within 2e-5."""
    from ance_amd.encoder import ARCH_ROBERTA, Encoder
    _, g, m, _ = _nll_models(golden_dir)
    enc = Encoder(m.reference_state_dict(), ARCH_ROBERTA, "roberta.", True, max_seq_len=64, max_tokens=2048, device=DEV, precision="fp32")
    ids, mask = _ids(g["f_a_ids"]), _mask(g["f_a_len"], 64)
    with torch.no_grad():
        want = _np(m.body_emb(ids, mask))
    got = _np(enc.embed(ids, mask))
    d = float(np.abs(got - want).max())
    print("hand-off max|d| %.3e" % d)
    assert got.shape == want.shape and d <= 4e-5, d
