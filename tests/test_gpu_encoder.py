"""Parity of the HIP dual encoder (through the C ABI) with the fp32 oracle and with golden vectors
of the real reference, in its three arithmetic modes.  Stated tolerances on unit-variance embeddings:
  split (the library's DEFAULT: fp16 pair operands, fp32-grade)   max |delta| <= 2e-5
  fp32  (ANCE_ENCODER_PRECISE=1, the audit path)                 max |delta| <= 2e-5
  fp16  (ANCE_ENCODER_FP16=1, the fast mode: fp16 MFMA operands, fp32 accumulation, fp16-pair residual stream)
        max |delta| <= 5e-3 and cosine >= 0.99999 per row (measured: 3.0e-3 / 0.9999997 at 12 layers; what
        that tolerance means for retrieval is measured by tests/test_gpu_retrieval.py).
The edge-case tests (interior pad ids, many short queries across micro-batches, L = 512, the 2-layer golden, the raw-record and
micro-batch identities, the random batches) run in all three modes, each at its stated tolerance, selected with ``precision=``.
The remaining tests that do not select a mode themselves run the fp16 fast mode (module fixture below: its kernels are the ones
with the loosest tolerance and the most A/B switches).  The same modes on trained-like weights at full depth:
tests/test_gpu_encoder_trained.py.  Needs an MI355X."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ABS_TOL = 5e-3
COS_TOL = 0.99999


@pytest.fixture(autouse=True)
def _fp16_fast_mode_unless_selected(monkeypatch):
    """ANCE_ENCODER_FP16=1 for every test of this module; a test that sets ANCE_ENCODER_SPLIT=1 / ANCE_ENCODER_PRECISE=1 (or
    passes precision=) overrides it (csrc/encoder.hip: split_env)."""
    monkeypatch.setenv("ANCE_ENCODER_FP16", "1")

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpurun_out")


def _report(name, got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    diff = np.abs(got - want)
    cos = (got * want).sum(-1) / (np.linalg.norm(got, axis=-1) * np.linalg.norm(want, axis=-1) + 1e-30)
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, "encoder_parity.jsonl"), "a") as f:
        f.write(json.dumps(dict(case=name, max_abs=float(diff.max()), mean_abs=float(diff.mean()),
                                min_cos=float(cos.min()), worst_row=int(diff.reshape(len(diff), -1).max(1).argmax()),
                                nan=bool(np.isnan(got).any()))) + "\n")
    assert not np.isnan(got).any(), name
    assert diff.max() <= ABS_TOL, "%s: max abs %.3e" % (name, diff.max())
    assert cos.min() >= COS_TOL, "%s: min cosine %.6f" % (name, cos.min())


# (mode, max |delta| against the fp32 oracle or a golden of the reference): the stated tolerances above; fp16 also keeps its cosine
MODES = [("split", 2e-5), ("fp32", 2e-5), ("fp16", ABS_TOL)]


def _check(name, mode, tol, got, want):
    """fp16: ``_report`` as before (ABS_TOL and COS_TOL, case name unchanged); split / fp32: finite and max |delta| <= tol."""
    if mode == "fp16":
        assert tol == ABS_TOL
        return _report(name, got, want)
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    diff = np.abs(got - want)
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, "encoder_parity.jsonl"), "a") as f:
        f.write(json.dumps(dict(case="%s_%s" % (name, mode), max_abs=float(diff.max()), mean_abs=float(diff.mean()),
                                worst_row=int(diff.reshape(len(diff), -1).max(1).argmax()), nan=bool(np.isnan(got).any()))) + "\n")
    assert np.isfinite(got).all(), (name, mode)
    assert diff.max() <= tol, "%s %s: max abs %.3e, row %d" % (name, mode, diff.max(), int(diff.reshape(len(diff), -1).max(1).argmax()))


_shared = {}


def _once(key, make):
    """A reference computed once per session and shared by the cases that need it (never modified)."""
    if key not in _shared:
        _shared[key] = make()
    return _shared[key]


def _manifest(golden_dir):
    with open(os.path.join(golden_dir, "manifest.json")) as f:
        return json.load(f)


from golden_util import golden_weights as _weights  # noqa: E402


@pytest.mark.parametrize("mode,tol", MODES)
def test_firstp_golden_of_reference(golden_dir, mode, tol):
    from ance_amd.encoder import ARCH_ROBERTA, AnceModel, Encoder
    sd = _once("firstp_weights", lambda: _weights(_manifest(golden_dir)["encoder"]["firstp"]))
    g = np.load(os.path.join(golden_dir, "encoder_firstp.npz"))
    enc = Encoder(sd, ARCH_ROBERTA, "roberta.", True, max_seq_len=128, max_tokens=4096, precision=mode)
    model = AnceModel("rdot_nll", enc)
    ids = torch.from_numpy(g["ids"]).cuda()
    mask = (torch.arange(ids.shape[1])[None, :] < torch.from_numpy(g["lens"])[:, None]).long().cuda()
    emb = model.module.body_emb(input_ids=ids.long(), attention_mask=mask)
    assert emb.shape == (len(g["lens"]), 768) and emb.dtype == torch.float32
    _check("firstp_golden", mode, tol, emb.cpu().numpy(), g["emb"])
    # query_emb is the same tower (model/models.py:156-157)
    emb_q = model.module.query_emb(input_ids=ids.long(), attention_mask=mask)
    assert torch.equal(emb_q, emb)


def test_maxp_golden_of_reference(golden_dir):
    from ance_amd.encoder import ARCH_ROBERTA, AnceModel, Encoder
    sd = _weights(_manifest(golden_dir)["encoder"]["maxp"])
    g = np.load(os.path.join(golden_dir, "encoder_maxp.npz"))
    enc = Encoder(sd, ARCH_ROBERTA, "roberta.", True, max_seq_len=512, max_tokens=8192)
    model = AnceModel("rdot_nll_multi_chunk", enc, chunks=4)
    ids = torch.from_numpy(g["ids"]).cuda()
    mask = (torch.arange(2048)[None, :] < torch.from_numpy(g["lens"])[:, None]).long().cuda()
    emb = model.module.body_emb(input_ids=ids.long(), attention_mask=mask)
    assert emb.shape == (len(g["lens"]), 4, 768)
    _report("maxp_golden", emb.cpu().numpy().reshape(-1, 768), g["emb"].reshape(-1, 768))
    e = emb.cpu().numpy()
    assert np.array_equal(e[4, 1], e[4, 3]) and np.array_equal(e[4, 1], e[3, 2])  # all-pad chunks: one vector


def test_bert_golden_of_reference(golden_dir):
    from ance_amd.encoder import ARCH_BERT, Encoder
    sd = _weights(_manifest(golden_dir)["encoder"]["bert"], kind="bert", vocab=30522, max_pos=512, head=False,
                  prefixes=("ctx_model.",))
    g = np.load(os.path.join(golden_dir, "encoder_bert.npz"))
    enc = Encoder(sd, ARCH_BERT, "ctx_model.", False, max_seq_len=256, max_tokens=4096)
    ids = torch.from_numpy(g["ids"]).cuda()
    emb = enc.embed(ids, (ids != 0).long())
    _report("bert_golden", emb.cpu().numpy(), g["emb"])


def test_full_depth_against_oracle():
    """12 layers, roberta-base shapes, random init with perturbed LayerNorm/bias parameters,
    variable lengths incl. 1, L, and lengths straddling the 32/64/128 tile edges."""
    from ance_amd.encoder import ARCH_ROBERTA, Encoder
    from oracle import encoder_ref, synth
    sd = encoder_ref.random_state_dict(seed=5, n_layers=12, ln_jitter=0.1)
    rng = np.random.default_rng(8)
    L = 128
    lens = np.array([1, 2, 31, 32, 33, 63, 64, 65, 96, 127, 128, 128, 70, 9, 100, 50, 77, 128, 3, 45], dtype=np.int32)
    ids = synth.make_records(rng, len(lens), L, lens.astype(np.int64))
    with torch.no_grad():
        want = encoder_ref.rdot_nll_ln_emb(sd, torch.from_numpy(ids), encoder_ref.mask_from_lengths(lens, L)).numpy()
    enc = Encoder(sd, ARCH_ROBERTA, "roberta.", True, max_seq_len=128, max_tokens=2048)
    got = enc.encode_ids(torch.from_numpy(ids).cuda(), torch.from_numpy(lens).cuda(), h_lens=lens)
    _report("full_depth_L128", got.cpu().numpy(), want)

    # raw cache records (big-endian header) give the same rows, with and without host lengths
    rec = np.empty((len(lens), 1 + L), dtype=np.int32)
    rec[:, 0] = lens.astype(">u4").view(np.int32)
    rec[:, 1:] = ids
    rd = torch.from_numpy(rec).cuda()
    a = enc.encode_records(rd, h_lens=lens)
    b = enc.encode_records(rd)
    assert torch.equal(a, got) and torch.equal(b, got)

    # micro-batch boundaries do not change any row (rows are independent)
    enc_small = Encoder(sd, ARCH_ROBERTA, "roberta.", True, max_seq_len=128, max_tokens=512)
    c = enc_small.encode_ids(torch.from_numpy(ids).cuda(), torch.from_numpy(lens).cuda(), h_lens=lens)
    assert torch.equal(c, got)
    del enc, enc_small

    # the same identities in the library's default arithmetic, at its own tolerance against the oracle
    enc = Encoder(sd, ARCH_ROBERTA, "roberta.", True, max_seq_len=128, max_tokens=2048, precision="split")
    got_s = enc.encode_ids(torch.from_numpy(ids).cuda(), torch.from_numpy(lens).cuda(), h_lens=lens)
    _check("full_depth_L128", "split", 2e-5, got_s.cpu().numpy(), want)
    assert torch.equal(enc.encode_records(rd, h_lens=lens), got_s) and torch.equal(enc.encode_records(rd), got_s)
    enc_small = Encoder(sd, ARCH_ROBERTA, "roberta.", True, max_seq_len=128, max_tokens=512, precision="split")
    assert torch.equal(enc_small.encode_ids(torch.from_numpy(ids).cuda(), torch.from_numpy(lens).cuda(), h_lens=lens), got_s)


def _oracle(sd, ids, lens, L, n_layers):
    from oracle import encoder_ref
    with torch.no_grad():
        return encoder_ref.rdot_nll_ln_emb(sd, torch.from_numpy(ids), encoder_ref.mask_from_lengths(lens, L), n_layers=n_layers).numpy()


@pytest.mark.parametrize("mode,tol", MODES)
def test_long_sequences_L512(mode, tol):
    from ance_amd.encoder import ARCH_ROBERTA, Encoder
    from oracle import encoder_ref, synth
    sd = _once("L512_weights", lambda: encoder_ref.random_state_dict(seed=6, n_layers=3, ln_jitter=0.1))
    rng = np.random.default_rng(9)
    lens = np.array([512, 511, 300, 129, 385, 512, 17, 256], dtype=np.int32)
    ids = synth.make_records(rng, len(lens), 512, lens.astype(np.int64))
    want = _once("L512_oracle", lambda: _oracle(sd, ids, lens, 512, 3))
    enc = Encoder(sd, ARCH_ROBERTA, "roberta.", True, max_seq_len=512, max_tokens=2048, precision=mode)
    got = enc.encode_ids(torch.from_numpy(ids).cuda(), torch.from_numpy(lens).cuda(), h_lens=lens)
    _check("L512", mode, tol, got.cpu().numpy(), want)


@pytest.mark.parametrize("mode,tol", MODES)
def test_interior_pad_token_positions(mode, tol):
    """RoBERTa position ids come from cumsum(id != pad), not from the index (modeling_roberta.py:142-155)."""
    from ance_amd.encoder import ARCH_ROBERTA, Encoder
    from oracle import encoder_ref, synth
    sd = _once("interior_pad_weights", lambda: encoder_ref.random_state_dict(seed=7, n_layers=2))
    rng = np.random.default_rng(10)
    lens = np.array([40, 64, 70], dtype=np.int32)
    ids = synth.make_records(rng, 3, 80, lens.astype(np.int64))
    ids[0, 5] = 1
    ids[1, 10:13] = 1
    ids[2, 66] = 1
    want = _once("interior_pad_oracle", lambda: _oracle(sd, ids, lens, 80, 2))
    enc = Encoder(sd, ARCH_ROBERTA, "roberta.", True, max_seq_len=80, max_tokens=1024, precision=mode)
    got = enc.encode_ids(torch.from_numpy(ids).cuda(), torch.from_numpy(lens).cuda(), h_lens=lens)
    _check("interior_pad", mode, tol, got.cpu().numpy(), want)


@pytest.mark.parametrize("mode,tol", MODES)
def test_many_short_queries_cross_micro_batches(mode, tol):
    """Query-shaped input (lengths ~9 of 64): thousands of sequences per micro-batch, several
    micro-batches, against the oracle on a sample of rows."""
    from ance_amd.encoder import ARCH_ROBERTA, Encoder
    from oracle import encoder_ref, synth
    sd = _once("short_queries_weights", lambda: encoder_ref.random_state_dict(seed=8, n_layers=2, ln_jitter=0.05))
    rng = np.random.default_rng(11)
    n = 3000
    lens = synth.lognormal_lengths(rng, n, 9, 0.35, 4, 64).astype(np.int32)
    ids = synth.make_records(rng, n, 64, lens.astype(np.int64))
    enc = Encoder(sd, ARCH_ROBERTA, "roberta.", True, max_seq_len=64, max_tokens=4096, precision=mode)
    got = enc.encode_ids(torch.from_numpy(ids).cuda(), torch.from_numpy(lens).cuda(), h_lens=lens).cpu().numpy()
    pick = np.concatenate([np.arange(0, 40), np.arange(n - 40, n), rng.integers(0, n, 48)])
    want = _once("short_queries_oracle", lambda: _oracle(sd, ids[pick], lens[pick], 64, 2))
    _check("short_queries", mode, tol, got[pick], want)


@pytest.mark.parametrize("precision", ["split", "fp16"])
def test_cls_only_tail_changes_no_bit(monkeypatch, precision):
    """The last layer runs K | V for every token and everything else -- the Q projection (a compact GEMM over the [CLS] rows),
    the attention (one query per sequence), attention-output, FFN -- for the [CLS] rows only.  Dead work of the reference's forward
    (model/models.py:149-157 reads token 0 only), not different arithmetic: against the full last layer (ANCE_CLS_TAIL=0) not one
    bit of an embedding may differ, in either matrix-core mode, with one and with several micro-batches."""
    from ance_amd.encoder import ARCH_ROBERTA, Encoder
    from oracle import encoder_ref, synth
    sd = encoder_ref.random_state_dict(seed=25, n_layers=3, ln_jitter=0.1)
    rng = np.random.default_rng(28)
    lens = np.concatenate([np.array([1, 2, 31, 32, 33, 64, 65, 96, 97, 128], dtype=np.int32), rng.integers(3, 129, 390).astype(np.int32)])
    ids = synth.make_records(rng, len(lens), 128, lens.astype(np.int64))

    def run(max_tokens):
        enc = Encoder(sd, ARCH_ROBERTA, "roberta.", True, max_seq_len=128, max_tokens=max_tokens, precision=precision)
        return enc.encode_ids(torch.from_numpy(ids).cuda(), torch.from_numpy(lens).cuda(), h_lens=lens)

    tail, tail_small = run(65536), run(4096)
    monkeypatch.setenv("ANCE_CLS_TAIL", "0")
    full = run(65536)
    assert torch.isfinite(tail).all()
    assert torch.equal(tail, full)
    assert torch.equal(tail_small, full)


@pytest.mark.parametrize("switch", ["ANCE_CLS_TAIL", "ANCE_ENCODER_STREAMS"])
def test_ab_switches_keep_parity(monkeypatch, switch):
    """The A/B switches of include/ance_amd.h select the previous form of one piece each (full last layer, one internal
    stream).  They are what the same-box A/B numbers of DESIGN.md are measured with, so they must stay inside the stated
    tolerance -- and rows must not depend on the micro-batch split under any of them."""
    from ance_amd.encoder import ARCH_ROBERTA, Encoder
    from oracle import encoder_ref, synth
    monkeypatch.setenv(switch, "1" if switch == "ANCE_ENCODER_STREAMS" else "0")
    sd = encoder_ref.random_state_dict(seed=15, n_layers=4, ln_jitter=0.1)
    rng = np.random.default_rng(18)
    lens = np.array([1, 2, 31, 32, 33, 64, 65, 96, 97, 128, 70, 9, 100, 50, 77, 128, 3, 45, 120, 12], dtype=np.int32)
    ids = synth.make_records(rng, len(lens), 128, lens.astype(np.int64))
    with torch.no_grad():
        want = encoder_ref.rdot_nll_ln_emb(sd, torch.from_numpy(ids), encoder_ref.mask_from_lengths(lens, 128), n_layers=4).numpy()
    enc = Encoder(sd, ARCH_ROBERTA, "roberta.", True, max_seq_len=128, max_tokens=2048)
    got = enc.encode_ids(torch.from_numpy(ids).cuda(), torch.from_numpy(lens).cuda(), h_lens=lens)
    _report("switch_%s" % switch, got.cpu().numpy(), want)
    enc_small = Encoder(sd, ARCH_ROBERTA, "roberta.", True, max_seq_len=128, max_tokens=512)
    assert torch.equal(enc_small.encode_ids(torch.from_numpy(ids).cuda(), torch.from_numpy(lens).cuda(), h_lens=lens), got)


def test_fp32_mode_against_oracle(monkeypatch):
    """ANCE_ENCODER_PRECISE=1 (csrc/precise32.h): fp32 operands on the fp32-input matrix cores, exact erf GELU, fp32
    softmax -- the reference's arithmetic (model/models.py:149-157).  Against the fp32 oracle only the summation order
    differs: stated tolerance 2e-5 on unit-variance rows (12 layers, L = 128; 3 layers, L = 512)."""
    from ance_amd.encoder import ARCH_ROBERTA, Encoder
    from oracle import encoder_ref, synth
    monkeypatch.setenv("ANCE_ENCODER_PRECISE", "1")
    sd = encoder_ref.random_state_dict(seed=5, n_layers=12, ln_jitter=0.1)
    rng = np.random.default_rng(8)
    lens = np.array([1, 2, 31, 32, 33, 63, 64, 65, 96, 127, 128, 128, 70, 9, 100, 50, 77, 128, 3, 45], dtype=np.int32)
    ids = synth.make_records(rng, len(lens), 128, lens.astype(np.int64))
    with torch.no_grad():
        want = encoder_ref.rdot_nll_ln_emb(sd, torch.from_numpy(ids), encoder_ref.mask_from_lengths(lens, 128)).numpy()
    enc = Encoder(sd, ARCH_ROBERTA, "roberta.", True, max_seq_len=128, max_tokens=2048)
    got = enc.encode_ids(torch.from_numpy(ids).cuda(), torch.from_numpy(lens).cuda(), h_lens=lens).cpu().numpy()
    assert np.isfinite(got).all()
    d = float(np.abs(got - want).max())
    with open(os.path.join(OUT, "encoder_parity.jsonl"), "a") as f:
        f.write(json.dumps(dict(case="fp32_mode_full_depth_L128", max_abs=d)) + "\n")
    assert d <= 2e-5, d
    del enc
    sd3 = encoder_ref.random_state_dict(seed=6, n_layers=3, ln_jitter=0.1)
    lens5 = np.array([512, 511, 300, 129, 385, 512, 17, 256], dtype=np.int32)
    ids5 = synth.make_records(np.random.default_rng(9), len(lens5), 512, lens5.astype(np.int64))
    with torch.no_grad():
        want5 = encoder_ref.rdot_nll_ln_emb(sd3, torch.from_numpy(ids5), encoder_ref.mask_from_lengths(lens5, 512), n_layers=3).numpy()
    enc = Encoder(sd3, ARCH_ROBERTA, "roberta.", True, max_seq_len=512, max_tokens=2048)
    got5 = enc.encode_ids(torch.from_numpy(ids5).cuda(), torch.from_numpy(lens5).cuda(), h_lens=lens5).cpu().numpy()
    d5 = float(np.abs(got5 - want5).max())
    with open(os.path.join(OUT, "encoder_parity.jsonl"), "a") as f:
        f.write(json.dumps(dict(case="fp32_mode_L512", max_abs=d5)) + "\n")
    assert d5 <= 2e-5, d5


def test_fp32_mode_bert_and_maxp_goldens(monkeypatch, golden_dir):
    """The fp32 mode on the other two model families, against golden vectors of the REFERENCE's own classes
    (HFBertEncoder raw [CLS] without a head; RobertaDot_CLF_ANN_NLL_MultiChunk with all-pad chunks): 2e-5."""
    from ance_amd.encoder import ARCH_BERT, ARCH_ROBERTA, AnceModel, Encoder
    monkeypatch.setenv("ANCE_ENCODER_PRECISE", "1")
    sd = _weights(_manifest(golden_dir)["encoder"]["bert"], kind="bert", vocab=30522, max_pos=512, head=False, prefixes=("ctx_model.",))
    g = np.load(os.path.join(golden_dir, "encoder_bert.npz"))
    enc = Encoder(sd, ARCH_BERT, "ctx_model.", False, max_seq_len=256, max_tokens=4096)
    ids = torch.from_numpy(g["ids"]).cuda()
    emb = enc.embed(ids, (ids != 0).long()).cpu().numpy()
    assert np.abs(emb - g["emb"]).max() <= 2e-5, np.abs(emb - g["emb"]).max()
    del enc
    sd = _weights(_manifest(golden_dir)["encoder"]["maxp"])
    g = np.load(os.path.join(golden_dir, "encoder_maxp.npz"))
    enc = Encoder(sd, ARCH_ROBERTA, "roberta.", True, max_seq_len=512, max_tokens=8192)
    model = AnceModel("rdot_nll_multi_chunk", enc, chunks=4)
    ids = torch.from_numpy(g["ids"]).cuda()
    mask = (torch.arange(2048)[None, :] < torch.from_numpy(g["lens"])[:, None]).long().cuda()
    e = model.module.body_emb(input_ids=ids.long(), attention_mask=mask).cpu().numpy()
    assert np.abs(e - g["emb"]).max() <= 2e-5, np.abs(e - g["emb"]).max()
    assert np.array_equal(e[4, 1], e[4, 3]) and np.array_equal(e[4, 1], e[3, 2])  # all-pad chunks: one vector


def _encode(sd, ids, lens, L, max_tokens=2048, arch=None):
    from ance_amd.encoder import ARCH_ROBERTA, Encoder
    enc = Encoder(sd, ARCH_ROBERTA, "roberta.", True, max_seq_len=L, max_tokens=max_tokens)
    return enc.encode_ids(torch.from_numpy(ids).cuda(), torch.from_numpy(lens).cuda(), h_lens=lens).cpu().numpy()


@pytest.mark.parametrize("mode,tol", [("fp16", ABS_TOL), ("split", 2e-5), ("fp32", 2e-5)])
def test_full_depth_golden_of_reference(monkeypatch, golden_dir, mode, tol):
    """12 layers against RobertaDot_NLL_LN.body_emb ITSELF (model/models.py:149-157; tests/golden/encoder_firstp12.npz) -- the
    depth every headline number is quoted at -- in the three arithmetic modes of the library, each at its stated tolerance."""
    if mode == "split":
        monkeypatch.setenv("ANCE_ENCODER_SPLIT", "1")
    if mode == "fp32":
        monkeypatch.setenv("ANCE_ENCODER_PRECISE", "1")
    sd = _weights(_manifest(golden_dir)["encoder"]["firstp12"])
    g = np.load(os.path.join(golden_dir, "encoder_firstp12.npz"))
    got = _encode(sd, g["ids"], g["lens"], 128)
    d = float(np.abs(got - g["emb"]).max())
    with open(os.path.join(OUT, "encoder_parity.jsonl"), "a") as f:
        f.write(json.dumps(dict(case="firstp12_golden_%s" % mode, max_abs=d)) + "\n")
    assert np.isfinite(got).all() and d <= tol, d


@pytest.mark.parametrize("mode,tol", [("fp16", ABS_TOL), ("split", 2e-5), ("fp32", 2e-5)])
def test_full_depth_goldens_of_the_other_towers(golden_dir, mode, tol):
    """12 layers against the reference's OWN classes for configs 3-5 (tests/golden/make_golden.py: golden_encoder12):
    RobertaDot_CLF_ANN_NLL_MultiChunk.body_emb on documents straddling the 512-token chunk borders with all-pad chunks behind
    them (model/models.py:165-199), HFBertEncoder at L = 256 (:223-244), RobertaDot_NLL_LN.body_emb at seq_len 512 with lengths
    at the 256-key borders of the long-sequence attention path (:149-157) -- each arithmetic mode at its stated tolerance."""
    from ance_amd.encoder import ARCH_BERT, ARCH_ROBERTA, AnceModel, Encoder
    man = _manifest(golden_dir)["encoder12"]
    rec = {}
    g = np.load(os.path.join(golden_dir, "encoder_maxp12.npz"))
    enc = Encoder(_weights(man["maxp12"]), ARCH_ROBERTA, "roberta.", True, max_seq_len=512, max_tokens=8192, precision=mode)
    model = AnceModel("rdot_nll_multi_chunk", enc, chunks=4)
    ids = torch.from_numpy(g["ids"]).cuda()
    mask = (torch.arange(2048)[None, :] < torch.from_numpy(g["lens"])[:, None]).long().cuda()
    e = model.module.body_emb(input_ids=ids.long(), attention_mask=mask).cpu().numpy()
    rec["maxp12"] = float(np.abs(e - g["emb"]).max())
    assert np.array_equal(e[1, 3], e[2, 2]) and np.array_equal(e[1, 3], e[5, 1])  # all-pad chunks: one vector
    del enc, model
    g = np.load(os.path.join(golden_dir, "encoder_bert12.npz"))
    enc = Encoder(_weights(man["bert12"], kind="bert", vocab=30522, max_pos=512, head=False, prefixes=("ctx_model.",)), ARCH_BERT,
                  "ctx_model.", False, max_seq_len=256, max_tokens=4096, precision=mode)
    ids = torch.from_numpy(g["ids"]).cuda()
    rec["bert12"] = float(np.abs(enc.embed(ids, (ids != 0).long()).cpu().numpy() - g["emb"]).max())
    del enc
    g = np.load(os.path.join(golden_dir, "encoder_firstp12_L512.npz"))
    enc = Encoder(_weights(man["firstp12_L512"]), ARCH_ROBERTA, "roberta.", True, max_seq_len=512, max_tokens=2048, precision=mode)
    got = enc.encode_ids(torch.from_numpy(g["ids"]).cuda(), torch.from_numpy(g["lens"]).cuda(), h_lens=g["lens"]).cpu().numpy()
    rec["firstp12_L512"] = float(np.abs(got - g["emb"]).max())
    with open(os.path.join(OUT, "encoder_parity.jsonl"), "a") as f:
        f.write(json.dumps(dict(case="golden12_other_towers_%s" % mode, **rec)) + "\n")
    assert all(np.isfinite(v) and v <= tol for v in rec.values()), rec


def test_split_mode_against_oracle(monkeypatch):
    """ANCE_ENCODER_SPLIT=1: fp16-pair operands, three MFMA passes per product, fp32 softmax, exact erf GELU.  Stated
    tolerance 2e-5 on unit-variance rows against the fp32 oracle (12 layers, L = 128; 3 layers, L = 512; rows independent
    of the micro-batch split; CLS-only tail on and off)."""
    from ance_amd.encoder import ARCH_ROBERTA, Encoder
    from oracle import encoder_ref, synth
    monkeypatch.setenv("ANCE_ENCODER_SPLIT", "1")
    sd = encoder_ref.random_state_dict(seed=5, n_layers=12, ln_jitter=0.1)
    rng = np.random.default_rng(8)
    lens = np.array([1, 2, 31, 32, 33, 63, 64, 65, 96, 127, 128, 128, 70, 9, 100, 50, 77, 128, 3, 45], dtype=np.int32)
    ids = synth.make_records(rng, len(lens), 128, lens.astype(np.int64))
    with torch.no_grad():
        want = encoder_ref.rdot_nll_ln_emb(sd, torch.from_numpy(ids), encoder_ref.mask_from_lengths(lens, 128)).numpy()
    got = _encode(sd, ids, lens, 128)
    assert np.isfinite(got).all()
    d = float(np.abs(got - want).max())
    with open(os.path.join(OUT, "encoder_parity.jsonl"), "a") as f:
        f.write(json.dumps(dict(case="split_mode_full_depth_L128", max_abs=d)) + "\n")
    assert d <= 2e-5, d
    assert np.array_equal(_encode(sd, ids, lens, 128, max_tokens=512), got)   # micro-batch boundaries change no row
    monkeypatch.setenv("ANCE_CLS_TAIL", "0")
    full_last_layer = _encode(sd, ids, lens, 128)
    monkeypatch.delenv("ANCE_CLS_TAIL")
    d_tail = float(np.abs(full_last_layer - want).max())
    assert d_tail <= 2e-5, d_tail
    # the CLS-only tail (K | V of every token, Q / attention-output / FFN of the [CLS] rows only, projected from compact rows) is the
    # same arithmetic per element as the full last layer: not one bit may differ
    assert np.array_equal(full_last_layer, got)
    sd3 = encoder_ref.random_state_dict(seed=6, n_layers=3, ln_jitter=0.1)
    lens5 = np.array([512, 511, 300, 129, 385, 512, 17, 256], dtype=np.int32)
    ids5 = synth.make_records(np.random.default_rng(9), len(lens5), 512, lens5.astype(np.int64))
    with torch.no_grad():
        want5 = encoder_ref.rdot_nll_ln_emb(sd3, torch.from_numpy(ids5), encoder_ref.mask_from_lengths(lens5, 512), n_layers=3).numpy()
    d5 = float(np.abs(_encode(sd3, ids5, lens5, 512) - want5).max())
    with open(os.path.join(OUT, "encoder_parity.jsonl"), "a") as f:
        f.write(json.dumps(dict(case="split_mode_L512", max_abs=d5)) + "\n")
    assert d5 <= 2e-5, d5


def test_split_mode_bert_and_maxp_goldens(monkeypatch, golden_dir):
    """The split mode on the other two model families, against golden vectors of the REFERENCE's own classes."""
    from ance_amd.encoder import ARCH_BERT, ARCH_ROBERTA, AnceModel, Encoder
    monkeypatch.setenv("ANCE_ENCODER_SPLIT", "1")
    sd = _weights(_manifest(golden_dir)["encoder"]["bert"], kind="bert", vocab=30522, max_pos=512, head=False, prefixes=("ctx_model.",))
    g = np.load(os.path.join(golden_dir, "encoder_bert.npz"))
    enc = Encoder(sd, ARCH_BERT, "ctx_model.", False, max_seq_len=256, max_tokens=4096)
    ids = torch.from_numpy(g["ids"]).cuda()
    emb = enc.embed(ids, (ids != 0).long()).cpu().numpy()
    assert np.abs(emb - g["emb"]).max() <= 2e-5, np.abs(emb - g["emb"]).max()
    del enc
    sd = _weights(_manifest(golden_dir)["encoder"]["maxp"])
    g = np.load(os.path.join(golden_dir, "encoder_maxp.npz"))
    enc = Encoder(sd, ARCH_ROBERTA, "roberta.", True, max_seq_len=512, max_tokens=8192)
    model = AnceModel("rdot_nll_multi_chunk", enc, chunks=4)
    ids = torch.from_numpy(g["ids"]).cuda()
    mask = (torch.arange(2048)[None, :] < torch.from_numpy(g["lens"])[:, None]).long().cuda()
    e = model.module.body_emb(input_ids=ids.long(), attention_mask=mask).cpu().numpy()
    assert np.abs(e - g["emb"]).max() <= 2e-5, np.abs(e - g["emb"]).max()
    assert np.array_equal(e[4, 1], e[4, 3]) and np.array_equal(e[4, 1], e[3, 2])  # all-pad chunks: one vector


def _offset_weights(sd, offset, n_layers):
    """A common offset of `offset` STANDARD DEVIATIONS on every pre-LayerNorm row: the embeddings (row std 0.035 at init, at
    either width) and the dense biases of both residual branches (row std ~ 1) -- |mean| >> std, the input distribution ADVICE r3
    showed the single-fp16 LayerNorm fold loses 20-80 x on."""
    sd = dict(sd)
    sd["roberta.embeddings.word_embeddings.weight"] = sd["roberta.embeddings.word_embeddings.weight"] + offset * 0.035
    for i in range(n_layers):
        for n in ("attention.output.dense.bias", "output.dense.bias"):
            k = "roberta.encoder.layer.%d.%s" % (i, n)
            sd[k] = sd[k] + offset
    return sd


@pytest.mark.parametrize("offset", [5.0, 30.0])
def test_rows_with_a_large_mean_keep_the_fp16_tolerance(offset):
    """Default mode on rows whose mean is 5 / 30 standard deviations away from 0: the folded GEMM tiles detect it
    (|mean| rstd > 2) and add the K loop over the lo halves of the token operand, so the stated 5e-3 holds on pretrained-like
    inputs too, not only on the zero-mean rows of a random init (CPU model of both behaviours: tests/test_ln_fold_model.py)."""
    from oracle import encoder_ref, synth
    n_layers = 4
    sd = _offset_weights(encoder_ref.random_state_dict(seed=5, n_layers=n_layers, ln_jitter=0.1), offset, n_layers)
    rng = np.random.default_rng(8)
    lens = np.array([1, 2, 31, 33, 64, 65, 96, 128, 70, 9, 100, 50], dtype=np.int32)
    ids = synth.make_records(rng, len(lens), 128, lens.astype(np.int64))
    with torch.no_grad():
        sd64 = {k: v.double() for k, v in sd.items()}
        want = encoder_ref.rdot_nll_ln_emb(sd64, torch.from_numpy(ids), encoder_ref.mask_from_lengths(lens, 128), n_layers=n_layers).float().numpy()
    _report("large_mean_offset_%g" % offset, _encode(sd, ids, lens, 128), want)


def test_fp16_rows_do_not_depend_on_their_tile_mates():
    """fp16 fast mode, a MIX of wide-mean and ordinary tokens inside the same 256-token GEMM tiles: the tokens of
    half of the sequences come from a part of the vocabulary whose embeddings sit 8 standard deviations off zero, so in layer 0
    the Q | K and V^T GEMM tiles hold both kinds and run their second K loop over the lo halves.  That pass is masked per row,
    so a row's bits depend on the row alone: the same sequence must come out bit-identical whatever the micro-batch split and
    whatever its neighbours (the batch in reverse order), and everything stays inside the mode's tolerance."""
    from ance_amd.encoder import ARCH_ROBERTA, Encoder
    from oracle import encoder_ref, synth
    n_layers = 3
    sd = dict(encoder_ref.random_state_dict(seed=21, n_layers=n_layers, ln_jitter=0.1))
    we = sd["roberta.embeddings.word_embeddings.weight"].clone()
    we[30000:] += 8 * 0.035
    sd["roberta.embeddings.word_embeddings.weight"] = we
    rng = np.random.default_rng(22)
    n = 96
    lens = rng.integers(1, 129, size=n).astype(np.int32)
    ids = synth.make_records(rng, n, 128, lens.astype(np.int64))
    wide_seq = (np.arange(n) % 2) == 1
    ids[wide_seq] = np.where(ids[wide_seq] > 3, 30000 + ids[wide_seq] % 20000, ids[wide_seq])   # keep <s>, </s>, pad as they are
    ids[~wide_seq] = np.where(ids[~wide_seq] >= 30000, ids[~wide_seq] - 25000, ids[~wide_seq])
    with torch.no_grad():
        sd64 = {k: v.double() for k, v in sd.items()}
        want = encoder_ref.rdot_nll_ln_emb(sd64, torch.from_numpy(ids), encoder_ref.mask_from_lengths(lens, 128), n_layers=n_layers).float().numpy()
    got = _encode(sd, ids, lens, 128, max_tokens=2048)
    _report("mixed_wide_and_ordinary_rows", got, want)
    assert np.array_equal(_encode(sd, ids, lens, 128, max_tokens=512), got)
    assert np.array_equal(_encode(sd, ids, lens, 128, max_tokens=1024), got)
    rev = np.arange(n)[::-1].copy()
    assert np.array_equal(_encode(sd, ids[rev].copy(), lens[rev].copy(), 128, max_tokens=768)[rev], got)


RANDOM_BATCHES = [(128, 900, 4096, 1), (64, 2000, 2048, 2), (512, 60, 4096, 3), (32, 1500, 512, 4)]


def _random_batch(L, n, max_tokens, seed):
    """(weights, ids, lens, rows of the fp32 mode on the device): made once per case and shared by the modes compared with it."""
    def make():
        from ance_amd.encoder import ARCH_ROBERTA, Encoder
        from oracle import encoder_ref, synth
        sd = encoder_ref.random_state_dict(seed=30 + seed, n_layers=3, ln_jitter=0.1)
        rng = np.random.default_rng(100 + seed)
        lens = rng.integers(1, L + 1, size=n).astype(np.int32)
        lens[:8] = [1, 1, L, L, 2, L - 1, 33 % L + 1, 1]
        ids = synth.make_records(rng, n, L, lens.astype(np.int64))
        enc32 = Encoder(sd, ARCH_ROBERTA, "roberta.", True, max_seq_len=L, max_tokens=max_tokens, precision="fp32")
        b = enc32.encode_ids(torch.from_numpy(ids).cuda(), torch.from_numpy(lens).cuda(), h_lens=lens)
        enc32.check_range(sync=True)
        assert torch.isfinite(b).all()
        return sd, ids, lens, b
    return _once(("random_batch", L, n, max_tokens, seed), make)


def _random_batch_against_fp32_mode(mode, bound, L, n, max_tokens, seed):
    from ance_amd.encoder import ARCH_ROBERTA, Encoder
    sd, ids, lens, b = _random_batch(L, n, max_tokens, seed)
    enc = Encoder(sd, ARCH_ROBERTA, "roberta.", True, max_seq_len=L, max_tokens=max_tokens, precision=mode)
    assert enc.precision == mode
    a = enc.encode_ids(torch.from_numpy(ids).cuda(), torch.from_numpy(lens).cuda(), h_lens=lens)
    assert torch.isfinite(a).all()
    d = (a - b).abs().max(dim=1).values
    worst = int(d.argmax())
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, "encoder_parity.jsonl"), "a") as f:
        f.write(json.dumps(dict(case="random_batches_%s_vs_fp32_mode_L%d_n%d" % (mode, L, n), max_abs=float(d.max()), worst_row=worst,
                                worst_len=int(lens[worst]))) + "\n")
    print("random batches %s vs fp32 mode, L %d n %d: max |delta| %.3e (row %d, length %d)" % (mode, L, n, float(d.max()), worst, int(lens[worst])))
    assert float(d.max()) <= bound, (float(d.max()), worst, int(lens[worst]))
    # identical inputs -> identical rows, wherever they sit in the batch
    same = np.flatnonzero((lens == 1))
    if len(same) > 1:
        first = ids[same[0], 0]
        twins = [int(r) for r in same if ids[r, 0] == first]
        assert len(twins) > 1 and all(torch.equal(a[twins[0]], a[r]) for r in twins)


@pytest.mark.parametrize("L,n,max_tokens,seed", RANDOM_BATCHES)
def test_random_batches_fp16_against_fp32_mode(L, n, max_tokens, seed):
    """Random lengths (uniform 1..L: many one-token sequences, every tile edge), batches that cross many micro-batch
    boundaries, both kinds of tail (more than 256 [CLS] rows in a micro-batch / fewer): the fp16 mode against the fp32
    mode of the same library on the same records -- two independent implementations of every kernel (fp16 MFMA + folded
    LayerNorm + LDS attention vs fp32 MFMA + LayerNorm kernels + vector-unit attention) must agree within the stated
    tolerance on every row."""
    _random_batch_against_fp32_mode("fp16", ABS_TOL, L, n, max_tokens, seed)


@pytest.mark.parametrize("L,n,max_tokens,seed", RANDOM_BATCHES)
def test_random_batches_split_against_fp32_mode(L, n, max_tokens, seed):
    """The same batches in the library's DEFAULT arithmetic: the split mode (fp16 pair operands, three MFMA passes, its own
    planner / pack / embed / CLS-tail launches) against the fp32 mode.  Each is stated to be within 2e-5 of the fp32 oracle on
    these 3-layer unit-variance rows, so the two are at most 4e-5 apart -- a bound 125 x tighter than the fp16 mode's, at which
    a position-id, packing or tail fault of one row shows."""
    _random_batch_against_fp32_mode("split", 4e-5, L, n, max_tokens, seed)


def test_missing_extension_is_loud(monkeypatch, tmp_path):
    from ance_amd import _lib
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", str(tmp_path / "nope.so"))
    from ance_amd.index import FlatIPIndex
    idx = FlatIPIndex(768)
    idx.add(np.ones((4, 768), np.float32))
    with pytest.raises(_lib.AnceLibraryError):
        idx.search(np.ones((1, 768), np.float32), 2)


def test_library_default_is_the_split_mode(monkeypatch):
    """No mode in the environment -> the split (fp32-grade) arithmetic: the reference runs its encoder in fp32
    (drivers/run_ann_data_gen.py:158,176-180), so the parity-grade mode is what a caller gets without asking."""
    from ance_amd.encoder import ARCH_ROBERTA, Encoder
    from oracle import encoder_ref, synth
    for k in ("ANCE_ENCODER_FP16", "ANCE_ENCODER_SPLIT", "ANCE_ENCODER_PRECISE"):
        monkeypatch.delenv(k, raising=False)
    sd = encoder_ref.random_state_dict(seed=5, n_layers=2, ln_jitter=0.1)
    rng = np.random.default_rng(8)
    lens = np.array([1, 17, 64, 128, 100, 33, 5, 96], dtype=np.int32)
    ids = synth.make_records(rng, len(lens), 128, lens.astype(np.int64))
    with torch.no_grad():
        want = encoder_ref.rdot_nll_ln_emb(sd, torch.from_numpy(ids), encoder_ref.mask_from_lengths(lens, 128), n_layers=2).numpy()
    enc = Encoder(sd, ARCH_ROBERTA, "roberta.", True, max_seq_len=128, max_tokens=2048)
    assert enc.precision == "split"
    got = enc.encode_ids(torch.from_numpy(ids).cuda(), torch.from_numpy(lens).cuda(), h_lens=lens).cpu().numpy()
    assert float(np.abs(got - want).max()) <= 2e-5
    fast = Encoder(sd, ARCH_ROBERTA, "roberta.", True, max_seq_len=128, max_tokens=2048, precision="fp16")
    assert fast.precision == "fp16"
    got16 = fast.encode_ids(torch.from_numpy(ids).cuda(), torch.from_numpy(lens).cuda(), h_lens=lens).cpu().numpy()
    assert 2e-5 < float(np.abs(got16 - want).max()) <= ABS_TOL


def test_re_encoding_into_a_searched_buffer_rebuilds_the_search_image():
    """``encode_ids(out=...)`` writes through a raw pointer.  It bumps the tensor's version counter, which is what
    FlatIPIndex keys its fp16 search image on: a second encode into a buffer that was already searched must be searched on ITS
    rows (a stale image would filter on the old fp16 rows and silently drop true neighbours)."""
    from ance_amd.encoder import ARCH_ROBERTA, Encoder
    from ance_amd.index import FlatIPIndex
    from oracle import encoder_ref, synth
    sd = encoder_ref.random_state_dict(seed=40, n_layers=1, ln_jitter=0.1)
    enc = Encoder(sd, ARCH_ROBERTA, "roberta.", True, max_seq_len=16, max_tokens=16384)
    rng = np.random.default_rng(41)
    n = 5000  # >= 4096 rows: the two-precision path with a search image
    out = torch.empty((n, 768), device="cuda")
    idx = FlatIPIndex(768)
    idx.add(out)
    results = []
    for round_ in range(2):
        lens = rng.integers(2, 17, size=n).astype(np.int32)
        ids = synth.make_records(rng, n, 16, lens.astype(np.int64))
        enc.encode_ids(torch.from_numpy(ids).cuda(), torch.from_numpy(lens).cuda(), h_lens=lens, out=out)
        q = out[rng.integers(0, n, 64)].clone()
        D, I = idx.search_device(q, 50)
        fresh = FlatIPIndex(768)
        fresh.add(out.clone())
        Df, If = fresh.search_device(q, 50)
        assert torch.equal(I, If) and torch.equal(D, Df), "round %d: stale search image" % round_
        results.append(I.clone())
    assert not torch.equal(results[0], results[1])


def test_large_micro_batches_change_no_row():
    """The job's default micro-batch is 131,072 tokens (ance_amd.ann_data_gen --max_tokens): 160 k tokens through two such
    micro-batches give bit for bit the rows that ten 16,384-token micro-batches give, in the default (split) arithmetic and in the
    fp16 fast mode -- operand matrices of 1.6 GB per GEMM stay below the 4 GiB of a buffer descriptor, token offsets below 2^31."""
    from ance_amd.encoder import ARCH_ROBERTA, Encoder
    from oracle import encoder_ref, synth
    sd = encoder_ref.random_state_dict(seed=50, n_layers=2, ln_jitter=0.1)
    rng = np.random.default_rng(51)
    n = 2200
    lens = synth.lognormal_lengths(rng, n, 70, 0.45, 8, 128).astype(np.int32)
    ids = synth.make_records(rng, n, 128, lens.astype(np.int64))
    assert 140_000 < int(lens.sum()) < 2 * 131072
    ids_d, lens_d = torch.from_numpy(ids).cuda(), torch.from_numpy(lens).cuda()
    for mode in ("split", "fp16"):
        big = Encoder(sd, ARCH_ROBERTA, "roberta.", True, max_seq_len=128, max_tokens=131072, precision=mode)
        a = big.encode_ids(ids_d, lens_d, h_lens=lens)
        del big
        small = Encoder(sd, ARCH_ROBERTA, "roberta.", True, max_seq_len=128, max_tokens=16384, precision=mode)
        b = small.encode_ids(ids_d, lens_d, h_lens=lens)
        del small
        assert torch.isfinite(a).all() and torch.equal(a, b), mode


def test_split_mode_with_weights_of_very_different_scales():
    """The split GEMM stores every weight matrix times its own power of two (largest element in [2^13, 2^14): csrc/encoder_kernels.h:
    weight_pair_scale) and undoes it in the epilogue.  Random-init weights are all ~0.02, so every other test exercises ONE
    exponent; here the matrices of a 3-layer model are rescaled by factors between 2^-7 and 2^9 (Q / K / V by different ones: they
    share a scale slot; one matrix gets a single huge outlier), and the result must stay fp32-grade: within 4 x the distance of the
    fp32 oracle from the fp64 oracle (+ the stated 2e-5)."""
    from oracle import encoder_ref, synth
    n_layers = 3
    sd = dict(encoder_ref.random_state_dict(seed=61, n_layers=n_layers, ln_jitter=0.1))
    factors = {"attention.self.query": 6.0, "attention.self.key": 1.0 / 6.0, "attention.self.value": 37.0, "attention.output.dense": 1.0 / 40.0,
               "intermediate.dense": 300.0, "output.dense": 1.0 / 120.0}
    for i in range(n_layers):
        for name, f in factors.items():
            k = "roberta.encoder.layer.%d.%s.weight" % (i, name)
            sd[k] = sd[k] * (f if i != 1 else 1.0 / f)       # the middle layer the other way round
    w = sd["roberta.encoder.layer.2.output.dense.weight"].clone()
    w[5, 77] = 9.0                                            # one outlier 50,000 x the typical element of that matrix
    sd["roberta.encoder.layer.2.output.dense.weight"] = w
    rng = np.random.default_rng(62)
    lens = np.array([1, 2, 31, 33, 64, 65, 96, 128, 70, 9, 100, 50], dtype=np.int32)
    ids = synth.make_records(rng, len(lens), 128, lens.astype(np.int64))
    with torch.no_grad():
        sd64 = {k: v.double() for k, v in sd.items()}
        want64 = encoder_ref.rdot_nll_ln_emb(sd64, torch.from_numpy(ids), encoder_ref.mask_from_lengths(lens, 128), n_layers=n_layers).numpy()
        want32 = encoder_ref.rdot_nll_ln_emb(sd, torch.from_numpy(ids), encoder_ref.mask_from_lengths(lens, 128), n_layers=n_layers).numpy()
    from ance_amd.encoder import ARCH_ROBERTA, Encoder
    enc = Encoder(sd, ARCH_ROBERTA, "roberta.", True, max_seq_len=128, max_tokens=2048, precision="split")
    got = enc.encode_ids(torch.from_numpy(ids).cuda(), torch.from_numpy(lens).cuda(), h_lens=lens).cpu().numpy()
    e32 = float(np.abs(want32.astype(np.float64) - want64).max())
    e = float(np.abs(got.astype(np.float64) - want64).max())
    with open(os.path.join(OUT, "encoder_parity.jsonl"), "a") as f:
        f.write(json.dumps(dict(case="split_mode_weight_scales", max_abs_vs_fp64=e, fp32_oracle_vs_fp64=e32)) + "\n")
    assert np.isfinite(got).all() and e <= 4.0 * e32 + 2e-5, (e, e32)


def _trained_like_weights(n_layers, ffn_drive=None, emb_scale=1.4, hidden=768, inter=3072, outliers=((17, 50.0), (400, -50.0))):
    """A 'trained-like' stress model (VERDICT r5 #4c): every parity fixture is random init (std 0.02, LayerNorm 1 / 0), where
    activations are O(1) and softmax is flat.  Here: embedding rows of the magnitude trained checkpoints have (0.05) with a common
    offset; hidden dimensions with x50 LayerNorm gains in every LayerNorm (the outlier dimensions of trained BERT / RoBERTa:
    ``outliers`` = (dimension, factor) pairs); Q / K scaled so that the softmax saturates (one key takes almost all the mass);
    optionally one FFN channel driven to ``ffn_drive`` in magnitude through its intermediate bias (GELU output and, through
    output.dense, the residual stream).  hidden / inter: the tower's width (768 / 3072: roberta-base)."""
    from oracle import encoder_ref
    sd = dict(encoder_ref.random_state_dict(seed=71, n_layers=n_layers, ln_jitter=0.1, hidden=hidden, inter=inter))
    we = sd["roberta.embeddings.word_embeddings.weight"].clone() * emb_scale
    we[:, 5] += 0.04
    sd["roberta.embeddings.word_embeddings.weight"] = we
    names = ["roberta.embeddings.LayerNorm"]
    for i in range(n_layers):
        names += ["roberta.encoder.layer.%d.attention.output.LayerNorm" % i, "roberta.encoder.layer.%d.output.LayerNorm" % i]
    for n in names:
        w = sd[n + ".weight"].clone()
        for dim, f in outliers:
            w[dim] *= f
        sd[n + ".weight"] = w
    for i in range(n_layers):
        p = "roberta.encoder.layer.%d." % i
        sd[p + "attention.self.query.weight"] = sd[p + "attention.self.query.weight"] * 6.0
        sd[p + "attention.self.key.weight"] = sd[p + "attention.self.key.weight"] * 6.0
    if ffn_drive is not None:
        b = sd["roberta.encoder.layer.1.intermediate.dense.bias"].clone()
        b[123] = ffn_drive
        sd["roberta.encoder.layer.1.intermediate.dense.bias"] = b
    return sd


def _oracle_pair(sd, ids, lens, L, n_layers, n_heads=12):
    """(fp64, fp32) outputs of the oracle tower on the same records"""
    from oracle import encoder_ref
    with torch.no_grad():
        sd64 = {k: v.double() for k, v in sd.items()}
        want64 = encoder_ref.rdot_nll_ln_emb(sd64, torch.from_numpy(ids), encoder_ref.mask_from_lengths(lens, L), n_layers=n_layers,
                                             n_heads=n_heads).numpy()
        want32 = encoder_ref.rdot_nll_ln_emb(sd, torch.from_numpy(ids), encoder_ref.mask_from_lengths(lens, L), n_layers=n_layers,
                                             n_heads=n_heads).numpy()
    return want64, want32


@pytest.mark.parametrize("ffn_drive", [None, 300.0, 2.0e4])
def test_split_mode_on_trained_like_activations(ffn_drive):
    """In-range stress cases: outlier LayerNorm gains, saturated softmax, small embedding rows, one FFN channel at 300 / 20,000
    (inside the fp16 range of the hi halves).  The split mode must stay fp32-grade -- within max(2e-5, 4 x the fp32 oracle's own
    distance from the fp64 oracle) -- and the range guard must stay silent."""
    from ance_amd.encoder import ARCH_ROBERTA, Encoder
    from oracle import synth
    n_layers = 3
    sd = _trained_like_weights(n_layers, ffn_drive)
    rng = np.random.default_rng(72)
    lens = np.array([1, 2, 31, 33, 64, 65, 96, 128, 70, 9, 100, 50], dtype=np.int32)
    ids = synth.make_records(rng, len(lens), 128, lens.astype(np.int64))
    want64, want32 = _oracle_pair(sd, ids, lens, 128, n_layers)
    enc = Encoder(sd, ARCH_ROBERTA, "roberta.", True, max_seq_len=128, max_tokens=2048, precision="split")
    got = enc.encode_ids(torch.from_numpy(ids).cuda(), torch.from_numpy(lens).cuda(), h_lens=lens).cpu().numpy()
    enc.check_range(sync=True)  # silent: every value is inside the range
    e32 = float(np.abs(want32.astype(np.float64) - want64).max())
    e = float(np.abs(got.astype(np.float64) - want64).max())
    with open(os.path.join(OUT, "encoder_parity.jsonl"), "a") as f:
        f.write(json.dumps(dict(case="split_mode_trained_like_ffn_%s" % ffn_drive, max_abs_vs_fp64=e, fp32_oracle_vs_fp64=e32)) + "\n")
    assert np.isfinite(got).all() and e <= max(2e-5, 4.0 * e32), (e, e32)


def test_split_mode_range_guard_raises_out_of_range():
    """Out-of-range stress case: one FFN channel driven to 1e5 -- fine in the reference's fp32, an overflow of the fp16 hi half in
    the split mode.  The precondition is CHECKED (ance_encoder_range_faults): the binding raises AnceRangeError naming the fp32
    mode, on the synchronous check and -- sticky -- on the next call; the fp32 mode encodes the same checkpoint to fp32 grade."""
    from ance_amd import _lib
    from ance_amd.encoder import ARCH_ROBERTA, Encoder
    from oracle import synth
    n_layers = 3
    sd = _trained_like_weights(n_layers, 1.0e5)
    rng = np.random.default_rng(73)
    lens = np.array([1, 2, 31, 33, 64, 65, 96, 128], dtype=np.int32)
    ids = synth.make_records(rng, len(lens), 128, lens.astype(np.int64))
    ids_d, lens_d = torch.from_numpy(ids).cuda(), torch.from_numpy(lens).cuda()
    enc = Encoder(sd, ARCH_ROBERTA, "roberta.", True, max_seq_len=128, max_tokens=2048, precision="split")
    enc.encode_ids(ids_d, lens_d, h_lens=lens)
    with pytest.raises(_lib.AnceRangeError, match="encoder_precision fp32"):
        enc.check_range(sync=True)
    with pytest.raises(_lib.AnceRangeError):   # sticky: the handle keeps refusing
        enc.encode_ids(ids_d, lens_d, h_lens=lens)
    del enc
    want64, want32 = _oracle_pair(sd, ids, lens, 128, n_layers)
    enc32 = Encoder(sd, ARCH_ROBERTA, "roberta.", True, max_seq_len=128, max_tokens=2048, precision="fp32")
    got = enc32.encode_ids(ids_d, lens_d, h_lens=lens).cpu().numpy()
    enc32.check_range(sync=True)
    e32 = float(np.abs(want32.astype(np.float64) - want64).max())
    e = float(np.abs(got.astype(np.float64) - want64).max())
    assert np.isfinite(got).all() and e <= max(2e-5, 4.0 * e32), (e, e32)


def test_range_guard_counts_nan_rows_in_every_mode():
    """A NaN in the checkpoint reaches every output row through the LayerNorm statistics: counter [1] of the range guard."""
    from ance_amd import _lib
    from ance_amd.encoder import ARCH_ROBERTA, Encoder
    from oracle import encoder_ref, synth
    sd = dict(encoder_ref.random_state_dict(seed=74, n_layers=1, ln_jitter=0.1))
    b = sd["roberta.encoder.layer.0.output.dense.bias"].clone()
    b[3] = float("nan")
    sd["roberta.encoder.layer.0.output.dense.bias"] = b
    lens = np.array([5, 9, 16], dtype=np.int32)
    ids = synth.make_records(np.random.default_rng(75), 3, 16, lens.astype(np.int64))
    for mode in ("split", "fp16", "fp32"):
        enc = Encoder(sd, ARCH_ROBERTA, "roberta.", True, max_seq_len=16, max_tokens=512, precision=mode)
        enc.encode_ids(torch.from_numpy(ids).cuda(), torch.from_numpy(lens).cuda(), h_lens=lens)
        with pytest.raises(_lib.AnceRangeError, match="3 output rows are NaN"):
            enc.check_range(sync=True)


def test_precision_is_chosen_by_the_descriptor_not_by_the_environment(monkeypatch):
    """ABI v5: ``precision=`` travels in AnceEncoderDesc.precision and wins over the environment; the environment only moves
    the DEFAULT (precision=None)."""
    from ance_amd.encoder import ARCH_ROBERTA, Encoder
    from oracle import encoder_ref
    sd = encoder_ref.random_state_dict(seed=5, n_layers=1, ln_jitter=0.1)
    monkeypatch.setenv("ANCE_ENCODER_PRECISE", "1")
    kw = dict(max_seq_len=16, max_tokens=512)
    assert Encoder(sd, ARCH_ROBERTA, "roberta.", True, **kw).precision == "fp32"
    assert Encoder(sd, ARCH_ROBERTA, "roberta.", True, precision="split", **kw).precision == "split"
    assert Encoder(sd, ARCH_ROBERTA, "roberta.", True, precision="fp16", **kw).precision == "fp16"
    assert os.environ["ANCE_ENCODER_PRECISE"] == "1" and "ANCE_ENCODER_SPLIT" not in os.environ
