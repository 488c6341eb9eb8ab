"""The large tower (RoBERTa-large width: hidden 1024, 16 heads, FFN 4096, 24 layers) on the GPU: golden vectors of the reference's own
RobertaDot_NLL_LN / MultiChunk classes (tests/golden/make_golden_large.py) in the three arithmetic modes, bit-stability under the
micro-batch split and the A/B switches, the split mode's range guard, and the refresh job on a large-width checkpoint.
Tolerances: split and fp32 max(2e-5, 4 x the reference's own fp32-vs-fp64 distance, large_manifest.json); fp16 1e-2 (the base
tower's 5e-3 doubled for twice the depth); random batches against the fp32 mode of the library: fp16 5e-3, split 4e-5.
Needs an MI355X."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from golden_util import golden_weights

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LARGE = dict(hidden=1024, inter=4096)


def _manifest(golden_dir):
    with open(os.path.join(golden_dir, "large_manifest.json")) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def large24(golden_dir):
    """The 24-layer weights of the encoder fixtures, built once for the module (checked against the manifest's sha256)."""
    return golden_weights(_manifest(golden_dir)["encoder"]["large24"], **LARGE)


def _encoder(sd, precision, L, max_tokens):
    from ance_amd.encoder import ARCH_ROBERTA, Encoder
    enc = Encoder(sd, ARCH_ROBERTA, "roberta.", True, max_seq_len=L, max_tokens=max_tokens, precision=precision)
    assert (enc.hidden, enc.n_heads, enc.n_layers) == (1024, 16, sd_layers(sd))
    return enc


def sd_layers(sd):
    from ance_amd.encoder import count_layers
    return count_layers(sd, "roberta.")


def _encode(enc, ids, lens, n_chunks=1):
    out = enc.encode_ids(torch.from_numpy(ids).cuda(), torch.from_numpy(lens).cuda(), n_chunks=n_chunks, h_lens=lens)
    enc.check_range(sync=True)
    return out


def _tol(mode, meta):
    return 1e-2 if mode == "fp16" else max(2e-5, 4.0 * meta["fp32_vs_fp64"])


@pytest.mark.parametrize("mode", ["split", "fp16", "fp32"])
@pytest.mark.parametrize("fixture,L,chunks", [("large24", 128, 1), ("large24_L512", 512, 1), ("large_maxp", 512, 4)])
def test_large_goldens_of_reference(golden_dir, large24, mode, fixture, L, chunks):
    meta = _manifest(golden_dir)["encoder"][fixture]
    assert meta["checksum"] == _manifest(golden_dir)["encoder"]["large24"]["checksum"]  # one weight set for the three fixtures
    g = np.load(os.path.join(golden_dir, "encoder_%s.npz" % fixture))
    enc = _encoder(large24, mode, L, 16384)
    got = _encode(enc, g["ids"].astype(np.int32), g["lens"].astype(np.int32), chunks).cpu().numpy().reshape(g["emb"].shape)
    d = float(np.abs(got.astype(np.float64) - g["emb"]).max())
    print("large golden %s %s: max |delta| %.3e (tolerance %.3e)" % (fixture, mode, d, _tol(mode, meta)))
    assert np.isfinite(got).all() and d <= _tol(mode, meta), (fixture, mode, d)


def _batch(seed, n=300, L=128):
    from oracle import synth
    rng = np.random.default_rng(seed)
    lens = np.concatenate([np.array([1, 2, 31, 32, 33, 64, 65, 96, 97, 128], dtype=np.int32),
                           rng.integers(3, L + 1, n - 10).astype(np.int32)])
    return synth.make_records(rng, len(lens), L, lens.astype(np.int64)).astype(np.int32), lens


@pytest.mark.parametrize("mode", ["split", "fp16"])
def test_large_rows_do_not_depend_on_the_micro_batch_split(large24, mode):
    ids, lens = _batch(91)
    a = _encode(_encoder(large24, mode, 128, 131072), ids, lens)
    b = _encode(_encoder(large24, mode, 128, 2048), ids, lens)  # ~20 micro-batches
    assert torch.isfinite(a).all() and torch.equal(a, b)


@pytest.mark.parametrize("switch,value", [("ANCE_CLS_TAIL", "0"), ("ANCE_GEMM_STREAM", "0"), ("ANCE_ENCODER_STREAMS", "1")])
def test_large_ab_switches_change_no_bit(monkeypatch, large24, switch, value):
    from ance_amd import _lib
    ids, lens = _batch(92)
    want = _encode(_encoder(large24, "split", 128, 8192), ids, lens)
    monkeypatch.setenv(switch, value)
    _lib.reload_env()
    try:
        got = _encode(_encoder(large24, "split", 128, 8192), ids, lens)
    finally:
        monkeypatch.delenv(switch)
        _lib.reload_env()
    assert torch.equal(got, want), switch


def test_large_split_range_guard_raises_out_of_range():
    """One FFN channel at 1e5 (layer 0's intermediate.dense bias): fine in fp32, an overflow of the split mode's fp16 hi half."""
    from ance_amd import _lib
    from oracle import encoder_ref
    sd = encoder_ref.det_state_dict(seed=95, n_layers=2, ln_jitter=0.1, **LARGE)
    sd["roberta.encoder.layer.0.intermediate.dense.bias"][7] = 1.0e5
    ids, lens = _batch(93, n=40)
    enc = _encoder(sd, "split", 128, 4096)
    enc.encode_ids(torch.from_numpy(ids).cuda(), torch.from_numpy(lens).cuda(), h_lens=lens)
    with pytest.raises(_lib.AnceRangeError, match="encoder_precision fp32"):
        enc.check_range(sync=True)


def test_large_refresh_job_against_the_reference_run(golden_dir, tmp_path):
    """`python -m ance_amd.ann_data_gen --model_type rdot_nll` on a 4-layer large-width checkpoint directory (with its config.json)
    against the reference's own generate_new_ann run (tests/golden/e2e_large.json): every differing line a proven near-tie
    (tests/test_gpu_e2e.py's allowance), the same dev NDCG, and the --inference dumps."""
    from ance_amd import ann_data_gen as adg
    from ance_amd.cache import TokenCache
    from ance_amd.encoder import load_model
    from oracle import ann_ref, encoder_ref, synth
    from test_gpu_config1 import chain_score_error, tau_needed
    with open(os.path.join(golden_dir, "e2e_large.json")) as f:
        e = json.load(f)
    w = e["weights"]
    sd = golden_weights(w, **LARGE)
    data = str(tmp_path / "data")
    synth.make_msmarco_like(data, **e["data"])
    ckpt = tmp_path / "train" / "checkpoint-100"
    ckpt.mkdir(parents=True)
    torch.save(sd, str(ckpt / "pytorch_model.bin"))
    (ckpt / "config.json").write_text(json.dumps({"hidden_size": 1024, "num_attention_heads": 16, "intermediate_size": 4096,
                                                  "num_hidden_layers": w["n_layers"], "model_type": "roberta"}))
    (ckpt / "scheduler.pt").write_text("commit marker")
    a = e["args"]
    env = {k: v for k, v in os.environ.items() if not k.startswith("ANCE_ENCODER_") and k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}

    def run(out, *extra):
        cmd = [sys.executable, "-m", "ance_amd.ann_data_gen", "--training_dir", str(tmp_path / "train"), "--init_model_dir",
               "/nonexistent", "--model_type", "rdot_nll", "--output_dir", out, "--cache_dir", out, "--data_dir", data,
               "--max_seq_length", str(a["max_seq_length"]), "--max_query_length", str(a["max_query_length"]),
               "--per_gpu_eval_batch_size", "16", "--topk_training", str(a["topk_training"]), "--negative_sample",
               str(a["negative_sample"]), "--end_output_num", "0", "--ann_chunk_factor", str(a["ann_chunk_factor"]),
               "--ann_measure_topk_mrr", "--seed", str(a["seed"]), "--max_tokens", "4096"] + list(extra)
        r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]

    out = str(tmp_path / "out")
    run(out)
    no, train_path, nd = adg.get_latest_ann_data(out)
    assert no == 0 and adg.get_checkpoint_no(nd["checkpoint"]) == 100

    # fp64 truth of the same tower
    sd64 = {k: v.to(device="cuda", dtype=torch.float64) for k, v in sd.items()}

    def enc64(name, L):
        lens, ids = ann_ref.read_cache(os.path.join(data, name))
        with torch.no_grad():
            return encoder_ref.rdot_nll_ln_emb(sd64, torch.from_numpy(ids).cuda(), encoder_ref.mask_from_lengths(lens, L).cuda(),
                                               n_layers=w["n_layers"], n_heads=16).cpu().numpy()

    p64, q64 = enc64("passages", a["max_seq_length"]), enc64("train-query", a["max_query_length"])
    model = load_model("rdot_nll", str(ckpt), max_seq_length=a["max_seq_length"], max_tokens=4096)
    assert (model.q.hidden, model.q.n_heads) == (1024, 16)
    eng = adg.HipEngine()

    def emb(name, is_q):
        with TokenCache(os.path.join(data, name)) as cc:
            return eng.encode_cache(model, cc, 0, len(cc), is_q).cpu().numpy()

    p_emb, train_q = emb("passages", False), emb("train-query", True)
    emb_err = max(float(np.abs(p_emb - p64).max()), float(np.abs(train_q - q64).max()))
    S64 = q64.astype(np.float64) @ p64.astype(np.float64).T
    tau_G = 1.0001 * chain_score_error(torch.from_numpy(p_emb), torch.from_numpy(train_q), S64)
    tau_R = 2e-3
    print("large refresh job: max |delta| of the embeddings %.3e, score error %.3e" % (emb_err, tau_G))
    assert emb_err <= 5e-5 and tau_G <= 2e-3, (emb_err, tau_G)
    ref_lines = dict(l.split("\t", 1) for l in e["ann_training_data_0"].splitlines())
    got_lines = dict(l.split("\t", 1) for l in open(train_path).read().splitlines())
    assert set(ref_lines) == set(got_lines)
    same, unexplained = 0, []
    for q in ref_lines:
        if ref_lines[q] == got_lines[q]:
            same += 1
            continue
        pos = int(ref_lines[q].split("\t")[0])
        ng = [int(x) for x in got_lines[q].split("\t")[1].split(",")]
        nr = [int(x) for x in ref_lines[q].split("\t")[1].split(",")]
        if tau_needed(S64[int(q)], ng, excluded=[pos]) > tau_G or tau_needed(S64[int(q)], nr, excluded=[pos]) > tau_R:
            unexplained.append(int(q))
    assert not unexplained, unexplained
    assert same >= 0.8 * len(ref_lines), (same, len(ref_lines))
    assert abs(nd["ndcg"] - e["ann_ndcg_0"]["ndcg"]) <= 0.02, (nd["ndcg"], e["ann_ndcg_0"]["ndcg"])

    # --inference: the embedding dumps of the same job
    inf = str(tmp_path / "inf")
    run(inf, "--inference")
    pe = np.load(os.path.join(inf, "passage_100__emb_p__data_obj_0.npy"))
    assert np.array_equal(pe, p_emb)


# ---- the base tower's adversarial encoder tests (tests/test_gpu_encoder.py) at the large width: 3-layer towers against the fp64
# oracle with 16 heads, the base tower's tolerances at the same depth (fp16 5e-3 and cosine 0.99999, split fp32-grade)

def _oracle64(sd, ids, lens, L, n_layers):
    from oracle import encoder_ref
    with torch.no_grad():
        sd64 = {k: v.double() for k, v in sd.items()}
        return encoder_ref.rdot_nll_ln_emb(sd64, torch.from_numpy(ids), encoder_ref.mask_from_lengths(lens, L), n_layers=n_layers,
                                           n_heads=16).float().numpy()


def _encode_np(sd, precision, ids, lens, L=128, max_tokens=2048):
    enc = _encoder(sd, precision, L, max_tokens)
    return _encode(enc, ids, lens).cpu().numpy()


LENS12 = np.array([1, 2, 31, 33, 64, 65, 96, 128, 70, 9, 100, 50], dtype=np.int32)


@pytest.mark.parametrize("offset", [5.0, 30.0])
def test_large_rows_with_a_large_mean_keep_the_fp16_tolerance(offset):
    """fp16 mode on rows whose mean is 5 / 30 standard deviations away from 0 (tests/test_gpu_encoder.py: _offset_weights): at
    hidden 1024 the folded GEMM tiles read eight 128-column slice statistics, detect the wide rows and add the K loop over their
    lo halves."""
    from oracle import encoder_ref, synth
    from test_gpu_encoder import _offset_weights, _report
    n_layers = 3
    sd = _offset_weights(encoder_ref.random_state_dict(seed=5, n_layers=n_layers, ln_jitter=0.1, **LARGE), offset, n_layers)
    ids = synth.make_records(np.random.default_rng(8), len(LENS12), 128, LENS12.astype(np.int64))
    _report("large_width_mean_offset_%g" % offset, _encode_np(sd, "fp16", ids, LENS12), _oracle64(sd, ids, LENS12, 128, n_layers))


def test_large_fp16_rows_do_not_depend_on_their_tile_mates():
    """fp16 mode, wide-mean and ordinary tokens inside the same 256-token GEMM tiles (half of the sequences draw their tokens from
    embeddings 8 standard deviations off zero): the masked second K loop keeps a row's bits independent of its neighbours --
    identical under three micro-batch splits and in reverse order -- and everything stays inside the fp16 tolerance."""
    from oracle import encoder_ref, synth
    from test_gpu_encoder import _report
    n_layers = 3
    sd = dict(encoder_ref.random_state_dict(seed=21, n_layers=n_layers, ln_jitter=0.1, **LARGE))
    we = sd["roberta.embeddings.word_embeddings.weight"].clone()
    we[30000:] += 8 * 0.035
    sd["roberta.embeddings.word_embeddings.weight"] = we
    rng = np.random.default_rng(22)
    n = 96
    lens = rng.integers(1, 129, size=n).astype(np.int32)
    ids = synth.make_records(rng, n, 128, lens.astype(np.int64))
    wide_seq = (np.arange(n) % 2) == 1
    ids[wide_seq] = np.where(ids[wide_seq] > 3, 30000 + ids[wide_seq] % 20000, ids[wide_seq])
    ids[~wide_seq] = np.where(ids[~wide_seq] >= 30000, ids[~wide_seq] - 25000, ids[~wide_seq])
    got = _encode_np(sd, "fp16", ids, lens, max_tokens=2048)
    _report("large_width_mixed_wide_and_ordinary_rows", got, _oracle64(sd, ids, lens, 128, n_layers))
    assert np.array_equal(_encode_np(sd, "fp16", ids, lens, max_tokens=512), got)
    assert np.array_equal(_encode_np(sd, "fp16", ids, lens, max_tokens=1024), got)
    rev = np.arange(n)[::-1].copy()
    assert np.array_equal(_encode_np(sd, "fp16", ids[rev].copy(), lens[rev].copy(), max_tokens=768)[rev], got)


def test_large_split_mode_with_weights_of_very_different_scales():
    """Split mode with every weight matrix of a 3-layer large tower rescaled by factors between 2^-7 and 2^9 (and one outlier
    element 50,000 x its matrix's typical one): within 4 x the fp32 oracle's distance from fp64, + 2e-5."""
    from oracle import encoder_ref, synth
    from test_gpu_encoder import _oracle_pair
    n_layers = 3
    sd = dict(encoder_ref.random_state_dict(seed=61, n_layers=n_layers, ln_jitter=0.1, **LARGE))
    factors = {"attention.self.query": 6.0, "attention.self.key": 1.0 / 6.0, "attention.self.value": 37.0, "attention.output.dense": 1.0 / 40.0,
               "intermediate.dense": 300.0, "output.dense": 1.0 / 120.0}
    for i in range(n_layers):
        for name, f in factors.items():
            k = "roberta.encoder.layer.%d.%s.weight" % (i, name)
            sd[k] = sd[k] * (f if i != 1 else 1.0 / f)
    w = sd["roberta.encoder.layer.2.output.dense.weight"].clone()
    w[1000, 3077] = 9.0
    sd["roberta.encoder.layer.2.output.dense.weight"] = w
    ids = synth.make_records(np.random.default_rng(62), len(LENS12), 128, LENS12.astype(np.int64))
    want64, want32 = _oracle_pair(sd, ids, LENS12, 128, n_layers, n_heads=16)
    got = _encode_np(sd, "split", ids, LENS12)
    e32 = float(np.abs(want32.astype(np.float64) - want64).max())
    e = float(np.abs(got.astype(np.float64) - want64).max())
    print("large split weight scales: max |delta| vs fp64 %.3e, fp32 oracle vs fp64 %.3e" % (e, e32))
    assert np.isfinite(got).all() and e <= 4.0 * e32 + 2e-5, (e, e32)


@pytest.mark.parametrize("ffn_drive", [None, 300.0, 2.0e4])
def test_large_split_mode_on_trained_like_activations(ffn_drive):
    """tests/test_gpu_encoder.py::test_split_mode_on_trained_like_activations at hidden 1024, with a third outlier LayerNorm gain in
    the last 128-column slice of the statistics (dimension 1000): fp32-grade -- max(2e-5, 4 x the fp32 oracle's distance from
    fp64) -- and the range guard silent."""
    from oracle import synth
    from test_gpu_encoder import _oracle_pair, _trained_like_weights
    n_layers = 3
    sd = _trained_like_weights(n_layers, ffn_drive, hidden=1024, inter=4096, outliers=((17, 50.0), (400, -50.0), (1000, 50.0)))
    ids = synth.make_records(np.random.default_rng(72), len(LENS12), 128, LENS12.astype(np.int64))
    want64, want32 = _oracle_pair(sd, ids, LENS12, 128, n_layers, n_heads=16)
    got = _encode_np(sd, "split", ids, LENS12)   # (_encode: the range guard must stay silent)
    e32 = float(np.abs(want32.astype(np.float64) - want64).max())
    e = float(np.abs(got.astype(np.float64) - want64).max())
    print("large split trained-like ffn %s: max |delta| vs fp64 %.3e, fp32 oracle vs fp64 %.3e" % (ffn_drive, e, e32))
    assert np.isfinite(got).all() and e <= max(2e-5, 4.0 * e32), (e, e32)


LARGE_RANDOM_BATCHES = [(128, 900, 4096, 1), (512, 60, 4096, 3), (32, 1500, 512, 4), (8, 3000, 4096, 5)]
_random_batches = {}


def _large_random_batch(L, n, max_tokens, seed):
    """(weights, ids, lens, rows of the fp32 mode): made once per case and shared by the modes compared with it."""
    key = (L, n, max_tokens, seed)
    if key not in _random_batches:
        from oracle import encoder_ref, synth
        sd = encoder_ref.random_state_dict(seed=30 + seed, n_layers=3, ln_jitter=0.1, **LARGE)
        rng = np.random.default_rng(100 + seed)
        lens = rng.integers(1, L + 1, size=n).astype(np.int32)
        lens[:8] = [1, 1, L, L, 2, L - 1, 33 % L + 1, 1]
        ids = synth.make_records(rng, n, L, lens.astype(np.int64)).astype(np.int32)
        b = _encode(_encoder(sd, "fp32", L, max_tokens), ids, lens)
        assert torch.isfinite(b).all()
        _random_batches[key] = (sd, ids, lens, b)
    return _random_batches[key]


def _large_random_batch_against_fp32_mode(mode, bound, L, n, max_tokens, seed):
    sd, ids, lens, b = _large_random_batch(L, n, max_tokens, seed)
    a = _encode(_encoder(sd, mode, L, max_tokens), ids, lens)
    assert torch.isfinite(a).all()
    d = (a - b).abs().max(dim=1).values
    print("large %s vs fp32 mode L %d n %d: max |delta| %.3e (row %d, length %d)"
          % (mode, L, n, float(d.max()), int(d.argmax()), int(lens[int(d.argmax())])))
    from test_gpu_encoder import OUT
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, "encoder_parity.jsonl"), "a") as f:
        f.write(json.dumps(dict(case="large_random_batches_%s_vs_fp32_mode_L%d_n%d" % (mode, L, n), max_abs=float(d.max()),
                                worst_row=int(d.argmax()), worst_len=int(lens[int(d.argmax())]))) + "\n")
    assert float(d.max()) <= bound, (float(d.max()), int(d.argmax()), int(lens[int(d.argmax())]))
    same = np.flatnonzero(lens == 1)
    if len(same) > 1:
        twins = [int(r) for r in same if ids[r, 0] == ids[same[0], 0]]
        assert len(twins) > 1 and all(torch.equal(a[twins[0]], a[r]) for r in twins)


@pytest.mark.parametrize("L,n,max_tokens,seed", LARGE_RANDOM_BATCHES)
def test_large_random_batches_fp16_against_fp32_mode(L, n, max_tokens, seed):
    """Random lengths 1..L across many micro-batches, with tails of more (L = 8: ~900 sequences per micro-batch) and fewer than 256
    [CLS] rows:
    the fp16 mode against the fp32 mode of the large tower (two independent implementations of every kernel) within 5e-3, and
    identical one-token inputs give identical rows."""
    _large_random_batch_against_fp32_mode("fp16", 5e-3, L, n, max_tokens, seed)


@pytest.mark.parametrize("L,n,max_tokens,seed", LARGE_RANDOM_BATCHES)
def test_large_random_batches_split_against_fp32_mode(L, n, max_tokens, seed):
    """The same batches in the library's default arithmetic: the split mode against the fp32 mode of the large tower.  Each is
    stated to be within 2e-5 of the fp32 oracle on these 3-layer unit-variance rows, so the two are at most 4e-5 apart; identical
    one-token inputs give identical rows."""
    _large_random_batch_against_fp32_mode("split", 4e-5, L, n, max_tokens, seed)
