"""SEED-Encoder (model_type seeddot_nll, ANCE_ARCH_SEED) on an MI355X: the reference's own SEEDEncoderDot_NLL_LN goldens in every
arithmetic, bit-identity with the RoBERTa tower on the compacted ids, the undefined inputs refused, and the refresh job."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from seed_util import make_seed_msmarco_like, seed_golden_weights, to_seed_names

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = {"split": 2e-5, "fp32": 2e-5, "fp16": 5e-3}  # those of test_full_depth_golden_of_reference


def _manifest(golden_dir):
    with open(os.path.join(golden_dir, "seed_manifest.json")) as f:
        return json.load(f)


def _encoder(sd_seed, arch_name, mode, max_seq_len, max_tokens):
    from ance_amd.encoder import ARCH_ROBERTA, ARCH_SEED, Encoder, seed_state_dict
    arch = ARCH_SEED if arch_name == "seed" else ARCH_ROBERTA
    return Encoder(seed_state_dict(sd_seed), arch, "seed.", True, max_seq_len=max_seq_len, max_tokens=max_tokens, precision=mode)


def _encode(enc, ids, lens):
    out = enc.encode_ids(torch.from_numpy(np.ascontiguousarray(ids, dtype=np.int32)).cuda(),
                         torch.from_numpy(np.ascontiguousarray(lens, dtype=np.int32)).cuda(), h_lens=lens).cpu().numpy()
    enc.check_range(sync=True)
    return out


def _compact(ids, lens, pad=1):
    c = np.full_like(ids, pad)
    cl = np.zeros_like(lens)
    for i in range(len(ids)):
        k = ids[i, :lens[i]]
        k = k[k != pad]
        c[i, :len(k)] = k
        cl[i] = len(k)
    return c, cl


@pytest.fixture(scope="module")
def seed12_weights(golden_dir):
    return seed_golden_weights(_manifest(golden_dir)["encoder"]["seed12"])


@pytest.mark.parametrize("mode", ["split", "fp32", "fp16"])
@pytest.mark.parametrize("name", ["seed12", "seed12_L512"])
def test_seed_golden_of_reference(golden_dir, name, mode):
    sd = seed_golden_weights(_manifest(golden_dir)["encoder"][name])
    g = np.load(os.path.join(golden_dir, "encoder_%s.npz" % name))
    ids, lens, want = g["ids"], g["lens"], g["emb"]
    enc = _encoder(sd, "seed", mode, ids.shape[1], 8192)
    got = _encode(enc, ids, lens)
    err = float(np.abs(got - want).max())
    assert np.isfinite(got).all() and err <= TOL[mode], (name, mode, err)


def _interior_pad_batch(seed=7, n=48, L=128):
    from oracle import synth
    from seed_util import interior_pads, into_seed_vocab
    rng = np.random.default_rng(seed)
    lens = rng.integers(1, L + 1, size=n).astype(np.int64)
    lens[:6] = [1, 2, 32, 33, 96, 128]
    ids = into_seed_vocab(synth.make_records(rng, n, L, lens))
    ids = interior_pads(rng, ids, lens, 0.3)
    ids[6, 1:lens[6]] = 1  # [CLS] + pads only
    return ids, lens.astype(np.int32)


@pytest.mark.parametrize("mode", ["split", "fp32", "fp16"])
def test_seed_is_the_roberta_tower_on_the_compacted_ids_bit_for_bit(seed12_weights, mode):
    """Dropping the pad-id tokens is exact (positions skip them): the SEED encode of records with pad ids inside their length
    must be the RoBERTa-arch encode (zero token-type row) of the compacted records, bit for bit -- and must not depend on the
    micro-batch the record lands in."""
    ids, lens = _interior_pad_batch()
    c, cl = _compact(ids, lens)
    assert (cl < lens).sum() > 30
    seed = _encode(_encoder(seed12_weights, "seed", mode, 128, 8192), ids, lens)
    rob = _encode(_encoder(seed12_weights, "roberta", mode, 128, 8192), c, cl)
    assert np.isfinite(seed).all()
    assert np.array_equal(seed.view(np.uint32), rob.view(np.uint32)), (mode, float(np.abs(seed - rob).max()))
    small = _encode(_encoder(seed12_weights, "seed", mode, 128, 512), ids, lens)  # many micro-batches of <= 512 tokens
    assert np.array_equal(seed.view(np.uint32), small.view(np.uint32)), (mode, float(np.abs(seed - small).max()))
    # rows alone and in reverse order
    rev = _encode(_encoder(seed12_weights, "seed", mode, 128, 8192), ids[::-1], lens[::-1])
    assert np.array_equal(seed.view(np.uint32), rev[::-1].view(np.uint32))


def test_seed_records_without_a_leading_cls_are_refused(seed12_weights):
    from ance_amd._lib import AnceLibraryError, AnceRangeError
    ids, lens = _interior_pad_batch(n=8)
    enc = _encoder(seed12_weights, "seed", "split", 128, 8192)
    _encode(enc, ids, lens)  # well-formed: no fault
    bad = ids.copy()
    bad[3, 0] = 1  # starts with the pad id
    enc.encode_ids(torch.from_numpy(bad).cuda(), torch.from_numpy(lens).cuda(), h_lens=lens)
    with pytest.raises(AnceRangeError, match="pad id"):
        enc.check_range(sync=True)
    enc2 = _encoder(seed12_weights, "seed", "split", 128, 8192)
    empty = lens.copy()
    empty[5] = 0
    with pytest.raises(AnceLibraryError, match="empty record"):
        enc2.encode_ids(torch.from_numpy(ids).cuda(), torch.from_numpy(empty).cuda(), h_lens=empty)
    with pytest.raises(AnceLibraryError, match="empty record"):
        enc2.encode_ids(torch.from_numpy(ids).cuda(), torch.from_numpy(empty).cuda())  # lengths read back by the library


def test_seed_refresh_job_against_the_reference_run(golden_dir, tmp_path):
    """`python -m ance_amd.ann_data_gen --model_type seeddot_nll` on a SEED checkpoint directory (fairseq names, plus the
    classification_heads.* / decoder.* keys it must ignore, and config.json) against the reference's own generate_new_ann run:
    every differing line a proven near-tie (tests/test_gpu_e2e.py's allowance), and the --inference dumps."""
    from ance_amd import ann_data_gen as adg
    from oracle import ann_ref, encoder_ref
    from test_gpu_config1 import chain_score_error, tau_needed
    with open(os.path.join(golden_dir, "e2e_seed.json")) as f:
        e = json.load(f)
    sd = seed_golden_weights(e["weights"])
    data = str(tmp_path / "data")
    make_seed_msmarco_like(data, **e["data"])
    ckpt = tmp_path / "train" / "checkpoint-100"
    ckpt.mkdir(parents=True)
    full = dict(sd)
    full["classification_heads.dense.weight"] = torch.zeros(768, 768)
    full["decoder.embed_tokens.weight"] = torch.zeros(4, 768)
    torch.save(full, str(ckpt / "pytorch_model.bin"))
    (ckpt / "config.json").write_text(json.dumps({"encoder_layers": e["weights"]["n_layers"], "pad_token_id": 1, "max_positions": 512}))
    (ckpt / "scheduler.pt").write_text("commit marker")
    a = e["args"]
    env = {k: v for k, v in os.environ.items() if not k.startswith("ANCE_ENCODER_") and k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE")}

    def run(out, *extra):
        cmd = [sys.executable, "-m", "ance_amd.ann_data_gen", "--training_dir", str(tmp_path / "train"), "--init_model_dir",
               "/nonexistent", "--model_type", "seeddot_nll", "--output_dir", out, "--cache_dir", out, "--data_dir", data,
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

    # fp64 truth: the RoBERTa tower (zero type row) on the compacted ids -- exact for SEED (tests above)
    from ance_amd.encoder import seed_state_dict
    sd64 = {k.replace("seed.", "roberta.", 1): v.to(device="cuda", dtype=torch.float64) for k, v in seed_state_dict(sd).items()}
    nl = e["weights"]["n_layers"]

    def enc64(name, L):
        lens, ids = ann_ref.read_cache(os.path.join(data, name))
        c, cl = _compact(ids, lens)
        with torch.no_grad():
            return encoder_ref.rdot_nll_ln_emb(sd64, torch.from_numpy(c).cuda(), encoder_ref.mask_from_lengths(cl, L).cuda(),
                                               n_layers=nl).cpu().numpy()

    p64, q64 = enc64("passages", a["max_seq_length"]), enc64("train-query", a["max_query_length"])
    from ance_amd.cache import TokenCache
    from ance_amd.encoder import load_model
    model = load_model("seeddot_nll", str(ckpt), max_seq_length=a["max_seq_length"], max_tokens=4096)
    eng = adg.HipEngine()

    def emb(name, is_q):
        with TokenCache(os.path.join(data, name)) as cc:
            return eng.encode_cache(model, cc, 0, len(cc), is_q).cpu().numpy()

    p_emb, train_q = emb("passages", False), emb("train-query", True)
    emb_err = max(float(np.abs(p_emb - p64).max()), float(np.abs(train_q - q64).max()))
    S64 = q64.astype(np.float64) @ p64.astype(np.float64).T
    tau_G = 1.0001 * chain_score_error(torch.from_numpy(p_emb), torch.from_numpy(train_q), S64)
    tau_R = 2e-3
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
