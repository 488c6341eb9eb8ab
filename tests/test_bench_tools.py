"""bench.py's own data tools (CPU): the synthetic tokenised cache `bench.py --refresh` writes is the reference's cache format
(utils/util.py:257-307) as `ance_amd.cache.TokenCache` reads it, block boundaries included, and deterministic.  One GPU test
runs the bench itself at a small size, with --full and without."""
import hashlib
import os

import numpy as np
import pytest


def test_synthetic_cache_round_trip(tmp_path):
    import bench
    from ance_amd.cache import TokenCache
    p = str(tmp_path / "passages")
    secs, mean_len = bench.write_synthetic_cache(p, 5000, 128, 70.0, 0.45, 8, seed=1, block=2048)  # 3 blocks, last one short
    c = TokenCache(p)
    assert len(c) == 5000 and c.embedding_size == 128 and c.record_size == 4 + 4 * 128
    assert os.path.getsize(p) == 5000 * c.record_size
    L, ids = c.lengths(), c.ids()
    assert L.min() >= 8 and L.max() <= 128 and abs(float(L.mean()) - mean_len) < 1e-9
    rows = np.arange(5000)
    assert np.all(ids[:, 0] == 0) and np.all(ids[rows, L - 1] == 2)          # <s> ... </s>
    assert np.all((np.arange(128)[None, :] < L[:, None]) | (ids == 1))       # pad = 1 after the length
    inner = (np.arange(128)[None, :] > 0) & (np.arange(128)[None, :] < (L - 1)[:, None])
    assert np.all(ids[inner] >= 3) and np.all(ids[inner] < 50265)
    plen, tok = c[4999]                                                       # the reference's __getitem__ contract
    assert plen == int(L[4999]) and np.array_equal(tok, ids[4999])
    # deterministic in (seed, block)
    p2 = str(tmp_path / "again")
    bench.write_synthetic_cache(p2, 5000, 128, 70.0, 0.45, 8, seed=1, block=2048)
    assert hashlib.sha256(open(p, "rb").read()).digest() == hashlib.sha256(open(p2, "rb").read()).digest()


def test_bench_records_match_cache_layout():
    import bench
    rng = np.random.default_rng(0)
    rec, lens = bench.synthetic_records(rng, 64, 32)
    assert rec.shape == (64, 33) and rec.dtype == np.int32
    assert np.array_equal(rec[:, 0].view(">u4").astype(np.int64).reshape(-1), lens.astype(np.int64))  # big-endian header


def test_gpus_flag_refuses_to_measure_fewer_devices(tmp_path):
    """`bench.py --gpus N` starts N ranks itself; with fewer visible GPUs than ranks it must fail loudly instead of
    printing a one-rank line (the flag used to be parsed and never read)."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    env["HIP_VISIBLE_DEVICES"] = ""
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0"],
                       capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 2 and "visible GPU" in r.stderr and r.stdout.strip() == ""
    # a launcher that started a different number of ranks than --gpus says is refused as well
    env["WORLD_SIZE"] = "1"
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "4"], capture_output=True, text=True, env=env,
                       timeout=300)
    assert r.returncode == 2 and "WORLD_SIZE" in r.stderr


def test_roofline_evidence_helpers_quote_only_this_round(tmp_path, monkeypatch):
    """bench.py reads counters (profiles/pmc_traffic.json) and kernel-trace averages (profiles/rNN_*.csv) into the JSON line:
    an entry of another round must not be quoted (stale round-1 counters were printed under round-2 kernels),
    and frac_from_profiles comes from the CSV row of the named kernel."""
    import json
    import bench
    prof = tmp_path / "profiles"
    prof.mkdir()
    (prof / "pmc_traffic.json").write_text(json.dumps({"encode": {
        "gemm_ffn1": {"round": bench.CURRENT_ROUND, "hbm_bytes_per_launch": 1.0},
        "gemm_qk": {"round": "r01", "hbm_bytes_per_launch": 2.0},
        "gemm_res": {"round": bench.CURRENT_ROUND + " (final)", "hbm_bytes_per_launch": 3.0}}}))
    (prof / ("%s_rocprofv3_encode_single_stream_kernel_stats.csv" % bench.CURRENT_ROUND)).write_text(
        '"Name","Calls","TotalDurationNs","AverageNs","Percentage","MinNs","MaxNs","StdDev"\n'
        '"void ance::(anonymous namespace)::gemm256_f16_desc_kernel<6>(ance::GemmArgs)",10,3000000,300000.0,50,1,2,3\n'
        '"void ance::(anonymous namespace)::gemm256_f16_desc_kernel<4>(ance::GemmArgs)",20,4000000,200000.0,50,1,2,3\n')
    monkeypatch.setattr(bench, "ROOT", str(tmp_path))
    assert bench.pmc_traffic("encode", "gemm_ffn1")["hbm_bytes_per_launch"] == 1.0
    assert bench.pmc_traffic("encode", "gemm_qk") is None                       # another round's counters
    assert bench.pmc_traffic("encode", "gemm_ffn2")["hbm_bytes_per_launch"] == 3.0  # both RES GEMMs are one kernel
    assert bench.pmc_traffic("search", "ip_topk_fast") is None
    name = "%s_rocprofv3_encode_single_stream_kernel_stats.csv" % bench.CURRENT_ROUND
    assert bench.trace_avg_ns(name, bench.KERNEL_OF["gemm_ffn1"]) == 300000.0
    assert bench.trace_avg_ns(name, bench.KERNEL_OF["gemm_attn_out"]) == 200000.0
    assert bench.trace_avg_ns("missing.csv", "x") is None


def test_power_sampler_reads_hwmon_files(tmp_path):
    """bench.PowerSampler: socket power (uW) and shader clock (Hz) from an amdgpu hwmon directory, sampled by a thread while a timed
    region runs; a platform without the files (and without rocm-smi devices) reports None instead of failing the bench."""
    import time
    import bench
    d = tmp_path / "hwmon7"
    d.mkdir()
    (d / "power1_input").write_text("1396000000\n")
    (d / "freq1_input").write_text("1572000000\n")
    (d / "power1_cap").write_text("1400000000\n")
    with bench.PowerSampler(None, 0, hwmon_dirs=[str(d)]) as ps:
        time.sleep(0.7)
    r = ps.report()
    assert r["samples"] >= 2 and r["power_cap_w"] == 1400.0
    assert r["socket_power_w"] == {"min": 1396.0, "mean": 1396.0, "max": 1396.0}
    assert r["sclk_mhz"]["mean"] == 1572.0 and r["measured_in_this_run"] is True
    empty = tmp_path / "hwmon8"
    empty.mkdir()
    ps2 = bench.PowerSampler(None, 0, hwmon_dirs=[str(empty)])
    assert ps2.files is None or ps2.report() is None


def test_dump_rows_are_a_fixed_sample_within_the_budget(tmp_path):
    """--dump-outputs: every row when the leg's budget holds them, else the same seeded, ascending sample on every run; the
    files are float32 / float64 and the legs' budgets stay under the 64 MB the option promises."""
    import bench
    assert np.array_equal(bench.dump_rows(100, 3072, 1 << 20, 0), np.arange(100))
    a = bench.dump_rows(16384, 3072, 24 << 20, 0)
    assert len(a) == 8192 and np.array_equal(a, np.unique(a)) and a[-1] < 16384
    assert np.array_equal(a, bench.dump_rows(16384, 3072, 24 << 20, 0))
    assert not np.array_equal(a, bench.dump_rows(16384, 3072, 24 << 20, 1))
    assert sum(bench.DUMP_BUDGET.values()) + 128 * 5 <= 64 * 10 ** 6
    bench.write_dumps(str(tmp_path / "d"), {"x": np.ones((4, 3), np.float32), "y": np.arange(3.0)})
    assert np.load(str(tmp_path / "d" / "x.npy")).dtype == np.float32 and np.load(str(tmp_path / "d" / "y.npy")).dtype == np.float64
    with pytest.raises(AssertionError):
        bench.write_dumps(str(tmp_path / "e"), {"ids": np.arange(3)})
    with pytest.raises(AssertionError):
        bench.write_dumps(str(tmp_path / "e"), {"big": np.zeros(8 * 10 ** 6 + 1)})


def test_result_stream_keeps_stdout_to_the_json_line():
    """The bench's stdout is its one JSON line: what the run prints otherwise (the refresh job's progress line, a child
    process) goes to stderr."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import json, subprocess, bench\n"
            "r = bench.result_stream()\n"
            "print('Rank:0 --- ANN NDCG@10:0.0')\n"
            "subprocess.run(['echo', 'child'])\n"
            "print(json.dumps({'ms_per_step': 1.0}), file=r, flush=True)\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=root, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout == '{"ms_per_step": 1.0}\n'
    assert "ANN NDCG" in r.stderr and "child" in r.stderr


def _bench_line(root, tmp_path, steps, dump, full=True):
    import json
    import subprocess
    import sys
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1", "--layers", "2",
           "--n-passages", "200000", "--encode-block", "2048", "--query-block", "2048", "--exact-check-queries", "8",
           "--skip-precise", "--skip-mfma-probe", "--skip-other-configs", "--no-cpu-baseline",
           "--slice-passages", "20000", "--slice-queries", "2048", "--slice-dev-queries", "256",
           "--slice-dir", str(tmp_path / ("slice%d" % steps)), "--dump-outputs", dump] + (["--full"] if full else [])
    r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.splitlines()
    assert len(lines) == 1, r.stdout[-3000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_bench_line_and_dumped_outputs(tmp_path):
    """bench.py --full on a small corpus, twice with different --steps: stdout is exactly the JSON line (the whole-refresh slice,
    which prints the job's NDCG line, included), `steps` / `ms_per_step` describe the timed steps, and --dump-outputs writes
    the same float arrays on both runs -- the inputs are seeded, the outputs of a step do not depend on how many ran."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    d1, d2 = str(tmp_path / "d1"), str(tmp_path / "d2")
    o1 = _bench_line(root, tmp_path, 3, d1)
    o2 = _bench_line(root, tmp_path, 2, d2)
    for o, k in ((o1, 3), (o2, 2)):
        assert "errors" not in o, o.get("errors")
        assert o["steps"] == k and o["ms_per_step"] > 0 and o["search"]["ms_per_step"] > 0
        assert abs(o["value"] - 2048 * 1e3 / o["ms_per_step"]) <= 1e-6 * o["value"]
        assert o["full_refresh_slice"]["lines_written"] == 2048
    shapes = {"encode_embeddings": (2048, 768), "search_scores": (2048, 200), "search_ids": (2048, 200),
              "search_encoder_like_scores": (2048, 200), "search_encoder_like_ids": (2048, 200)}
    assert sorted(os.listdir(d1)) == sorted(n + ".npy" for n in shapes)
    assert sum(os.path.getsize(os.path.join(d1, f)) for f in os.listdir(d1)) <= 64 * 10 ** 6
    for n, shape in shapes.items():
        a, b = np.load(os.path.join(d1, n + ".npy")), np.load(os.path.join(d2, n + ".npy"))
        assert a.shape == shape and a.dtype == (np.float64 if n.endswith("_ids") else np.float32) and np.isfinite(a).all()
        assert np.array_equal(a, b), n
    ids = np.load(os.path.join(d1, "search_ids.npy"))
    assert ids.min() >= 0 and ids.max() < 200000 and np.array_equal(ids, np.rint(ids))
    assert (np.diff(np.load(os.path.join(d1, "search_scores.npy")), axis=1) <= 0).all()


DUMP_NAMES = ("encode_embeddings", "search_scores", "search_ids", "search_encoder_like_scores", "search_encoder_like_ids")


@pytest.mark.gpu
def test_plain_bench_line_is_the_headline_alone(tmp_path):
    """bench.py without --full times the headline encode leg alone: the line carries the headline fields and none of what
    --full measures, and --dump-outputs still writes every array, equal to what a --full run dumps."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    dp, df = str(tmp_path / "plain"), str(tmp_path / "full")
    o = _bench_line(root, tmp_path, 2, dp, full=False)
    assert "errors" not in o, o.get("errors")
    assert o["metric"] == "passages_encoded_per_sec" and o["unit"] == "passages/s" and o["higher_is_better"] is True
    assert o["steps"] == 2 and o["warmup"] == 1 and o["encoder_precision"] == "split" and o["dtype"].startswith("f16 pair")
    assert o["ms_per_step"] > 0 and abs(o["value"] - 2048 * 1e3 / o["ms_per_step"]) <= 1e-6 * o["value"]
    for k in ("search", "roofline", "power", "encode_fp16_fast", "encode_fp32", "other_configs", "full_refresh_slice",
              "cpu_baseline", "retrieval_agreement"):
        assert k not in o, k
    _bench_line(root, tmp_path, 1, df)
    assert sorted(os.listdir(dp)) == sorted(n + ".npy" for n in DUMP_NAMES)
    for n in DUMP_NAMES:
        a, b = np.load(os.path.join(dp, n + ".npy")), np.load(os.path.join(df, n + ".npy"))
        assert a.dtype == b.dtype and np.array_equal(a, b), n


def test_full_is_off_by_default_and_refresh_has_its_own_flag(monkeypatch):
    import sys
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1"])
    a = bench.parse()
    assert not a.full and not a.refresh and a.steps == 3 and a.warmup == 1
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full"])
    assert bench.parse().full
    monkeypatch.setattr(sys, "argv", ["bench.py", "--refresh", "--refresh-queries", "10", "--refresh-dev-queries", "5"])
    a = bench.parse()
    assert a.refresh and not a.full and a.refresh_queries == 10 and a.refresh_dev_queries == 5
