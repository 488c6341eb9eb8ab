#!/usr/bin/env python
"""SHA-256 fingerprints of the encoder's output bytes on fixed synthetic inputs: the check that a restructuring of the encoder's
source moved no bit, which the suite's tolerances cannot show.

    python scripts/encoder_fingerprint.py                          # {"case": sha256, ...} of the library in the tree (or ANCE_AMD_LIB)
    python scripts/encoder_fingerprint.py --libs A.so B.so --out F  # one fresh child process per library; exit 1 unless all agree

Cases: RoBERTa + head, BERT without head, SEED with interior pad ids, MaxP (4 chunks, all-pad chunks among them), hidden 1024, the
record path without host lengths and a batch of several micro-batches per lane -- in the three arithmetic modes, and RoBERTa + head
also with ANCE_CLS_TAIL=0 and with ANCE_ENCODER_STREAMS=1.  Weights: 2 layers, oracle.encoder_ref.random_state_dict, fixed seeds."""
import argparse
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MODES = ("split", "fp16", "fp32")


def fingerprints():
    import numpy as np
    import torch
    from ance_amd.encoder import ARCH_BERT, ARCH_ROBERTA, ARCH_SEED, Encoder
    from oracle import encoder_ref, synth

    out = {}

    def records(seed, lens, L, vocab):
        lens = np.asarray(lens, dtype=np.int64)
        return synth.make_records(np.random.default_rng(seed), len(lens), L, lens, vocab=vocab), lens.astype(np.int32)

    def run(name, sd, arch, prefix, head, ids, lens, L, env=None, n_chunks=1, max_tokens=2048, as_records=False):
        for mode in MODES:
            for k, v in (env or {}).items():
                os.environ[k] = v
            try:
                enc = Encoder(sd, arch, prefix, head, max_seq_len=L // n_chunks, max_tokens=max_tokens, device="cuda:0", precision=mode)
            finally:
                for k in env or {}:
                    del os.environ[k]
            if as_records:  # [n, 1 + L] int32 rows with the big-endian length header; the lengths are read back from the device
                rec = np.concatenate([lens.astype(">i4").view(np.int32)[:, None], ids], axis=1)
                got = enc.encode_records(torch.from_numpy(np.ascontiguousarray(rec)).cuda(), n_chunks=n_chunks)
            else:
                got = enc.encode_ids(torch.from_numpy(ids).cuda(), torch.from_numpy(lens).cuda(), n_chunks=n_chunks, h_lens=lens)
            enc.check_range(sync=True)
            got = got.cpu().numpy()
            assert np.isfinite(got).all(), name
            out["%s/%s" % (name, mode)] = hashlib.sha256(np.ascontiguousarray(got).tobytes()).hexdigest()
            del enc

    V = 2000
    sd = encoder_ref.random_state_dict(seed=3, n_layers=2, vocab=V, ln_jitter=0.1)
    ids, lens = records(11, [1, 2, 7, 8, 9, 31, 32, 33, 64, 65, 96, 97, 127, 128, 128, 100, 50, 17, 5, 128, 3, 77, 120, 40], 128, V)
    run("roberta_head", sd, ARCH_ROBERTA, "roberta.", True, ids, lens, 128)
    run("roberta_head_cls_tail_0", sd, ARCH_ROBERTA, "roberta.", True, ids, lens, 128, env={"ANCE_CLS_TAIL": "0"})
    run("roberta_head_streams_1", sd, ARCH_ROBERTA, "roberta.", True, ids, lens, 128, env={"ANCE_ENCODER_STREAMS": "1"})
    run("records_no_h_lens", sd, ARCH_ROBERTA, "roberta.", True, ids, lens, 128, as_records=True)

    sd_b = encoder_ref.random_state_dict(kind="bert", seed=4, n_layers=2, vocab=V, head=False, prefixes=("bert.",), ln_jitter=0.1)
    ids_b = np.where(ids == synth.PAD, 0, ids).astype(np.int32)  # BERT pads with id 0
    run("bert_no_head", sd_b, ARCH_BERT, "bert.", False, ids_b, lens, 128)

    ids_s = ids.copy()  # interior pad ids: every fifth token from the third on, inside the length as well
    ids_s[:, 3::5] = synth.PAD
    run("seed_interior_pads", sd, ARCH_SEED, "roberta.", True, ids_s, lens, 128)

    ids_m, lens_m = records(12, [256, 255, 193, 192, 129, 128, 65, 64, 63, 1, 0, 200, 30, 256], 256, V)
    run("maxp_4_chunks", sd, ARCH_ROBERTA, "roberta.", True, ids_m, lens_m, 256, n_chunks=4)

    sd_l = encoder_ref.random_state_dict(seed=5, n_layers=2, hidden=1024, inter=4096, vocab=V, ln_jitter=0.1)
    run("hidden_1024", sd_l, ARCH_ROBERTA, "roberta.", True, ids, lens, 128)

    rng = np.random.default_rng(13)  # 400 sequences, ~26,000 tokens, 2,048 per micro-batch: six or more micro-batches on each lane
    ids_x, lens_x = records(14, synth.lognormal_lengths(rng, 400, 60, 0.5, 1, 128), 128, V)
    run("many_micro_batches", sd, ARCH_ROBERTA, "roberta.", True, ids_x, lens_x, 128)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--libs", nargs="+", help="libraries to compare (ANCE_AMD_LIB of one fresh child process each)")
    ap.add_argument("--out", help="write the result as JSON")
    a = ap.parse_args()
    if not a.libs:
        res = fingerprints()
    else:
        res = {}
        for lib in a.libs:
            env = dict(os.environ, ANCE_AMD_LIB=os.path.abspath(lib))
            p = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, stdout=subprocess.PIPE, text=True, timeout=900)
            if p.returncode != 0:
                sys.exit("fingerprint run of %s failed (%d)" % (lib, p.returncode))
            res[lib] = json.loads(p.stdout.strip().splitlines()[-1])
        first = res[a.libs[0]]
        res["unequal"] = sorted(k for lib in a.libs[1:] for k in set(first) | set(res[lib]) if first.get(k) != res[lib].get(k))
    text = json.dumps(res, indent=1, sort_keys=True) if a.out else json.dumps(res, sort_keys=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text)
    if a.libs and res["unequal"]:
        sys.exit(1)


if __name__ == "__main__":
    main()
