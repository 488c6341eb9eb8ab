#!/usr/bin/env python
"""SHA-256 fingerprints of everything the trainers' attention calls write (ance_amd.attention -> csrc/attention_train_kernels.h behind
attention_train.hip and attention_train_half.hip, csrc/attention_row0.hip): the check that a restructuring of the kernels or of their
host front end moved no bit.

    python scripts/attention_fingerprint.py                                  # the library in the tree (or ANCE_AMD_LIB)
    python scripts/attention_fingerprint.py --libs PARENT.so NEW.so --out F  # one fresh child process per library; exit 1 unless they agree

Per call the raw bytes of ctx, lse, dq, dk, dv (first-row calls: ctx0, dq0, dk, dv) are hashed; a NaN in any of them fails the run.
Cases, in fp32, fp16 and bf16:
  padded   L = 96, lengths (0, 1, 31, 32, 33, 64, 65, 96): an empty sequence, a single key, both sides of the 32-row block edge and of
           the 64-row tile edge, a full row; 12 heads (hidden 768), and once more with 16 heads (hidden 1024);
  packed   the same lengths concatenated under max_seq_len 96, then one sequence of 120 rows (cut at 96) and 5 rows no sequence covers;
  long     L = 512, lengths (512, 257), 12 heads: the longest walk;
each with q, k, v as three contiguous tensors and as the thirds of one fused [.., 3H] buffer, and with dropout off, p = 0.1 under the
host pair after manual_seed, and p = 0.1 under the device stream (dropout_state.to_device()): the forward and backward of one call,
then of a second one, so that the offset moves.
  first-row  attention_first_row at L = 96 with the same lengths, dropout off and under the host pair.
Inputs: numpy.random.RandomState with fixed seeds, q, k, v ~ N(0, 1) and dctx ~ N(0, 0.1) as in tests/attention_train_util.py, cast to
the dtype.  Every row of every output is written by the kernels or zeroed by the wrapper (the packed form), so whole buffers are hashed."""
import argparse
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LENS = (0, 1, 31, 32, 33, 64, 65, 96)
P_DROP = 0.1
SEED = 20240
# name -> (form, lengths, L or max_seq_len, n_heads)
CASES = {
    "padded96/h12": ("padded", LENS, 96, 12),
    "padded96/h16": ("padded", LENS, 96, 16),
    "packed96/h12": ("packed", LENS + (120,), 96, 12),
    "padded512/h12": ("padded", (512, 257), 512, 12),
}
PACKED_TAIL = 5   # rows behind the last sequence


def fingerprints():
    import numpy as np
    import torch
    from ance_amd import attention as A

    dev = torch.device("cuda", 0)
    dtypes = {"fp32": torch.float32, "fp16": torch.float16, "bf16": torch.bfloat16}
    out = {}

    def record(name, **tensors):
        for what, t in tensors.items():
            assert not bool(torch.isnan(t.float()).any()), "%s/%s: NaN" % (name, what)
            out["%s/%s" % (name, what)] = hashlib.sha256(t.detach().contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()

    def normal(seed, shape, std, dtype):
        return torch.from_numpy((np.random.RandomState(seed).standard_normal(shape) * std).astype(np.float32)).to(dev).to(dtype)

    def leaves(seed, shape, dtype, fused):
        """q, k, v as autograd inputs: (the leaves to differentiate, q, k, v, the gradients of q, k, v from the leaves')."""
        q, k, v = (normal(seed + i, shape, 1.0, dtype) for i in range(3))
        if not fused:
            ts = [t.requires_grad_() for t in (q, k, v)]
            return ts, ts[0], ts[1], ts[2], lambda gs: gs
        H = shape[-1]
        buf = torch.cat([q, k, v], dim=-1).requires_grad_()
        return [buf], buf[..., :H], buf[..., H:2 * H], buf[..., 2 * H:], lambda gs: [gs[0][..., i * H:(i + 1) * H] for i in range(3)]

    def with_dropout(mode, body):
        """body(p, call) twice under one mode: off, the host pair, or the device stream."""
        A.manual_seed(SEED)
        if mode == "device":
            A.dropout_state.to_device(dev)
        for call in range(2):
            body(0.0 if mode == "off" else P_DROP, call)
        if mode == "device":
            A.dropout_state.to_host(dev)

    for pname, dtype in dtypes.items():
        precision = "fp32" if dtype == torch.float32 else "half"
        for cname, (form, lens, L, n_heads) in CASES.items():
            H = 64 * n_heads
            d_lens = torch.tensor(lens, dtype=torch.int32, device=dev)
            if form == "padded":
                shape = (len(lens), L, H)
            else:
                off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
                shape = (int(off[-1]) + PACKED_TAIL, H)
                d_off = torch.from_numpy(off).to(dev)
            for fused in (False, True):
                for mode in ("off", "host", "device"):
                    def body(p, call):
                        ins, q, k, v, split = leaves(100 + call, shape, dtype, fused)
                        if form == "padded":
                            ctx, lse = A._padded(q, k, v, d_lens, n_heads, p, True, precision)
                        else:
                            ctx, lse = A._packed(q, k, v, d_off, L, n_heads, p, True, precision)
                        dq, dk, dv = split(torch.autograd.grad(ctx, ins, normal(200 + call, shape, 0.1, dtype)))
                        torch.cuda.synchronize()
                        record("%s/%s/%s/%s/call%d" % (pname, cname, "fused" if fused else "separate", mode, call),
                               ctx=ctx, lse=lse, dq=dq, dk=dk, dv=dv)
                    with_dropout(mode, body)
        # the first-row core
        L, n_heads, H = 96, 12, 768
        d_lens = torch.tensor(LENS, dtype=torch.int32, device=dev)
        for mode in ("off", "host"):
            def body(p, call):
                q0 = normal(300 + call, (len(LENS), H), 1.0, dtype).requires_grad_()
                k, v = (normal(310 + 10 * call + i, (len(LENS), L, H), 1.0, dtype).requires_grad_() for i in range(2))
                ctx0 = A.attention_first_row(q0, k, v, d_lens, n_heads, p, True, precision)
                dq0, dk, dv = torch.autograd.grad(ctx0, [q0, k, v], normal(400 + call, (len(LENS), H), 0.1, dtype))
                torch.cuda.synchronize()
                record("%s/first_row96/h12/%s/call%d" % (pname, mode, call), ctx0=ctx0, dq0=dq0, dk=dk, dv=dv)
            with_dropout(mode, body)
    return dict(hashes=out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--libs", nargs="+", help="PARENT.so NEW.so ...: ANCE_AMD_LIB of one fresh child process each")
    ap.add_argument("--out", help="write the result as JSON")
    ap.add_argument("--timeout", type=int, default=300, help="seconds each child process may take")
    a = ap.parse_args()
    if not a.libs:
        res = fingerprints()
    else:
        got = {}
        for lib in a.libs:
            env = dict(os.environ, ANCE_AMD_LIB=os.path.abspath(lib))
            p = subprocess.run(["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__)], env=env,
                               stdout=subprocess.PIPE, text=True)
            if p.returncode != 0:
                sys.exit("fingerprint run of %s failed (%d)" % (lib, p.returncode))   # nothing more is started after a failure
            got[lib] = json.loads(p.stdout.strip().splitlines()[-1])
        first = got[a.libs[0]]
        # the first library's hashes in full; of the others only what differs
        res = dict(libs=a.libs, n_hashes=len(first["hashes"]), hashes=first["hashes"])
        res["unequal"] = {lib: {k: got[lib]["hashes"].get(k) for k in sorted(set(first["hashes"]) | set(got[lib]["hashes"]))
                                if first["hashes"].get(k) != got[lib]["hashes"].get(k)} for lib in a.libs[1:]}
    text = json.dumps(res, indent=1, sort_keys=True) if a.out else json.dumps(res, sort_keys=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    print(text if not a.out else "%d hashes; unequal: %s" % (len(res["hashes"]), res.get("unequal")))
    if a.libs and any(res["unequal"].values()):
        sys.exit(1)


if __name__ == "__main__":
    main()
