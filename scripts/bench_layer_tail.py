"""Times the row-wise seams of a BertLayer and the whole layer with device events, in ONE process, the variants alternated --rounds
times (each round times every variant once: --steps calls after --warmup), forward + backward, fp32, training mode, dropout 0.1:
  tail    LayerNorm(dropout(x + bias) + input_tensor)      eager torch  against  ance_amd.layers.dropout_add_layer_norm
  gelu    gelu(x + bias), the erf form                     eager torch  against  ance_amd.layers.bias_gelu
  layer   transformers 2.3.0's BertLayer restated in eager torch (six Linear, the eager attention expression, two dropouts + LayerNorm,
          the erf GELU)                                    against  ance_amd.layers.BertLayer (the same six matmuls, everything else fused)
Shapes: 8 x 512 and 32 x 128 rows (all sequences full), hidden 768 (12 heads, FFN 3072) and 1024 (16 heads, FFN 4096).
Per variant: the median over the rounds of the window medians, the spread over the rounds, torch.cuda.max_memory_allocated over one
forward + backward above what was allocated before it, the launches and the summed device time of one traced forward + backward (the
event times of a single seam at these sizes are bounded by the host on both sides), and for the seams the bytes the expressions have to move (12 B/element forward
for the fused tail: x, residual in, y out) over the event time.  Writes one JSON object (--out)."""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

P_DROP = 0.1
SHAPES = {"8x512": (8, 512), "32x128": (32, 128)}
WIDTHS = {768: (12, 3072), 1024: (16, 4096)}


def time_calls(fn, steps, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return statistics.median(a.elapsed_time(b) for a, b in ev)


def peak_bytes(fn):
    import torch
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return int(torch.cuda.max_memory_allocated() - base)


def traced(fn):
    """Kernel launches, copies and the summed device time of one forward + backward, from torch.profiler (after the timing): what the
    GPU itself spends, where the event times of so small a call are bounded by the host."""
    import torch
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA, ProfilerActivity.CPU]) as prof:
        fn()
        torch.cuda.synchronize()
    kernels = copies = 0
    device_us = 0.0
    for e in prof.events():
        if e.device_type == torch.autograd.DeviceType.CUDA:
            if "memcpy" in e.name.lower() or "memset" in e.name.lower():
                copies += 1
            else:
                kernels += 1
            device_us += float(getattr(e, "device_time", getattr(e, "cuda_time", 0.0)))
    return dict(kernels=kernels, copies_and_memsets=copies, device_time_us=round(device_us, 1))


def eager_gelu(t):
    import torch
    return t * 0.5 * (1.0 + torch.erf(t / math.sqrt(2.0)))


class EagerBertLayer:
    """transformers 2.3.0's BertLayer.forward on the parameters of an ance_amd.layers.BertLayer (shared, not copied)."""

    def __init__(self, layer):
        self.m = layer

    def __call__(self, hs, add_mask):
        import torch
        F = torch.nn.functional
        m, nh = self.m, self.m.num_attention_heads
        B, L, H = hs.shape

        def tfs(x):
            return x.view(B, L, nh, 64).permute(0, 2, 1, 3)

        a = m.attention
        q, k, v = a.self.query(hs), a.self.key(hs), a.self.value(hs)
        s = torch.matmul(tfs(q), tfs(k).transpose(-1, -2)) / math.sqrt(64) + add_mask
        p = F.dropout(torch.softmax(s, dim=-1), m.attention_probs_dropout_prob, True)
        ctx = torch.matmul(p, tfs(v)).permute(0, 2, 1, 3).contiguous().view(B, L, H)
        h = a.output.LayerNorm(F.dropout(a.output.dense(ctx), m.hidden_dropout_prob, True) + hs)
        t = eager_gelu(m.intermediate.dense(h))
        return m.output.LayerNorm(F.dropout(m.output.dense(t), m.hidden_dropout_prob, True) + h)


def alternate(variants, rounds, steps, warmup, tag):
    seen = {v: [] for v in variants}
    for _ in range(rounds):
        for name, fn in variants.items():
            seen[name].append(time_calls(fn, steps, warmup))
        print(tag, "round", {k: round(v[-1], 4) for k, v in seen.items()}, flush=True)
    out = {}
    for name, fn in variants.items():
        xs = seen[name]
        out[name] = dict(fwdbwd_ms=dict(median=round(statistics.median(xs), 4), rounds=[round(x, 4) for x in xs], spread=round(max(xs) - min(xs), 4)),
                         peak_bytes_over_the_pair=peak_bytes(fn))
        try:
            out[name]["traced_fwdbwd"] = traced(fn)
        except Exception as e:  # pragma: no cover - depends on the profiler of the torch build
            out[name]["traced_fwdbwd"] = dict(unavailable=repr(e))
    e, f = out["eager"], out["fused"]
    gain = e["fwdbwd_ms"]["median"] - f["fwdbwd_ms"]["median"]
    return dict(variants=out, eager_over_fused_fwdbwd=round(e["fwdbwd_ms"]["median"] / f["fwdbwd_ms"]["median"], 3),
                fused_faster_than_eager_by_more_than_the_spread=bool(gain > max(e["fwdbwd_ms"]["spread"], f["fwdbwd_ms"]["spread"])),
                fused_peak_memory_lower_than_eager=bool(f["peak_bytes_over_the_pair"] < e["peak_bytes_over_the_pair"]))


def bench_shape(B, L, hidden, rounds, steps, warmup):
    import torch
    from ance_amd.layers import BertLayer, bias_gelu, dropout_add_layer_norm
    F = torch.nn.functional
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(1)
    heads, inter = WIDTHS[hidden]
    rows = B * L
    rnd = lambda *s: torch.randn(*s, device=dev, generator=gen)  # noqa: E731
    x, res, dy = rnd(B, L, hidden), rnd(B, L, hidden), rnd(B, L, hidden)
    bias, gamma, beta = (rnd(hidden).requires_grad_(True) for _ in range(3))
    gx, gdy, gbias = rnd(B, L, inter), rnd(B, L, inter), rnd(inter).requires_grad_(True)
    res_out = {}

    def leaves(*ts):
        return [t.detach().requires_grad_(True) for t in ts]

    def tail_eager():
        a, r = leaves(x, res)
        F.layer_norm(F.dropout(a + bias, P_DROP, True) + r, (hidden,), gamma, beta, 1e-5).backward(dy)

    def tail_fused():
        a, r = leaves(x, res)
        dropout_add_layer_norm(a, bias, r, gamma, beta, 1e-5, P_DROP, True).backward(dy)

    def gelu_eager():
        (a,) = leaves(gx)
        eager_gelu(a + gbias).backward(gdy)

    def gelu_fused():
        (a,) = leaves(gx)
        bias_gelu(a, gbias).backward(gdy)

    r = alternate(dict(eager=tail_eager, fused=tail_fused), rounds, steps, warmup, "tail %dx%d H%d" % (B, L, hidden))
    # fused: forward reads x, res, writes y (12 B/element); backward reads x, res, dy, writes dx, dres (20 B/element)
    r["fused_bytes_moved"] = 32 * rows * hidden
    r["fused_tb_per_s"] = round(r["fused_bytes_moved"] / (r["variants"]["fused"]["fwdbwd_ms"]["median"] * 1e-3) / 1e12, 3)
    res_out["tail"] = r
    r = alternate(dict(eager=gelu_eager, fused=gelu_fused), rounds, steps, warmup, "gelu %dx%d N%d" % (B, L, inter))
    # fused: forward reads x, writes y (8 B/element); backward reads x, dy, writes dx (12 B/element)
    r["fused_bytes_moved"] = 20 * rows * inter
    r["fused_tb_per_s"] = round(r["fused_bytes_moved"] / (r["variants"]["fused"]["fwdbwd_ms"]["median"] * 1e-3) / 1e12, 3)
    res_out["gelu"] = r

    layer = BertLayer(hidden, heads, inter, 1e-5, P_DROP, P_DROP).to(dev).train()
    eager_layer = EagerBertLayer(layer)
    hs, dout = rnd(B, L, hidden), rnd(B, L, hidden)
    lens = torch.full((B,), L, dtype=torch.int32, device=dev)
    add_mask = torch.zeros(B, 1, 1, L, device=dev)

    def layer_eager():
        (a,) = leaves(hs)
        eager_layer(a, add_mask).backward(dout)
        layer.zero_grad(set_to_none=True)

    def layer_fused():
        (a,) = leaves(hs)
        layer(a, lens).backward(dout)
        layer.zero_grad(set_to_none=True)

    res_out["layer"] = alternate(dict(eager=layer_eager, fused=layer_fused), rounds, steps, warmup, "layer %dx%d H%d" % (B, L, hidden))
    return res_out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13_layer_tail.json"))
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "bench_layer_tail.py times the GPU; there is no CPU measurement"
    from ance_amd import attention
    attention.manual_seed(0)
    out = dict(what="the row-wise seams of one BertLayer and the whole layer, forward + backward, fp32, training mode, dropout 0.1, all "
                    "sequences full; eager torch against ance_amd.layers",
               device=torch.cuda.get_device_name(0), torch=torch.__version__,
               timing=dict(rounds=a.rounds, calls_per_window=a.steps, warmup_calls=a.warmup))
    for sname, (B, L) in SHAPES.items():
        for hidden in WIDTHS:
            key = "%s_h%d" % (sname, hidden)
            out[key] = bench_shape(B, L, hidden, a.rounds, a.steps, a.warmup)
            print(key, json.dumps(out[key]), flush=True)
            torch.cuda.empty_cache()
    if a.out != "-":
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
