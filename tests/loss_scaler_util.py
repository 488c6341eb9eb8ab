"""What the loss scaler's tests share: a restatement of the scale's update rule in Python (pinned to torch._amp_update_scale_ by
tests/test_loss_scaler.py, bit for bit), the table of cases both the CPU and the GPU test walk, and the schedule of scales that
rule gives for a known sequence of overflows."""
import math
import struct

import numpy as np

NAN = float("nan")


def f32(x):
    """x rounded to fp32, as a Python float."""
    return float(np.float32(x))


def update_rule(scale, tracker, flag, growth_factor, backoff_factor, growth_interval):
    """(scale, tracker) after one update: scale an fp32 value held in a Python float, tracker an int, flag the fp32 overflow flag.
    A flag that is not 0 (NaN included) backs off and resets the tracker; otherwise the tracker counts, and at the interval the
    scale grows -- unless the grown scale is not finite in fp32 -- and the tracker restarts.  Every product is formed in fp64 from
    the fp32 scale and the fp64 factor and rounded once to fp32."""
    if flag != 0.0:   # NaN != 0.0 is True
        with np.errstate(over="ignore"):
            return f32(np.float64(scale) * np.float64(backoff_factor)), 0
    n = tracker + 1
    if n == growth_interval:
        with np.errstate(over="ignore"):
            grown = f32(np.float64(scale) * np.float64(growth_factor))
        return (grown if math.isfinite(grown) else scale), 0
    return scale, n


def cases():
    """[(scale, tracker, flag, growth_factor, backoff_factor, growth_interval)]: flags 0 / 1 / 7 / NaN; the tracker two and one
    below the interval; scales 2^16, 3.0 and 2^127 (whose growth overflows fp32: the scale is kept); factors 2 / 0.5 and 1.1 / 0.3;
    interval 1 as well."""
    out = []
    for scale in (65536.0, 3.0, 2.0 ** 127):
        for gf, bf in ((2.0, 0.5), (1.1, 0.3)):
            for flag in (0.0, 1.0, 7.0, NAN):
                for interval in (5, 1):
                    for tracker in sorted({max(interval - 2, 0), interval - 1}):
                        out.append((scale, tracker, flag, gf, bf, interval))
    return out


def bits32(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def schedule(init_scale, overflow_steps, n_steps, growth_factor=2.0, backoff_factor=0.5, growth_interval=2):
    """([the scale after each step], the tracker at the end) by update_rule, for overflows at the steps of overflow_steps."""
    s, t, out = f32(init_scale), 0, []
    for k in range(n_steps):
        s, t = update_rule(s, t, 1.0 if k in overflow_steps else 0.0, growth_factor, backoff_factor, growth_interval)
        out.append(s)
    return out, t
