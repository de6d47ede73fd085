#!/usr/bin/env python3
"""Two measurements behind DESIGN 7.4, both at n = 2^20 elements, inputs from tf_debug_fill_random_dev, every figure the median over
--reps steps of ten calls between two HIP events, per call, after --warmup calls:

  fused against composed   tf_get_colinear_y_dev for the width pairs (1, 1), (3, 3), (1, 3) against the same result composed from
                           the calls a user had before it: tf_poly_sub_dev (dx, dy), tf_poly_scalar_mul_dev (dy * p2x),
                           tf_hadamard_*_dev (dy * x0, dx * y0), tf_poly_sub_dev, tf_poly_add_dev, tf_batch_inversion_*_dev_async
                           (dx^-1) and tf_hadamard_*_dev: nine launches and five full-length temporaries.  The composition has no
                           mixed-field form: for (1, 3) it runs over the lifted x-coordinates (the lift itself is not timed).
                           The composition is the baseline; its words must be the fused call's.
  table against general    tf_mod_pow_dev with one base and 32-bit exponents (the broadcast-base route: a table of repeated squares
                           per workgroup) against the general route on the same inputs, the base written out n times (which
                           costs that route one more read of 8 or 24 bytes per element).  The words must agree.

The two sides of each comparison alternate within one process.
usage: field_points_bench.py [--reps 20] [--warmup 3] [--log-n 20] [--out profiles/field_points_bench.json]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)


CALLS = 10  # calls per timed step: one call at 2^20 elements is tens of microseconds, too close to the events' own resolution


def _timed(fn):
    """ms per call of a step of CALLS calls between two HIP events"""
    import torch

    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(CALLS):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / CALLS


def _alternate(a, b, warmup, reps):
    import torch

    for _ in range(warmup):
        a()
        b()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(reps):
        ta.append(_timed(a))
        tb.append(_timed(b))
    return statistics.median(ta), statistics.median(tb)


def colinear(tf, n, wx, wy, warmup, reps):
    import torch

    dev = tf.device

    def rnd(words, seed):
        t = torch.empty(words, dtype=torch.int64, device="cuda")
        dev.fill_random(t, seed)
        return t

    x0, x1 = rnd(n * wx, 0xC0 + wx), rnd(n * wx, 0xC1 + wx)
    y0, y1 = rnd(n * wy, 0xC2 + wy), rnd(n * wy, 0xC3 + wy)
    p2x = rnd(wy, 0xC4)
    torch.cuda.synchronize()
    p2x_host = p2x.cpu().numpy().view("uint64")  # (tf_poly_scalar_mul_dev takes its scalar from the host)
    st = torch.zeros(1, dtype=torch.int32, device="cuda")
    fused = torch.empty(n * wy, dtype=torch.int64, device="cuda")
    # the composition works in one width: the lifted x-coordinates for (1, 3)
    if wx != wy:
        lx0, lx1 = torch.zeros(n * wy, dtype=torch.int64, device="cuda"), torch.zeros(n * wy, dtype=torch.int64, device="cuda")
        lx0[::wy], lx1[::wy] = x0, x1
    else:
        lx0, lx1 = x0, x1
    dx, dy, a, b, dxi = (torch.empty(n * wy, dtype=torch.int64, device="cuda") for _ in range(5))
    composed = torch.empty(n * wy, dtype=torch.int64, device="cuda")

    def run_fused():
        dev.get_colinear_y(x0, y0, x1, y1, p2x, fused, width_x=wx, width_y=wy, status=st)

    def run_composed():
        dev.poly_sub(lx0, n, lx1, n, dx, width=wy)
        dev.poly_sub(y0, n, y1, n, dy, width=wy)
        dev.poly_scalar_mul(dy, n, p2x_host, a, width=wy, width_s=wy)  # dy * p2x
        dev.hadamard(dy, lx0, b, width=wy)                              # dy * x0
        dev.poly_sub(a, n, b, n, a, width=wy)
        dev.hadamard(dx, y0, b, width=wy)                               # dx * y0
        dev.poly_add(a, n, b, n, a, width=wy)
        dev.batch_inversion(dx, dxi, width=wy, status=st)
        dev.hadamard(a, dxi, composed, width=wy)

    t_fused, t_comp = _alternate(run_fused, run_composed, warmup, reps)
    torch.cuda.synchronize()
    assert int(st.item()) == 0
    return {"width_x": wx, "width_y": wy, "n": n, "fused_ms": t_fused, "composed_ms": t_comp, "composed_launches": 9,
            "speedup": t_comp / t_fused, "same_words": bool(torch.equal(fused, composed))}


def mod_pow(tf, n, w, warmup, reps):
    import torch

    dev = tf.device
    base = torch.empty(w, dtype=torch.int64, device="cuda")
    dev.fill_random(base, 0xD0 + w)
    bases = base.repeat(n)
    exps = torch.empty(n, dtype=torch.int64, device="cuda")
    dev.fill_random(exps, 0xD1)
    exps &= 0xFFFFFFFF
    out_t, out_g = torch.empty(n * w, dtype=torch.int64, device="cuda"), torch.empty(n * w, dtype=torch.int64, device="cuda")
    t_table, t_general = _alternate(lambda: dev.mod_pow(base, exps, out_t, width=w), lambda: dev.mod_pow(bases, exps, out_g, width=w),
                                    warmup, reps)
    torch.cuda.synchronize()
    return {"width": w, "n": n, "exponent_bits": 32, "table_ms": t_table, "general_ms": t_general, "speedup": t_general / t_table,
            "same_words": bool(torch.equal(out_t, out_g))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--log-n", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch

    import twenty_first_amd as tf

    if not torch.cuda.is_available() or tf.lib().tf_device_count() == 0:
        raise SystemExit("field_points_bench.py needs a GPU: a time from anything else says nothing")
    n = 1 << args.log_n
    rec = {"what": "get_colinear_y fused against composed, mod_pow table against general route; median ms per call of warm steps between HIP events",
           "source_hash": tf.lib().tf_source_hash().decode(), "reps": args.reps, "calls_per_step": CALLS, "warmup": args.warmup,
           "get_colinear_y": [colinear(tf, n, wx, wy, args.warmup, args.reps) for wx, wy in ((1, 1), (3, 3), (1, 3))],
           "mod_pow": [mod_pow(tf, n, w, args.warmup, args.reps) for w in (1, 3)]}
    text = json.dumps(rec, indent=1)
    if args.out:
        open(args.out, "w").write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
