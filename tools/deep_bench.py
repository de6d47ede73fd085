#!/usr/bin/env python3
"""Times of the DEEP quotient codeword (twenty_first_amd.deep.quotient) against two yardsticks taken in the same process.

For n = 2^20 rows, (k1, k3) in {(128, 32), (16, 4)} main / aux columns and 1 and 2 out-of-domain points, on device buffers filled
by tf_debug_fill_random_dev, timed with device events around one call (median over --reps after --warmup):
    fused_ms        one deep.quotient call: the per-point constants, then one pass over both tables
    lincomb_ms      tf_poly_linear_combination_dev over the same columns under XFieldElement weights, one call per table and point:
                    the same products and no division; the table is read once PER POINT, the fused call reads it once
    composed_ms     the composition of existing calls that gives the same codeword, per point: the two linear combinations and their
                    sum, the broadcast subtraction of C_p (torch), tf_powers_dev for the domain, the broadcast subtraction of z_p
                    (torch), tf_batch_inversion_xfe_dev, a Hadamard product, and the sum over the points.  C_p = sum_c w v is formed
                    outside the timed region.  Its result is compared with the fused call's, word for word, before anything is timed.
    ratios          lincomb_ms / fused_ms and composed_ms / fused_ms (above 1: the fused call is faster)
No time is a pass condition; the record (profiles/deep_bench.json) is what DESIGN 7.8 quotes.
usage: python tools/deep_bench.py [--reps 10] [--warmup 3] [--out profiles/deep_bench.json]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import twenty_first_amd as tf  # noqa: E402

P = (1 << 64) - (1 << 32) + 1
LOG_N = 20
SHAPES = [(128, 32), (16, 4)]
POINTS = [1, 2]
MIN64 = -(1 << 63)
P_I64 = P - (1 << 64)


def to_raw(v):
    return v * (1 << 64) % P


def timed(call, reps, warmup):
    for _ in range(warmup):
        call()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        call()
        stop.record()
        stop.synchronize()
        times.append(start.elapsed_time(stop))
    return statistics.median(times), min(times), max(times)


def random_words(count, seed):
    t = torch.empty(count, dtype=torch.int64, device="cuda")
    tf.device.fill_random(t, seed)
    return t


def sub_mod(a, b):
    """a - b in the field on canonical raw words held in int64 tensors (the one step the library cannot express on codewords)"""
    t = a - b
    return torch.where((a ^ MIN64) < (b ^ MIN64), t + P_I64, t)


def xfe_mul(a, b):
    c = [0] * 5
    for i in range(3):
        for j in range(3):
            c[i + j] += a[i] * b[j]
    return [(c[0] - c[3]) % P, (c[1] + c[3] - c[4]) % P, (c[2] + c[4]) % P]


def consts(weights, values, n_points, k):
    """C_p = sum_c w[p][c] v[p][c] as raw words, on the host (outside every timed region)"""
    r_inv = pow(1 << 64, P - 2, P)
    w = [int(x) * r_inv % P for x in weights.cpu().numpy().view(np.uint64)]
    v = [int(x) * r_inv % P for x in values.cpu().numpy().view(np.uint64)]
    out = []
    for p in range(n_points):
        s = [0, 0, 0]
        for c in range(p * k, (p + 1) * k):
            s = [(x + y) % P for x, y in zip(s, xfe_mul(w[3 * c:3 * c + 3], v[3 * c:3 * c + 3]))]
        out += [to_raw(x) for x in s]
    return torch.from_numpy(np.array(out, dtype=np.uint64).view(np.int64)).cuda()


def measure(reps, warmup):
    n = 1 << LOG_N
    offset, omega = to_raw(7), to_raw(pow(7, (P - 1) // n, P))
    rows = []
    for k1, k3 in SHAPES:
        k = k1 + k3
        main, aux = random_words(k1 * n, 1), random_words(3 * k3 * n, 2)
        for n_points in POINTS:
            points, weights, values = random_words(3 * n_points, 3), random_words(3 * n_points * k, 4), random_words(3 * n_points * k, 5)
            out = torch.empty(3 * n, dtype=torch.int64, device="cuda")
            status = torch.zeros(1, dtype=torch.int32, device="cuda")
            work = torch.empty(tf.deep.workspace(n, k1, k3, n_points) // 8, dtype=torch.int64, device="cuda")
            fused = lambda: tf.deep.quotient(main, aux, n, k1, k3, offset, points, weights, values, out, status, work)  # noqa: E731

            a, b, s, x, den, q = (torch.empty(3 * n, dtype=torch.int64, device="cuda") for _ in range(6))
            xs = torch.empty(n, dtype=torch.int64, device="cuda")
            c_p = consts(weights, values, n_points, k)
            w_of = lambda p: (weights[3 * p * k:3 * (p * k + k1)], weights[3 * (p * k + k1):3 * (p + 1) * k])  # noqa: E731

            def lincomb():
                for p in range(n_points):
                    wm, wa = w_of(p)
                    tf.device.linear_combination(main, n, k1, wm, a, width=1, width_w=3)
                    tf.device.linear_combination(aux, n, k3, wa, b, width=3, width_w=3)

            def composed():
                for p in range(n_points):
                    wm, wa = w_of(p)
                    tf.device.linear_combination(main, n, k1, wm, a, width=1, width_w=3)
                    tf.device.linear_combination(aux, n, k3, wa, b, width=3, width_w=3)
                    tf.device.poly_add(a, n, b, n, s, width=3)
                    num = sub_mod(s.view(n, 3), c_p[3 * p:3 * p + 3])
                    tf.device.powers(offset, omega, xs, width=1)
                    den.view(n, 3).copy_(sub_mod(torch.cat([xs.view(n, 1), torch.zeros(n, 2, dtype=torch.int64, device="cuda")], dim=1), points[3 * p:3 * p + 3]))
                    tf.device.batch_inversion(den, den, width=3, status=status)
                    tf.device.hadamard(num.reshape(-1), den, x if p else q, width=3)
                    if p:
                        tf.device.poly_add(q, n, x, n, q, width=3)

            fused()
            composed()
            torch.cuda.synchronize()
            same = bool(torch.equal(out, q)) and int(status.item()) == 0
            assert same, "the composition of existing calls and the fused call disagree"
            f_ms, f_lo, f_hi = timed(fused, reps, warmup)
            l_ms, l_lo, l_hi = timed(lincomb, reps, warmup)
            c_ms, c_lo, c_hi = timed(composed, reps, warmup)
            table_bytes = (k1 + 3 * k3) * n * 8
            rows.append({"log_n": LOG_N, "k1": k1, "k3": k3, "n_points": n_points, "plan": tf.deep.plan(n, k1, k3, n_points)._asdict(),
                         "table_bytes": table_bytes, "composition_equals_fused": same,
                         "fused_ms": f_ms, "fused_ms_min": f_lo, "fused_ms_max": f_hi, "fused_table_bytes_per_s": table_bytes / (f_ms * 1e-3),
                         "lincomb_ms": l_ms, "lincomb_ms_min": l_lo, "lincomb_ms_max": l_hi,
                         "composed_ms": c_ms, "composed_ms_min": c_lo, "composed_ms_max": c_hi,
                         "lincomb_over_fused": l_ms / f_ms, "composed_over_fused": c_ms / f_ms})
            print(f"k1={k1:3d} k3={k3:2d} points={n_points}: fused {f_ms:8.4f} ms ({table_bytes / (f_ms * 1e-3) / 1e9:7.1f} GB/s of table) | lincomb {l_ms:8.4f} ms "
                  f"(x{l_ms / f_ms:5.2f}) | composed {c_ms:8.4f} ms (x{c_ms / f_ms:5.2f})", flush=True)
            del a, b, s, x, den, q, xs, out, work
        del main, aux
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "deep_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("deep_bench.py needs a GPU: there is nothing to time without one")
    rec = {"tool": "tools/deep_bench.py", "device": torch.cuda.get_device_name(0),
           "library": {"tf_version": int(tf.lib().tf_version()), "source_hash": tf.lib().tf_source_hash().decode()},
           "reps": args.reps, "warmup": args.warmup, "timing": "device events around one call, median",
           "yardsticks": {"lincomb": "tf_poly_linear_combination_dev per table and point (XFieldElement weights): the same products, no division",
                          "composed": "per point: two linear combinations, poly_add, C_p subtracted with torch, tf_powers_dev, z_p subtracted with torch, "
                                      "tf_batch_inversion_xfe_dev, hadamard; poly_add over the points; C_p formed outside the timed region"},
           "rows": measure(args.reps, args.warmup)}
    json.dump(rec, open(args.out, "w"), indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
