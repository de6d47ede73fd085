#!/usr/bin/env python3
"""Division with remainder and the power-series inverse on the GPU (tf_poly_divide_*_dev, tf_poly_fps_inverse_newton_*_dev) at the
shapes of the issue that introduced them:
  S1 balanced BFE 2^20 / 2^19 + 1    S2 long numerator, short modulus BFE 2^20 / 257    S3 256 x 2^16 over one 2^12 + 1 (BFE)
  S4 balanced XFE 2^18 / 2^17 + 1    S5 latency BFE 1024 / 33                          S6 formal_power_series_inverse_newton, d = 256,
                                                                                         precision 1024 (BFE)
For every shape: `ms` (median of --reps calls between HIP events, warmed shape), the parity of the words against the identity
a == q b + r (oracle.poly_mul; S6: the recurrence over oracle.poly_mul), and the oracle's long division on one host core where its
estimated time (k m operations, rate measured in this run) stays under 10 s, "not run" otherwise.
  --trace: a short run (one warm-up and two timed calls per shape, synchronised) for `rocprofv3 --kernel-trace --stats`;
  --merge REC --kernels DIR: no GPU; add to the record REC of a timing run, per shape, the launches per call and the kernel time of
             its phases (Newton, quotient, remainder) read from the --trace run's kernel trace in DIR.
usage: poly_divide_bench.py [--reps 20] [--out FILE] [--trace] | --merge REC --kernels DIR [--out FILE]"""
import argparse
import csv
import glob
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

P = (1 << 64) - (1 << 32) + 1
SHAPES = [("S1 balanced", 1, 1 << 20, (1 << 19) + 1, 1), ("S2 long numerator, short modulus", 1, 1 << 20, 257, 1),
          ("S3 many over one zerofier", 1, 1 << 16, (1 << 12) + 1, 256), ("S4 balanced", 3, 1 << 18, (1 << 17) + 1, 1),
          ("S5 latency", 1, 1024, 33, 1)]
FPS = ("S6 fps_inverse_newton", 1, 257, 1024)  # (name, width, nf = d + 1, precision)


def fadd(x, y):
    s = x + y
    s = np.where(s < x, s + np.uint64(0xFFFFFFFF), s)
    return np.where(s >= np.uint64(P), s - np.uint64(P), s)


def identity(oracle, a, b, q, r, w):
    prod = oracle.poly_mul(q, b, width=w)
    lhs = np.zeros(max(a.size, prod.size), dtype=np.uint64)
    lhs[:prod.size] = prod
    lhs[:r.size] = fadd(lhs[:r.size], r)
    return np.array_equal(lhs[:a.size], a) and not lhs[a.size:].any()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--kernels", default=None)
    ap.add_argument("--merge", default=None)
    args = ap.parse_args()
    if args.merge:
        rec = json.load(open(args.merge))
        add_kernel_breakdown(rec, args.kernels)
        rec["kernel_trace"] = "rocprofv3 --kernel-trace --stats -- python tools/poly_divide_bench.py --trace (a run of its own)"
        text = json.dumps(rec, indent=1)
        if args.out:
            open(args.out, "w").write(text + "\n")
        print(text)
        return
    import torch

    import twenty_first_amd as tf
    from oracle import tfo

    torch.cuda.set_device(0)
    cuda = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.int64)).cuda()  # noqa: E731
    host = lambda t: t.cpu().numpy().view(np.uint64)  # noqa: E731
    reps = 2 if args.trace else args.reps
    # the oracle's long division rate on one core (k m multiply-subtracts per second), measured here
    a0, b0 = tfo.fill_random(1 << 13, 1), tfo.fill_random(1 << 12, 2)
    t0 = time.perf_counter()
    tfo.naive_divide(a0, b0)
    rate = ((1 << 13) - (1 << 12) + 1) * ((1 << 12) - 1) / (time.perf_counter() - t0)
    rec = {"tool": "tools/poly_divide_bench.py", "library": {"tf_version": tf.lib().tf_version(), "source_hash": tf.lib().tf_source_hash().decode()},
           "device": torch.cuda.get_device_name(0), "reps": reps, "oracle_long_division_ops_per_s": rate, "shapes": []}
    for name, w, na, nb, batch in SHAPES:
        a = tfo.fill_random(batch * na * w, na + nb)
        b = tfo.fill_random(nb * w, nb)
        b[(nb - 1) * w:] = 0
        b[(nb - 1) * w] = tfo.bfe_new(3)
        k, m = na - nb + 1, nb - 1
        da, db = cuda(a), cuda(b)
        dq = torch.zeros(batch * k * w, dtype=torch.int64, device="cuda")
        dr = torch.zeros(batch * m * w, dtype=torch.int64, device="cuda")
        st = torch.zeros(1, dtype=torch.int32, device="cuda")
        call = lambda: tf.device.divide(da, na, db, dq, dr, batch=batch, width=w, status=st)  # noqa: E731
        call()
        torch.cuda.synchronize()
        times = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            torch.cuda.synchronize()
            times.append(e0.elapsed_time(e1))
        q, r = host(dq), host(dr)
        ok = st.item() == 0
        for i in range(min(batch, 2)):
            ok = ok and identity(tfo, a[i * na * w:(i + 1) * na * w], b, q[i * k * w:(i + 1) * k * w], r[i * m * w:(i + 1) * m * w], w)
        entry = {"shape": name, "field": "BFE" if w == 1 else "XFE", "na": na, "nb": nb, "batch": batch, "ms": statistics.median(times),
                 "ms_min": min(times), "parity": "green (a == q b + r)" if ok else "RED"}
        est = batch * k * m / rate
        if args.trace:
            entry["cpu_long_division"] = "not run (--trace)"
        elif w == 3:
            entry["cpu_long_division"] = "not run (the oracle's long division is BFieldElement only)"
        elif est > 10:
            entry["cpu_long_division"] = f"not run (estimated {est:.0f} s on one core)"
        else:
            t0 = time.perf_counter()
            for i in range(batch):
                wq, wr = tfo.naive_divide(a[i * na:(i + 1) * na], b)
            entry["cpu_long_division"] = {"ms": 1e3 * (time.perf_counter() - t0), "cores": 1, "same_words": bool(
                np.array_equal(np.trim_zeros(q[(batch - 1) * k:], "b"), wq) and np.array_equal(np.trim_zeros(r[(batch - 1) * m:], "b"), wr))}
        rec["shapes"].append(entry)
        print(json.dumps(entry), file=sys.stderr)
    name, w, nf, precision = FPS
    f = tfo.fill_random(nf * w, 66)
    f[0], f[(nf - 1) * w] = tfo.bfe_new(5), tfo.bfe_new(7)
    n = tf.lib().tf_poly_fps_inverse_newton_len(nf, precision)
    df, dout = cuda(f), torch.zeros(n * w, dtype=torch.int64, device="cuda")
    st = torch.zeros(1, dtype=torch.int32, device="cuda")
    call = lambda: tf.device.fps_inverse_newton(df, precision, dout, width=w, status=st)  # noqa: E731
    call()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
    t0 = time.perf_counter()
    g = np.array([tfo.bfe_inverse(int(f[0]))], dtype=np.uint64)
    rounds = (1 << (max(precision, 1) - 1).bit_length()).bit_length() - 1
    for _ in range(rounds):
        sq = tfo.poly_mul(tfo.poly_mul(g, g), f)
        neg = np.where(sq == 0, sq, np.uint64(P) - sq)
        neg[:g.size] = fadd(neg[:g.size], fadd(g, g))
        g = neg
    cpu_ms = 1e3 * (time.perf_counter() - t0)
    entry = {"shape": name, "field": "BFE", "d": nf - 1, "precision": precision, "coefficients": n, "ms": statistics.median(times),
             "ms_min": min(times), "parity": "green (the recurrence)" if st.item() == 0 and np.array_equal(host(dout), g) else "RED",
             "cpu_recurrence": {"ms": cpu_ms, "cores": 1, "what": "the same iterates by oracle.poly_mul (NTT products), not the reference's code"}}
    rec["shapes"].append(entry)
    print(json.dumps(entry), file=sys.stderr)
    text = json.dumps(rec, indent=1)
    if args.out:
        open(args.out, "w").write(text + "\n")
    print(text)


def add_kernel_breakdown(rec, d):
    """Per shape, from the --trace run's kernel trace: the last call's launches and the kernel time of its phases.  A division's
    kernels run in a fixed order on one stream: the Newton doublings, then the quotient (the reversal of h, its transform and the
    dividends', the first bcast_mul_kernel, the inverse transform, the copy of q), then the remainder (folds, the cyclic product,
    sub_low_kernel).  Calls are told apart by their first kernel (newton_lds_kernel); S6 is everything after the last division."""
    rows = []
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            if "tfk::" in r["Kernel_Name"]:
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    calls, cur = [], None
    for row in rows:
        if "newton_lds_kernel" in row[2]:
            cur = []
            calls.append(cur)
        if cur is not None:
            cur.append(row)
    per_shape = 3  # --trace: one warm-up and two timed calls
    for i, entry in enumerate(rec["shapes"][:len(SHAPES)]):
        if (i + 1) * per_shape > len(calls):
            break
        call = calls[(i + 1) * per_shape - 1]
        if i == len(SHAPES) - 1:  # the last division call also holds the S6 kernels behind it: cut at sub_low_kernel
            end = max(j for j, r in enumerate(call) if "sub_low_kernel" in r[2])
            fps, call = call[end + 1:], call[:end + 1]
        names = [r[2] for r in call]
        i1 = next(j for j, n in enumerate(names) if "bcast_mul_kernel" in n)
        qs = max(j for j in range(i1) if "reverse_kernel" in names[j])
        qe = next(j for j in range(i1, len(names)) if "copy_pad_kernel" in names[j])
        us = lambda rs: sum(e - s for s, e, _ in rs) / 1e3  # noqa: E731
        entry["launches_per_call"] = len(call)
        entry["kernel_us"] = {"newton": us(call[:qs]), "quotient": us(call[qs:qe + 1]), "remainder": us(call[qe + 1:]), "total": us(call)}
        entry["wall_us_first_to_last_kernel"] = (call[-1][1] - call[0][0]) / 1e3
    if len(calls) >= len(SHAPES) * per_shape:
        # S6: its three identical calls (one warm-up, two timed) follow the last division
        e6 = rec["shapes"][len(SHAPES)]
        e6["launches_per_call"] = len(fps) / per_shape
        e6["kernel_us"] = {"newton": sum(e - s for s, e, _ in fps) / 1e3 / per_shape, "total": sum(e - s for s, e, _ in fps) / 1e3 / per_shape}

if __name__ == "__main__":
    main()
