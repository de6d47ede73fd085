#!/usr/bin/env python3
"""Batch inversion on the GPU (tf_batch_inversion_*_dev_async, tf_batch_inversion_*_dev) at the sizes of the issue that introduced it:
n = 2^16, 2^20, 2^24 BFieldElements and 2^16, 2^20, 2^23 XFieldElements, inputs from tf_debug_fill_random_dev.
For every size: `ms` (median of --reps warm calls of the enqueue-only form between HIP events), `blocking_ms` (the plain _dev form,
which copies its zero flag back), the HBM floor of 16 / 48 bytes per element at the chip's measured copy rate (6.29 TB/s,
MI355X float4 copy) and a device-to-device copy of the same bytes timed in the same run.  (The comparison with one exponentiation
per element is recorded in profiles/batch_inversion_bench.json.)
  --trace: a short run (one warm-up and two calls per size, synchronised) for `rocprofv3 --kernel-trace --stats` (a run of its own).
usage: batch_inversion_times.py [--reps 20] [--out profiles/batch_inversion_bench.json] [--trace]"""
import argparse
import hashlib
import json
import os
import statistics
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

SIZES = [(1, 1 << 16), (1, 1 << 20), (1, 1 << 24), (3, 1 << 16), (3, 1 << 20), (3, 1 << 23)]
COPY_RATE = 6.29e12  # bytes/s, MI355X float4 copy (the chip's measured HBM rate)


def measure(reps, trace):
    import torch

    import twenty_first_amd as tf

    res = []
    for w, n in SIZES:
        x = torch.empty(w * n, dtype=torch.int64, device="cuda")
        tf.device.fill_random(x, 0xB17 + w * n)
        y = torch.empty_like(x)
        st = torch.zeros(1, dtype=torch.int32, device="cuda")
        calls = 2 if trace else reps
        tf.device.batch_inversion(x, y, width=w, status=st)  # warm-up
        torch.cuda.synchronize()
        times, blocking, copies = [], [], []
        for _ in range(calls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            tf.device.batch_inversion(x, y, width=w, status=st)
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1))
            if trace:
                continue
            e0.record()
            tf.device.batch_inversion(x, y, width=w)
            e1.record()
            e1.synchronize()
            blocking.append(e0.elapsed_time(e1))
            e0.record()
            y.copy_(x)
            e1.record()
            e1.synchronize()
            copies.append(e0.elapsed_time(e1))
        tf.device.batch_inversion(x, y, width=w, status=st)
        torch.cuda.synchronize()
        assert int(st.item()) == 0
        entry = {"width": w, "n": n, "ms": statistics.median(times), "reps": calls,
                 "words_sha256": hashlib.sha256(y.cpu().numpy().tobytes()).hexdigest()[:16]}
        if not trace:
            entry["blocking_ms"] = statistics.median(blocking)
            entry["copy_ms"] = statistics.median(copies)
        res.append(entry)
        print(json.dumps(entry), file=sys.stderr)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", action="store_true")
    args = ap.parse_args()
    if args.trace:
        print(json.dumps(measure(args.reps, args.trace)))
        return
    import twenty_first_amd as tf

    rec = {"what": "batch inversion, tf_batch_inversion_*_dev_async between HIP events, median of warm calls",
           "source_hash": tf.lib().tf_source_hash().decode(), "copy_rate_bytes_per_s": COPY_RATE, "sizes": measure(args.reps, False)}
    for e in rec["sizes"]:
        bytes_ = 16 * e["n"] * e["width"]
        e["hbm_bytes"] = bytes_
        e["floor_us"] = bytes_ / COPY_RATE * 1e6
        e["x_floor"] = e["ms"] * 1e3 / e["floor_us"]
        e["x_copy"] = e["ms"] / e["copy_ms"]
    text = json.dumps(rec, indent=1)
    if args.out:
        open(args.out, "w").write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
