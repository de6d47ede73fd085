#!/usr/bin/env python3
"""Times of the prefix scans (twenty_first_amd.scan) against the streaming yardstick that moves the same bytes.

For n = 2^20 .. 2^24 rows, every mode and width, and a batch that fills the device (n * batch * width = 2^25 words per operand, at
least one column), on device buffers, timed with device events around one call (median over --reps after --warmup):
    ms           one scan call: three launches (tile maps, spine, tiles)
    bytes_per_s  the algebraic bytes -- every operand read once, out written once -- over that time
    yardstick    tf_poly_add_dev on the same n * batch * width in the same process: two operands read, one written, no product
    ratio        scan bytes_per_s / yardstick bytes_per_s
No time is a pass condition; the record (profiles/scan_bench.json) is what DESIGN 7.7 quotes.
usage: python tools/scan_bench.py [--reps 20] [--warmup 3] [--out profiles/scan_bench.json]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import twenty_first_amd as tf  # noqa: E402

SUM, PRODUCT, AFFINE = tf.scan.SUM, tf.scan.PRODUCT, tf.scan.AFFINE
# (name, mode, width_a, width_b, a_len == 1)
KINDS = [("sum 1", SUM, 1, 1, False), ("sum 3", SUM, 3, 3, False), ("product 1", PRODUCT, 1, 1, False), ("product 3", PRODUCT, 3, 3, False),
         ("affine (1, 1)", AFFINE, 1, 1, False), ("affine (3, 3)", AFFINE, 3, 3, False), ("affine (3, 1)", AFFINE, 3, 1, False),
         ("affine (3, 1), one multiplier", AFFINE, 3, 1, True)]
WORDS = 1 << 25


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


def measure(reps, warmup):
    rows = []
    for log_n in range(20, 25):
        n = 1 << log_n
        for name, mode, wa, wb, one in KINDS:
            w = wb if mode == SUM else wa
            batch = max(1, WORDS // (n * w))
            rows_w = n * batch
            a = None if mode == SUM else random_words(3 if one else rows_w * w, 1)
            b = None if mode == PRODUCT else random_words(rows_w * wb, 2)
            out = torch.empty(rows_w * w, dtype=torch.int64, device="cuda")
            ws = tf.scan.workspace(mode, n, batch, w)
            work = torch.empty(ws // 8, dtype=torch.int64, device="cuda") if ws else None
            if mode == SUM:
                call = lambda: tf.scan.sum_(b, n, out, batch=batch, width=w, work=work)  # noqa: E731
            elif mode == PRODUCT:
                call = lambda: tf.scan.product(a, n, out, batch=batch, width=w, work=work)  # noqa: E731
            else:
                call = lambda: tf.scan.affine(a, b, n, out, batch=batch, width_a=wa, width_b=wb, a_len=1 if one else n, work=work)  # noqa: E731
            ms, lo, hi = timed(call, reps, warmup)
            words_moved = rows_w * ((0 if a is None or one else w) + (0 if b is None else wb) + w)
            # the yardstick on the same n * batch * width: out = x + y
            x, y = random_words(rows_w * w, 3), random_words(rows_w * w, 4)
            yms, ylo, yhi = timed(lambda: tf.device.poly_add(x, n, y, n, out, batch=batch, width=w), reps, warmup)
            rate, yrate = words_moved * 8 / (ms * 1e-3), 3 * rows_w * w * 8 / (yms * 1e-3)
            rows.append({"kind": name, "log_n": log_n, "batch": batch, "width_out": w, "workspace_bytes": ws, "ms": ms, "ms_min": lo, "ms_max": hi,
                         "algebraic_bytes": words_moved * 8, "bytes_per_s": rate, "yardstick_ms": yms, "yardstick_ms_min": ylo, "yardstick_ms_max": yhi,
                         "yardstick_bytes_per_s": yrate, "ratio_to_yardstick": rate / yrate})
            print(f"{name:32s} n=2^{log_n} batch={batch:3d}: {ms:8.4f} ms {rate / 1e9:8.1f} GB/s | poly_add {yms:8.4f} ms {yrate / 1e9:8.1f} GB/s | ratio {rate / yrate:5.2f}",
                  flush=True)
            del a, b, out, work, x, y
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "scan_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("scan_bench.py needs a GPU: there is nothing to time without one")
    plan = {f"width {w}": tf.scan.plan(AFFINE, 1 << 20, 1, w)._asdict() for w in (1, 3)}
    rec = {"tool": "tools/scan_bench.py", "device": torch.cuda.get_device_name(0),
           "library": {"tf_version": int(tf.lib().tf_version()), "source_hash": tf.lib().tf_source_hash().decode()},
           "reps": args.reps, "warmup": args.warmup, "timing": "device events around one call, median",
           "bytes": "algebraic: every operand read once, out written once; the yardstick tf_poly_add_dev reads two operands and writes one",
           "plan_at_2p20": plan, "rows": measure(args.reps, args.warmup)}
    json.dump(rec, open(args.out, "w"), indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
