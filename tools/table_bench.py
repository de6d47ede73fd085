#!/usr/bin/env python3
"""The measurements behind DESIGN 7.5.  Every figure is the median over --reps timed calls, each between two HIP events, after
--warmup calls of every variant; the variants of one comparison alternate call by call within one process.

  transpose   tf_table_transpose_dev on tables of 2^20 x 64 BFieldElements, 2^20 x 32 XFieldElements and 2^16 x 512 BFieldElements,
              both directions, exact strides, against two yardsticks on the same buffers that do not involve the library:
                (a) copy     dst.copy_(src): a device-to-device copy of the same bytes, the floor for moving the data at all
                (b) strided  dst.view(...).copy_(src.view(...).permute(...)): torch's strided copy, what a caller had before
              (b) is timed twice per round (b1, b2); |median b1 - median b2| / min is the run's own spread.  The gate: the kernel is
              not slower than (b) beyond max(3 %, that spread).  The words must be (b)'s.
  lde_rows    2^18 -> 2^20, 64 columns of BFieldElements: tf_table_lde_rows_bfe_dev with the automatic block size and with
              cols_per_block = n_cols, against tf_lde_bfe_dev on the same data already column-major (the cost of the two
              transposes, and of blocking).  Recorded, not gated.
  gather_rows k = 256 rows of a 2^20 x 400 table of BFieldElements from both layouts, time per call.  Recorded only.

usage: table_bench.py [--reps 20] [--warmup 3] [--out profiles/table_bench.json] [--small]   (--small: a rehearsal at toy sizes)"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)


def _timed(fn):
    import torch

    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def _alternate(variants, warmup, reps):
    """{name: median ms per call}: the variants take turns, call by call"""
    import torch

    for _ in range(warmup):
        for fn in variants.values():
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in variants}
    for _ in range(reps):
        for name, fn in variants.items():
            times[name].append(_timed(fn))
    return {name: statistics.median(t) for name, t in times.items()}


def _rnd(tf, words, seed):
    import torch

    t = torch.empty(words, dtype=torch.int64, device="cuda")
    tf.device.fill_random(t, seed)
    return t


def transpose(tf, w, n_rows, n_cols, direction, warmup, reps):
    import torch

    n_outer, n_inner = (n_cols, n_rows) if direction == "columns_to_rows" else (n_rows, n_cols)
    words = n_outer * n_inner * w
    src = _rnd(tf, words, 0x7AB + w + n_cols)
    dst, dst_copy, dst_strided = (torch.zeros(words, dtype=torch.int64, device="cuda") for _ in range(3))

    def kernel():
        tf.table.transpose(src, n_outer, n_inner, dst, width=w)

    def copy():
        dst_copy.copy_(src)

    def strided():
        dst_strided.view(n_inner, n_outer, w).copy_(src.view(n_outer, n_inner, w).permute(1, 0, 2))

    t = _alternate({"kernel": kernel, "copy": copy, "strided_1": strided, "strided_2": strided}, warmup, reps)
    torch.cuda.synchronize()
    strided_ms = min(t["strided_1"], t["strided_2"])
    spread = abs(t["strided_1"] - t["strided_2"]) / strided_ms
    allowance = max(0.03, spread)
    gbytes = 2 * words * 8 / 1e9  # read once, written once
    return {"width": w, "n_rows": n_rows, "n_cols": n_cols, "direction": direction, "kernel_ms": t["kernel"], "copy_ms": t["copy"],
            "strided_1_ms": t["strided_1"], "strided_2_ms": t["strided_2"], "spread": spread, "allowance": allowance,
            "kernel_over_copy": t["kernel"] / t["copy"], "kernel_over_strided": t["kernel"] / strided_ms,
            "kernel_gb_per_s": gbytes / (t["kernel"] * 1e-3), "copy_gb_per_s": gbytes / (t["copy"] * 1e-3),
            "same_words": bool(torch.equal(dst, dst_strided)), "gate_holds": bool(t["kernel"] <= strided_ms * (1 + allowance))}


def lde_rows(tf, log_n, log_m, n_cols, warmup, reps):
    import torch

    n, m = 1 << log_n, 1 << log_m
    off_in, off_out = tf.BFieldElement.new(7), tf.BFieldElement.new(49)
    rows = _rnd(tf, n * n_cols, 0x1DE)
    cols = torch.empty_like(rows)
    tf.table.rows_to_columns(rows, n, n_cols, cols)
    out_auto, out_whole, out_cols = (torch.zeros(m * n_cols, dtype=torch.int64, device="cuda") for _ in range(3))
    t = _alternate({"rows_auto": lambda: tf.table.lde_rows(rows, n, n_cols, off_in, out_auto, m, off_out),
                    "rows_one_block": lambda: tf.table.lde_rows(rows, n, n_cols, off_in, out_whole, m, off_out, cols_per_block=n_cols),
                    "column_major": lambda: tf.device.lde(cols, n, off_in, out_cols, m, off_out, batch=n_cols)}, warmup, reps)
    torch.cuda.synchronize()
    back = torch.empty_like(out_cols)
    tf.table.rows_to_columns(out_auto, m, n_cols, back)
    torch.cuda.synchronize()
    auto_cols = tf.table.lde_rows_workspace(n, m, n_cols) // ((n + m) * 8)
    return {"n": n, "m": m, "n_cols": n_cols, "width": 1, "auto_cols_per_block": auto_cols, "rows_auto_ms": t["rows_auto"],
            "rows_one_block_ms": t["rows_one_block"], "column_major_lde_ms": t["column_major"],
            "transposes_cost": t["rows_one_block"] / t["column_major"], "blocking_cost": t["rows_auto"] / t["rows_one_block"],
            "same_words": bool(torch.equal(out_auto, out_whole) and torch.equal(back, out_cols))}


def gather_rows(tf, n_rows, n_cols, k, warmup, reps):
    import torch

    table = _rnd(tf, n_rows * n_cols, 0x6A7)
    idx = torch.randint(0, n_rows, (k,), dtype=torch.int32, device="cuda", generator=torch.Generator(device="cuda").manual_seed(5))
    st = torch.zeros(1, dtype=torch.int32, device="cuda")
    outs = {layout: torch.zeros(k * n_cols, dtype=torch.int64, device="cuda") for layout in (0, 1)}
    t = _alternate({"column_major": lambda: tf.table.gather_rows(table, n_rows, n_cols, idx, outs[0], layout=0, status=st),
                    "row_major": lambda: tf.table.gather_rows(table, n_rows, n_cols, idx, outs[1], layout=1, status=st)}, warmup, reps)
    torch.cuda.synchronize()
    i64 = idx.to(torch.int64)
    same = torch.equal(outs[1].view(k, n_cols), table.view(n_rows, n_cols)[i64]) and torch.equal(outs[0].view(k, n_cols), table.view(n_cols, n_rows)[:, i64].t())
    return {"n_rows": n_rows, "n_cols": n_cols, "k": k, "width": 1, "column_major_ms": t["column_major"], "row_major_ms": t["row_major"],
            "same_words": bool(same), "status": int(st.item())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--small", action="store_true")
    args = ap.parse_args()
    import torch

    import twenty_first_amd as tf

    if not torch.cuda.is_available() or tf.lib().tf_device_count() == 0:
        raise SystemExit("table_bench.py needs a GPU: a time from anything else says nothing")
    s = 8 if args.small else 0  # --small: 2^8 times fewer rows
    shapes = [(1, 1 << (20 - s), 64), (3, 1 << (20 - s), 32), (1, 1 << (16 - s), 512)]
    rec = {"tool": "tools/table_bench.py", "what": "median ms per call between HIP events, variants alternating call by call",
           "library": {"tf_version": int(tf.lib().tf_version()), "source_hash": tf.lib().tf_source_hash().decode()},
           "device": torch.cuda.get_device_name(0), "reps": args.reps, "warmup": args.warmup, "small": args.small,
           "transpose": [transpose(tf, w, r, c, d, args.warmup, args.reps) for w, r, c in shapes for d in ("columns_to_rows", "rows_to_columns")],
           "lde_rows": lde_rows(tf, 18 - s, 20 - s, 64, args.warmup, args.reps),
           "gather_rows": gather_rows(tf, 1 << (20 - s), 400, 256, args.warmup, args.reps)}
    rec["transpose_gate_holds"] = all(t["gate_holds"] and t["same_words"] for t in rec["transpose"])
    text = json.dumps(rec, indent=1)
    if args.out:
        open(args.out, "w").write(text + "\n")
    print(text)
    if not rec["transpose_gate_holds"]:
        raise SystemExit("the transpose gate does not hold")


if __name__ == "__main__":
    main()
