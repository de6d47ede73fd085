#!/usr/bin/env python3
"""Device-resident Tip5 sponges (tf_tip5_sponge_*_dev) at the three transcript shapes of DESIGN 4.7:
  T1      1 sponge    pad_and_absorb_all of 16 384 words; sample_scalars(512); sample_indices(2^20, 160)
  T2  4 096 sponges   pad_and_absorb_all of 330 words;    sample_scalars(64);  sample_indices(2^20, 80)
  T3 65 536 sponges   ragged pad_and_absorb_all of 20 .. 60 words; sample_scalars(10); sample_indices(2^20, 40)
One process measures ONE side, so that the new library and the parent commit's (TF_HIP_LIBRARY=..., TF_HIP_ALLOW_OLDER_LIBRARY=1)
can alternate in one GPU session:
  --mode new      every part as the one call it is now, and the three calls in a row ("program")
  --mode permute  baseline 1, the device-resident route a caller had before: as many tf_tip5_permute_dev calls as the part has
                  steps, on the same number of states, back to back on one stream (the permutations only: it neither loads
                  input nor stores output, and pays a launch per step; called through ctypes with prebuilt arguments).  A ragged
                  absorb is stepped to its longest member, as a caller stepping the whole batch must.
  --mode host     baseline 2, the host-stepped loop of Tip5Sponge before this change: one tf_tip5_permute (host pointers: the
                  states go to the device and back) per step, the rate words overwritten in numpy between steps (T1 and T2)
Times: HIP events around --reps calls, median of the per-call means of three rounds (mode host: wall clock, median of three).
  --merge A B ... writes the record: per shape and part the median over the repeats of each side, the run-to-run spread of
                  baseline 1 (max - min over its repeats) and whether the one-call time is at or below baseline 1 + that spread;
  --stats DIR     (with --merge) adds the kernel_stats.csv of a `rocprofv3 --kernel-trace --stats` run of --mode new --trace,
                  and compares the launches of the sponge kernels with the library calls that run made.
usage: tip5_sponge_bench.py --mode new|permute|host [--reps 10] [--trace] --out FILE
       tip5_sponge_bench.py --merge FILE... [--stats DIR] --out FILE"""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

SHAPES = {
    "T1": {"count": 1, "absorb": 16384, "scalars": 512, "indices": 160},
    "T2": {"count": 4096, "absorb": 330, "scalars": 64, "indices": 80},
    "T3": {"count": 65536, "absorb": "ragged 20..60", "scalars": 10, "indices": 40},
}
UPPER_BOUND = 1 << 20


def lengths_of(shape):
    c = shape["count"]
    if isinstance(shape["absorb"], int):
        return np.full(c, shape["absorb"], dtype=np.uint64)
    return (20 + (np.arange(c, dtype=np.uint64) * 7) % 41).astype(np.uint64)


def steps_of(shape):
    """permutations per part (the sampler counts hold unless a squeezed element is BFieldElement::MAX: probability 2^-64 each)"""
    return {"absorb": int(lengths_of(shape).max()) // 10 + 1, "scalars": -(-3 * shape["scalars"] // 10), "indices": -(-shape["indices"] // 10)}


def timed(fn, reps):
    import torch

    fn()
    torch.cuda.synchronize()
    means = []
    for _ in range(3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        means.append(a.elapsed_time(b) / reps)
    return statistics.median(means)


def identity(tf):
    return {"tf_version": int(tf.lib().tf_version()), "source_hash": tf.lib().tf_source_hash().decode()}


def run_new(args):
    import torch

    import twenty_first_amd as tf

    dev = tf.device
    rec = {"mode": "new", "device": torch.cuda.get_device_name(0), "library": identity(tf), "reps": args.reps, "shapes": {}}
    calls = [0]  # library calls that launch a sponge kernel

    def counted(fn):
        def f():
            calls[0] += fn()
        return f

    for name, shape in SHAPES.items():
        count, lens = shape["count"], lengths_of(shape)
        off = np.zeros(count + 1, dtype=np.uint64)
        off[1:] = np.cumsum(lens)
        words = torch.zeros(int(off[-1]), dtype=torch.int64, device="cuda")
        dev.fill_random(words, 0x5B + count)
        st = torch.zeros(16 * count, dtype=torch.int64, device="cuda")
        sc = torch.zeros(count * shape["scalars"] * 3, dtype=torch.int64, device="cuda")
        idx = torch.zeros(count * shape["indices"], dtype=torch.int32, device="cuda")
        offsets = None if isinstance(shape["absorb"], int) else off

        def absorb():
            dev.tip5_sponge_pad_and_absorb_all_(st, words, offsets=offsets)
            return 1

        def scalars():
            dev.tip5_sponge_sample_scalars(st, sc)
            return 1

        def indices():
            dev.tip5_sponge_sample_indices(st, UPPER_BOUND, idx)
            return 1

        def program():
            return absorb() + scalars() + indices()

        parts = {"absorb": absorb, "scalars": scalars, "indices": indices, "program": program}
        reps = 1 if args.trace else args.reps
        rec["shapes"][name] = {"shape": shape, "steps": steps_of(shape), "ms": {k: timed(counted(f), reps) for k, f in parts.items()}}
    rec["sponge_api_calls"] = calls[0]
    return rec


def run_permute(args):
    import torch

    import twenty_first_amd as tf

    fn = tf.lib().tf_tip5_permute_dev
    rec = {"mode": "permute", "device": torch.cuda.get_device_name(0), "library": identity(tf), "reps": args.reps, "shapes": {}}
    for name, shape in SHAPES.items():
        count, steps = shape["count"], steps_of(shape)
        st = torch.zeros(16 * count, dtype=torch.int64, device="cuda")
        tf.device.fill_random(st, 0x5C + count)
        p, n, s = C.c_void_p(st.data_ptr()), C.c_size_t(count), C.c_void_p(torch.cuda.current_stream().cuda_stream)

        def chain(k):
            def f():
                for _ in range(k):
                    if fn(p, n, s):
                        raise RuntimeError("tf_tip5_permute_dev failed")
            return f

        ms = {k: timed(chain(v), args.reps) for k, v in steps.items()}
        ms["program"] = timed(chain(sum(steps.values())), args.reps)
        rec["shapes"][name] = {"shape": shape, "steps": steps, "ms": ms}
    return rec


def run_host(args):
    import twenty_first_amd as tf

    rec = {"mode": "host", "library": identity(tf), "shapes": {}}
    rng = np.random.default_rng(3)
    for name in ("T1", "T2"):
        shape = SHAPES[name]
        count, steps = shape["count"], steps_of(shape)
        rows = rng.integers(0, 0xFFFFFFFF00000001, size=(count, shape["absorb"]), dtype=np.uint64)
        ms = {}

        def absorb(state):
            full = rows.shape[1] // 10
            for c in range(full):
                state[:, :10] = rows[:, 10 * c:10 * c + 10]
                tf.Tip5.permute_states(state.reshape(-1))
            last = np.zeros((count, 10), dtype=np.uint64)
            last[:, : rows.shape[1] - 10 * full] = rows[:, 10 * full:]
            last[:, rows.shape[1] - 10 * full] = 0xFFFFFFFF
            state[:, :10] = last
            tf.Tip5.permute_states(state.reshape(-1))

        def squeezes(k):
            def f(state):
                out = np.empty((count, k, 10), dtype=np.uint64)
                for i in range(k):
                    out[:, i] = state[:, :10]
                    tf.Tip5.permute_states(state.reshape(-1))
            return f

        def program(state):
            absorb(state)
            squeezes(steps["scalars"])(state)
            squeezes(steps["indices"])(state)

        for part, f in {"absorb": absorb, "scalars": squeezes(steps["scalars"]), "indices": squeezes(steps["indices"]), "program": program}.items():
            state = np.zeros((count, 16), dtype=np.uint64)
            f(state)
            ts = []
            for _ in range(3):
                t = time.perf_counter()
                f(state)
                ts.append((time.perf_counter() - t) * 1e3)
            ms[part] = statistics.median(ts)
        rec["shapes"][name] = {"shape": shape, "steps": steps, "ms": ms}
    return rec


def merge(paths, stats_dir):
    recs = [json.load(open(p)) for p in paths]
    by = {m: [r for r in recs if r["mode"] == m] for m in ("new", "permute", "host")}
    out = {"tool": "tools/tip5_sponge_bench.py", "device": by["new"][0]["device"], "library": by["new"][0]["library"],
           "baseline_library": by["permute"][0]["library"], "repeats": {m: len(v) for m, v in by.items()}, "upper_bound": UPPER_BOUND, "shapes": {}}
    for name, shape in SHAPES.items():
        e = {"shape": shape, "steps": steps_of(shape), "parts": {}}
        for part in ("absorb", "scalars", "indices", "program"):
            new = [r["shapes"][name]["ms"][part] for r in by["new"]]
            base = [r["shapes"][name]["ms"][part] for r in by["permute"]]
            host = [r["shapes"][name]["ms"][part] for r in by["host"] if name in r["shapes"]]
            spread = max(base) - min(base)
            p = {"one_call_ms": statistics.median(new), "one_call_ms_repeats": new, "permute_dev_chain_ms": statistics.median(base),
                 "permute_dev_chain_ms_repeats": base, "permute_dev_chain_spread_ms": spread,
                 "at_or_below_baseline_1": statistics.median(new) <= statistics.median(base) + spread}
            if host:
                p["host_stepped_ms"] = statistics.median(host)
            e["parts"][part] = p
        if name == "T1":
            e["us_per_dependent_permutation"] = {k: 1e3 * e["parts"][k]["one_call_ms"] / e["steps"][k] for k in ("absorb", "scalars", "indices")}
        out["shapes"][name] = e
    if stats_dir:
        rows = []
        for f in glob.glob(os.path.join(stats_dir, "**", "*kernel_stats.csv"), recursive=True):
            for r in csv.DictReader(open(f)):
                rows.append({"kernel": r["Name"], "calls": int(r["Calls"]), "total_ms": float(r["TotalDurationNs"]) / 1e6, "avg_us": float(r["AverageNs"]) / 1e3})
        out["kernel_stats"] = sorted(rows, key=lambda r: -r["total_ms"])
        traced = [r for r in recs if r["mode"] == "new-trace"]
        if traced:
            launches = sum(r["calls"] for r in rows if "tip5_sponge" in r["kernel"])
            out["one_launch_per_call"] = {"sponge_library_calls": traced[0]["sponge_api_calls"], "sponge_kernel_launches": launches,
                                          "holds": launches == traced[0]["sponge_api_calls"]}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["new", "permute", "host"])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--trace", action="store_true", help="one call per round: for a run under rocprofv3 --kernel-trace --stats")
    ap.add_argument("--merge", nargs="+", default=None)
    ap.add_argument("--stats", default=None)
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    if args.merge:
        rec = merge(args.merge, args.stats)
    else:
        rec = {"new": run_new, "permute": run_permute, "host": run_host}[args.mode](args)
        if args.trace:
            rec["mode"] = "new-trace"
    with open(args.out, "w") as f:
        f.write(json.dumps(rec, indent=1) + "\n")
    print(json.dumps(rec if args.merge else {k: v for k, v in rec.items() if k != "shapes"} | {n: s["ms"] for n, s in rec["shapes"].items()}))


if __name__ == "__main__":
    main()
