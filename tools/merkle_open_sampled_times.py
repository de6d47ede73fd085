#!/usr/bin/env python3
"""Commit and open at indices a Tip5 sponge sampled into device memory: the route with a host round trip against the one without.
A timing record, not a gate.  Two shapes, both with leafs from tf_debug_fill_random_dev and indices from
tf_tip5_sponge_sample_indices_dev:
    three trees of 2^20 leafs under one list of 160 indices          (a prover's main, auxiliary and quotient tree)
    1024 lists of 80 indices, one tree of 2^12 leafs each            (many transcripts at once)
  (a) host_index_ms   copy the indices back, wait, then tf_merkle_auth_structure_from_leafs_dev with host indices (one call per list);
  (b) sampled_ms      tf_merkle_auth_structure_from_leafs_sampled_dev on the same stream: nothing is read back.
Both in one process, alternating, between HIP events, median of --reps warm calls; (a) is code this tool does not touch and is the
yardstick.  The planner kernel's own duration and the gap to the launch behind it come from a `rocprofv3 --kernel-trace --stats` run
of its own over (b) alone: (b) is expected within (a) + planner + one gap.

Without arguments the tool is the driver: it starts each GPU step as a child process under its own `timeout`, stops at the first
step that fails, and writes the merged record.
usage: merkle_open_sampled_times.py [--reps 20] [--out profiles/merkle_open_sampled.json] [--work DIR]
       merkle_open_sampled_times.py --step measure|trace --result FILE      (the children)"""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
sys.path.insert(0, ROOT)

# (height, n_lists, trees_per_list, indices per list)
SHAPES = [(20, 1, 3, 160), (12, 1024, 1, 80)]
TRACE_CALLS = 3
STEP_SECONDS = {"measure": 240, "trace": 240}


def setup(tf, height, n_lists, tpl, k):
    import torch

    n, trees = 1 << height, n_lists * tpl
    leafs = torch.empty(trees * n * 5, dtype=torch.int64, device="cuda")
    tf.device.fill_random(leafs, 0x5A3D + height)
    states = torch.empty(16 * n_lists, dtype=torch.int64, device="cuda")
    tf.device.fill_random(states, 0x5B00 + height)
    indices = torch.empty(n_lists * k, dtype=torch.int32, device="cuda")
    tf.device.tip5_sponge_sample_indices(states, n, indices)
    cap = tf.merkle_sampled.max_nodes(n, k)
    mk = lambda words, dt=torch.int64: torch.zeros(words, dtype=dt, device="cuda")  # noqa: E731
    return dict(n=n, trees=trees, leafs=leafs, indices=indices, cap=cap, out_a=mk(trees * cap * 5), out_b=mk(trees * cap * 5),
                roots_a=mk(trees * 5), roots_b=mk(trees * 5), counts=mk(n_lists, torch.int32), status=mk(1, torch.int32))


def route_host_indices(tf, s, n_lists, tpl, k):
    """(a): the indices come back to the host (a copy that waits for the stream), then one host-index call per list"""
    import numpy as np
    import torch

    fn = tf.lib().tf_merkle_auth_structure_from_leafs_dev
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    idx = s["indices"].cpu().numpy().view(np.uint32).astype(np.uint64).reshape(n_lists, k)
    cnt = C.c_size_t(0)
    counts = []
    for l in range(n_lists):
        first = l * tpl
        rc = fn(C.c_void_p(s["leafs"].data_ptr() + first * s["n"] * 40), s["n"], tpl, C.c_void_p(idx[l].ctypes.data), k,
                C.c_void_p(s["out_a"].data_ptr() + first * s["cap"] * 40), s["cap"], C.byref(cnt),
                C.c_void_p(s["roots_a"].data_ptr() + first * 40), stream)
        assert rc == 0, rc
        counts.append(cnt.value)
    return counts


def route_sampled(tf, s, n_lists, tpl, k):
    tf.merkle_sampled.structure_from_leafs(s["leafs"], s["n"], s["indices"], s["out_b"], s["counts"], n_lists=n_lists, trees_per_list=tpl,
                                           roots=s["roots_b"], status=s["status"])


def event_ms(fn):
    import torch

    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def same_words(s, counts_a, n_lists, tpl):
    """(a) packs a list's trees count digests apart, (b) capacity digests apart: the structures and the roots must be the same words"""
    import numpy as np

    a, b = s["out_a"].cpu().numpy(), s["out_b"].cpu().numpy().reshape(s["trees"], s["cap"], 5)
    if s["counts"].cpu().numpy().tolist() != counts_a or int(s["status"].item()) != 0:
        return False
    for l in range(n_lists):
        got_a = a[l * tpl * s["cap"] * 5:][:tpl * counts_a[l] * 5].reshape(tpl, counts_a[l], 5)
        if not np.array_equal(got_a, b[l * tpl:(l + 1) * tpl, :counts_a[l]]):
            return False
    return bool(np.array_equal(s["roots_a"].cpu().numpy(), s["roots_b"].cpu().numpy()))


def step_measure(reps):
    import torch

    import twenty_first_amd as tf

    rows = []
    for height, n_lists, tpl, k in SHAPES:
        s = setup(tf, height, n_lists, tpl, k)
        a = lambda: route_host_indices(tf, s, n_lists, tpl, k)  # noqa: E731
        b = lambda: route_sampled(tf, s, n_lists, tpl, k)  # noqa: E731
        counts_a = a()  # warm-up of both routes
        b()
        torch.cuda.synchronize()
        t_a, t_b = [], []
        for _ in range(reps):  # alternating, so that both see the same machine
            t_a.append(event_ms(a))
            t_b.append(event_ms(b))
        rows.append({"height": height, "n_lists": n_lists, "trees_per_list": tpl, "indices_per_list": k, "capacity": s["cap"],
                     "structure_nodes_first_list": counts_a[0], "host_index_ms": statistics.median(t_a), "sampled_ms": statistics.median(t_b),
                     "host_index_spread_ms": max(t_a) - min(t_a), "sampled_spread_ms": max(t_b) - min(t_b),
                     "workspace_bytes": tf.merkle_sampled.from_leafs_workspace(s["n"], s["trees"], k, n_lists),
                     "same_words_both_routes": same_words(s, counts_a, n_lists, tpl)})
        del s
        torch.cuda.empty_cache()
    return {"source_hash": tf.lib().tf_source_hash().decode(), "reps": reps, "shapes": rows}


def step_trace():
    """(b) alone, a warm-up and TRACE_CALLS synchronised calls per shape, in the order of SHAPES: the run rocprofv3 wraps"""
    import torch

    import twenty_first_amd as tf

    for height, n_lists, tpl, k in SHAPES:
        s = setup(tf, height, n_lists, tpl, k)
        for _ in range(1 + TRACE_CALLS):
            route_sampled(tf, s, n_lists, tpl, k)
            torch.cuda.synchronize()
        del s
        torch.cuda.empty_cache()
    return {"calls_per_shape": 1 + TRACE_CALLS}


def planner_from_trace(trace_dir):
    """per shape: median duration of merkle_plan_kernel and median gap to the kernel launched behind it, warm calls only"""
    rows = []
    for f in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        rows += [(int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(open(f))]
    rows.sort()
    plans = [i for i, r in enumerate(rows) if "merkle_plan_kernel" in r[2]]
    per = 1 + TRACE_CALLS
    if len(plans) != per * len(SHAPES):
        raise SystemExit(f"expected {per * len(SHAPES)} planner dispatches in the trace, found {len(plans)}")
    out = []
    for j in range(len(SHAPES)):
        warm = plans[j * per + 1:(j + 1) * per]
        out.append({"planner_kernel_us": statistics.median((rows[i][1] - rows[i][0]) / 1e3 for i in warm),
                    "gap_behind_planner_us": statistics.median((rows[i + 1][0] - rows[i][1]) / 1e3 for i in warm)})
    return out


def child(step, result, work, wrap=()):
    cmd = ["timeout", "-k", "10", str(STEP_SECONDS[step]), *wrap, sys.executable, os.path.abspath(__file__), "--step", step, "--result", result]
    print("+", " ".join(cmd), file=sys.stderr)
    rc = subprocess.call(cmd, cwd=ROOT, stdout=open(os.path.join(work, step + ".log"), "w"), stderr=subprocess.STDOUT)
    if rc:
        raise SystemExit(f"step {step} ended with status {rc} (log: {os.path.join(work, step + '.log')}); nothing more is started")
    return json.load(open(result))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "merkle_open_sampled.json"))
    ap.add_argument("--work", default=os.path.join(ROOT, "build", "merkle_open_sampled"), help="logs, step results and the raw trace")
    ap.add_argument("--step", choices=["measure", "trace"])
    ap.add_argument("--result")
    args = ap.parse_args()
    if args.step:
        res = step_measure(args.reps) if args.step == "measure" else step_trace()
        json.dump(res, open(args.result, "w"))
        return
    os.makedirs(args.work, exist_ok=True)
    rec = child("measure", os.path.join(args.work, "measure.json"), args.work)
    trace_dir = os.path.join(args.work, "trace")
    child("trace", os.path.join(args.work, "trace.json"), args.work,
          wrap=("rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", trace_dir, "-o", "sampled", "--"))
    for row, planner in zip(rec["shapes"], planner_from_trace(trace_dir)):
        row.update(planner)
        row["sampled_minus_host_index_us"] = (row["sampled_ms"] - row["host_index_ms"]) * 1e3
        row["within_planner_plus_one_gap"] = row["sampled_minus_host_index_us"] <= row["planner_kernel_us"] + row["gap_behind_planner_us"]
    rec = {"what": "commit and open at device-resident sampled indices: (a) indices copied back + host-index call per list, (b) the sampled "
                   "call; HIP events, medians of alternating warm calls; planner kernel and the gap behind it from a rocprofv3 kernel trace "
                   "of (b) alone", **rec}
    text = json.dumps(rec, indent=1)
    open(args.out, "w").write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
