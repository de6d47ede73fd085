#!/usr/bin/env python3
"""Authentication structure + root straight from the leafs (tf_merkle_auth_structure_from_leafs_dev) against the two things it stands
between: heights 12, 16, 20 and 24 with 160 random indices at batch 1, and height 16 at batch 16, leafs from tf_debug_fill_random_dev.
For every shape, in one process, between HIP events, median of --reps warm calls after a warm-up:
  (a) open_ms      the new call with roots;
  (b) root_ms      tf_merkle_root_dev alone;
  (c) build_ms     tf_merkle_build_dev followed by the device gather of the same structure (tf_merkle_authentication_structure_dev per
                   tree, which copies its digests back -- what a caller of the node-array route pays);
and the work-space bytes of (a) (tf_merkle_auth_structure_from_leafs_workspace) against the 2 n * 40 * batch bytes of (c)'s node array.
`root_spread_ms` is max - min of (b)'s own samples and `emission_launches` the copy-out launches of (a) (one per wide level that holds
a structure node, one for the top block): (a) is expected at (b) plus a few microseconds per emission launch.
  --trace: one warm-up and two synchronised calls of (a) per shape, for `rocprofv3 --kernel-trace --stats` (a run of its own).
usage: merkle_open_times.py [--reps 20] [--out profiles/merkle_open_bench.json] [--trace]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

SHAPES = [(12, 1), (16, 1), (20, 1), (24, 1), (16, 16)]
K = 160


def timed(fn, reps):
    import torch

    fn()  # warm-up
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return times


def emission_launches(n, batch, node_ids):
    """Copy-out launches of the sweep: one per level wider than the top block that holds a structure node, one for the top block."""
    narrow = lambda w: w <= 64 or (w // 2) * batch <= (1 << 13)  # noqa: E731  (kTopWidth, kCoopMaxCount)
    w = n
    while not narrow(w):
        w //= 2
    levels = {int(v).bit_length() - 1 for v in node_ids}
    top_level = w.bit_length() - 1
    return len({lv for lv in levels if lv > top_level}) + (1 if any(lv <= top_level for lv in levels) else 0)


def measure(reps, trace):
    import numpy as np
    import torch

    import twenty_first_amd as tf

    res = []
    for height, batch in SHAPES:
        n = 1 << height
        leafs = torch.empty(batch * n * 5, dtype=torch.int64, device="cuda")
        tf.device.fill_random(leafs, 0x09E7 + height + batch)
        idx = np.random.default_rng(height * 100 + batch).integers(0, n, size=K).astype(np.uint64)
        node_ids = tf.MerkleTree.authentication_structure_node_indices(n, idx)
        count = node_ids.size
        out = torch.empty(batch * count * 5, dtype=torch.int64, device="cuda")
        roots = torch.empty(batch * 5, dtype=torch.int64, device="cuda")
        open_call = lambda: tf.device.authentication_structure_from_leafs(leafs, n, idx, out=out, roots=roots, batch=batch)  # noqa: E731
        entry = {"height": height, "batch": batch, "indices": K, "structure_nodes": int(count),
                 "emission_launches": emission_launches(n, batch, node_ids),
                 "workspace_bytes": tf.device.authentication_structure_from_leafs_workspace(n, batch, count),
                 "node_array_bytes": 2 * n * 40 * batch}
        t_open = timed(open_call, 2 if trace else reps)
        entry["open_ms"] = statistics.median(t_open)
        if not trace:
            roots_b = torch.empty_like(roots)
            t_root = timed(lambda: tf.device.merkle_root(leafs, n, roots_b, batch=batch), reps)
            nodes = torch.empty(batch * n * 10, dtype=torch.int64, device="cuda")

            def build_and_gather():
                tf.device.merkle_build(leafs, n, nodes, batch=batch)
                return [tf.device.authentication_structure(nodes[t * n * 10:(t + 1) * n * 10], n, idx) for t in range(batch)]

            t_build = timed(build_and_gather, reps)
            torch.cuda.synchronize()
            gathered = np.stack(build_and_gather())
            entry.update(root_ms=statistics.median(t_root), root_spread_ms=max(t_root) - min(t_root), build_ms=statistics.median(t_build),
                         open_spread_ms=max(t_open) - min(t_open),
                         same_words_as_build=bool(np.array_equal(out.cpu().numpy().view(np.uint64).reshape(batch, count, 5), gathered)),
                         same_roots_as_root_only=bool(torch.equal(roots, roots_b)))
            entry["open_minus_root_us"] = (entry["open_ms"] - entry["root_ms"]) * 1e3
            entry["workspace_over_node_array"] = entry["workspace_bytes"] / entry["node_array_bytes"]
            del nodes
        res.append(entry)
        print(json.dumps(entry), file=sys.stderr)
        del leafs
        torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", action="store_true")
    args = ap.parse_args()
    import twenty_first_amd as tf

    rec = {"what": "authentication structure + root from the leafs (a) vs root only (b) vs build + gather (c), HIP events, median of warm calls",
           "source_hash": tf.lib().tf_source_hash().decode(), "reps": args.reps, "shapes": measure(args.reps, args.trace)}
    text = json.dumps(rec, indent=1)
    if args.out:
        open(args.out, "w").write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
