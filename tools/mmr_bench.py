#!/usr/bin/env python3
"""Merkle Mountain Range operations on the GPU (tf_mmr_*_dev) at the shapes of DESIGN 4.6:
  S1  new_from_leafs of 2^24 - 1 leafs, next to tf_merkle_root_dev of 2^24 leafs in the same run
  S2  65 536 membership proofs verified against one accumulator of 2^32 - 1 leafs
  S3  4 096 mutations and 65 536 own proofs at 2^32 - 1 leafs (batch_mutate_leaf_and_update_mps)
  S4  an append of 1 024 leafs with their proofs
  S5  bag_peaks of 65 536 accumulators
Call time: HIP events around --reps calls of the _dev form (median of the per-call means of three rounds).  Kernel time comes from the
same run under `rocprofv3 --kernel-trace --stats`: --stats DIR merges that directory's kernel_stats.csv into the record afterwards.
CPU figure: the oracle's single-core hash_pairs over as many pairs as the shape hashes, a LOWER BOUND for the reference (it does the
same hashes one at a time, plus its own bookkeeping).  Inputs are synthetic.  S2: random leafs and full-length random paths in the
highest peak; the peak is fitted to proof 0 only, so proof 0 verifies and every other proof runs all its h steps and then fails the
peak comparison (status 25) -- the same work as a valid proof; the record counts the statuses.  S3: random mutation and own paths of
full length (an inconsistent batch: every step is still hashed, which is what the shape times).
usage: mmr_bench.py [--reps 10] [--out FILE] | mmr_bench.py --merge FILE --stats DIR"""
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


def cuda(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).reshape(-1).view(np.int64).copy()).cuda()


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


def cpu_pairs_ms(oracle, pairs):
    """single-core hash_pairs of `pairs` pairs (timed on at most 2^16 and scaled)"""
    m = min(pairs, 1 << 16)
    x = np.asarray(oracle.fill_random(10 * m, 5), dtype=np.uint64)
    t = time.perf_counter()
    oracle.hash_pairs(x)
    return (time.perf_counter() - t) * 1e3 * pairs / m


def synthetic_proofs(oracle, rng, n_leafs, n_proofs):
    """n_proofs leafs of the highest peak of an accumulator of n_leafs leafs, with random paths of full length; the peaks are random
    except the highest, which is fitted to proof 0 (the others fail at the peak comparison after hashing their whole path)"""
    import twenty_first_amd as tf

    h = n_leafs.bit_length() - 1  # the highest peak: 2^h leafs starting at 0
    idx = rng.integers(0, 1 << h, size=n_proofs, dtype=np.uint64)
    leaf = rng.integers(0, 0xFFFFFFFF00000001, size=(n_proofs, 5), dtype=np.uint64)
    paths = rng.integers(0, 0xFFFFFFFF00000001, size=(n_proofs, h, 5), dtype=np.uint64)
    peaks = rng.integers(0, 0xFFFFFFFF00000001, size=(bin(n_leafs).count("1"), 5), dtype=np.uint64)
    acc = leaf[0]
    for lv in range(h):
        acc = oracle.hash_pair(paths[0, lv], acc) if (int(idx[0]) >> lv) & 1 else oracle.hash_pair(acc, paths[0, lv])
    peaks[tf.mmr_index.leaf_index_to_mt_index_and_peak_index(int(idx[0]), n_leafs)[1]] = acc
    return idx, leaf, paths, peaks, h


def run(args):
    import torch

    import twenty_first_amd as tf
    from oracle import tfo as oracle

    dev = tf.device
    rng = np.random.default_rng(1)
    props = torch.cuda.get_device_properties(0)
    rec = {"device": torch.cuda.get_device_name(0) or getattr(props, "gcnArchName", "") or "unknown", "library": tf.lib().tf_source_hash().decode(), "shapes": {}}

    # S1
    n = (1 << 24) - 1
    leafs = torch.zeros(5 * (1 << 24), dtype=torch.int64, device="cuda")
    dev.fill_random(leafs, 11)
    peaks = torch.zeros(5 * 24, dtype=torch.int64, device="cuda")
    root = torch.zeros(5, dtype=torch.int64, device="cuda")
    s1 = timed(lambda: dev.mmr_append(0, None, leafs[: 5 * n], peaks), args.reps)
    mr = timed(lambda: dev.merkle_root(leafs, 1 << 24, root), args.reps)
    rec["shapes"]["S1"] = {"what": "new_from_leafs(2^24 - 1)", "call_ms": s1, "merkle_root_2^24_call_ms": mr, "ratio": s1 / mr,
                           "hash_pairs": n - 24, "cpu_hash_pairs_ms_lower_bound": cpu_pairs_ms(oracle, n - 24)}
    del leafs

    # S2
    L = (1 << 32) - 1
    idx, leaf, paths, pk, h = synthetic_proofs(oracle, rng, L, 65536)
    off = np.arange(0, 65536 * h + 1, h, dtype=np.uint64)
    d = [cuda(pk), cuda(idx), cuda(leaf), cuda(paths)]
    st = torch.zeros(65536, dtype=torch.int32, device="cuda")
    s2 = timed(lambda: dev.mmr_verify_membership_proofs(L, d[0], d[1], d[2], off, d[3], st), args.reps)
    torch.cuda.synchronize()
    codes, counts = np.unique(st.cpu().numpy(), return_counts=True)
    rec["shapes"]["S2"] = {"what": "65 536 verifications at 2^32 - 1 leafs (proof 0 valid, the rest fail at the peak)", "call_ms": s2,
                           "statuses": {str(int(c)): int(m) for c, m in zip(codes, counts)}, "hash_pairs": 65536 * h,
                           "cpu_hash_pairs_ms_lower_bound": cpu_pairs_ms(oracle, 65536 * h)}

    # S3: 4 096 distinct mutations and 65 536 own proofs, every path of full length
    M, P = 4096, 65536
    mut = rng.choice(1 << 31, size=M, replace=False).astype(np.uint64)
    own = rng.integers(0, 1 << 31, size=P, dtype=np.uint64)
    mpaths = rng.integers(0, 0xFFFFFFFF00000001, size=(M * h, 5), dtype=np.uint64)
    opaths = rng.integers(0, 0xFFFFFFFF00000001, size=(P * h, 5), dtype=np.uint64)
    moff = np.arange(0, M * h + 1, h, dtype=np.uint64)
    ooff = np.arange(0, P * h + 1, h, dtype=np.uint64)
    d3 = [cuda(pk), cuda(rng.integers(0, 0xFFFFFFFF00000001, size=(M, 5), dtype=np.uint64)), cuda(mpaths), cuda(opaths)]
    mod = torch.zeros(P, dtype=torch.int32, device="cuda")
    s3 = timed(lambda: dev.mmr_batch_mutate_leafs(L, d3[0], mut, d3[1], moff, d3[2], own, ooff, d3[3], mod), args.reps)
    t = time.perf_counter()
    for _ in range(3):
        dev.mmr_batch_mutate_leafs(L, d3[0], mut, d3[1], moff, d3[2], own, ooff, d3[3], mod)
    torch.cuda.synchronize()
    rec["shapes"]["S3"] = {"what": "4 096 mutations + 65 536 own proofs at 2^32 - 1 leafs", "call_ms": s3,
                           "host_inclusive_ms": (time.perf_counter() - t) * 1e3 / 3, "hash_pairs": M * h,
                           "cpu_hash_pairs_ms_lower_bound": cpu_pairs_ms(oracle, M * h)}

    # S4: an append of 1 024 leafs with proofs, to an accumulator of 2^32 - 1 leafs
    new = cuda(rng.integers(0, 0xFFFFFFFF00000001, size=(1024, 5), dtype=np.uint64))
    words = 5 * sum(tf.mmr_index.trailing_ones(L + i) for i in range(1024))
    outp = torch.zeros(5 * 32, dtype=torch.int64, device="cuda")
    proofs = torch.zeros(words, dtype=torch.int64, device="cuda")
    s4 = timed(lambda: dev.mmr_append(L, d[0], new, outp, proofs), args.reps)
    rec["shapes"]["S4"] = {"what": "append of 1 024 leafs with proofs at 2^32 - 1 leafs", "call_ms": s4, "hash_pairs": 1024 + 31,
                           "cpu_hash_pairs_ms_lower_bound": cpu_pairs_ms(oracle, 1024 + 31)}

    # S5
    counts = rng.integers(0, 1 << 62, size=65536, dtype=np.uint64)
    npk = int(sum(bin(int(c)).count("1") for c in counts))
    bp = cuda(rng.integers(0, 0xFFFFFFFF00000001, size=(npk, 5), dtype=np.uint64))
    bo = torch.zeros(5 * 65536, dtype=torch.int64, device="cuda")
    s5 = timed(lambda: dev.mmr_bag_peaks(counts, bp, bo), args.reps)
    rec["shapes"]["S5"] = {"what": "bag_peaks of 65 536 accumulators", "call_ms": s5, "hash_pairs": npk + 65536,
                           "cpu_hash_pairs_ms_lower_bound": cpu_pairs_ms(oracle, npk + 65536)}
    return rec


def merge(path, stats_dir):
    rec = json.load(open(path))
    rows = []
    for f in glob.glob(os.path.join(stats_dir, "**", "*kernel_stats.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            rows.append({"kernel": r["Name"], "calls": int(r["Calls"]), "total_ms": float(r["TotalDurationNs"]) / 1e6,
                         "avg_us": float(r["AverageNs"]) / 1e3})
    rec["kernel_stats"] = sorted(rows, key=lambda r: -r["total_ms"])
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--merge", default=None)
    ap.add_argument("--stats", default=None)
    args = ap.parse_args()
    rec = merge(args.merge, args.stats) if args.merge else run(args)
    text = json.dumps(rec, indent=1)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
