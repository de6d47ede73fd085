#!/usr/bin/env python3
"""Batched Merkle inclusion-proof verification on the GPU (tf_merkle_verify_proofs[_dev]) at the reference's bench shape
(benches/merkle_tree_authenticate.rs: trees of height 16 and 20, 40 opened leafs per proof).

Prints one JSON document:
  * single-proof latency of the host API (MerkleTreeInclusionProof.try_verify_batch of one proof) and of the _dev API (one
    device.verify_inclusion_proofs + synchronise), median of --calls warm calls;
  * batch throughput of the _dev API at batches of 1, 64, 1 024 and 16 384 proofs (HIP events around --reps calls);
  * for every number, the parity of a sample against a CPU checker (honest proofs verify, a corrupted structure digest gives
    RootMismatch, and the checker's root, filled from a proof alone with the oracle, equals the device tree's root);
  * the hash_pairs each batch needs, and the oracle's single-core hash_pairs over that many pairs -- a LOWER BOUND for the
    reference's sequential verify of the batch (it does the same hashes plus its hash-map work).
Kernel times come from a separate `rocprofv3 --kernel-trace --stats` run (--quick keeps that run short).
usage: merkle_proof_bench.py [--calls 200] [--reps 20] [--quick] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

ROOT_MISMATCH = 21


def checker_root(oracle, height, idx, dig, auth):
    """Node 1 of the partial tree a proof defines: every level's known nodes pair up (2q, 2q + 1) into hash_pair inputs."""
    n = 1 << height
    ids = oracle.auth_structure_indices(n, np.asarray(idx, dtype=np.uint64))
    known = {int(v): auth[j] for j, v in enumerate(ids)}
    for i, d in zip(np.asarray(idx).tolist(), dig):
        known.setdefault(n + int(i), d)
    level = sorted({n + int(i) for i in np.asarray(idx).tolist()})
    for _ in range(height):
        both = sorted(set(level) | {v ^ 1 for v in level})
        outs = oracle.hash_pairs(np.concatenate([known[v] for v in both])).reshape(-1, 5)
        level = both[0::2]
        level = [v >> 1 for v in level]
        known.update(zip(level, outs))
    return known[1]


def hash_pairs_needed(height, idx):
    """Parents the fill computes: sum over the levels of the distinct ancestors one level up."""
    x = np.unique(np.asarray(idx, dtype=np.uint64))
    total = 0
    for lv in range(1, height + 1):
        total += np.unique(x >> np.uint64(lv)).size
    return int(total)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--quick", action="store_true", help="few calls (for the rocprofv3 kernel-trace run)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if args.quick:
        args.calls, args.reps = 20, 3

    import torch

    import twenty_first_amd as tf
    from oracle import tfo as oracle

    assert torch.cuda.is_available() and tf.lib().tf_device_count() > 0, "needs a GPU"
    res = {"tool": "tools/merkle_proof_bench.py", "library": {"tf_version": tf.lib().tf_version(), "source_hash": tf.lib().tf_source_hash().decode()},
           "device": torch.cuda.get_device_name(0), "opened_leafs": 40, "shapes": {}}
    batches = (1, 64, 1024, 16384)
    for height in (16, 20):
        n = 1 << height
        leaves = torch.empty(5 * n, dtype=torch.int64, device="cuda")
        tf.device.fill_random(leaves, 0x7E57 + height)
        nodes = torch.empty(10 * n, dtype=torch.int64, device="cuda")
        tf.device.merkle_build(leaves, n, nodes)
        nv = nodes.view(-1, 5)
        root = nv[1].clone()
        rng = np.random.default_rng(height)
        P = max(batches)
        idx_all, lo, ao, ids_all = [], [0], [0], []
        for _ in range(P):
            idx = rng.integers(0, n, size=40, dtype=np.uint64)
            ids = tf.MerkleTree.authentication_structure_node_indices(n, idx)
            idx_all.append(idx)
            ids_all.append(ids)
            lo.append(lo[-1] + 40)
            ao.append(ao[-1] + ids.size)
        li = torch.from_numpy(np.concatenate(idx_all).astype(np.int64)).cuda()
        ld = nv[li + n].reshape(-1).contiguous()
        ad = nv[torch.from_numpy(np.concatenate(ids_all).astype(np.int64)).cuda()].reshape(-1).contiguous()
        roots = root.repeat(P)
        heights = np.full(P, height, dtype=np.uint32)
        lo, ao = np.array(lo, dtype=np.uint64), np.array(ao, dtype=np.uint64)
        st = torch.full((P,), -1, dtype=torch.int32, device="cuda")
        shape = {}

        # parity sample: the checker's root from proof 0 alone, honest batch, one corrupted digest
        h_root = root.cpu().numpy().view(np.uint64)
        ld0 = ld[:200].cpu().numpy().view(np.uint64).reshape(-1, 5)
        ad0 = ad[: 5 * int(ao[1])].cpu().numpy().view(np.uint64).reshape(-1, 5)
        checker_ok = bool(np.array_equal(checker_root(oracle, height, idx_all[0], ld0, ad0), h_root))

        def parity(b):
            st.fill_(-1)
            tf.device.verify_inclusion_proofs(heights[:b], lo[: b + 1], li, ld, ao[: b + 1], ad, roots, st)
            bad = ad.clone()
            bad[0] = (bad[0] + 1) % 0xFFFFFFFF
            st_bad = torch.full((b,), -1, dtype=torch.int32, device="cuda")
            tf.device.verify_inclusion_proofs(heights[:b], lo[: b + 1], li, ld, ao[: b + 1], bad, roots, st_bad)
            torch.cuda.synchronize()
            s, sb = st[:b].cpu().numpy(), st_bad.cpu().numpy()
            return bool(checker_ok and (s == 0).all() and sb[0] == ROOT_MISMATCH and (sb[1:] == 0).all())

        # single proof, host API
        from twenty_first_amd import MerkleTreeInclusionProof as MTIP

        proof0 = MTIP(height, idx_all[0], ld0, ad0)
        for _ in range(10):
            MTIP.try_verify_batch([proof0], h_root)
        t = []
        for _ in range(args.calls):
            t0 = time.perf_counter()
            s0 = MTIP.try_verify_batch([proof0], h_root)
            t.append(time.perf_counter() - t0)
        shape["single_host_api_us_median"] = round(statistics.median(t) * 1e6, 2)
        shape["single_host_api_parity"] = bool(s0[0] == 0 and checker_ok)
        # single proof, _dev API (enqueue + synchronise)
        for _ in range(10):
            tf.device.verify_inclusion_proofs(heights[:1], lo[:2], li, ld, ao[:2], ad, roots, st)
        torch.cuda.synchronize()
        t = []
        for _ in range(args.calls):
            t0 = time.perf_counter()
            tf.device.verify_inclusion_proofs(heights[:1], lo[:2], li, ld, ao[:2], ad, roots, st)
            torch.cuda.synchronize()
            t.append(time.perf_counter() - t0)
        shape["single_dev_api_us_median"] = round(statistics.median(t) * 1e6, 2)
        shape["single_dev_api_parity"] = parity(1)
        # batches, _dev API, HIP events around `reps` calls
        shape["batches"] = {}
        for b in batches:
            tf.device.verify_inclusion_proofs(heights[:b], lo[: b + 1], li, ld, ao[: b + 1], ad, roots, st)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.reps):
                tf.device.verify_inclusion_proofs(heights[:b], lo[: b + 1], li, ld, ao[: b + 1], ad, roots, st)
            e1.record()
            torch.cuda.synchronize()
            ms = e0.elapsed_time(e1) / args.reps
            pairs = sum(hash_pairs_needed(height, idx_all[i]) for i in range(b))
            x = oracle.fill_random(10 * min(pairs, 200000), 0xC0DE + b)
            t0 = time.perf_counter()
            oracle.hash_pairs(x)
            cpu_s = (time.perf_counter() - t0) * pairs / min(pairs, 200000)
            shape["batches"][str(b)] = {"ms_per_call": round(ms, 4), "proofs_per_s": round(b / (ms * 1e-3), 1), "hash_pairs": pairs,
                                        "cpu_one_core_hash_pairs_ms_lower_bound": round(cpu_s * 1e3, 3),
                                        "cpu_lower_bound_proofs_per_s": round(b / cpu_s, 1), "parity": parity(b)}
        res["shapes"][f"height_{height}"] = shape
        del leaves, nodes, nv
        torch.cuda.empty_cache()
    res["note"] = ("single_* = wall-clock of one call on the host, median of --calls warm calls; batches = HIP events around --reps calls; "
                   "cpu_one_core = oracle hash_pairs on one core over the same number of pairs (a lower bound for the reference's "
                   "sequential verify, which also does hash-map work)")
    line = json.dumps(res, indent=1)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
