#!/usr/bin/env python3
"""MMR successor proofs and membership proofs under appends, each beside what the library offered for the same result before.
In one process, between HIP events (the host's planning is inside the interval), median of --reps warm calls after a warm-up:
  successor   tf_mmr_successor_proof_new_dev with the new peaks, (n, k) = (2^20 + 2^10, 2^20) and (3, 2^24), against one
              tf_merkle_root_dev per proof digest plus tf_mmr_append_dev (a digest that is a single leaf is a copy there);
  verify      tf_mmr_verify_successor_proofs_dev of 2^16 proofs of old counts near 2^40 (synthetic digests: every chain is hashed
              to its end and then fails the comparison, which costs what a match costs), against the oracle's hash_pairs over as many
              pairs on one host core in the same run;
  update      tf_mmr_update_proofs_from_append_dev of 2^20 proofs, n = 2^20 + 12345, k in {1, 64, 2^16} (synthetic paths of the right
              lengths), against a device-to-device copy of the output's size as the floor.
usage: mmr_successor_times.py [--reps 10] [--out profiles/mmr_successor_bench.json]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)


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
    return {"median_ms": statistics.median(times), "min_ms": min(times), "max_ms": max(times)}


def random_words(tf, words, seed):
    import torch

    t = torch.empty(max(words, 5), dtype=torch.int64, device="cuda")
    tf.device.fill_random(t, seed)
    return t


def proof_subtrees(n, k):
    """(first new leaf, leafs) of every digest of the successor proof: the roots new_from_batch_append takes one tree at a time."""
    t = (n & -n).bit_length() - 1
    if n == 0 or k < 1 << t:
        return []
    H = (n ^ (n + k)).bit_length() - 1
    out = [(0, 1 << t)]
    for g in range(t, H):
        if not (n >> g) & 1:
            out.append(((((n >> g) + 1) << g) - n, 1 << g))
    return out


def successor(tf, reps):
    import torch

    res = []
    for n, k in (((1 << 20) + (1 << 10), 1 << 20), (3, 1 << 24)):
        leafs = random_words(tf, 5 * k, 0x5CC0 + n)
        old = random_words(tf, 5 * bin(n).count("1"), 0x5CC1 + n)
        length = tf.device.mmr_successor_proof_len(n, k)
        paths, peaks = torch.zeros(5 * length, dtype=torch.int64, device="cuda"), torch.zeros(5 * bin(n + k).count("1"), dtype=torch.int64, device="cuda")
        paths_b, peaks_b = torch.zeros_like(paths), torch.zeros_like(peaks)
        runs = proof_subtrees(n, k)
        assert len(runs) == length

        def per_subtree():
            for d, (first, size) in enumerate(runs):
                if size == 1:
                    paths_b[5 * d: 5 * d + 5].copy_(leafs[5 * first: 5 * first + 5])
                else:
                    tf.device.merkle_root(leafs[5 * first: 5 * (first + size)], size, paths_b[5 * d: 5 * d + 5])
            tf.device.mmr_append(n, old, leafs, peaks_b)

        one = timed(lambda: tf.device.mmr_successor_proof_new(n, old, leafs, paths, peaks), reps)
        many = timed(per_subtree, reps)
        append_only = timed(lambda: tf.device.mmr_append(n, old, leafs, peaks_b), reps)
        res.append({"old_leafs": n, "new_leafs": k, "proof_digests": length, "one_call": one, "root_per_digest_plus_append": many,
                    "append_alone": append_only, "same_words": bool(torch.equal(paths, paths_b) and torch.equal(peaks, peaks_b))})
        print(json.dumps(res[-1]), file=sys.stderr)
        del leafs
        torch.cuda.empty_cache()
    return res


def verify(tf, reps):
    import numpy as np
    import torch

    from oracle import tfo

    P = 1 << 16
    rng = np.random.default_rng(40)
    n = (1 << 40) + rng.integers(1, 1 << 20, size=P, dtype=np.uint64)
    k = rng.integers(1 << 20, 1 << 30, size=P, dtype=np.uint64)
    N = n + k
    pop = lambda a: np.array([bin(int(x)).count("1") for x in a], dtype=np.uint64)  # noqa: E731
    lens = np.array([tf.device.mmr_successor_proof_len(int(a), int(b)) for a, b in zip(n, k)], dtype=np.uint64)
    steps = sum((int(a) ^ int(b)).bit_length() - 1 - ((int(a) & -int(a)).bit_length() - 1) for a, b in zip(n, N))
    off = lambda c: np.concatenate([[0], np.cumsum(c)]).astype(np.uint64)  # noqa: E731
    oo, no, po = off(pop(n)), off(pop(N)), off(lens)
    # shared peaks equal (copied), everything else random: every proof passes the host's checks and the shared-peak comparison
    old = rng.integers(0, 0xFFFFFFFF00000001, size=(int(oo[-1]), 5), dtype=np.uint64)
    new = rng.integers(0, 0xFFFFFFFF00000001, size=(int(no[-1]), 5), dtype=np.uint64)
    for p in range(P):
        shared = bin(int(n[p]) >> ((int(n[p]) ^ int(N[p])).bit_length())).count("1")
        new[int(no[p]): int(no[p]) + shared] = old[int(oo[p]): int(oo[p]) + shared]
    d_old, d_new = torch.from_numpy(old.view(np.int64)).cuda(), torch.from_numpy(new.view(np.int64)).cuda()
    d_paths = random_words(tf, 5 * int(po[-1]), 0x5CC7)
    st = torch.zeros(P, dtype=torch.int32, device="cuda")
    call = timed(lambda: tf.device.mmr_verify_successor_proofs(n, N, oo, d_old, no, d_new, po, d_paths, st), reps)
    statuses = sorted(set(st.cpu().tolist()))
    pairs = rng.integers(0, 0xFFFFFFFF00000001, size=(1 << 16, 10), dtype=np.uint64)
    t0 = time.perf_counter()
    tfo.hash_pairs(pairs)
    per_pair = (time.perf_counter() - t0) / (1 << 16)
    res = {"proofs": P, "old_leafs": "2^40 + (1 .. 2^20)", "new_minus_old": "2^20 .. 2^30", "hash_pairs_in_all": steps, "path_digests": int(po[-1]),
           "call": call, "statuses_seen": statuses, "one_host_core_ms": per_pair * steps * 1e3,
           "one_host_core_note": "the oracle's hash_pairs timed over 2^16 pairs in this run, scaled to hash_pairs_in_all"}
    print(json.dumps(res), file=sys.stderr)
    return res


def update(tf, reps):
    import numpy as np
    import torch

    P, n = 1 << 20, (1 << 20) + 12345
    rng = np.random.default_rng(41)
    idx = rng.integers(0, n, size=P, dtype=np.uint64)
    old_len = np.array([(int(i) ^ n).bit_length() - 1 for i in idx], dtype=np.uint64)
    own_off = np.concatenate([[0], np.cumsum(old_len)]).astype(np.uint64)
    d_own = random_words(tf, 5 * int(own_off[-1]), 0x5CC8)
    d_old = random_words(tf, 5 * bin(n).count("1"), 0x5CC9)
    res = []
    for k in (1, 64, 1 << 16):
        d_leafs = random_words(tf, 5 * k, 0x5CCA + k)[: 5 * k]
        out_off, mod = tf.device.mmr_update_proofs_from_append(n, d_old, d_leafs, idx, own_off, d_own)
        total = int(out_off[-1])
        d_out = torch.zeros(5 * total, dtype=torch.int64, device="cuda")
        d_peaks = torch.zeros(5 * bin(n + k).count("1"), dtype=torch.int64, device="cuda")
        call = timed(lambda: tf.device.mmr_update_proofs_from_append(n, d_old, d_leafs, idx, own_off, d_own, d_out, d_peaks), reps)
        t0 = time.perf_counter()
        tf.device.mmr_update_proofs_from_append(n, d_old, d_leafs, idx, own_off, d_own, d_out, d_peaks)
        enqueue_ms = (time.perf_counter() - t0) * 1e3
        torch.cuda.synchronize()
        src = torch.zeros_like(d_out)
        copy = timed(lambda: d_out.copy_(src), reps)
        res.append({"proofs": P, "old_leafs": n, "new_leafs": k, "proofs_that_grew": int(mod.sum()), "digests_in": int(own_off[-1]), "digests_out": total,
                    "bytes_out": 40 * total, "call": call, "host_time_of_the_call_ms": enqueue_ms, "device_copy_of_the_output": copy})
        print(json.dumps(res[-1]), file=sys.stderr)
        del d_out, src
        torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import twenty_first_amd as tf

    rec = {"what": "MMR successor proofs (one sweep vs one root per digest + append), their verification (vs one host core) and membership "
                   "proofs under appends (vs a device copy of the output): HIP events around the call, median of warm calls",
           "source_hash": tf.lib().tf_source_hash().decode(), "reps": args.reps, "successor": successor(tf, args.reps),
           "verify": verify(tf, args.reps), "update": update(tf, args.reps)}
    text = json.dumps(rec, indent=1)
    if args.out:
        open(args.out, "w").write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
