#!/usr/bin/env python3
"""Polynomial arithmetic on the GPU (tf_poly_*_dev, include/tf_hip.h "Polynomial arithmetic") at the prover's shapes:
  linear combination   k = 256 BFieldElement columns of 2^20 with XFieldElement weights; k = 64 XFieldElement columns of 2^20 with
                       XFieldElement weights; the latency shape n = 2^10, k = 500 (BFieldElement columns, XFieldElement weights)
  scale, scalar_mul    2^24 BFieldElements, 2^23 XFieldElements (scalar of the coefficients' field)
  add                  2^24 BFieldElements
For every shape: `ms` (median of --reps warm calls of the _dev form between HIP events), the bytes the call has to move, that traffic
over the time as a fraction of the 6.29 TB/s the project prices against, and a device-to-device copy moving the same bytes in the
same run.  For the linear combination also the unfused chain (k x scalar_mul + add) in the same run; outputs are hashed: both must
return the same words.  (The comparison of the deferred-reduction kernel with one product and one modular addition per term is
recorded in profiles/poly_algebra_bench.json.)
  --trace: a short run (one warm-up and two calls per shape, synchronised) for `rocprofv3 --kernel-trace --stats` (a run of its own).
usage: poly_algebra_times.py [--reps 20] [--out profiles/poly_algebra_bench.json] [--trace]"""
import argparse
import hashlib
import json
import os
import statistics
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

COPY_RATE = 6.29e12  # bytes/s, MI355X float4 copy (the chip's measured HBM rate)
LINCOMB = [("lincomb_bfe256_xfe_weights", 1 << 20, 256, 1, 3), ("lincomb_xfe64_xfe_weights", 1 << 20, 64, 3, 3),
           ("lincomb_latency_n1024_k500", 1 << 10, 500, 1, 3)]
ELEMENTWISE = [("scale", 1, 1 << 24), ("scale", 3, 1 << 23), ("scalar_mul", 1, 1 << 24), ("scalar_mul", 3, 1 << 23), ("add", 1, 1 << 24)]


def _time(fn, calls):
    import torch

    fn()  # warm-up
    torch.cuda.synchronize()
    times = []
    for _ in range(calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return statistics.median(times)


def _copy_ms(bytes_moved, calls):
    """a device-to-device copy whose reads plus writes are `bytes_moved`"""
    import torch

    words = max(bytes_moved // 16, 1)
    src = torch.empty(words, dtype=torch.int64, device="cuda")
    dst = torch.empty_like(src)
    return _time(lambda: dst.copy_(src), calls)


def _sha(t):
    return hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()[:16]


def _entry(name, ms, bytes_moved, calls, **more):
    e = {"shape": name, "ms": ms, "reps": calls, "hbm_bytes": bytes_moved, "frac_of_6.29TBps": bytes_moved / (ms * 1e-3) / COPY_RATE}
    e.update(more)
    return e


def measure_lincomb(reps, trace):
    import torch

    import twenty_first_amd as tf

    d = tf.device
    calls = 2 if trace else reps
    res = []
    for name, n, k, wp, ww in LINCOMB:
        wo = max(wp, ww)
        cols = torch.empty(k * n * wp, dtype=torch.int64, device="cuda")
        d.fill_random(cols, 0xA16 + k)
        wts = torch.empty(k * ww, dtype=torch.int64, device="cuda")
        d.fill_random(wts, 0xA17 + k)
        out = torch.empty(n * wo, dtype=torch.int64, device="cuda")
        run = lambda: d.linear_combination(cols, n, k, wts, out, width=wp, width_w=ww)  # noqa: E731
        bytes_moved = 8 * (k * n * wp + k * ww + n * wo)
        e = _entry(name, _time(run, calls), bytes_moved, calls, n=n, k=k, width_p=wp, width_w=ww, words_sha256=_sha(out))
        if not trace:
            e["copy_ms"] = _copy_ms(bytes_moved, calls)
            wts_host = wts.cpu().numpy().view("uint64")
            acc = torch.empty(n * wo, dtype=torch.int64, device="cuda")
            term = torch.empty(n * wo, dtype=torch.int64, device="cuda")

            def chain():
                acc.zero_()
                for j in range(k):
                    d.poly_scalar_mul(cols[j * n * wp:(j + 1) * n * wp], n, wts_host[j * ww:(j + 1) * ww], term, width=wp, width_s=ww)
                    d.poly_add(acc, n, term, n, acc, width=wo)

            e["chain_ms"] = _time(chain, max(3, calls // 4))
            e["chain_same_words"] = _sha(acc) == e["words_sha256"]
        res.append(e)
        print(json.dumps(e), file=sys.stderr)
        del cols, out
    return res


def measure_elementwise(reps, trace):
    import torch

    import twenty_first_amd as tf

    d = tf.device
    calls = 2 if trace else reps
    res = []
    for op, w, n in ELEMENTWISE:
        a = torch.empty(n * w, dtype=torch.int64, device="cuda")
        d.fill_random(a, 0xA18 + n + w)
        out = torch.empty_like(a)
        s = a[:w].cpu().numpy().view("uint64").copy()
        if op == "add":
            b = torch.empty_like(a)
            d.fill_random(b, 0xA19)
            run, bytes_moved = (lambda: d.poly_add(a, n, b, n, out, width=w)), 24 * n * w
        elif op == "scale":
            run, bytes_moved = (lambda: d.poly_scale(a, n, s, out, width=w, width_alpha=w)), 16 * n * w
        else:
            run, bytes_moved = (lambda: d.poly_scalar_mul(a, n, s, out, width=w, width_s=w)), 16 * n * w
        e = _entry(f"{op}_{'bfe' if w == 1 else 'xfe'}_2p{n.bit_length() - 1}", _time(run, calls), bytes_moved, calls, n=n, width=w)
        if not trace:
            e["copy_ms"] = _copy_ms(bytes_moved, calls)
        res.append(e)
        print(json.dumps(e), file=sys.stderr)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace", action="store_true")
    args = ap.parse_args()
    if args.trace:
        print(json.dumps(measure_lincomb(args.reps, True) + measure_elementwise(args.reps, True)))
        return
    import twenty_first_amd as tf

    rec = {"what": "polynomial arithmetic, tf_poly_*_dev between HIP events, median of warm calls",
           "source_hash": tf.lib().tf_source_hash().decode(), "copy_rate_bytes_per_s": COPY_RATE,
           "linear_combination": measure_lincomb(args.reps, False), "elementwise": measure_elementwise(args.reps, False)}
    text = json.dumps(rec, indent=1)
    if args.out:
        open(args.out, "w").write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
