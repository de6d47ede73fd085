#!/usr/bin/env python3
"""The measurements behind DESIGN 7.6: the FRI fold against what it replaces, inputs from tf_debug_fill_random_dev, every figure the
median over --reps steps of ten calls between two HIP events, per call, after --warmup rounds; the two sides of each comparison
alternate within one process on the same words, and their outputs must be the same words.

  one level        fri.fold, levels = 1, against the composition a caller had before: tf_powers_dev twice (the domain halves x and
                   -x) and tf_get_colinear_y_dev in its (1, 3) form with the challenge as p2x -- three launches and two n/2-element
                   domain arrays written and read back.  For the (1, 3) fold the composition reads the lifted codeword (the lift is
                   not timed); for (3, 3) it reads the codeword itself.
  several levels   fri.fold, levels = 2, 3, 4, against the chain of single-level fri.fold calls (intermediates allocated once).

Sizes n = 2^21 (2^20 pairs, the size of DESIGN 7.4), 2^20 and 2^10; forms (1, 3) and (3, 3).  Each record carries the bytes the call
must move (codewords in, result out, intermediates out and in again) and their floor at the 6.29 TB/s of DESIGN 7.2.

R_max, the levels one launch folds, is a compile-time constant (TF_FRI_MAX_LEVELS of csrc/fri_kernels.h).  With --candidates every
library listed is measured in a fresh process of its own (through TF_HIP_LIBRARY, the variable _lib.py reads) and the records are
merged; `make -C twenty-first_amd/csrc fri_candidates` builds libtf_hip_fri2.so, _fri3.so and _fri4.so.  Without it the product
library is measured alone.

usage: fri_fold_times.py [--reps 20] [--warmup 3] [--candidates LIB[,LIB...]] [--out profiles/fri_fold_times.json]"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

CALLS = 10  # calls per timed step: one call is tens of microseconds, too close to the events' own resolution
BANDWIDTH = 6.29e12  # bytes per second, the figure DESIGN 7.2 and 7.4 price against
SIZES = (21, 20, 10)
FORMS = ((1, 3), (3, 3))
CHILD_TIMEOUT = 240  # seconds per measured library


def _timed(fn):
    """ms per call of a step of CALLS calls between two HIP events"""
    import torch

    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(CALLS):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / CALLS


def _alternate(a, b, warmup, reps):
    import torch

    for _ in range(warmup):
        a()
        b()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(reps):
        ta.append(_timed(a))
        tb.append(_timed(b))
    return ta, tb


def _side(ms, nbytes, launches):
    """median, and the spread of the steps around it, of one side of a comparison"""
    return {"ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "launches": launches, "bytes": nbytes,
            "floor_us": nbytes / BANDWIDTH * 1e6}


def fold_bytes(n, wc, wa, passes):
    """bytes a fold of these passes must move: every pass reads its input and writes its output once"""
    total, w = 0, wc
    for r in passes:
        total += 8 * (n * w + (n >> r) * wa)
        n, w = n >> r, wa
    return total


def _rnd(tf, words, seed):
    import torch

    t = torch.empty(words, dtype=torch.int64, device="cuda")
    tf.device.fill_random(t, seed)
    return t


def one_level(tf, log_n, wc, wa, warmup, reps):
    import torch

    n, h = 1 << log_n, 1 << (log_n - 1)
    g = tf.BFieldElement.new(7)
    cw, ch = _rnd(tf, n * wc, 0xF0 + wc), _rnd(tf, wa, 0xF4)
    y = cw
    if wc != wa:  # the composition has no BFieldElement y next to an XFieldElement p2x: it reads the lift
        y = torch.zeros(n * wa, dtype=torch.int64, device="cuda")
        y[::wa] = cw
    x0, x1 = torch.empty(h, dtype=torch.int64, device="cuda"), torch.empty(h, dtype=torch.int64, device="cuda")
    w_raw, minus_g = tf.BFieldElement.primitive_root_of_unity(n), tf.BFieldElement.new(tf.P - 7)
    st = torch.zeros(1, dtype=torch.int32, device="cuda")
    folded, composed = torch.empty(h * wa, dtype=torch.int64, device="cuda"), torch.empty(h * wa, dtype=torch.int64, device="cuda")

    def run_fold():
        tf.fri.fold(cw, n, g, ch, folded, width_c=wc, width_a=wa)

    def run_composed():
        tf.device.powers(g, w_raw, x0)
        tf.device.powers(minus_g, w_raw, x1)
        tf.device.get_colinear_y(x0, y[:h * wa], x1, y[h * wa:], ch, composed, width_x=1, width_y=wa, status=st)

    t_fold, t_comp = _alternate(run_fold, run_composed, warmup, reps)
    torch.cuda.synchronize()
    assert int(st.item()) == 0
    comp_bytes = 8 * (2 * h + 2 * h + n * wa + h * wa)  # the domain halves written and read, y0 and y1 read, the result written
    rec = {"comparison": "one level against the composition", "log_n": log_n, "width_c": wc, "width_a": wa, "levels": 1,
           "fold": _side(t_fold, fold_bytes(n, wc, wa, [1]), 1), "composed": _side(t_comp, comp_bytes, 3),
           "same_words": bool(torch.equal(folded, composed))}
    rec["speedup"] = rec["composed"]["ms"] / rec["fold"]["ms"]
    return rec


def several_levels(tf, log_n, wc, wa, levels, warmup, reps):
    import torch

    n = 1 << log_n
    g = tf.BFieldElement.new(7)
    cw, ch = _rnd(tf, n * wc, 0xE0 + wc), _rnd(tf, levels * wa, 0xE4)
    steps = [torch.empty((n >> r) * wa, dtype=torch.int64, device="cuda") for r in range(1, levels + 1)]
    folded = torch.empty((n >> levels) * wa, dtype=torch.int64, device="cuda")
    offsets = [g]
    for _ in range(levels - 1):
        offsets.append(tf.BFieldElement.new(tf.BFieldElement.value(offsets[-1]) ** 2 % tf.P))

    def run_fold():
        tf.fri.fold(cw, n, g, ch, folded, levels=levels, width_c=wc, width_a=wa)

    def run_chain():
        src, w = cw, wc
        for r in range(levels):
            tf.fri.fold(src, n >> r, offsets[r], ch[r * wa:(r + 1) * wa], steps[r], width_c=w, width_a=wa)
            src, w = steps[r], wa

    t_fold, t_chain = _alternate(run_fold, run_chain, warmup, reps)
    torch.cuda.synchronize()
    passes = tf.fri.plan(n, levels, wc, wa)
    rec = {"comparison": "several levels against the chain of single folds", "log_n": log_n, "width_c": wc, "width_a": wa, "levels": levels,
           "passes": passes, "fold": _side(t_fold, fold_bytes(n, wc, wa, passes), len(passes)),
           "chain": _side(t_chain, fold_bytes(n, wc, wa, [1] * levels), levels), "same_words": bool(torch.equal(folded, steps[-1]))}
    rec["speedup"] = rec["chain"]["ms"] / rec["fold"]["ms"]
    return rec


def measure(warmup, reps):
    """everything, for the library this process has loaded"""
    import torch

    import twenty_first_amd as tf

    if not torch.cuda.is_available() or tf.lib().tf_device_count() == 0:
        raise SystemExit("fri_fold_times.py needs a GPU: a time from anything else says nothing")
    rmax = max(tf.fri.plan(1 << 12, 12))
    records = []
    for log_n in SIZES:
        for wc, wa in FORMS:
            records.append(one_level(tf, log_n, wc, wa, warmup, reps))
            for levels in (2, 3, 4):
                records.append(several_levels(tf, log_n, wc, wa, levels, warmup, reps))
    return {"r_max": rmax, "library": os.path.basename(tf._lib.SO_PATH), "source_hash": tf.lib().tf_source_hash().decode(), "records": records}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--candidates", default=None, help="comma-separated libraries, each measured in a fresh process of its own")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        print(json.dumps(measure(args.warmup, args.reps)))
        return
    runs = []
    if args.candidates:
        for lib in args.candidates.split(","):
            env = dict(os.environ, TF_HIP_LIBRARY=os.path.abspath(lib))
            cmd = [sys.executable, os.path.abspath(__file__), "--child", "--reps", str(args.reps), "--warmup", str(args.warmup)]
            done = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, timeout=CHILD_TIMEOUT)  # (a failure ends the whole run)
            if done.returncode:
                raise SystemExit(f"measuring {lib} failed with status {done.returncode}")
            runs.append(json.loads(done.stdout.decode().strip().splitlines()[-1]))
    else:
        runs.append(measure(args.warmup, args.reps))
    rec = {"what": "fri.fold against the composition (two powers, one get_colinear_y) and against the chain of single-level folds; median ms per "
                   "call of warm steps between HIP events, min and max of the steps next to it",
           "reps": args.reps, "calls_per_step": CALLS, "warmup": args.warmup, "bandwidth_bytes_per_s": BANDWIDTH, "runs": runs}
    text = json.dumps(rec, indent=1)
    if args.out:
        open(args.out, "w").write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
