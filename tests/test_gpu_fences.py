"""Where the device entry points touch memory: every public function of twenty-first_amd/device.py (the methods of ZerofierTree
included) runs inside the guard-word arena of tests/fence.py -- 20 480 poisoned words (more than any kernel's per-workgroup tile) in front of and behind every tensor argument,
the payload on a 16-byte boundary and one word off it, three poisons (zero, all ones, canonical pseudo-random words), every pure
output poisoned as well.  One synchronisation, then: the guards are untouched, the const inputs are as uploaded, every output word
is the reference's, and the slots the documentation leaves "as they were" (and the padding of strided operands) hold their poison.

The file is a table, ROWS: entry point -> (cases, generator); the generator yields (shape, operands, call) for its case.  The
expected values come from the references the suite already trusts -- oracle.tfo, tests/algebra_ref, points_ref, inversion_ref,
sponge_ref and the Merkle / MMR models of the existing tests --, never from another call into the library.  The shapes straddle the
boundaries the kernel headers name, one count below, at and above; nothing exceeds 2^16 points or 2^17 words per tensor.
tests/test_fence_cpu.py proves on CPU tensors that the harness reports each kind of defect, and fails when device.py grows a public
callable without a row here.  No row here can see the library's own pool temporaries or the host-pointer / numpy API: those are
fenced inside the library (tf_debug_temp_guard), and tests/test_gpu_temp_guard.py runs every row of this table again with that mode
on.  What remains unseen after both: memory the library keeps for the life of the process (cached tables, Tip5 constants, a
persistent zerofier-tree arena) and its page-locked staging blocks."""
import itertools

import numpy as np
import pytest

from tests import algebra_ref, fence, inversion_ref, points_ref, sponge_ref
from tests.test_gpu_poly_algebra import COMBOS, LENGTHS, SCALE_RUN   # the boundaries of the algebra kernels, kept in one place

P = fence.P
ROWS = {}
ORDERS = [(1, 1), (3, 4), (11, 16), (700, 1024), (1024, 1024)]
HEIGHTS = [0, 1, 2, 3, 6, 10, 12]
TIP5_COUNTS = [1, 7, 8, 9, 15, 17, 2047, 2049]
TREE_SIZES = [1, 2, 127, 128, 129, 257, 1025]
DIVIDE_SHAPES = [(3, 5), (7, 2), (40, 17), (700, 600), (5000, 257)]


def row(names, cases):
    """register a generator of (shape, operands, call) triples: under one entry point's name, or -- names a dict -- under the name
    its cases' first element selects"""
    def register(gen):
        for tag, name in (names.items() if isinstance(names, dict) else [(None, names)]):
            assert name not in ROWS, name
            ROWS[name] = ([c for c in cases if tag is None or c[0] == tag], gen)
            assert ROWS[name][0], name
        return gen
    return register


def rnd(oracle, words, seed):
    return oracle.fill_random(words, seed) if words else np.zeros(0, dtype=np.uint64)


def cat(parts, dtype=np.uint64):
    parts = [np.asarray(p, dtype=dtype).reshape(-1) for p in parts]
    return np.concatenate(parts) if parts else np.zeros(0, dtype=dtype)


def i32(values):
    return np.asarray(values, dtype=np.int32).reshape(-1)


def status_kept():
    """a status word nobody pre-set: a clean call leaves it as it was (the first non-zero code wins, zero is never written)"""
    return fence.out("status", i32([0]), dtype="int32", kept=[True])


def switched(lib, setter, value, restore, call):
    """`call` under one of the library's routing switches, restored afterwards as the existing tests do"""
    def run(**t):
        getattr(lib, setter)(value)
        try:
            call(**t)
        finally:
            getattr(lib, setter)(restore)
    return run


# ------------------------------------------------------------------ synthetic inputs
@row("fill_random", cases=[1, 255, 257, 1025])
def _fill_random(tf, oracle, d, n):
    for first in (0, 5):
        yield f"n={n} first={first}", [fence.out("out", oracle.fill_random(n, 0xF11, first))], lambda out, first=first: d.fill_random(out, 0xF11, first)


# ------------------------------------------------------------------ NTT
def _ntt_cases():
    c = [(w, inv, n, batch, None) for w in (1, 3) for inv in (False, True) for n in (2, 8, 32, 64) for batch in (1, 21, 22, 65)]
    c += [(w, inv, n, batch, None) for w in (1, 3) for inv in (False, True) for n in (1 << 7, 1 << 10, 1 << 12, 1 << 13, 1 << 15) for batch in (1, 3)
          if n * batch * w <= 1 << 17]
    c += [(1, inv, 1 << 16, 1, ("tf_set_ntt_small_launch", mode, -1)) for inv in (False, True) for mode in (0, 1)]
    c += [(w, inv, 1 << 15, 1, ("tf_set_ntt_min_passes", 3, 0)) for w in (1, 3) for inv in (False, True)]
    return c


@row("ntt_", cases=_ntt_cases())
def _ntt(tf, oracle, d, w, inv, n, batch, switch):
    x = rnd(oracle, n * batch * w, 0x1000 + n + batch)
    call = lambda x: d.ntt_(x, n, batch=batch, width=w, inverse=inv)  # noqa: E731
    if switch:
        call = switched(tf.lib(), *switch, call)
    yield f"w={w} inverse={inv} n={n} batch={batch} {switch}", [fence.inout("x", x, oracle.ntt(x, width=w, inverse=inv, batch=batch))], call


@row("coset_evaluate", cases=[(w, batch) for w in (1, 3) for batch in (1, 3)])
def _coset_evaluate(tf, oracle, d, w, batch):
    off = oracle.bfe_new(7)
    for nc, order in ORDERS:
        c = rnd(oracle, nc * batch * w, 0x1100 + nc)
        want = oracle.coset_evaluate_batch(c, off, order, batch, width=w)
        yield (f"w={w} batch={batch} n_coeffs={nc} order={order}", [fence.inp("coeffs", c), fence.out("out", want)],
               lambda coeffs, out, nc=nc, order=order: d.coset_evaluate(coeffs, nc, off, out, order, batch=batch, width=w))


@row("coset_interpolate", cases=[(w, batch) for w in (1, 3) for batch in (1, 3)])
def _coset_interpolate(tf, oracle, d, w, batch):
    off = oracle.bfe_new(7)
    for n in (1, 4, 16, 1024):
        v = rnd(oracle, n * batch * w, 0x1200 + n)
        want = cat([oracle.coset_interpolate(r, off, width=w) for r in v.reshape(batch, -1)])
        yield (f"w={w} batch={batch} n={n}", [fence.inp("values", v), fence.out("out", want)],
               lambda values, out, n=n: d.coset_interpolate(values, n, off, out, batch=batch, width=w))
        yield (f"w={w} batch={batch} n={n} in place", [fence.inout("values", v, want)],
               lambda values, n=n: d.coset_interpolate(values, n, off, values, batch=batch, width=w))


@row("lde", cases=[(w, batch) for w in (1, 3) for batch in (1, 3)])
def _lde(tf, oracle, d, w, batch):
    one, seven = oracle.bfe_new(1), oracle.bfe_new(7)
    for n, m in ((1, 1), (4, 4), (16, 64), (1024, 1024), (256, 1024)):
        v = rnd(oracle, n * batch * w, 0x1300 + n)
        want = cat([oracle.coset_evaluate(oracle.coset_interpolate(r, one, width=w), seven, m, width=w) for r in v.reshape(batch, -1)])
        yield (f"w={w} batch={batch} n={n} m={m}", [fence.inp("values", v), fence.out("out", want)],
               lambda values, out, n=n, m=m: d.lde(values, n, one, out, m, seven, batch=batch, width=w))


def _evaluate(oracle, coeffs, points, w):
    """f(points[i]) by the oracle's Horner, f and the points of one width"""
    if coeffs.size == 0:
        return np.zeros(points.size, dtype=np.uint64)
    if w == 1:
        return cat([oracle.poly_eval(coeffs, int(p)) for p in points])
    return cat([oracle.poly_eval_xfe_point(coeffs, points[3 * i:3 * i + 3]) for i in range(points.size // 3)])


@row("coset_extrapolate", cases=[(w, batch) for w in (1, 3) for batch in (1, 3)])
def _coset_extrapolate(tf, oracle, d, w, batch):
    off = oracle.bfe_new(7)
    for n, n_points in ((1, 1), (4, 7), (16, 65), (1024, 130)):
        cw, pts = rnd(oracle, n * batch * w, 0x1400 + n), rnd(oracle, n_points * w, 0x1401 + n)
        want = cat([_evaluate(oracle, oracle.coset_interpolate(r, off, width=w), pts, w) for r in cw.reshape(batch, -1)])
        yield (f"w={w} batch={batch} n={n} points={n_points}", [fence.inp("codewords", cw), fence.inp("points", pts), fence.out("out", want)],
               lambda codewords, points, out, n=n: d.coset_extrapolate(off, codewords, n, points, out, batch=batch, width=w))


# ------------------------------------------------------------------ pointwise products and the algebra unit
@row("hadamard", cases=[(1, 1), (3, 3), (3, 1)])
def _hadamard(tf, oracle, d, wa, wb):
    for n in (1, 2, 7, 255, 256, 257, 1025):
        a, b = rnd(oracle, n * wa, 0x2000 + n), rnd(oracle, n * wb, 0x2001 + n)
        want = oracle.hadamard(a, b, width=wa) if wa == wb else algebra_ref.hadamard_xfe_bfe(a, b)
        shape = f"widths=({wa},{wb}) n={n}"
        yield (shape, [fence.inp("a", a), fence.inp("b", b), fence.out("out", want)],
               lambda a, b, out: d.hadamard(a, b, out, width=wa, width_b=wb))
        yield (shape + " out=a", [fence.inout("a", a, want), fence.inp("b", b)], lambda a, b: d.hadamard(a, b, a, width=wa, width_b=wb))
        if wa == wb:
            yield (shape + " out=b", [fence.inp("a", a), fence.inout("b", b, want)], lambda a, b: d.hadamard(a, b, b, width=wa, width_b=wb))


@row({"add": "poly_add", "sub": "poly_sub"}, cases=[(op, w, batch) for op in ("add", "sub") for w in (1, 3) for batch in (1, 3)])
def _poly_add_sub(tf, oracle, d, op, w, batch):
    fn, ref = (d.poly_add, algebra_ref.add) if op == "add" else (d.poly_sub, algebra_ref.sub)
    for n in LENGTHS:
        short = n // 2 + 1
        for na, nb in sorted({(n, n), (n, short), (short, n)}):
            a, b = rnd(oracle, na * batch * w, 0x3000 + n), rnd(oracle, nb * batch * w, 0x3100 + n)
            want = ref(a, na, b, nb, w, batch)
            shape = f"{op} w={w} batch={batch} na={na} nb={nb}"
            yield (shape, [fence.inp("a", a), fence.inp("b", b), fence.out("out", want)],
                   lambda a, b, out, na=na, nb=nb: fn(a, na, b, nb, out, batch=batch, width=w))
            if na >= nb:
                yield (shape + " out=a", [fence.inout("a", a, want), fence.inp("b", b)],
                       lambda a, b, na=na, nb=nb: fn(a, na, b, nb, a, batch=batch, width=w))


@row("poly_neg_", cases=[(w, batch) for w in (1, 3) for batch in (1, 3)])
def _poly_neg(tf, oracle, d, w, batch):
    for n in LENGTHS:
        a = rnd(oracle, n * batch * w, 0x3200 + n)
        want = algebra_ref.neg(a, w)
        yield f"w={w} batch={batch} n={n}", [fence.inp("a", a), fence.out("out", want)], lambda a, out, n=n: d.poly_neg_(a, n, out, batch=batch, width=w)
        yield f"w={w} batch={batch} n={n} in place", [fence.inout("a", a, want)], lambda a, n=n: d.poly_neg_(a, n, batch=batch, width=w)


@row({"scalar_mul": "poly_scalar_mul", "scale": "poly_scale"}, cases=[(op, wa, ws, batch) for op in ("scalar_mul", "scale") for wa, ws in COMBOS for batch in (1, 3)])
def _poly_by_scalar(tf, oracle, d, op, wa, ws, batch):
    lengths = list(LENGTHS)
    if op == "scale" and (wa, ws) == (1, 1) and batch == 1:
        lengths += [512 * SCALE_RUN[1] - 1, 512 * SCALE_RUN[1] + 1]   # where a row's thread count doubles
    for n in lengths:
        a, s = rnd(oracle, n * batch * wa, 0x3300 + n), rnd(oracle, ws, 0x3400 + n)
        if op == "scalar_mul":
            want, fn = algebra_ref.scalar_mul(a, wa, s, ws), lambda a, out, n=n, s=s: d.poly_scalar_mul(a, n, s, out, batch=batch, width=wa, width_s=ws)
        else:
            want, fn = algebra_ref.scale(a, n, wa, s, ws, batch), lambda a, out, n=n, s=s: d.poly_scale(a, n, s, out, batch=batch, width=wa, width_alpha=ws)
        shape = f"{op} widths=({wa},{ws}) batch={batch} n={n}"
        yield shape, [fence.inp("a", a), fence.out("out", want)], fn
        if wa >= ws:
            yield shape + " in place", [fence.inout("a", a, want)], lambda a, fn=fn: fn(a, a)


@row("poly_formal_derivative", cases=[(w, batch) for w in (1, 3) for batch in (1, 3)])
def _poly_derivative(tf, oracle, d, w, batch):
    for n in LENGTHS:
        a = rnd(oracle, n * batch * w, 0x3500 + n)
        yield (f"w={w} batch={batch} n={n}", [fence.inp("a", a), fence.out("out", algebra_ref.formal_derivative(a, n, w, batch))],
               lambda a, out, n=n: d.poly_formal_derivative(a, n, out, batch=batch, width=w))


@row("poly_degree", cases=[(w, batch) for w in (1, 3) for batch in (1, 3)])
def _poly_degree(tf, oracle, d, w, batch):
    for n in LENGTHS:
        a = rnd(oracle, n * batch * w, 0x3600 + n).reshape(batch, n, w)
        for r in range(batch):                      # rows of full degree, with a zero tail, all zero
            a[r, (n, n // 2, 0)[r]:] = 0
        a = a.reshape(-1)
        yield (f"w={w} batch={batch} n={n}", [fence.inp("a", a), fence.out("degrees", algebra_ref.degree(a, n, w, batch).view(np.uint64))],
               lambda a, degrees, n=n: d.poly_degree(a, n, degrees, batch=batch, width=w))


@row("linear_combination", cases=list(COMBOS))
def _linear_combination(tf, oracle, d, wp, ww):
    for n, k in itertools.product((1, 65, 257), (0, 1, 3, 5)):
        stride = n * wp + 5
        words = (k - 1) * stride + n * wp if k else 0
        cols, weights = rnd(oracle, words, 0x3700 + n + k), rnd(oracle, k * ww, 0x3701 + n + k)
        padding = np.zeros(words, dtype=bool)
        for j in range(k - 1):
            padding[j * stride + n * wp:(j + 1) * stride] = True
        want = algebra_ref.linear_combination(cols, n, wp, stride, k, weights, ww)
        yield (f"widths=({wp},{ww}) n={n} k={k} stride={stride}",
               [fence.inp("columns", cols, padding=padding), fence.inp("weights", weights), fence.out("out", want)],
               lambda columns, weights, out, n=n, k=k, stride=stride: d.linear_combination(columns, n, k, weights, out, width=wp, width_w=ww, stride=stride))


@row("poly_mul", cases=[1, 3])
def _poly_mul(tf, oracle, d, w):
    for na, nb in ((1, 1), (2, 3), (17, 16), (300, 513)):
        for batch in (1, 3):
            a, b = rnd(oracle, na * batch * w, 0x4000 + na), rnd(oracle, nb * batch * w, 0x4001 + nb)
            want = cat([oracle.poly_mul(x, y, width=w) for x, y in zip(a.reshape(batch, -1), b.reshape(batch, -1))])
            yield (f"w={w} na={na} nb={nb} batch={batch}", [fence.inp("a", a), fence.inp("b", b), fence.out("out", want)],
                   lambda a, b, out, na=na, nb=nb, batch=batch: d.poly_mul(a, na, b, nb, out, batch=batch, width=w))


@row("poly_mul_shared", cases=[1, 3])
def _poly_mul_shared(tf, oracle, d, w):
    for na, nb in ((1, 1), (2, 3), (17, 16), (300, 513)):
        for batch in (1, 3):
            a, b = rnd(oracle, na * batch * w, 0x4100 + na), rnd(oracle, nb * w, 0x4101 + nb)
            want = cat([oracle.poly_mul(x, b, width=w) for x in a.reshape(batch, -1)])
            yield (f"w={w} na={na} nb={nb} batch={batch}", [fence.inp("a", a), fence.inp("b", b), fence.out("out", want)],
                   lambda a, b, out, na=na, batch=batch: d.poly_mul_shared(a, na, b, out, batch, width=w))


# ------------------------------------------------------------------ evaluation, interpolation, zerofier trees
@row("batch_evaluate", cases=[1, 3])
def _batch_evaluate(tf, oracle, d, w):
    for nc, n_points in ((0, 5), (1, 1), (7, 300), (1025, 257)):
        c, pts = rnd(oracle, nc * w, 0x5000 + nc), rnd(oracle, n_points * w, 0x5001 + n_points)
        ops = [fence.inp("coeffs", c), fence.inp("points", pts), fence.out("out", _evaluate(oracle, c, pts, w))]
        call = lambda coeffs, points, out, nc=nc: d.batch_evaluate(coeffs, nc, points, out, width=w)  # noqa: E731
        yield f"w={w} n_coeffs={nc} points={n_points} routed", ops, call
        # forced routes: 1 is Horner, which takes the lane-per-point kernel below 1024 coefficients -- (7, 300) -- and the split kernel
        # from 1024 on -- (1025, 257), the only shape here that reaches it --; 2 is the zerofier tree
        if nc > 1:
            for route in (1, 2):
                yield f"w={w} n_coeffs={nc} points={n_points} route={route}", ops, switched(tf.lib(), "tf_set_batch_eval_route", route, 0, call)


@row("evaluate_bfe_at_xfe", cases=[1, 3])
def _evaluate_bfe_at_xfe(tf, oracle, d, batch):
    for nc, n_points in ((0, 5), (1, 1), (7, 300), (1025, 257)):
        c, pts = rnd(oracle, nc * batch, 0x5100 + nc), rnd(oracle, 3 * n_points, 0x5101 + n_points)
        pts[1:3] = 0   # a lifted base-field point
        lifted = np.zeros((batch, nc, 3), dtype=np.uint64)
        lifted[:, :, 0] = c.reshape(batch, nc)
        want = cat([_evaluate(oracle, r.reshape(-1), pts, 3) for r in lifted])
        yield (f"batch={batch} n_coeffs={nc} points={n_points}", [fence.inp("coeffs", c), fence.inp("points", pts), fence.out("out", want)],
               lambda coeffs, points, out, nc=nc: d.evaluate_bfe_at_xfe(coeffs, nc, points, out, batch=batch))


@row({"call": "zerofier", "ctor": "ZerofierTree", "tree": "ZerofierTree.zerofier"}, cases=[(kind, w, n) for kind in ("call", "ctor", "tree") for w in (1, 3) for n in TREE_SIZES])
def _zerofier(tf, oracle, d, kind, w, n):
    roots = rnd(oracle, n * w, 0x5200 + n)
    want = oracle.zerofier(roots, w)
    if kind == "call":
        yield f"w={w} n={n}", [fence.inp("roots", roots), fence.out("out", want)], lambda roots, out: d.zerofier(roots, out, width=w)
    elif kind == "ctor":
        def build(domain, asynchronous):
            import torch

            with d.ZerofierTree(domain, width=w, asynchronous=asynchronous) as t:
                assert t.num_points == n
                torch.cuda.synchronize()   # an asynchronous build must have ended before close() releases its memory
        for asynchronous in (False, True):
            yield f"w={w} n={n} asynchronous={asynchronous}", [fence.inp("domain", roots)], lambda domain, a=asynchronous: build(domain, a)
    else:
        def call(domain, out):
            with d.ZerofierTree(domain, width=w) as t:
                t.zerofier(out)
        yield f"tree w={w} n={n}", [fence.inp("domain", roots), fence.out("out", want)], call


@row({"call": "interpolate", "tree": "ZerofierTree.interpolate"}, cases=[(kind, w, n) for kind in ("call", "tree") for w in (1, 3) for n in TREE_SIZES])
def _interpolate(tf, oracle, d, kind, w, n):
    dom = rnd(oracle, n * w, 0x5300 + n)
    for rows in (1, 3):
        vals = rnd(oracle, rows * n * w, 0x5301 + n)
        want = cat([oracle.lagrange_interpolate(dom, v, w) for v in vals.reshape(rows, -1)])
        for with_status in (False, True):
            ops = [fence.inp("domain", dom), fence.inp("values", vals), fence.out("out", want)] + ([status_kept()] if with_status else [])

            def call(domain, values, out, status=None, rows=rows):
                if kind == "call":
                    d.interpolate(domain, values, out, rows=rows, width=w, status=status)
                else:
                    with d.ZerofierTree(domain, width=w) as t:
                        t.interpolate(values, out, rows=rows, status=status)
            yield f"{kind} w={w} n={n} rows={rows} status={with_status}", ops, call


@row("ZerofierTree.batch_evaluate", cases=[(w, n) for w in (1, 3) for n in TREE_SIZES])
def _tree_batch_evaluate(tf, oracle, d, w, n):
    dom = rnd(oracle, n * w, 0x5400 + n)
    for batch, nc in ((1, n), (3, n), (1, 2 * n + 3), (3, max(n // 2, 1))):
        c = rnd(oracle, batch * nc * w, 0x5401 + nc)
        want = cat([_evaluate(oracle, r, dom, w) for r in c.reshape(batch, -1)])

        def call(domain, coeffs, out, batch=batch, nc=nc):
            with d.ZerofierTree(domain, width=w) as t:
                t.batch_evaluate(coeffs, nc, out, batch=batch)
        yield f"w={w} n={n} batch={batch} n_coeffs={nc}", [fence.inp("domain", dom), fence.inp("coeffs", c), fence.out("out", want)], call


@row("barycentric_evaluate", cases=[(w, batch) for w in (1, 3) for batch in (1, 3)])
def _barycentric(tf, oracle, d, w, batch):
    for log_n in (0, 1, 6, 11):
        n = 1 << log_n
        cw, x = rnd(oracle, batch * n * w, 0x5500 + log_n), rnd(oracle, 3, 0x5501 + log_n)
        want = cat([oracle.barycentric_evaluate(r, x, w) for r in cw.reshape(batch, -1)])
        yield (f"w={w} batch={batch} n=2^{log_n}", [fence.inp("codewords", cw), fence.out("out", want)],
               lambda codewords, out, n=n, x=x: d.barycentric_evaluate(codewords, n, x, out, batch=batch, width=w))


# ------------------------------------------------------------------ division and power series
def _divisor(oracle, nb, w, seed):
    b = rnd(oracle, nb * w, seed)
    b[(nb - 1) * w:] = 0
    b[(nb - 1) * w] = oracle.bfe_new(3 + seed % 1000)
    return b


def _pad(x, words):
    out = np.zeros(words, dtype=np.uint64)
    out[:np.asarray(x).size] = np.asarray(x, dtype=np.uint64).reshape(-1)
    return out


@row("divide", cases=[(1, s) for s in DIVIDE_SHAPES] + [(3, s) for s in DIVIDE_SHAPES[:3]])
def _divide(tf, oracle, d, w, shape):
    """width 3 at the three small shapes only: its reference is the schoolbook loop of tests/test_gpu_poly_divide.py over the
    oracle's XFieldElement products, one ctypes call per product"""
    from tests.test_gpu_poly_divide import xfe_long_divide

    na, nb = shape
    b = _divisor(oracle, nb, w, 0x6000 + nb)
    k, m = max(na - nb + 1, 0), nb - 1
    for batch in (1, 3):
        a = rnd(oracle, batch * na * w, 0x6001 + na)
        qs, rs = [], []
        for r in a.reshape(batch, -1):
            q, rem = oracle.naive_divide(r, b) if w == 1 else xfe_long_divide(oracle, r.copy(), b)
            qs.append(_pad(q, k * w))
            rs.append(_pad(rem, m * w))
        ops = [fence.inp("a", a), fence.inp("b", b), fence.out("q", cat(qs)), fence.out("r", cat(rs))]
        call = lambda a, b, q, r, status=None, batch=batch: d.divide(a, na, b, q, r, batch=batch, width=w, status=status)  # noqa: E731
        yield f"w={w} na={na} nb={nb} batch={batch}", ops, call
        yield f"w={w} na={na} nb={nb} batch={batch} status", ops + [status_kept()], call
        if k:   # (an empty quotient is a null pointer, and a call that asks for neither output is refused)
            yield (f"w={w} na={na} nb={nb} batch={batch} q only", ops[:3] + [status_kept()],
                   lambda a, b, q, status, batch=batch: d.divide(a, na, b, q, None, batch=batch, width=w, status=status))
        if m:
            yield (f"w={w} na={na} nb={nb} batch={batch} r only", ops[:2] + [ops[3], status_kept()],
                   lambda a, b, r, status, batch=batch: d.divide(a, na, b, None, r, batch=batch, width=w, status=status))


@row({"one": "clean_divide", "many": "clean_divide_many"}, cases=[(kind, s) for kind in ("one", "many") for s in DIVIDE_SHAPES[1:]])
def _clean_divide(tf, oracle, d, kind, shape):
    na, nb = shape
    b = _divisor(oracle, nb, 1, 0x6100 + nb)
    batch = 1 if kind == "one" else 3
    q = rnd(oracle, batch * (na - nb + 1), 0x6101 + na)
    a = cat([oracle.poly_mul(r, b) for r in q.reshape(batch, -1)])
    for with_status in (False, True):
        ops = [fence.inp("a", a), fence.inp("b", b), fence.out("out", q)] + ([status_kept()] if with_status else [])
        if kind == "one":
            yield f"na={na} nb={nb} status={with_status}", ops, lambda a, b, out, status=None: d.clean_divide(a, b, out, status=status)
        else:
            yield f"na={na} nb={nb} batch=3 status={with_status}", ops, lambda a, b, out, status=None: d.clean_divide_many(a, na, b, out, 3, status=status)


@row("fps_inverse_newton", cases=[(w, nf) for w in (1, 3) for nf in (1, 3, 40, 300)])  # (nf = 300: while the untruncated iterate fits 2^17 words)
def _fps_inverse_newton(tf, oracle, d, w, nf):
    from tests.test_gpu_poly_divide import newton_reference

    f = _divisor(oracle, nf, w, 0x6200 + nf)
    f[0] = oracle.bfe_new(9)
    for precision in (1, 3, 255, 256, 257):
        words = tf.lib().tf_poly_fps_inverse_newton_len(nf, precision) * w
        if words > 1 << 17:
            continue
        want = newton_reference(oracle, f, precision, w)
        assert want.size == words
        for with_status in (False, True):
            yield (f"w={w} nf={nf} precision={precision} status={with_status}", [fence.inp("f", f), fence.out("out", want)] + ([status_kept()] if with_status else []),
                   lambda f, out, status=None, precision=precision: d.fps_inverse_newton(f, precision, out, width=w, status=status))


# ------------------------------------------------------------------ inversion
@row({"batch": "batch_inversion", "or_zero": "inverse_or_zero"}, cases=[(op, w, n) for op in ("batch", "or_zero") for w in (1, 3) for n in (1, 63, 65, 257, 65537)
                                                  if n * w <= 1 << 17])
def _inversion(tf, oracle, d, op, w, n):
    """65537 XFieldElements would be 196 611 words, beyond the 2^17 words of a tensor here: that width stops at 257"""
    x = rnd(oracle, n * w, 0x7000 + n)
    if op == "or_zero":
        x[(n // 2) * w:(n // 2 + 1) * w] = 0
        fn = lambda x, out, status=None: d.inverse_or_zero(x, out, width=w)  # noqa: E731
    else:
        fn = lambda x, out, status=None: d.batch_inversion(x, out, width=w, status=status)  # noqa: E731
    want = inversion_ref.expected(x, w, or_zero=op == "or_zero")
    yield f"{op} w={w} n={n}", [fence.inp("x", x), fence.out("out", want)], fn
    yield f"{op} w={w} n={n} in place", [fence.inout("x", x, want)], lambda x: fn(x, x)
    if op == "batch":
        yield f"{op} w={w} n={n} status", [fence.inp("x", x), fence.out("out", want), status_kept()], fn


# ------------------------------------------------------------------ points, powers, gathers
@row("get_colinear_y", cases=[(wx, wy, each) for wx, wy in points_ref.PAIRS for each in (False, True)])
def _get_colinear_y(tf, oracle, d, wx, wy, each):
    for n in (1, 7, 8, 9, 511, 513, 2049):
        x0, x1 = rnd(oracle, n * wx, 0x8000 + n), rnd(oracle, n * wx, 0x8001 + n)
        y0, y1 = rnd(oracle, n * wy, 0x8002 + n), rnd(oracle, n * wy, 0x8003 + n)
        p2x = rnd(oracle, (n if each else 1) * wy, 0x8004 + n)
        want, bad = points_ref.get_colinear_y(x0, y0, x1, y1, p2x, wx, wy)
        assert not bad
        ops = [fence.inp("x0", x0), fence.inp("y0", y0), fence.inp("x1", x1), fence.inp("y1", y1), fence.inp("p2x", p2x), fence.out("out", want)]
        call = lambda x0, y0, x1, y1, p2x, out, status=None: d.get_colinear_y(x0, y0, x1, y1, p2x, out, width_x=wx, width_y=wy, status=status)  # noqa: E731
        yield f"widths=({wx},{wy}) n={n} p2x per triple={each}", ops, call
        yield f"widths=({wx},{wy}) n={n} p2x per triple={each} status", ops + [status_kept()], call


@row("are_colinear", cases=list(points_ref.PAIRS))
def _are_colinear(tf, oracle, d, wx, wy):
    for k, groups in itertools.product((2, 3, 16, 17, 65), (1, 3, 65)):
        xs = rnd(oracle, groups * k * wx, 0x8100 + k + groups)
        ys = rnd(oracle, groups * k * wy, 0x8101 + k + groups)
        ex, ey = points_ref.elements(xs, wx), points_ref.elements(ys, wy)
        for g in range(0, groups, 2):      # every other group lies on a line, the last of them but for its last point
            a, b = ey[g * k], ey[g * k + 1]
            for i in range(g * k, (g + 1) * k - (g == groups - 1 and g > 0)):
                ey[i] = points_ref.f_add(points_ref.f_mul(a, points_ref.lift(ex[i], wx, wy), wy), b, wy)
        ys = points_ref.words(ey, wy)
        want = points_ref.are_colinear(xs, ys, groups, k, wx, wy)
        assert k < 3 or want[0] == 1
        yield (f"widths=({wx},{wy}) k={k} groups={groups}", [fence.inp("xs", xs), fence.inp("ys", ys), fence.out("flags", want, dtype="int32")],
               lambda xs, ys, flags, k=k: d.are_colinear(xs, ys, k, flags, width_x=wx, width_y=wy))


@row("mod_pow", cases=[(w, one_base) for w in (1, 3) for one_base in (True, False)])
def _mod_pow(tf, oracle, d, w, one_base):
    for n in (1, 65, 257):
        bases = rnd(oracle, (1 if one_base else n) * w, 0x8200 + n)
        exps = rnd(oracle, n, 0x8201 + n) | np.uint64(1 << 63)
        exps[0] = 0
        yield (f"w={w} n={n} one base={one_base}", [fence.inp("bases", bases), fence.inp("exps", exps), fence.out("out", points_ref.mod_pow(bases, exps, w, n))],
               lambda bases, exps, out: d.mod_pow(bases, exps, out, width=w))
        yield (f"w={w} n={n} one base={one_base} one exponent", [fence.inp("bases", bases), fence.inp("exps", exps[-1:]),
                                                                  fence.out("out", points_ref.mod_pow(bases, exps[-1:], w, n))],
               lambda bases, exps, out: d.mod_pow(bases, exps, out, width=w))


@row("powers", cases=[1, 3])
def _powers(tf, oracle, d, w):
    for n in (1, 255, 257, 1025):
        first, ratio = rnd(oracle, w, 0x8300 + n), rnd(oracle, w, 0x8301 + n)
        yield f"w={w} n={n}", [fence.out("out", points_ref.powers(first, ratio, w, n))], lambda out, first=first, ratio=ratio: d.powers(first, ratio, out, width=w)


@row("gather_elements", cases=[1, 3, 5, 16])
def _gather(tf, oracle, d, width):
    m = 40
    src = rnd(oracle, m * width, 0x8400 + width)
    for n in (1, 65):
        idx = np.random.default_rng(n).integers(0, m, size=n).astype(np.uint32)
        want, bad = points_ref.gather(src, width, idx)
        assert not bad
        ops = [fence.inp("src", src), fence.inp("indices", idx, dtype="int32"), fence.out("out", want)]
        yield f"width={width} n={n}", ops, lambda src, indices, out: d.gather_elements(src, indices, out, width=width)
        yield f"width={width} n={n} status", ops + [status_kept()], lambda src, indices, out, status: d.gather_elements(src, indices, out, width=width, status=status)
        # one index beyond src: 17 in the status, and its slot of out stays as it was
        idx = idx.copy()
        idx[n // 2] = m
        want, bad = points_ref.gather(src, width, idx)
        kept = np.zeros(n * width, dtype=bool)
        kept[bad[0] * width:(bad[0] + 1) * width] = True
        yield (f"width={width} n={n} index {n // 2} out of range",
               [fence.inp("src", src), fence.inp("indices", idx, dtype="int32"), fence.out("out", want, kept=kept), fence.inout("status", i32([0]), i32([17]), dtype="int32")],
               lambda src, indices, out, status: d.gather_elements(src, indices, out, width=width, status=status))


# ------------------------------------------------------------------ Tip5
@row({"permute": "tip5_permute_", "trace": "tip5_trace_", "pairs": "tip5_hash_pairs"}, cases=[(op, count) for op in ("permute", "trace", "pairs") for count in TIP5_COUNTS
                                                                                                    if op != "trace" or 96 * count <= 1 << 17]
                                                                                                   + [("trace", 1363), ("trace", 1365)])  # (96 words per trace: 2^17 words end at 1365)
def _tip5(tf, oracle, d, op, count):
    if op == "pairs":
        x = rnd(oracle, 10 * count, 0x9000 + count)
        yield f"count={count}", [fence.inp("inp", x), fence.out("out", oracle.hash_pairs(x))], lambda inp, out: d.tip5_hash_pairs(inp, out)
        return
    s = rnd(oracle, 16 * count, 0x9001 + count)
    if op == "permute":
        yield f"count={count}", [fence.inout("states", s, cat([oracle.tip5_permutation(r) for r in s.reshape(-1, 16)]))], lambda states: d.tip5_permute_(states)
    else:
        traces = [oracle.tip5_trace(r) for r in s.reshape(-1, 16)]
        yield (f"count={count}", [fence.inout("states", s, cat([t[1] for t in traces])), fence.out("trace", cat([t[0] for t in traces]))],
               lambda states, trace: d.tip5_trace_(states, trace))


def _hash_rows(oracle, rows, row_len, n_rows):
    return oracle.hash_varlen_rows(rows, row_len) if row_len else np.tile(oracle.hash_varlen(np.zeros(0, dtype=np.uint64)), n_rows)


@row("tip5_hash_varlen_rows", cases=[0, 1, 9, 10, 11, 21])
def _tip5_rows(tf, oracle, d, row_len):
    for count in TIP5_COUNTS:
        rows = rnd(oracle, count * row_len, 0x9100 + count)
        yield (f"row_len={row_len} rows={count}", [fence.inp("rows", rows), fence.out("out", _hash_rows(oracle, rows, row_len, count))],
               lambda rows, out: d.tip5_hash_varlen_rows(rows, row_len, out))


# ------------------------------------------------------------------ Merkle trees
def _leafs_and_nodes(oracle, height, batch):
    n = 1 << height
    leafs = rnd(oracle, batch * n * 5, 0xA000 + height)
    return n, leafs, [oracle.merkle_build(t).reshape(2 * n, 5) for t in leafs.reshape(batch, -1)]


@row({"build": "merkle_build", "root": "merkle_root"}, cases=[(op, h) for op in ("build", "root") for h in HEIGHTS])
def _merkle(tf, oracle, d, op, height):
    for batch in (1, 3):
        n, leafs, nodes = _leafs_and_nodes(oracle, height, batch)
        if op == "build":
            yield (f"height={height} batch={batch}", [fence.inp("leaves", leafs), fence.out("nodes_out", cat(nodes))],
                   lambda leaves, nodes_out, batch=batch: d.merkle_build(leaves, n, nodes_out, batch=batch))
        else:
            want = cat([oracle.merkle_frugal_root(t) for t in leafs.reshape(batch, -1)])
            assert np.array_equal(want, cat([t[1] for t in nodes]))
            yield (f"height={height} batch={batch}", [fence.inp("leaves", leafs), fence.out("root_out", want)],
                   lambda leaves, root_out, batch=batch: d.merkle_root(leaves, n, root_out, batch=batch))


@row("merkle_from_rows", cases=HEIGHTS)
def _merkle_from_rows(tf, oracle, d, height):
    n = 1 << height
    for batch, row_len in ((1, 7), (3, 7), (1, 21)):
        rows = rnd(oracle, batch * n * row_len, 0xA100 + height)
        want = cat([oracle.merkle_from_rows(t, row_len) for t in rows.reshape(batch, -1)])
        yield (f"height={height} batch={batch} row_len={row_len}", [fence.inp("rows", rows), fence.out("nodes_out", want)],
               lambda rows, nodes_out, batch=batch, row_len=row_len: d.merkle_from_rows(rows, row_len, n, nodes_out, batch=batch))


@row({"rows": "hash_table_rows", "tree": "merkle_from_columns"}, cases=[(op, h) for op in ("rows", "tree") for h in HEIGHTS])
def _tables(tf, oracle, d, op, height):
    n_rows, n_cols = 1 << height, 3
    for batch, width in ((1, 1), (3, 1), (1, 3), (3, 3)):
        cs = n_rows * width + 5
        words = (batch * n_cols - 1) * cs + n_rows * width
        raw = rnd(oracle, words, 0xA200 + height + width)
        padding = np.zeros(words, dtype=bool)
        for j in range(batch * n_cols - 1):
            padding[j * cs + n_rows * width:(j + 1) * cs] = True
        full = _pad(raw, batch * n_cols * cs)
        digests = []
        for b in range(batch):
            t = full[b * n_cols * cs:(b + 1) * n_cols * cs].reshape(n_cols, cs)[:, :n_rows * width].reshape(n_cols, n_rows, width)
            digests.append(oracle.hash_varlen_rows(np.ascontiguousarray(t.transpose(1, 0, 2)).reshape(-1), n_cols * width))
        shape = f"height={height} batch={batch} width={width} col_stride={cs}"
        if op == "rows":
            yield (shape, [fence.inp("table", raw, padding=padding), fence.out("out", cat(digests))],
                   lambda table, out, batch=batch, width=width, cs=cs: d.hash_table_rows(table, n_rows, n_cols, out, width=width, col_stride=cs, batch=batch))
        else:
            yield (shape, [fence.inp("table", raw, padding=padding), fence.out("nodes_out", cat([oracle.merkle_build(x) for x in digests]))],
                   lambda table, nodes_out, batch=batch, width=width, cs=cs: d.merkle_from_columns(table, n_rows, n_cols, nodes_out, width=width, col_stride=cs, batch=batch))


def _index_sets(n):
    rng = np.random.default_rng(n + 17)
    sets = [[0], [n - 1], [0, n - 1], [3 % n, 3 % n, 5 % n], rng.integers(0, n, size=17).tolist()]
    return [np.array(s, dtype=np.uint64) for s in sets]


@row("authentication_structure", cases=HEIGHTS)
def _auth_structure(tf, oracle, d, height):
    n, _, nodes = _leafs_and_nodes(oracle, height, 1)
    for idx in _index_sets(n):
        want = nodes[0][oracle.auth_structure_indices(n, idx).astype(np.int64)]

        def call(nodes, idx=idx, want=want):
            got = d.authentication_structure(nodes, n, idx)
            assert np.array_equal(got, want.reshape(-1, 5)), "authentication_structure: the returned digests"
        yield f"height={height} indices={idx.tolist()}", [fence.inp("nodes", cat(nodes))], call


@row("authentication_structure_from_leafs", cases=HEIGHTS)
def _auth_structure_from_leafs(tf, oracle, d, height):
    for batch in (1, 3):
        n, leafs, nodes = _leafs_and_nodes(oracle, height, batch)
        for idx in _index_sets(n):
            ids = oracle.auth_structure_indices(n, idx).astype(np.int64)
            words = batch * ids.size * 5
            want = _pad(cat([t[ids] for t in nodes]), words + 7)   # an out with room to spare: the spare words stay as they were
            kept = np.arange(words + 7) >= words
            roots = cat([t[1] for t in nodes])

            def call(leafs, out, roots=None, idx=idx, batch=batch, words=words):
                got = d.authentication_structure_from_leafs(leafs, n, idx, out=out, roots=roots, batch=batch)
                assert got.numel() == words and (words == 0 or got.data_ptr() == out.data_ptr())
            shape = f"height={height} batch={batch} indices={idx.tolist()}"
            yield shape + " with roots", [fence.inp("leafs", leafs), fence.out("out", want, kept=kept), fence.out("roots", roots)], call
            yield shape, [fence.inp("leafs", leafs), fence.out("out", want, kept=kept)], call


def _proof_batch(oracle, heights, seed):
    """honest proofs of the Merkle model of tests/test_gpu_merkle_proofs.py, the last one with one corrupted structure digest (if
    it has any) -> the CSR arrays, the expected statuses and the expected paths"""
    from tests import test_gpu_merkle_proofs as mp

    rng = np.random.default_rng(seed)
    idxs, digs, auths, roots, statuses, paths = [], [], [], [], [], []
    for j, h in enumerate(heights):
        idx, dig, auth, root = mp.honest(oracle, rng, h, min(3, 1 << h) if h else 1)
        if j == len(heights) - 1 and len(auth):
            auth = mp.corrupt(auth, rng)
        st, path = mp.check(oracle, h, idx, dig, auth, paths=True)   # (no root in this check: the corrupted digest is copied as it is)
        assert st == mp.OK
        paths.append(path)
        statuses.append(mp.check(oracle, h, idx, dig, auth, root)[0])
        idxs.append(idx), digs.append(dig), auths.append(auth), roots.append(root)
    lo = np.cumsum([0] + [len(i) for i in idxs]).astype(np.uint64)
    ao = np.cumsum([0] + [len(a) for a in auths]).astype(np.uint64)
    return lo, ao, cat(idxs), cat(digs), cat(auths), cat(roots), statuses, cat(paths)


@row({"verify": "verify_inclusion_proofs", "paths": "authentication_paths"}, cases=[(op, h) for op in ("verify", "paths") for h in HEIGHTS])
def _inclusion_proofs(tf, oracle, d, op, height):
    for batch in (1, 3):
        heights = [height] * batch
        lo, ao, idx, dig, auth, roots, statuses, paths = _proof_batch(oracle, heights, 0xA300 + height + batch)
        spare = np.arange(batch + 3) >= batch           # statuses.numel() >= n: the spare entries stay as they were
        common = [fence.inp("leaf_indices", idx), fence.inp("leaf_digests", dig), fence.inp("auth_digests", auth)]
        if op == "verify":
            yield (f"height={height} proofs={batch}", common + [fence.inp("expected_roots", roots), fence.out("statuses", i32(statuses + [0] * 3), dtype="int32", kept=spare)],
                   lambda leaf_indices, leaf_digests, auth_digests, expected_roots, statuses, lo=lo, ao=ao, heights=heights:
                   d.verify_inclusion_proofs(heights, lo, leaf_indices, leaf_digests, ao, auth_digests, expected_roots, statuses))
        else:
            assert paths.size == d.authentication_path_words(heights, lo)
            yield (f"height={height} proofs={batch}", common + [fence.out("paths_out", _pad(paths, paths.size + 5), kept=np.arange(paths.size + 5) >= paths.size),
                                                               fence.out("statuses", i32([0] * batch + [0] * 3), dtype="int32", kept=spare)],
                   lambda leaf_indices, leaf_digests, auth_digests, paths_out, statuses, lo=lo, ao=ao, heights=heights:
                   d.authentication_paths(heights, lo, leaf_indices, leaf_digests, ao, auth_digests, paths_out, statuses))


# ------------------------------------------------------------------ Tip5 sponges
SPONGE_COUNTS = [1, 3, 16, 17]


@row({"init": "tip5_sponge_init_", "absorb": "tip5_sponge_absorb_", "squeeze": "tip5_sponge_squeeze"}, cases=[(op, c) for op in ("init", "absorb", "squeeze") for c in SPONGE_COUNTS])
def _sponge(tf, oracle, d, op, count):
    s = rnd(oracle, 16 * count, 0xB000 + count)
    if op == "init":
        for fixed in (False, True):
            yield f"count={count} fixed_length={fixed}", [fence.out("states", np.tile(sponge_ref.init(fixed), count))], lambda states, fixed=fixed: d.tip5_sponge_init_(states, fixed)
    elif op == "absorb":
        for k in (1, 3):
            x = rnd(oracle, count * k * 10, 0xB001 + k)
            want = cat([sponge_ref.absorb_many(st, c) for st, c in zip(s.reshape(count, 16), x.reshape(count, -1))])
            yield f"count={count} chunks={k}", [fence.inout("states", s, want), fence.inp("inp", x)], lambda states, inp: d.tip5_sponge_absorb_(states, inp)
    else:
        for k in (1, 3):
            got = [sponge_ref.squeeze_many(st, k) for st in s.reshape(count, 16)]
            yield (f"count={count} squeezes={k}", [fence.inout("states", s, cat([g[0] for g in got])), fence.out("out", cat([g[1] for g in got]))],
                   lambda states, out: d.tip5_sponge_squeeze(states, out))


@row("tip5_sponge_pad_and_absorb_all_", cases=SPONGE_COUNTS)
def _sponge_pad(tf, oracle, d, count):
    s = rnd(oracle, 16 * count, 0xB100 + count)
    for length in (0, 1, 9, 10, 11, 21):
        x = rnd(oracle, count * length, 0xB101 + length)
        want = cat([sponge_ref.pad_and_absorb_all(st, x[i * length:(i + 1) * length]) for i, st in enumerate(s.reshape(count, 16))])
        yield f"count={count} length={length}", [fence.inout("states", s, want), fence.inp("inp", x)], lambda states, inp: d.tip5_sponge_pad_and_absorb_all_(states, inp)
    lengths = [(0, 10, 1, 21, 9, 11, 30)[i % 7] for i in range(count)]
    off = np.cumsum([0] + lengths).astype(np.uint64)
    x = rnd(oracle, int(off[-1]) + 4, 0xB102 + count)   # four words behind the last offset: never looked at
    want = cat([sponge_ref.pad_and_absorb_all(st, x[int(off[i]):int(off[i + 1])]) for i, st in enumerate(s.reshape(count, 16))])
    yield (f"count={count} ragged {lengths}", [fence.inout("states", s, want), fence.inp("inp", x, padding=np.arange(x.size) >= int(off[-1]))],
           lambda states, inp: d.tip5_sponge_pad_and_absorb_all_(states, inp, offsets=off))


@row({"scalars": "tip5_sponge_sample_scalars", "indices": "tip5_sponge_sample_indices"}, cases=[(op, c) for op in ("scalars", "indices") for c in SPONGE_COUNTS])
def _sponge_samplers(tf, oracle, d, op, count):
    s = rnd(oracle, 16 * count, 0xB200 + count)
    if op == "scalars":
        for n in (0, 1, 4, 10):
            got = [sponge_ref.sample_scalars(st, n) for st in s.reshape(count, 16)]
            yield (f"count={count} n={n}", [fence.inout("states", s, cat([g[0] for g in got])), fence.out("out", cat([g[1] for g in got]))],
                   lambda states, out: d.tip5_sponge_sample_scalars(states, out))
    else:
        for upper_bound, num in ((8, 9), (1 << 31, 40)):      # two of the INDEX_CASES of tests/test_gpu_sponge.py
            got = [sponge_ref.sample_indices(st, upper_bound, num) for st in s.reshape(count, 16)]
            yield (f"count={count} upper_bound={upper_bound} n={num}",
                   [fence.inout("states", s, cat([g[0] for g in got])), fence.out("out", cat([g[1] for g in got], np.uint32), dtype="int32")],
                   lambda states, out, upper_bound=upper_bound: d.tip5_sponge_sample_indices(states, upper_bound, out))


# ------------------------------------------------------------------ Merkle Mountain Ranges
def _popcount(x):
    return bin(x).count("1")


def _digests(rng, n):
    return rng.integers(0, P, size=(n, 5), dtype=np.uint64)


@row("mmr_append", cases=[(0, 1), (3, 13), (7, 9)])
def _mmr_append(tf, oracle, d, n, k):
    from tests import test_gpu_mmr as mm

    rng = np.random.default_rng(1000 * n + k)
    old, new = _digests(rng, n), _digests(rng, k)
    peaks = old_peaks = mm.model_peaks(oracle, old)
    proofs = []
    for i in range(k):
        peaks, path = mm.model_append(oracle, n + i, peaks, new[i])
        proofs.append(path)
    proofs = cat(proofs)
    ops = [fence.inp("old_peaks", old_peaks), fence.inp("new_leafs", new), fence.out("new_peaks", peaks)]
    yield f"n={n} k={k}", ops, lambda old_peaks, new_leafs, new_peaks: d.mmr_append(n, old_peaks, new_leafs, new_peaks)
    yield (f"n={n} k={k} with proofs", ops + [fence.out("proofs", _pad(proofs, proofs.size + 5), kept=np.arange(proofs.size + 5) >= proofs.size)],
           lambda old_peaks, new_leafs, new_peaks, proofs: d.mmr_append(n, old_peaks, new_leafs, new_peaks, proofs))


@row("mmr_bag_peaks", cases=[[0], [5], [0, 1, 7, 13, 1 << 63]])
def _mmr_bag_peaks(tf, oracle, d, counts):
    rng = np.random.default_rng(len(counts))
    peaks = [_digests(rng, _popcount(c)) for c in counts]
    want = []
    for c, p in zip(counts, peaks):
        acc = oracle.hash_10(np.array([oracle.bfe_new(c & 0xFFFFFFFF), oracle.bfe_new(c >> 32)] + [0] * 8, dtype=np.uint64))
        for dg in p[::-1]:
            acc = oracle.hash_pair(dg, acc)
        want.append(acc)
    yield f"counts={counts}", [fence.inp("peaks", cat(peaks)), fence.out("out", cat(want))], lambda peaks, out: d.mmr_bag_peaks(counts, peaks, out)


@row("mmr_verify_membership_proofs", cases=[1, 16, 17])
def _mmr_verify(tf, oracle, d, n_proofs):
    from tests import test_gpu_mmr as mm

    n = 13
    rng = np.random.default_rng(n_proofs)
    leafs = _digests(rng, n)
    peaks, honest = mm.model_peaks(oracle, leafs), mm.honest_proofs(oracle, leafs)
    idx = np.array([(5 * i) % (n + 2) for i in range(n_proofs)], dtype=np.uint64)   # some beyond the last leaf
    paths = [honest[int(i) % n].copy() for i in idx]
    if n_proofs > 1 and len(paths[1]):
        paths[1][0, 0] ^= np.uint64(3)
    digs = leafs[(idx % n).astype(np.int64)]
    want = [mm.model_verify(oracle, int(i), g, p, peaks, n, tf.mmr_index) for i, g, p in zip(idx, digs, paths)]
    off = np.cumsum([0] + [len(p) for p in paths]).astype(np.uint64)
    spare = np.arange(n_proofs + 3) >= n_proofs
    yield (f"leafs={n} proofs={n_proofs}",
           [fence.inp("peaks", peaks), fence.inp("leaf_indices", idx), fence.inp("leaf_digests", digs), fence.inp("paths", cat(paths)),
            fence.out("statuses", i32(want + [0] * 3), dtype="int32", kept=spare)],
           lambda peaks, leaf_indices, leaf_digests, paths, statuses: d.mmr_verify_membership_proofs(n, peaks, leaf_indices, leaf_digests, off, paths, statuses))


@row("mmr_batch_mutate_leafs", cases=[True, False])
def _mmr_mutate(tf, oracle, d, with_peaks):
    from tests import test_gpu_mmr as mm

    n, mut_idx, own_idx = 13, [3, 8, 12], [3, 4, 9, 12, 0]
    rng = np.random.default_rng(77)
    leafs = _digests(rng, n)
    peaks, honest = mm.model_peaks(oracle, leafs), mm.honest_proofs(oracle, leafs)
    new = _digests(rng, len(mut_idx))
    want_peaks, want_paths, flags = mm.model_mutate(oracle, tf.mmr_index, peaks if with_peaks else None, n, [honest[i] for i in own_idx], own_idx,
                                                    [(i, new[j], honest[i]) for j, i in enumerate(mut_idx)])
    mo = np.cumsum([0] + [len(honest[i]) for i in mut_idx]).astype(np.uint64)
    oo = np.cumsum([0] + [len(honest[i]) for i in own_idx]).astype(np.uint64)
    ops = [fence.inp("new_leafs", new), fence.inp("mut_paths", cat([honest[i] for i in mut_idx])),
           fence.inout("own_paths", cat([honest[i] for i in own_idx]), cat(want_paths)),
           fence.out("modified", i32([int(f) for f in flags] + [0] * 3), dtype="int32", kept=np.arange(len(own_idx) + 3) >= len(own_idx))]
    if with_peaks:
        yield ("leafs=13 mutations=3 proofs=5 with peaks", ops + [fence.inout("peaks", peaks, want_peaks)],
               lambda new_leafs, mut_paths, own_paths, modified, peaks: d.mmr_batch_mutate_leafs(n, peaks, mut_idx, new_leafs, mo, mut_paths, own_idx, oo, own_paths, modified))
    else:
        yield ("leafs=13 mutations=3 proofs=5", ops,
               lambda new_leafs, mut_paths, own_paths, modified: d.mmr_batch_mutate_leafs(n, None, mut_idx, new_leafs, mo, mut_paths, own_idx, oo, own_paths, modified))


@row("mmr_successor_proof_new", cases=[(0, 1), (3, 13), (7, 9)])
def _mmr_successor_new(tf, oracle, d, n, k):
    from tests import test_gpu_mmr_successor as ms

    leafs = ms.random_leafs()[:n + k]
    old_peaks, new_peaks = ms.model_peaks(oracle, leafs[:n]), ms.model_peaks(oracle, leafs)
    paths = ms.model_successor_new(oracle, tf.mmr_index, n, leafs[n:]).reshape(-1)
    assert paths.size == 5 * d.mmr_successor_proof_len(n, k)
    out = fence.out("paths_out", _pad(paths, paths.size + 5), kept=np.arange(paths.size + 5) >= paths.size)

    def call(new_leafs, paths_out, old_peaks=None, new_peaks=None):
        assert d.mmr_successor_proof_new(n, old_peaks, new_leafs, paths_out, new_peaks) == paths.size // 5
    yield f"n={n} k={k} with peaks", [fence.inp("old_peaks", old_peaks), fence.inp("new_leafs", leafs[n:]), out, fence.out("new_peaks", new_peaks)], call
    yield f"n={n} k={k}", [fence.inp("new_leafs", leafs[n:]), out], call


@row("mmr_verify_successor_proofs", cases=[1, 16, 17])
def _mmr_verify_successors(tf, oracle, d, n_proofs):
    from tests import test_gpu_mmr_successor as ms

    m, cases = tf.mmr_index, []
    for j in range(n_proofs):
        n, k = ((3, 13), (7, 9), (0, 1), (4, 4), (5, 0))[j % 5]
        leafs = ms.random_leafs()[j:j + n + k]
        old, new = ms.model_peaks(oracle, leafs[:n]), ms.model_peaks(oracle, leafs)
        paths = ms.model_successor_new(oracle, m, n, leafs[n:])
        if j % 4 == 1 and len(paths):
            paths = paths.copy()
            paths[0, 0] ^= np.uint64(1)
        cases.append((n, old, n + k, new, paths))
    want = [ms.model_verify(oracle, m, *c) for c in cases]
    assert want[0] == 0 and (n_proofs == 1 or want[1] != 0)
    off = lambda col: np.cumsum([0] + [len(c[col]) for c in cases]).astype(np.uint64)  # noqa: E731
    oo, no, po = off(1), off(3), off(4)
    yield (f"proofs={n_proofs}",
           [fence.inp("old_peaks", cat([c[1] for c in cases])), fence.inp("new_peaks", cat([c[3] for c in cases])), fence.inp("paths", cat([c[4] for c in cases])),
            fence.out("statuses", i32(want + [0] * 3), dtype="int32", kept=np.arange(n_proofs + 3) >= n_proofs)],
           lambda old_peaks, new_peaks, paths, statuses: d.mmr_verify_successor_proofs([c[0] for c in cases], [c[2] for c in cases], oo, old_peaks, no, new_peaks,
                                                                                       po, paths, statuses))


@row("mmr_update_proofs_from_append", cases=[(7, 9)])
def _mmr_update(tf, oracle, d, n, k):
    from tests import test_gpu_mmr_successor as ms

    m = tf.mmr_index
    leafs = ms.random_leafs()[:n + k]
    indices = [0, 3, 6, 6, 2]
    paths = [list(p) for p in (ms.honest_proofs(n)[i] for i in indices)]
    own = cat([np.array(p, dtype=np.uint64) for p in paths])
    own_off = np.cumsum([0] + [len(p) for p in paths]).astype(np.uint64)
    peaks, flags = ms.model_peaks(oracle, leafs[:n]), np.zeros(len(indices), dtype=np.int32)
    old_peaks = peaks
    for i in range(k):
        flags[ms.model_update_from_append(oracle, m, paths, indices, n + i, leafs[n + i], peaks)] = 1
        peaks = ms.model_append(oracle, n + i, peaks, leafs[n + i])
    want = cat([np.array(p, dtype=np.uint64) for p in paths])
    want_off = np.cumsum([0] + [len(p) for p in paths]).astype(np.uint64)

    def call(old_peaks, new_leafs, own_paths, out_paths=None, new_peaks=None):
        out_off, modified = d.mmr_update_proofs_from_append(n, old_peaks, new_leafs, indices, own_off, own_paths, out_paths, new_peaks)
        assert np.array_equal(out_off, want_off) and (out_paths is None or np.array_equal(modified, flags))
    ops = [fence.inp("old_peaks", old_peaks), fence.inp("new_leafs", leafs[n:]), fence.inp("own_paths", own)]
    yield f"n={n} k={k} sizing", ops, call
    yield (f"n={n} k={k}", ops + [fence.out("out_paths", _pad(want, want.size + 5), kept=np.arange(want.size + 5) >= want.size), fence.out("new_peaks", peaks)], call)


# ------------------------------------------------------------------ the one test
def _ids():
    return [pytest.param(name, case, id=f"{name}-{k}") for name in ROWS for k, case in enumerate(ROWS[name][0])]


def triples(tf, oracle, name, case):
    """the (shape, operands, call) triples of one case of one row"""
    _, gen = ROWS[name]
    args = case if isinstance(case, tuple) else (case,)
    return gen(tf, oracle, tf.device, *args)


@pytest.mark.gpu
@pytest.mark.parametrize("name,case", _ids())
def test_fenced(tf, oracle, name, case):
    assert tf.lib().tf_device_count() > 0, "no HIP device visible: the product has no CPU fallback"
    for shape, operands, call in triples(tf, oracle, name, case):
        fence.run(name, shape, operands, call)
