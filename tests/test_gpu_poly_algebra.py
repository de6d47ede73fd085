"""Polynomial arithmetic on the GPU (include/tf_hip.h, "Polynomial arithmetic"): add, sub, neg, scalar_mul, scale, formal_derivative,
degree, the XFieldElement x BFieldElement product and the weighted sum of columns, every width combination, word for word.

Expected values come from tests/algebra_ref (Python integers; pinned against the oracle and tests/pyref by the CPU tests).  The
lengths sit on the boundaries of the kernels (csrc/algebra_kernels.h): one wave, one workgroup of 256 lanes, the lengths at which
scale doubles its thread count (512 runs of ScaleRun coefficients), the grid-stride wrap of a launch of eight workgroups per compute
unit.  scale is also checked against independent device code (a transform of the scaled coefficients is a coset evaluation), the
derivative against the product rule, and the fused weighted sum against the chain of scalar_mul and add calls."""
import os
import subprocess

import numpy as np
import pytest

from tests import algebra_ref as ref

pytestmark = pytest.mark.gpu

P = ref.P
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXTREME = [0, 1, P - 1, P - 2, (1 << 32) - 1, 1 << 32]
LENGTHS = [1, 2, 63, 64, 65, 255, 256, 257]
SCALE_RUN = {1: 16, 3: 64}  # tfk::ScaleRun<width of alpha>
COMBOS = [(1, 1), (3, 3), (3, 1), (1, 3)]  # (coefficients / columns, scalar / weights)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(tf):
    assert tf.lib().tf_device_count() > 0, "no HIP device visible: the product has no CPU fallback"


def _to_dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def _to_host(t):
    import torch

    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint64)


def _empty(words):
    """an output buffer: every word 2^64 - 1, which no kernel stores (it is not canonical), so a word that is never stored shows --
    torch.empty would hand back the block the previous call of the same size freed, right words included"""
    import torch

    return torch.full((words,), -1, dtype=torch.int64, device="cuda")


def _wrap():
    """words one launch covers before its grid-stride loop wraps: eight workgroups of 256 lanes per compute unit"""
    import torch

    return torch.cuda.get_device_properties(0).multi_processor_count * 8 * 256


def _mix(oracle, words, seed):
    """random raw words with the extreme operands mixed in, as values (BFieldElement::new of them) and as raw words"""
    x = oracle.fill_random(words, seed)
    special = [oracle.bfe_new(v) for v in EXTREME] + [r for r in EXTREME if r < P]
    pos = np.random.default_rng(seed).permutation(words)[:min(words, 2 * len(special))]
    for i, p in enumerate(pos):
        x[p] = special[i % len(special)]
    return x


def _scalars(oracle, w, seed):
    """scalars of width w: a random one, and the extreme ones"""
    out = [oracle.fill_random(w, seed)]
    for v in (0, 1, P - 1):
        s = oracle.fill_random(w, seed + 1)
        s[0] = oracle.bfe_new(v)
        out.append(s)
        if w == 3:
            out.append(np.array([oracle.bfe_new(v), 0, 0], dtype=np.uint64))
    return out


# ------------------------------------------------------------------ 1. add, sub, neg
@pytest.mark.parametrize("w", [1, 3])
def test_add_sub_neg(tf, oracle, w):
    d = tf.device
    for batch in (1, 3):
        for n in LENGTHS:
            short = n // 2 + 1
            for na, nb in {(n, n), (n, short), (short, n)}:
                a = _mix(oracle, na * batch * w, 0x3000 + n)
                b = _mix(oracle, nb * batch * w, 0x3100 + n)
                da, db = _to_dev(a), _to_dev(b)
                nmax = max(na, nb)
                for op, want in ((d.poly_add, ref.add(a, na, b, nb, w, batch)), (d.poly_sub, ref.sub(a, na, b, nb, w, batch))):
                    out = _empty(nmax * batch * w)
                    op(da, na, db, nb, out, batch=batch, width=w)
                    assert np.array_equal(_to_host(out), want), (op.__name__, na, nb, batch)
                    if na == nmax:  # in place on the operand of the result's length
                        x = da.clone()
                        op(x, na, db, nb, x, batch=batch, width=w)
                        assert np.array_equal(_to_host(x), want), (op.__name__, "out = a", na, nb, batch)
                    if nb == nmax:
                        y = db.clone()
                        op(da, na, y, nb, y, batch=batch, width=w)
                        assert np.array_equal(_to_host(y), want), (op.__name__, "out = b", na, nb, batch)
            a = _mix(oracle, n * batch * w, 0x3200 + n)
            want = ref.neg(a, w)
            da = _to_dev(a)
            out = _empty(a.size)
            d.poly_neg_(da, n, out, batch=batch, width=w)
            assert np.array_equal(_to_host(out), want), n
            d.poly_neg_(da, n, batch=batch, width=w)
            assert np.array_equal(_to_host(da), want), n
    # one operand without coefficients: the other one, or its negative
    a = _mix(oracle, 5 * w, 0x32FF)
    out = _empty(5 * w)
    d.poly_sub(_empty(0), 0, _to_dev(a), 5, out, width=w)
    assert np.array_equal(_to_host(out), ref.neg(a, w))
    d.poly_add(_to_dev(a), 5, _empty(0), 0, out, width=w)
    assert np.array_equal(_to_host(out), a)
    # the host-pointer forms, two rows against b = NULL: the empty operand takes no device words
    a = _mix(oracle, 3 * 2 * w, 0x32FE)
    none = np.zeros(0, dtype=np.uint64)
    for fn, want in ((tf.lib().tf_poly_add, ref.add(a, 3, none, 0, w, 2)), (tf.lib().tf_poly_sub, ref.sub(a, 3, none, 0, w, 2))):
        host = np.zeros_like(a)
        assert fn(a.ctypes.data, 3, None, 0, w, host.ctypes.data, 2) == 0
        assert np.array_equal(host, want)
    # the numpy API trims: (a + b) - b == a, a - a == 0
    pa, pb = tf.Polynomial(_mix(oracle, 70 * w, 1), width=w), tf.Polynomial(_mix(oracle, 33 * w, 2), width=w)
    assert np.array_equal(((pa + pb) - pb).coefficients, pa.coefficients) and (pa - pa).degree() == -1
    assert np.array_equal((-(-pb)).coefficients, pb.coefficients) and (pb + (-pb)).degree() == -1


# ------------------------------------------------------------------ 2. scalar_mul, scale, the mixed pointwise product
@pytest.mark.parametrize("wa,ws", COMBOS)
def test_scalar_mul(tf, oracle, wa, ws):
    d = tf.device
    wo = max(wa, ws)
    for batch in (1, 3):
        for n in LENGTHS:
            a = _mix(oracle, n * batch * wa, 0x3300 + n)
            da = _to_dev(a)
            for s in _scalars(oracle, ws, 0x3400 + n)[:4 if n == 65 else 1]:
                want = ref.scalar_mul(a, wa, s, ws)
                out = _empty(n * batch * wo)
                d.poly_scalar_mul(da, n, s, out, batch=batch, width=wa, width_s=ws)
                assert np.array_equal(_to_host(out), want), (n, batch)
                if wa == wo:
                    x = da.clone()
                    d.poly_scalar_mul(x, n, s, x, batch=batch, width=wa, width_s=ws)
                    assert np.array_equal(_to_host(x), want), ("in place", n, batch)
    p = tf.Polynomial(_mix(oracle, 40 * wa, 3), width=wa)
    s = oracle.fill_random(ws, 4)
    assert np.array_equal(p.scalar_mul(s if ws == 3 else int(s[0]), width_s=ws).coefficients, ref.scalar_mul(p.coefficients, wa, s, ws))
    assert p.scalar_mul(np.zeros(ws, dtype=np.uint64), width_s=ws).degree() == -1


@pytest.mark.parametrize("wa,ws", COMBOS)
def test_scale(tf, oracle, wa, ws):
    d = tf.device
    wo = max(wa, ws)
    edge = 512 * SCALE_RUN[ws]  # the thread count of a row doubles here
    for batch, lengths in ((1, LENGTHS + [SCALE_RUN[ws] - 1, SCALE_RUN[ws], SCALE_RUN[ws] + 1, edge - 1, edge, edge + 1]), (3, LENGTHS + [1000])):
        for n in lengths:
            a = _mix(oracle, n * batch * wa, 0x3500 + n)
            da = _to_dev(a)
            for al in _scalars(oracle, ws, 0x3600 + n)[:4 if n == 257 else 1]:
                want = ref.scale(a, n, wa, al, ws, batch)
                out = _empty(n * batch * wo)
                d.poly_scale(da, n, al, out, batch=batch, width=wa, width_alpha=ws)
                assert np.array_equal(_to_host(out), want), (n, batch)
                if wa == wo:
                    x = da.clone()
                    d.poly_scale(x, n, al, x, batch=batch, width=wa, width_alpha=ws)
                    assert np.array_equal(_to_host(x), want), ("in place", n, batch)
    p = tf.Polynomial(_mix(oracle, 40 * wa, 5), width=wa)
    al = oracle.fill_random(ws, 6)
    assert np.array_equal(p.scale(al if ws == 3 else int(al[0]), width_alpha=ws).coefficients, ref.scale(p.coefficients, p.coefficients.size // wa, wa, al, ws))


def test_hadamard_xfe_bfe(tf, oracle):
    d = tf.device
    for n in LENGTHS:
        a, b = _mix(oracle, 3 * n, 0x3700 + n), _mix(oracle, n, 0x3800 + n)
        want = ref.hadamard_xfe_bfe(a, b)
        da, db = _to_dev(a), _to_dev(b)
        out = _empty(3 * n)
        d.hadamard(da, db, out, width=3, width_b=1)
        assert np.array_equal(_to_host(out), want), n
        d.hadamard(da, db, da, width=3, width_b=1)
        assert np.array_equal(_to_host(da), want), n
    with pytest.raises(ValueError):
        d.hadamard(_empty(6), _empty(3), _empty(6), width=3, width_b=1)


# ------------------------------------------------------------------ 3. one grid-stride wrap + 7
@pytest.mark.parametrize("op", ["add", "sub", "neg", "scalar_mul_11", "scalar_mul_13", "scalar_mul_31", "scalar_mul_33", "scale_11", "scale_33",
                                "hadamard_xfe_bfe", "derivative_1", "derivative_3"])
def test_grid_stride_wrap(tf, oracle, op):
    d = tf.device
    wrap = _wrap()
    seed = 0x3900 + len(op)
    if op in ("add", "sub"):  # unequal lengths: rows stay rows
        n, nb = wrap + 7, wrap // 2
        a, b = _mix(oracle, n, seed), _mix(oracle, nb, seed + 1)
        out = _empty(n)
        getattr(d, "poly_" + op)(_to_dev(a), n, _to_dev(b), nb, out)
        want = getattr(ref, op)(a, n, b, nb)
    elif op == "neg":
        n = wrap // 3 + 7  # XFieldElements: the kernel runs over words
        a = _mix(oracle, 3 * n, seed)
        out = _empty(3 * n)
        d.poly_neg_(_to_dev(a), n, out, width=3)
        want = ref.neg(a, 3)
    elif op.startswith("scalar_mul") or op.startswith("scale"):
        wa, ws = int(op[-2]), int(op[-1])
        n = wrap + 7 if (wa, ws) in ((1, 1), (3, 3)) else wrap // 3 + 7
        a, s = _mix(oracle, wa * n, seed), oracle.fill_random(ws, seed + 1)
        out = _empty(max(wa, ws) * n)
        if op.startswith("scalar_mul"):
            d.poly_scalar_mul(_to_dev(a), n, s, out, width=wa, width_s=ws)
            want = ref.scalar_mul(a, wa, s, ws)
        else:
            d.poly_scale(_to_dev(a), n, s, out, width=wa, width_alpha=ws)
            want = ref.scale(a, n, wa, s, ws)
    elif op == "hadamard_xfe_bfe":
        n = wrap // 3 + 7
        a, b = _mix(oracle, 3 * n, seed), _mix(oracle, n, seed + 1)
        out = _empty(3 * n)
        d.hadamard(_to_dev(a), _to_dev(b), out, width=3, width_b=1)
        want = ref.hadamard_xfe_bfe(a, b)
    else:
        w = int(op[-1])
        n = (wrap + 7) // w + 2
        a = _mix(oracle, w * n, seed)
        out = _empty(w * (n - 1))
        d.poly_formal_derivative(_to_dev(a), n, out, width=w)
        want = ref.formal_derivative(a, n, w)
    assert np.array_equal(_to_host(out), want)


# ------------------------------------------------------------------ 4. scale against independent device code
@pytest.mark.parametrize("w", [1, 3])
def test_scale_then_ntt_is_a_coset_evaluation(tf, oracle, w):
    """ntt(zero-padded scale(c, offset)) == fast_coset_evaluate(c, offset, order) (polynomial.rs:1374-1399 is exactly this); BFieldElement
    coefficients and offset, XFieldElement coefficients with an XFieldElement offset"""
    order, n = 1 << 12, (1 << 12) - 5
    c = _mix(oracle, w * n, 0x3A00 + w)
    offset = oracle.fill_random(w, 0x3A10 + w)
    scaled = tf.Polynomial(c, width=w).scale(offset if w == 3 else int(offset[0]), width_alpha=w).coefficients
    x = np.zeros(w * order, dtype=np.uint64)
    x[:scaled.size] = scaled
    tf.ntt(x, width=w)
    assert np.array_equal(x, tf.fast_coset_evaluate(c, offset if w == 3 else int(offset[0]), order, width=w))
    # scale(scale(c, alpha), alpha^-1) == c
    inv = oracle.xfe_inverse(offset) if w == 3 else np.array([oracle.bfe_inverse(int(offset[0]))], dtype=np.uint64)
    dc = _to_dev(c)
    t = _empty(w * n)
    tf.device.poly_scale(dc, n, offset, t, width=w, width_alpha=w)
    tf.device.poly_scale(t, n, inv, t, width=w, width_alpha=w)
    assert np.array_equal(_to_host(t), c)


# ------------------------------------------------------------------ 5. degree
def _degrees(tf, a, na, w, batch):
    import torch

    deg = torch.full((batch,), 77, dtype=torch.int64, device="cuda")
    tf.device.poly_degree(_to_dev(a) if a.size else _empty(0), na, deg, batch=batch, width=w)
    torch.cuda.synchronize()
    got = deg.cpu().numpy()
    host = np.full(batch, 77, dtype=np.int64)
    import ctypes as C

    rc = tf.lib().tf_poly_degree(C.c_void_p(a.ctypes.data) if a.size else None, na, w, batch, C.c_void_p(host.ctypes.data))
    assert rc == 0 and np.array_equal(host, got)
    return got


@pytest.mark.parametrize("w", [1, 3])
def test_degree(tf, oracle, w):
    zeros = lambda n: np.zeros(n * w, dtype=np.uint64)  # noqa: E731
    assert _degrees(tf, zeros(1000), 1000, w, 1).tolist() == [-1]
    assert _degrees(tf, zeros(0), 0, w, 3).tolist() == [-1, -1, -1]
    for lead in (0, 1, 63, 64, 65, 4097):  # leading zeros above the highest coefficient
        for n in (lead + 1, lead + 300, lead + 70000):
            a = _mix(oracle, n * w, 0x3B00 + lead)
            a[(n - lead) * w:] = 0
            a[(n - lead - 1) * w:(n - lead) * w] = 0
            a[(n - lead - 1) * w + (w - 1)] = 5  # the only non-zero limb of the leading coefficient is the last one
            assert _degrees(tf, a, n, w, 1).tolist() == [n - lead - 1] == ref.degree(a, n, w).tolist(), (lead, n)
    # three rows with different degrees, one of them zero
    n = 5000
    a = _mix(oracle, 3 * n * w, 0x3BFF)
    a[(0 * n + 4000) * w:1 * n * w] = 0
    a[1 * n * w:2 * n * w] = 0
    a[(3 * n - 1) * w:] = 1
    a[(0 * n + 3999) * w] = 9
    assert _degrees(tf, a, n, w, 3).tolist() == [3999, -1, n - 1] == ref.degree(a, n, w, 3).tolist()
    # the lowest coefficient alone
    a = zeros(70000)
    a[w - 1] = 3
    assert _degrees(tf, a, 70000, w, 1).tolist() == [0]


# ------------------------------------------------------------------ 6. formal_derivative
@pytest.mark.parametrize("w", [1, 3])
def test_formal_derivative(tf, oracle, w):
    import torch

    d = tf.device
    for batch in (1, 3):
        for n in (0, 1, 2, 257):
            a = _mix(oracle, n * batch * w, 0x3C00 + n) if n else np.zeros(0, dtype=np.uint64)
            out = torch.full((max(n - 1, 0) * batch * w + 1,), 123, dtype=torch.int64, device="cuda")
            d.poly_formal_derivative(_to_dev(a) if n else _empty(0), n, out[:-1], batch=batch, width=w)
            got = _to_host(out)
            assert got[-1] == 123  # the word after the result
            if n > 1:
                assert np.array_equal(got[:-1], ref.formal_derivative(a, n, w, batch)), (n, batch)
    assert tf.Polynomial(_mix(oracle, w, 9), width=w).formal_derivative().degree() == -1
    # the product rule through poly_mul and the new add: (a b)' == a' b + a b', na = nb = 300
    n = 300
    a, b = _to_dev(_mix(oracle, n * w, 0x3CA0)), _to_dev(_mix(oracle, n * w, 0x3CA1))
    ab, da, db = _empty((2 * n - 1) * w), _empty((n - 1) * w), _empty((n - 1) * w)
    d.poly_mul(a, n, b, n, ab, width=w)
    lhs = _empty((2 * n - 2) * w)
    d.poly_formal_derivative(ab, 2 * n - 1, lhs, width=w)
    d.poly_formal_derivative(a, n, da, width=w)
    d.poly_formal_derivative(b, n, db, width=w)
    t1, t2 = _empty((2 * n - 2) * w), _empty((2 * n - 2) * w)
    d.poly_mul(da, n - 1, b, n, t1, width=w)
    d.poly_mul(a, n, db, n - 1, t2, width=w)
    d.poly_add(t1, 2 * n - 2, t2, 2 * n - 2, t1, width=w)
    torch.cuda.synchronize()
    assert torch.equal(lhs, t1)


# ------------------------------------------------------------------ 7. the weighted sum of columns
def _table(oracle, n, wp, k, pad, seed):
    """k columns of n elements, `pad` words of p - 1 after each (they must not reach the result)"""
    stride = n * wp + pad
    cols = _mix(oracle, max(k * stride, 1), seed)[:k * stride]
    for j in range(k):
        cols[j * stride + n * wp:(j + 1) * stride] = P - 1
    return cols, stride


def _lincomb(tf, cols, n, wp, stride, k, wts, ww):
    out = _empty(n * max(wp, ww))
    tf.device.linear_combination(_to_dev(cols) if cols.size else _empty(0), n, k, _to_dev(wts) if wts.size else _empty(0), out, width=wp, width_w=ww,
                                 stride=stride)
    return _to_host(out)


@pytest.mark.parametrize("wp,ww", COMBOS)
def test_linear_combination(tf, oracle, wp, ww):
    for n in (1, 63, 64, 65, 255, 256, 257, 1000):
        for k in (0, 1, 2, 3, 17):
            cols, stride = _table(oracle, n, wp, k, 5, 0x3D00 + n + k)
            wts = _mix(oracle, max(k * ww, 1), 0x3E00 + n + k)[:k * ww]
            want = ref.linear_combination(cols, n, wp, stride, k, wts, ww)
            assert np.array_equal(_lincomb(tf, cols, n, wp, stride, k, wts, ww), want), (n, k)
            if n == 257:  # the host form packs the columns on the way up
                assert np.array_equal(tf.linear_combination(cols, wts, n, width=wp, width_w=ww, stride=stride), want), (n, k)
    # every operand p - 1, 300 terms: the products carry into the third accumulator word in every lane
    n, k = 65, 300
    cols = np.full(k * n * wp, P - 1, dtype=np.uint64)
    wts = np.full(k * ww, P - 1, dtype=np.uint64)
    assert np.array_equal(_lincomb(tf, cols, n, wp, n * wp, k, wts, ww), ref.linear_combination(cols, n, wp, n * wp, k, wts, ww))


def test_linear_combination_of_65535_columns(tf, oracle):
    k = 65535
    for fill in (None, P - 1):
        cols = _mix(oracle, k, 0x3F00) if fill is None else np.full(k, fill, dtype=np.uint64)
        wts = _mix(oracle, k, 0x3F01) if fill is None else np.full(k, fill, dtype=np.uint64)
        assert np.array_equal(_lincomb(tf, cols, 1, 1, 1, k, wts, 1), ref.linear_combination(cols, 1, 1, 1, k, wts, 1))


@pytest.mark.parametrize("wp,ww", COMBOS)
def test_fused_sum_equals_the_chain_of_scalar_mul_and_add(tf, oracle, wp, ww):
    import torch

    d = tf.device
    n, k = (1 << 16) + 7, 24
    wo = max(wp, ww)
    stride = n * wp + 3
    cols = _empty(k * stride)
    d.fill_random(cols, 0x4000 + wp)
    wts = oracle.fill_random(k * ww, 0x4001 + ww)
    fused = _empty(n * wo)
    d.linear_combination(cols, n, k, _to_dev(wts), fused, width=wp, width_w=ww, stride=stride)
    acc = torch.zeros(n * wo, dtype=torch.int64, device="cuda")
    term = _empty(n * wo)
    for j in range(k):
        d.poly_scalar_mul(cols[j * stride:j * stride + n * wp], n, wts[j * ww:(j + 1) * ww], term, width=wp, width_s=ww)
        d.poly_add(acc, n, term, n, acc, width=wo)
    torch.cuda.synchronize()
    assert torch.equal(fused, acc)


# ------------------------------------------------------------------ 8. the C++ mirror
def test_cpp_mirror_doc_examples_pass():
    host = os.path.join(ROOT, "twenty-first_amd", "host")
    subprocess.check_call(["make", "-C", host, "selftest"], stdout=subprocess.DEVNULL)
    r = subprocess.run([os.path.join(host, "selftest")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "polynomial arithmetic: formal_derivative and scalar_mul doc examples, add / sub / neg, scale, linear_combination: PASS" in r.stdout
