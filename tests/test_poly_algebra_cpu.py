"""Polynomial arithmetic (add, sub, neg, scalar_mul, scale, formal_derivative, degree, the XFieldElement x BFieldElement product and the
weighted sum of columns): the parts that need no GPU -- the exported symbols, the argument errors every flavour returns before any
HIP call and their order, the shape checks of the Python wrappers, and the expected-value builder the GPU tests compare against
(tests/algebra_ref.py), pinned here against the oracle and tests/pyref."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import algebra_ref as ref
from tests import pyref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = ref.P

NEW = ("tf_poly_add", "tf_poly_add_dev", "tf_poly_sub", "tf_poly_sub_dev", "tf_poly_neg", "tf_poly_neg_dev", "tf_poly_scalar_mul",
       "tf_poly_scalar_mul_dev", "tf_poly_scale", "tf_poly_scale_dev", "tf_poly_formal_derivative", "tf_poly_formal_derivative_dev",
       "tf_poly_degree", "tf_poly_degree_dev", "tf_hadamard_xfe_bfe_dev", "tf_poly_linear_combination", "tf_poly_linear_combination_dev")
OK, LEN_TOO_LARGE, NULL, NO_DEVICE, INVALID = 0, 5, 7, 8, 17
BIG = (1 << 30) + 1

# values every carry path of the field arithmetic meets; used as values AND as raw words
EXTREME = [0, 1, P - 1, P - 2, (1 << 32) - 1, 1 << 32]


def _p(a):
    return C.c_void_p(a.ctypes.data)


def test_symbols_declared_and_exported(tf):
    from twenty_first_amd import _lib

    header = open(os.path.join(ROOT, "include", "tf_hip.h")).read()
    lib = tf.lib()
    for name in NEW:
        assert name + "(" in header, name
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
    assert lib.tf_version() == 1002  # new entry points are found by their symbols, not by a version bump


def _calls(lib, x, s, out, deg, bad_width=None, big=None, null=None):
    """One call of every entry point as (name, thunk): valid arguments (4 coefficients, width 1) except for the one thing asked
    for: bad_width replaces every width, big every length, null = index of the pointer argument to replace by NULL."""
    w = 1 if bad_width is None else bad_width
    n = 4 if big is None else big
    S = None  # the stream

    def ptrs(*ps):
        return [None if null is not None and i == null else _p(p) for i, p in enumerate(ps)]

    calls = []
    for dev in (False, True):
        tail = (S,) if dev else ()
        sfx = "_dev" if dev else ""
        a, b, o = ptrs(x, x, out)
        calls.append((f"tf_poly_add{sfx}", 3, lambda a=a, b=b, o=o, f=getattr(lib, f"tf_poly_add{sfx}"), t=tail: f(a, n, b, n, w, o, 1, *t)))
        calls.append((f"tf_poly_sub{sfx}", 3, lambda a=a, b=b, o=o, f=getattr(lib, f"tf_poly_sub{sfx}"), t=tail: f(a, n, b, n, w, o, 1, *t)))
        a, o = ptrs(x, out)
        calls.append((f"tf_poly_neg{sfx}", 2, lambda a=a, o=o, f=getattr(lib, f"tf_poly_neg{sfx}"), t=tail: f(a, n, w, o, 1, *t)))
        calls.append((f"tf_poly_formal_derivative{sfx}", 2,
                      lambda a=a, o=o, f=getattr(lib, f"tf_poly_formal_derivative{sfx}"), t=tail: f(a, n, w, o, 1, *t)))
        a, sc, o = ptrs(x, s, out)
        for nm in ("scalar_mul", "scale"):
            calls.append((f"tf_poly_{nm}{sfx}", 3, lambda a=a, sc=sc, o=o, f=getattr(lib, f"tf_poly_{nm}{sfx}"), t=tail: f(a, n, w, sc, w, o, 1, *t)))
        a, d = ptrs(x, deg)
        calls.append((f"tf_poly_degree{sfx}", 2, lambda a=a, d=d, f=getattr(lib, f"tf_poly_degree{sfx}"), t=tail: f(a, n, w, 1, d, *t)))
        c, wt, o = ptrs(x, s, out)
        calls.append((f"tf_poly_linear_combination{sfx}", 3,
                      lambda c=c, wt=wt, o=o, f=getattr(lib, f"tf_poly_linear_combination{sfx}"), t=tail: f(c, n, w, n * max(w, 1), 1, wt, w, o, *t)))
    return calls


def test_argument_errors_in_the_documented_order_without_device(tf):
    lib = tf.lib()
    x = np.ones(12, dtype=np.uint64)
    s = np.ones(3, dtype=np.uint64)
    out = np.zeros(12, dtype=np.uint64)
    deg = np.zeros(1, dtype=np.int64)
    no_gpu = lib.tf_device_count() == 0
    # 1. a NULL pointer, whichever it is -- also when a width is wrong and a length too large
    for null in range(3):
        for kw in ({}, {"bad_width": 2}, {"big": BIG}, {"bad_width": 2, "big": BIG}):
            for name, n_ptrs, call in _calls(lib, x, s, out, deg, null=null, **kw):
                if null < n_ptrs:
                    assert call() == NULL, (name, null, kw)
    a, b, o = _p(x), _p(x), _p(out)
    assert lib.tf_hadamard_xfe_bfe_dev(None, b, o, 4, None) == NULL
    assert lib.tf_hadamard_xfe_bfe_dev(a, None, o, 4, None) == NULL
    assert lib.tf_hadamard_xfe_bfe_dev(a, b, None, 4, None) == NULL
    # 2. a width other than 1 or 3 -- also when a length is too large
    for bad in (0, 2, 4, -1):
        for kw in ({}, {"big": BIG}):
            for name, _, call in _calls(lib, x, s, out, deg, bad_width=bad, **kw):
                assert call() == INVALID, (name, bad, kw)
    # a good width on one side does not excuse the other
    for fn in (lib.tf_poly_scalar_mul, lib.tf_poly_scale):
        assert fn(a, 4, 1, _p(s), 2, o, 1) == INVALID and fn(a, 4, 2, _p(s), 3, o, 1) == INVALID
    for fn in (lib.tf_poly_scalar_mul_dev, lib.tf_poly_scale_dev):
        assert fn(a, 4, 1, _p(s), 2, o, 1, None) == INVALID and fn(a, 4, 2, _p(s), 3, o, 1, None) == INVALID
    assert lib.tf_poly_linear_combination(a, 4, 1, 4, 1, _p(s), 2, o) == INVALID
    assert lib.tf_poly_linear_combination_dev(a, 4, 3, 12, 1, _p(s), 0, o, None) == INVALID
    # stride < n * width_p, before the length limits
    assert lib.tf_poly_linear_combination(a, 4, 1, 3, 1, _p(s), 1, o) == INVALID
    assert lib.tf_poly_linear_combination_dev(a, 4, 3, 11, 1, _p(s), 1, o, None) == INVALID
    assert lib.tf_poly_linear_combination(a, 4, 1, 3, 65536, _p(s), 1, o) == INVALID
    assert lib.tf_poly_linear_combination_dev(a, BIG, 1, BIG - 1, 1, _p(s), 1, o, None) == INVALID
    # 3. a length above 2^30, k above 65 535
    for name, _, call in _calls(lib, x, s, out, deg, big=BIG):
        assert call() == LEN_TOO_LARGE, name
    assert lib.tf_poly_add(a, 4, b, BIG, 1, o, 1) == LEN_TOO_LARGE and lib.tf_poly_sub_dev(a, BIG, b, 4, 1, o, 1, None) == LEN_TOO_LARGE
    assert lib.tf_poly_linear_combination(a, 4, 1, 4, 65536, _p(s), 1, o) == LEN_TOO_LARGE
    assert lib.tf_poly_linear_combination_dev(a, 4, 1, 4, 65536, _p(s), 3, o, None) == LEN_TOO_LARGE
    # 4. a valid call: TF_ERR_NO_DEVICE without a GPU; with one, the host forms run (the _dev forms want device pointers)
    for name, _, call in _calls(lib, x, s, out, deg):
        if no_gpu:
            assert call() == NO_DEVICE, name
        elif not name.endswith("_dev"):
            assert call() == OK, name
    if no_gpu:
        assert lib.tf_hadamard_xfe_bfe_dev(a, b, o, 4, None) == NO_DEVICE
        assert not out.any()


def test_empty_calls_return_ok_and_touch_nothing(tf):
    lib = tf.lib()
    x = np.ones(12, dtype=np.uint64)
    s = np.ones(3, dtype=np.uint64)
    out = np.zeros(12, dtype=np.uint64)
    deg = np.full(2, 5, dtype=np.int64)
    for dev in (False, True):
        t = (None,) if dev else ()
        sfx = "_dev" if dev else ""
        f = lambda nm: getattr(lib, f"tf_poly_{nm}{sfx}")  # noqa: E731
        for w in (1, 3):
            for args in ((None, 0, None, 0, w, None, 3), (None, 4, None, 4, w, None, 0)):
                assert f("add")(*args, *t) == OK and f("sub")(*args, *t) == OK
            for nm in ("neg", "formal_derivative"):
                assert f(nm)(None, 0, w, None, 3, *t) == OK and f(nm)(None, 4, w, None, 0, *t) == OK
            assert f("formal_derivative")(None, 1, w, None, 3, *t) == OK  # a constant: nothing to write
            for nm in ("scalar_mul", "scale"):
                assert f(nm)(None, 0, w, None, w, None, 3, *t) == OK and f(nm)(None, 4, w, None, w, None, 0, *t) == OK
            assert f("degree")(None, 4, w, 0, None, *t) == OK
            assert f("linear_combination")(None, 0, w, 0, 5, None, w, None, *t) == OK
        # pointers that are given stay untouched
        assert f("add")(_p(x), 0, _p(x), 0, 1, _p(out), 3, *t) == OK
        assert f("scale")(_p(x), 0, 1, _p(s), 1, _p(out), 3, *t) == OK
        assert f("linear_combination")(_p(x), 0, 1, 0, 3, _p(s), 1, _p(out), *t) == OK
    assert lib.tf_hadamard_xfe_bfe_dev(None, None, None, 0, None) == OK
    assert not out.any() and (deg == 5).all()
    # degree of polynomials without coefficients: -1 per row, by length alone (host form; no device needed)
    assert lib.tf_poly_degree(None, 0, 3, 2, _p(deg)) == OK
    assert (deg == -1).all()
    assert lib.tf_poly_degree(None, 0, 1, 2, None) == NULL


def test_python_shapes_are_checked_on_the_host(tf):
    u = lambda *v: np.array(v, dtype=np.uint64)  # noqa: E731
    a, x = tf.Polynomial(u(1, 2, 3)), tf.Polynomial(u(1, 2, 3), width=3)
    with pytest.raises(TypeError):
        a + x
    with pytest.raises(TypeError):
        x - a
    with pytest.raises(ValueError):
        a.scalar_mul(u(1, 2), width_s=3)
    with pytest.raises(ValueError):
        a.scalar_mul(5, width_s=2)
    with pytest.raises(ValueError):
        a.scale(u(1, 2, 3))
    with pytest.raises(ValueError):
        tf.linear_combination(u(1, 2, 3, 4), u(1, 1), 2, stride=1)
    with pytest.raises(ValueError):
        tf.linear_combination(u(1, 2, 3), u(1, 1), 2)  # two columns of two need four words
    with pytest.raises(ValueError):
        tf.linear_combination(u(1, 2, 3, 4), u(1, 1), 2, width_w=3)
    with pytest.raises(ValueError):
        tf.linear_combination(u(1, 2, 3, 4), u(1, 1), 2, width=2)
    # empty operands never reach a device
    z = tf.Polynomial(u())
    assert (z + z).degree() == -1 and (-z).degree() == -1 and z.scalar_mul(3).degree() == -1 and z.scale(3).degree() == -1
    assert z.formal_derivative().degree() == -1 and tf.Polynomial(u(7)).formal_derivative().degree() == -1
    assert tf.linear_combination(u(), u(), 0).size == 0


# ------------------------------------------------------------------ the expected-value builder
def _operands(oracle, seed, count):
    """raw words: random ones, the extreme VALUES as raw words (BFieldElement::new of them) and the extreme numbers AS raw words"""
    raws = [int(v) for v in oracle.fill_random(count, seed)]
    raws += [oracle.bfe_new(v) for v in EXTREME]
    raws += [r for r in EXTREME if r < P]
    return raws


def test_ref_base_field_against_the_oracle(oracle):
    xs = _operands(oracle, 0xA1, 12)
    for a in xs:
        assert int(ref.neg(np.array([a], dtype=np.uint64))[0]) == oracle.bfe_neg(a)
        for b in xs:
            A, B = np.array([a], dtype=np.uint64), np.array([b], dtype=np.uint64)
            assert int(ref.add(A, 1, B, 1)[0]) == oracle.bfe_add(a, b)
            assert int(ref.sub(A, 1, B, 1)[0]) == oracle.bfe_sub(a, b)
            assert int(ref.scalar_mul(A, 1, B, 1)[0]) == oracle.bfe_mul(a, b)
            assert ref.to_raw(ref.to_val(a) * ref.to_val(b)) == oracle.bfe_mul(a, b)
    assert ref.to_raw(1) == 0xFFFFFFFF and ref.to_val(0xFFFFFFFF) == 1


def test_ref_extension_field_against_the_oracle_and_pyref(oracle):
    xs = _operands(oracle, 0xA2, 9)
    rng = np.random.default_rng(5)
    elems = [np.array(rng.choice(xs, 3), dtype=np.uint64) for _ in range(40)]
    elems += [np.array([x, 0, 0], dtype=np.uint64) for x in xs[-6:]] + [np.array([0, 0, x], dtype=np.uint64) for x in xs[-12:-6]]
    elems.append(np.array([P - 1] * 3, dtype=np.uint64))
    for i, a in enumerate(elems):
        b = elems[(7 * i + 3) % len(elems)]
        assert np.array_equal(ref.add(a, 1, b, 1, w=3), oracle.xfe_add(a, b))
        assert np.array_equal(ref.sub(a, 1, b, 1, w=3), oracle.xfe_sub(a, b))
        assert np.array_equal(ref.scalar_mul(a, 3, b, 3), oracle.xfe_mul(a, b))
        va, vb = ref.elements(a, 3)[0], ref.elements(b, 3)[0]
        assert ref.f_mul(va, vb) == pyref.xfe_mul(va, vb)
        assert ref.f_pow(va, 1000 + i) == pyref.xfe_pow(va, 1000 + i)
        # the mixed products are products with the lift (x_field_element.rs:491-556)
        lifted = np.array([b[0], 0, 0], dtype=np.uint64)
        assert np.array_equal(ref.scalar_mul(a, 3, b[:1], 1), oracle.xfe_mul(a, lifted))
        assert np.array_equal(ref.scalar_mul(b[:1], 1, a, 3), oracle.xfe_mul(lifted, a))
        assert np.array_equal(ref.hadamard_xfe_bfe(a, b[:1]), oracle.xfe_mul(a, lifted))
        assert np.array_equal(ref.neg(a, 3), oracle.xfe_sub(np.zeros(3, dtype=np.uint64), a))


def test_ref_scale_against_the_oracle(oracle):
    for w in (1, 3):
        c = oracle.fill_random(w * 70, 0xA3 + w)
        c[:len(EXTREME)] = EXTREME[:2] + [P - 1, P - 2] + EXTREME[4:]
        for alpha in (oracle.bfe_new(7), oracle.bfe_new(P - 1), oracle.bfe_new(1 << 32), 0, int(oracle.fill_random(1, 0xA5)[0])):
            assert np.array_equal(ref.scale(c, 70, w, np.array([alpha], dtype=np.uint64), 1), oracle.poly_scale(c, alpha, width=w)), (w, alpha)
    # an XFieldElement alpha: powers against pyref
    al = oracle.fill_random(3, 0xA6)
    one = np.zeros(3 * 20, dtype=np.uint64)
    one[::3] = 0xFFFFFFFF
    got = ref.elements(ref.scale(one, 20, 3, al, 3), 3)
    va = ref.elements(al, 3)[0]
    assert got == [pyref.xfe_pow(va, j) for j in range(20)]
    # two rows: the power restarts
    c = oracle.fill_random(10, 0xA7)
    a7 = np.array([oracle.bfe_new(7)], dtype=np.uint64)
    assert np.array_equal(ref.scale(c, 5, 1, a7, 1, batch=2), np.concatenate([oracle.poly_scale(c[:5], int(a7[0])), oracle.poly_scale(c[5:], int(a7[0]))]))


def test_ref_derivative_degree_and_linear_combination(oracle):
    new = oracle.bfe_new
    u = lambda *v: np.array([new(x) for x in v], dtype=np.uint64)  # noqa: E731
    # the reference's doc example, polynomial.rs:265-273: 1 + 2x + 3x^2 + 4x^3 -> 2 + 6x + 12x^2
    assert np.array_equal(ref.formal_derivative(u(1, 2, 3, 4), 4), u(2, 6, 12))
    assert np.array_equal(ref.formal_derivative(u(2, 5, 12, 4), 4), u(5, 24, 12))
    assert np.array_equal(ref.formal_derivative(u(2, 5, 12, 1, 1, 1), 3, batch=2), u(5, 24, 1, 2))
    assert ref.formal_derivative(u(9), 1).size == 0
    assert ref.degree(u(1, 2, 0, 0, 0, 0, 7, 0, 0), 3, batch=3).tolist() == [1, -1, 0]
    assert ref.degree(np.array([0, 0, 0, 0, 0, 5], dtype=np.uint64), 2, w=3).tolist() == [1]
    assert ref.degree(np.zeros(0, dtype=np.uint64), 0, batch=2).tolist() == [-1, -1]
    # add with unequal lengths, both ways
    assert np.array_equal(ref.add(u(1, 2, 3), 3, u(10), 1), u(11, 2, 3)) and np.array_equal(ref.sub(u(10), 1, u(1, 2, 3), 3), u(9, P - 2, P - 3))
    # the weighted sum is the chain scalar_mul, add -- padding words never enter
    for wp, ww in ((1, 1), (3, 3), (3, 1), (1, 3)):
        n, k = 5, 3
        stride = n * wp + 2
        cols = oracle.fill_random(k * stride, 0xB0 + wp + 2 * ww)
        wts = oracle.fill_random(k * ww, 0xC0 + wp)
        want = ref.linear_combination(cols, n, wp, stride, k, wts, ww)
        wo = max(wp, ww)
        acc = np.zeros(n * wo, dtype=np.uint64)
        for j in range(k):
            acc = ref.add(acc, n, ref.scalar_mul(cols[j * stride:j * stride + n * wp], wp, wts[j * ww:(j + 1) * ww], ww), n, w=wo)
        assert np.array_equal(want, acc)
        poisoned = cols.copy()
        for j in range(k):
            poisoned[j * stride + n * wp:(j + 1) * stride] = P - 1
        assert np.array_equal(ref.linear_combination(poisoned, n, wp, stride, k, wts, ww), want)
        assert not ref.linear_combination(cols, n, wp, stride, 0, wts[:0], ww).any()
