"""Colinearity checks, element-wise powers, geometric sequences and index gathers: the parts that need no GPU -- the expected-value
model the GPU tests compare against (tests/points_ref.py) pinned to the reference's doc examples, to tests/pyref and to the oracle;
the exported symbols; the argument errors every flavour returns before any HIP call, and their order."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import points_ref as ref
from tests import pyref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = ref.P

NEW = ("tf_get_colinear_y", "tf_get_colinear_y_dev", "tf_are_colinear", "tf_are_colinear_dev", "tf_mod_pow", "tf_mod_pow_dev", "tf_powers",
       "tf_powers_dev", "tf_gather_elements_dev")
OK, LEN_TOO_LARGE, NULL, NO_DEVICE, INVALID = 0, 5, 7, 8, 17
BIG = (1 << 30) + 1
EXPONENTS = [0, 1, 2, (1 << 32) - 1, 1 << 32, 1 << 63, (1 << 64) - 1, P - 1, P - 2]


def _p(a):
    return C.c_void_p(a.ctypes.data)


def _rand_elem(rng, w):
    v = [int(x) % P for x in rng.integers(0, 1 << 63, 2 * w, dtype=np.uint64)]
    v = [(v[2 * i] << 1 ^ v[2 * i + 1]) % P for i in range(w)]
    return v[0] if w == 1 else tuple(v)


# ------------------------------------------------------------------ the model, pinned to the reference
def test_model_doc_examples():
    pts = lambda *xy: [(x % P, y % P) for x, y in xy]  # noqa: E731
    # polynomial.rs:340-346
    assert ref.are_colinear_elem(pts((0, 0), (1, 1), (2, 2)), 1, 1)
    assert not ref.are_colinear_elem(pts((0, 0), (1, 1), (2, 3)), 1, 1)
    # :376-384
    y = ref.colinear_y_elem((0, 0), (2, 4), 1, 1, 1)
    assert y == 2
    assert ref.are_colinear_elem(pts((0, 0), (2, 4), (1, y)), 1, 1)
    # the same through the raw-word layouts
    raw = lambda *v: np.array([pyref.to_raw(x) for x in v], dtype=np.uint64)  # noqa: E731
    out, bad = ref.get_colinear_y(raw(0), raw(0), raw(2), raw(4), raw(1), 1, 1)
    assert out.tolist() == raw(2).tolist() and bad == []
    assert ref.are_colinear(raw(0, 1, 2, 0, 1, 2), raw(0, 1, 2, 0, 1, 3), 2, 3, 1, 1).tolist() == [1, 0]
    # x0 == x1 is the reference's panic (:387)
    assert ref.colinear_y_elem((5, 1), (5, 2), 7, 1, 1) is None
    assert ref.get_colinear_y(raw(5, 1), raw(1, 1), raw(5, 2), raw(2, 3), raw(7), 1, 1)[1] == [0]


def test_model_are_colinear_short_groups_and_repeated_x():
    for wx, wy in ref.PAIRS:
        lx, ly = (lambda v: v) if wx == 1 else pyref.xfe, (lambda v: v) if wy == 1 else pyref.xfe
        line = [(lx(x), ly(3 * x + 5)) for x in (1, 2, 3, 4)]
        assert ref.are_colinear_elem(line, wx, wy) and ref.are_colinear_elem(line[:3], wx, wy)
        assert not ref.are_colinear_elem(line[:2], wx, wy) and not ref.are_colinear_elem(line[:1], wx, wy) and not ref.are_colinear_elem([], wx, wy)
        # a repeated x, although every point lies on the line
        assert not ref.are_colinear_elem(line + [line[0]], wx, wy) and not ref.are_colinear_elem(line[:2] + [line[1]] + line[2:], wx, wy)
    # XFieldElements that differ in one limb only are different x-coordinates
    a, b = (7, 1, 2), (7, 1, 3)
    slope, icpt = (3, 4, 5), (9, 0, 1)
    on = lambda x: (x, pyref.xfe_add(pyref.xfe_mul(slope, x), icpt))  # noqa: E731
    assert ref.are_colinear_elem([on(a), on(b), on((1, 1, 1))], 3, 3)
    assert not ref.are_colinear_elem([on(a), on(b), on(a)], 3, 3)


@pytest.mark.parametrize("wx,wy", ref.PAIRS)
def test_model_colinear_y_lies_on_the_line(wx, wy):
    rng = np.random.default_rng(0x70 + wx + wy)
    for _ in range(200):
        p0, p1 = (_rand_elem(rng, wx), _rand_elem(rng, wy)), (_rand_elem(rng, wx), _rand_elem(rng, wy))
        # the third x-coordinate has to be a legal x of the width pair for are_colinear; get_colinear_y itself takes any p2x of width_y
        x2 = _rand_elem(rng, wx)
        y2 = ref.colinear_y_elem(p0, p1, ref.lift(x2, wx, wy), wx, wy)
        assert ref.are_colinear_elem([p0, p1, (x2, y2)], wx, wy)
        off = ref.f_add(y2, ref.one(wy), wy)
        assert not ref.are_colinear_elem([p0, p1, (x2, off)], wx, wy)


def test_model_mixed_equals_extension_on_lifted_inputs():
    rng = np.random.default_rng(0x7A)
    for _ in range(200):
        p0, p1 = (_rand_elem(rng, 1), _rand_elem(rng, 3)), (_rand_elem(rng, 1), _rand_elem(rng, 3))
        q = _rand_elem(rng, 3)
        lifted = [(pyref.xfe(x), y) for x, y in (p0, p1)]
        y = ref.colinear_y_elem(p0, p1, q, 1, 3)
        assert y == ref.colinear_y_elem(lifted[0], lifted[1], q, 3, 3)
        x2 = _rand_elem(rng, 1)
        for y2 in (ref.colinear_y_elem(p0, p1, pyref.xfe(x2), 1, 3), q):
            assert ref.are_colinear_elem([p0, p1, (x2, y2)], 1, 3) == ref.are_colinear_elem(lifted + [(pyref.xfe(x2), y2)], 3, 3)
    # the model's XFieldElement inverse (cofactors) against Fermat in the field of p^3 elements
    for _ in range(10):
        a = _rand_elem(rng, 3)
        assert ref.f_inv(a, 3) == pyref.xfe_inv(a) and pyref.xfe_mul(a, ref.f_inv(a, 3)) == (1, 0, 0)
    assert ref.f_inv((5, 0, 0), 3) == (pow(5, P - 2, P), 0, 0)


def test_model_mod_pow(oracle):
    rng = np.random.default_rng(0x7B)
    vals = [0, 1, P - 1, 7] + [_rand_elem(rng, 1) for _ in range(4)]
    for v in vals:
        raw = np.array([pyref.to_raw(v)], dtype=np.uint64)
        got = ref.mod_pow(raw, np.array(EXPONENTS, dtype=np.uint64), 1, len(EXPONENTS))
        assert [pyref.to_val(int(g)) for g in got] == [pow(v, e, P) for e in EXPONENTS]
        assert int(got[0]) == pyref.to_raw(1)  # x^0 = 1, zero included
        if v:
            assert int(got[EXPONENTS.index(P - 2)]) == oracle.bfe_inverse(int(raw[0]))
        for e in EXPONENTS[:5]:
            assert int(ref.mod_pow(raw, np.array([e], dtype=np.uint64), 1, 1)[0]) == oracle.bfe_mod_pow(int(raw[0]), e)
    xs = [(0, 0, 0), (1, 0, 0), (P - 1, 0, 0), (0, 5, 0), (0, 0, 5)] + [_rand_elem(rng, 3) for _ in range(3)]
    for x in xs:
        raw = ref.words([x], 3)
        got = ref.elements(ref.mod_pow(raw, np.array(EXPONENTS, dtype=np.uint64), 3, len(EXPONENTS)), 3)
        assert got == [pyref.xfe_pow(x, e) for e in EXPONENTS]
        assert got[0] == (1, 0, 0)
    # both broadcasts
    b = ref.words([3, 5], 1)
    assert ref.elements(ref.mod_pow(b, np.array([2], dtype=np.uint64), 1, 2), 1) == [9, 25]
    assert ref.elements(ref.mod_pow(b[:1], np.array([2, 3], dtype=np.uint64), 1, 2), 1) == [9, 27]


def test_model_powers():
    rng = np.random.default_rng(0x7C)
    for w in (1, 3):
        for ratio in (ref.zero(w), ref.one(w), _rand_elem(rng, w)):
            first = _rand_elem(rng, w)
            got = ref.elements(ref.powers(ref.words([first], w), ref.words([ratio], w), w, 9), w)
            assert got == [ref.f_mul(first, ref.f_pow(ratio, i, w), w) for i in range(9)]
        assert ref.powers(ref.words([first], w), ref.words([ratio], w), w, 0).size == 0
    # a cyclic group: the eight powers of a root of unity of order 8 (b_field_element.rs:656-668)
    g = pyref.root_of_unity(8)
    grp = ref.elements(ref.powers(ref.words([1], 1), ref.words([g], 1), 1, 9), 1)
    assert grp[8] == 1 and len(set(grp[:8])) == 8


def test_model_gather():
    src = np.arange(15, dtype=np.uint64)
    out, bad = ref.gather(src, 5, [2, 0, 2, 3, 1])
    assert out.tolist() == [10, 11, 12, 13, 14, 0, 1, 2, 3, 4, 10, 11, 12, 13, 14, 0, 0, 0, 0, 0, 5, 6, 7, 8, 9] and bad == [3]


# ------------------------------------------------------------------ the ABI on a machine without a GPU
def test_symbols_declared_and_exported(tf):
    from twenty_first_amd import _lib

    header = open(os.path.join(ROOT, "include", "tf_hip.h")).read()
    exports = open(os.path.join(ROOT, "twenty-first_amd", "csrc", "tf_exports.map")).read()
    assert "global: tf_*;" in exports  # every tf_ symbol of the library is exported, and nothing else
    lib = tf.lib()
    for name in NEW:
        assert name + "(" in header, name
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
    assert lib.tf_version() == 1002  # new entry points are found by their symbols, not by a version bump
    for name in ("get_colinear_y", "are_colinear", "mod_pow", "powers"):
        assert name in tf.__all__ and hasattr(tf.device, name), name
    assert hasattr(tf.device, "gather_elements")


def _calls(lib, bufs, null=None, widths=(1, 1), n=4, counts=None, k=3, gw=1):
    """One call of every entry point as (name, number of pointers, thunk): valid arguments (4 elements / groups) except for what is
    asked for.  null = index of the pointer argument to replace by NULL; counts = n_p2x / n_bases / n_exps."""
    x, y, q, o, f, e, idx, st = bufs
    wx, wy = widths
    cnt = 1 if counts is None else counts

    def ptrs(*ps):
        return [None if null is not None and i == null else _p(p) for i, p in enumerate(ps)]

    calls = []
    a, b, c, d, pq, out = ptrs(x, y, x, y, q, o)
    calls.append(("tf_get_colinear_y", 6, lambda: lib.tf_get_colinear_y(a, b, c, d, n, pq, cnt, wx, wy, out)))
    a2, b2, c2, d2, pq2, out2, st2 = ptrs(x, y, x, y, q, o, st)
    calls.append(("tf_get_colinear_y_dev", 7, lambda: lib.tf_get_colinear_y_dev(a2, b2, c2, d2, n, pq2, cnt, wx, wy, out2, None, st2)))
    xs, ys, fl = ptrs(x, y, f)
    calls.append(("tf_are_colinear", 3, lambda: lib.tf_are_colinear(xs, ys, n, k, wx, wy, fl)))
    calls.append(("tf_are_colinear_dev", 3, lambda: lib.tf_are_colinear_dev(xs, ys, n, k, wx, wy, fl, None)))
    bs, ex, out3 = ptrs(x, e, o)
    calls.append(("tf_mod_pow", 3, lambda: lib.tf_mod_pow(bs, cnt, ex, cnt, wy, out3, n)))
    calls.append(("tf_mod_pow_dev", 3, lambda: lib.tf_mod_pow_dev(bs, cnt, ex, cnt, wy, out3, n, None)))
    fi, ra, out4 = ptrs(q, q, o)
    calls.append(("tf_powers", 3, lambda: lib.tf_powers(fi, ra, wy, out4, n)))
    calls.append(("tf_powers_dev", 3, lambda: lib.tf_powers_dev(fi, ra, wy, out4, n, None)))
    src, ix, out5, st5 = ptrs(x, idx, o, st)
    calls.append(("tf_gather_elements_dev", 4, lambda: lib.tf_gather_elements_dev(src, 4 if n == 4 else n, gw, ix, n, out5, None, st5)))
    return calls


@pytest.fixture
def bufs():
    x = np.arange(1, 37, dtype=np.uint64)
    return (x, x.copy(), np.ones(12, dtype=np.uint64), np.zeros(64, dtype=np.uint64), np.full(4, 7, dtype=np.int32),
            np.full(4, 3, dtype=np.uint64), np.zeros(4, dtype=np.uint32), np.zeros(1, dtype=np.int32))


def test_argument_errors_in_the_documented_order_without_device(tf, bufs):
    lib = tf.lib()
    no_gpu = lib.tf_device_count() == 0
    out, flags, status = bufs[3], bufs[4], bufs[7]
    # 1. a NULL pointer, whichever it is -- also when a width is wrong, a count is wrong and a length too large
    for null in range(7):
        for kw in ({}, {"widths": (2, 2), "gw": 0}, {"counts": 2}, {"n": BIG}, {"widths": (3, 1), "gw": 17, "counts": 3, "n": BIG, "k": 2000}):
            for name, n_ptrs, call in _calls(lib, bufs, null=null, **kw):
                if null < n_ptrs:
                    assert call() == NULL, (name, null, kw)
    # 2. widths and counts -- also when a length is too large
    for big in ({}, {"n": BIG}, {"k": 1025}):
        for widths in ((0, 1), (2, 2), (3, 1), (1, 2), (4, 3), (-1, 1), (1, 0)):
            for name, _, call in _calls(lib, bufs, widths=widths, gw=17 if widths[1] else 0, **big):
                if name.startswith(("tf_mod_pow", "tf_powers")) and widths[1] in (1, 3):
                    continue  # one width: theirs is fine here
                assert call() == INVALID, (name, widths, big)
        for counts in (0, 2, 3, 5):
            for name, _, call in _calls(lib, bufs, counts=counts, **big):
                if name.startswith(("tf_get_colinear_y", "tf_mod_pow")):
                    assert call() == INVALID, (name, counts, big)
    x, e, o = _p(bufs[0]), _p(bufs[5]), _p(out)
    assert lib.tf_mod_pow(x, 4, e, 2, 1, o, 4) == INVALID and lib.tf_mod_pow(x, 3, e, 4, 1, o, 4) == INVALID
    assert lib.tf_mod_pow_dev(x, 1, e, 0, 3, o, 4, None) == INVALID
    assert lib.tf_gather_elements_dev(x, 4, -1, _p(bufs[6]), 4, o, None, _p(status)) == INVALID
    # 3. lengths: n, n_groups, n_groups * k and src_len above 2^30, k above 1024
    for name, _, call in _calls(lib, bufs, n=BIG, counts=BIG):
        assert call() == LEN_TOO_LARGE, name
    for name, _, call in _calls(lib, bufs, k=1025):
        if name.startswith("tf_are_colinear"):
            assert call() == LEN_TOO_LARGE, name
    fl = _p(flags)
    assert lib.tf_are_colinear(x, x, 1 << 21, 1024, 1, 1, fl) == LEN_TOO_LARGE  # n_groups * k = 2^31
    assert lib.tf_are_colinear_dev(x, x, (1 << 20) + 1, 1024, 1, 3, fl, None) == LEN_TOO_LARGE
    assert lib.tf_gather_elements_dev(x, BIG, 1, _p(bufs[6]), 4, o, None, _p(status)) == LEN_TOO_LARGE
    # 4. a valid call, every width pair / width: TF_ERR_NO_DEVICE without a GPU; with one, the host forms run
    for widths in ((1, 1), (3, 3), (1, 3)):
        for counts in (1, 4):
            for name, _, call in _calls(lib, bufs, widths=widths, counts=counts, gw=5):
                if no_gpu:
                    assert call() == NO_DEVICE, (name, widths)
                elif not name.endswith("_dev"):
                    assert call() in (OK, 12), (name, widths)  # (the buffers are not meant as points: x0 == x1)
    if no_gpu:
        assert not out.any() and (flags == 7).all() and not status.any()
    # groups of fewer than three points: the host form answers by the size alone, on any machine
    for k in (0, 1, 2):
        flags[:] = 7
        assert lib.tf_are_colinear(x, x, 4, k, 1, 3, fl) == OK and not flags.any()
    flags[:] = 7
    assert lib.tf_are_colinear(None, None, 4, 0, 1, 1, fl) == OK and not flags.any()  # no points, no arrays
    assert lib.tf_are_colinear(None, x, 4, 1, 1, 1, fl) == NULL


def test_empty_calls_return_ok_and_touch_nothing(tf, bufs):
    lib = tf.lib()
    out, flags, status = bufs[3], bufs[4], bufs[7]
    for w in ((1, 1), (3, 3), (1, 3), (2, 7)):  # (nothing is looked at when there is nothing to do)
        assert lib.tf_get_colinear_y(None, None, None, None, 0, None, 0, w[0], w[1], None) == OK
        assert lib.tf_get_colinear_y_dev(None, None, None, None, 0, None, 1, w[0], w[1], None, None, None) == OK
        assert lib.tf_are_colinear(None, None, 0, 3, w[0], w[1], None) == OK
        assert lib.tf_are_colinear_dev(None, None, 0, 2000, w[0], w[1], None, None) == OK
        assert lib.tf_mod_pow(None, 0, None, 0, w[1], None, 0) == OK and lib.tf_mod_pow_dev(None, 1, None, 1, w[1], None, 0, None) == OK
        assert lib.tf_powers(None, None, w[1], None, 0) == OK and lib.tf_powers_dev(None, None, w[1], None, 0, None) == OK
        assert lib.tf_gather_elements_dev(None, 0, w[1], None, 0, None, None, None) == OK
    # pointers that are given stay untouched
    x, o = _p(bufs[0]), _p(out)
    assert lib.tf_get_colinear_y_dev(x, x, x, x, 0, x, 1, 1, 1, o, None, _p(status)) == OK
    assert lib.tf_mod_pow(x, 1, x, 1, 1, o, 0) == OK and lib.tf_powers(x, x, 3, o, 0) == OK
    assert lib.tf_are_colinear(x, x, 0, 3, 1, 1, _p(flags)) == OK
    assert lib.tf_gather_elements_dev(x, 4, 1, _p(bufs[6]), 0, o, None, _p(status)) == OK
    assert not out.any() and (flags == 7).all() and not status.any()


def test_python_shapes_are_checked_on_the_host(tf):
    u = lambda *v: np.array(v, dtype=np.uint64)  # noqa: E731
    with pytest.raises(ValueError):
        tf.get_colinear_y(u(1), u(1), u(2), u(2), u(3), width_x=3, width_y=1)
    with pytest.raises(ValueError):
        tf.get_colinear_y(u(1, 2), u(1, 2), u(2, 3), u(2), u(3))
    with pytest.raises(ValueError):
        tf.get_colinear_y(u(1, 2, 3), u(1, 2, 3), u(2, 3, 4), u(2, 3, 4), u(3, 4))
    with pytest.raises(ValueError):
        tf.are_colinear(u(1, 2, 3, 4), u(1, 2, 3, 4), 3)
    with pytest.raises(ValueError):
        tf.are_colinear(u(1, 2, 3), u(1, 2, 3), 0)
    with pytest.raises(ValueError):
        tf.mod_pow(u(1, 2, 3), u(1, 2))
    with pytest.raises(ValueError):
        tf.mod_pow(u(1, 2), u(1), width=3)
    with pytest.raises(ValueError):
        tf.powers(u(1, 2), 3, 4)
    with pytest.raises(ValueError):
        tf.powers(1, 3, -1)
    # empty operands never reach a device
    z = u()
    assert tf.get_colinear_y(z, z, z, z, u(3)).size == 0 and tf.are_colinear(z, z, 3).size == 0
    assert tf.mod_pow(z, u(5)).size == 0 and tf.powers(1, 3, 0).size == 0
    # groups of fewer than three points are answered without one
    assert tf.are_colinear(u(1, 2, 3, 4), u(1, 2, 3, 4), 2).tolist() == [False, False]
