"""What tests/test_gpu_slab_edges.py rests on, as far as a machine without a GPU can check it:

  * the constants mirrored in tests/slab_ref.py stand at their sites in csrc/ (a changed slab size, limit or loop then fails here
    instead of silently taking a boundary out of the reach of the GPU shapes), and the GPU file's shapes cross what they claim;
  * oracle.combine_rows and the rank-2 family builders of tests/slab_ref.py against Python integers, the oracle's element-wise
    products and tests/pyref on tiny shapes: every row of a family goes through pyref on its own and must give the combined result;
  * the router's answers for the largest batches (tf_batch_eval_plan is host logic) and the error side of the batch limits that is
    reached before a device is asked for.  (barycentric_evaluate's limit is checked behind current_ctx: its error side runs on the
    GPU only; the 65 536 dividends of tf_poly_divide_* are in tests/test_poly_divide_cpu.py through the host form, here through the
    device form.)"""
import ctypes as C
import os
import random

import numpy as np
import pytest

from tests import pyref
from tests import slab_ref as S
from tests import test_gpu_slab_edges as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "twenty-first_amd", "csrc")
LEN_TOO_LARGE = 5
EDGE_VALUES = [0, 1, 2, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, S.P - 1, S.P - 2, S.P - (1 << 32), (1 << 63), S.P >> 1, 0xFFFFFFFF00000000]


def _p(a):
    return C.c_void_p(a.ctypes.data)


# ------------------------------------------------------------------ the constants at their sites, the shapes across them
@pytest.mark.parametrize("k", range(len(S.SITES)))
def test_mirrored_constant_stands_at_its_site(k):
    name, text, count = S.SITES[k]
    source = open(os.path.join(CSRC, name)).read()
    assert source.count(text) == count, f"{name}: `{text}` stands {source.count(text)} times, not {count}: tests/slab_ref.py mirrors a constant of this site"


def test_no_other_batch_slab_in_the_three_sources():
    """the three sources of the issue hold no further `+= 65535` walk than the mirrored ones"""
    for name, want in (("tf_poly.hip", 2), ("tf_divide.hip", 0), ("tf_algebra.hip", 0)):
        assert open(os.path.join(CSRC, name)).read().count(f"+= {S.GRID_Y}") == want, name


def test_header_states_the_barycentric_limit_the_code_enforces():
    header = open(os.path.join(ROOT, "include", "tf_hip.h")).read()
    assert S.BARY_MAX_BATCH == 131069
    assert "at most 131 069 codewords per call" in header and "65 534 x 8" not in header


def test_gpu_shapes_cross_what_they_claim():
    for name in G.A_CASES:
        G.a_arithmetic(name)
    for name, (_, _, widths) in G.C_CASES.items():
        for w in widths:
            G.c_arithmetic(name, w)
    for n, batch in G.B_LANE + G.B_SPLIT + G.B_ONE_SHOT:
        G._b_arithmetic(n, batch)
        assert n & (n - 1) == 0 or (n, batch) in G.B_LANE
    for batch in G.D_BATCHES:
        G._d_arithmetic(batch)
    assert G.E_BARY_BATCHES == (131068, 131069)
    # memory: the largest work space of A (A3 over XFieldElement) stays below 10 GiB, that of C below 3 GiB
    _, units, slab = G.a_arithmetic("A3")
    assert (2 * units + S.TREE_WORK_ARRAYS * slab) * G.M_EVAL * 3 * 8 < 10 << 30
    for name, (_, rows, widths) in G.C_CASES.items():
        for w in widths:
            m, slab = G.c_arithmetic(name, w)
            assert S.INTERP_ROW_ARRAYS * slab * m * w * 8 < 3 << 30


# ------------------------------------------------------------------ the arithmetic of the builders
def _raw(values):
    return np.array([pyref.to_raw(v) for v in values], dtype=np.uint64)


def _vals(raw):
    return [pyref.to_val(int(r)) for r in np.asarray(raw, dtype=np.uint64).reshape(-1)]


def test_combine_rows_against_integers_and_the_oracles_products(oracle):
    rng = random.Random(0x51AB)
    x = np.array([v % S.P for v in EDGE_VALUES + [rng.randrange(S.P) for _ in range(28)]], dtype=np.uint64)   # canonical raw words
    f0, f1 = x, x[::-1].copy()
    a, b = np.repeat(x, x.size), np.tile(x, x.size)                         # every pair of scalars, the edges among them
    got = oracle.combine_rows(f0, f1, a, b)
    assert got.shape == (a.size, x.size)
    r_inv = pow(1 << 64, S.P - 2, S.P)
    for r in range(0, a.size, 7):
        assert got[r].tolist() == [(int(a[r]) * int(p) + int(b[r]) * int(q)) * r_inv % S.P for p, q in zip(f0.tolist(), f1.tolist())]
    # the oracle's element-wise product, one term at a time (b = 0 leaves the first term alone)
    zero = np.zeros_like(a)
    assert np.array_equal(oracle.combine_rows(f0, f1, a, zero)[:, 3], oracle.hadamard(a, np.full_like(a, f0[3])))
    assert np.array_equal(oracle.combine_rows(f0, f1, zero, b)[:, 5], oracle.hadamard(b, np.full_like(b, f1[5])))
    # a span of rows, into a caller's array
    out = np.zeros((10, x.size), dtype=np.uint64)
    assert oracle.combine_rows(f0, f1, a, b, 100, 110, out) is out and np.array_equal(out, got[100:110])


def test_scalars_are_non_zero_and_fixed(oracle):
    a, b = S.scalars(oracle, 1000, 5)
    a2, b2 = S.scalars(oracle, 1000, 5)
    assert a.all() and b.all() and np.array_equal(a, a2) and np.array_equal(b, b2) and not np.array_equal(a, b)
    assert (a < np.uint64(S.P)).all()


def test_family_rows_are_the_combination_and_all_distinct(oracle):
    f0, f1 = oracle.fill_random(7, 1), oracle.fill_random(7, 2)
    a, b = S.scalars(oracle, 300, 3)
    rows = S.family(oracle, f0, f1, a, b)
    v0, v1 = _vals(f0), _vals(f1)
    for r in (0, 1, 150, 299):
        ar, br = pyref.to_val(int(a[r])), pyref.to_val(int(b[r]))
        assert _vals(rows[r]) == [(ar * p + br * q) % S.P for p, q in zip(v0, v1)]
    assert len({tuple(r) for r in rows.tolist()}) == 300
    # more rows than one block and than one thread's share: the same words as one row at a time
    a, b = S.scalars(oracle, 70000, 4)
    big = S.family(oracle, f0, f1, a, b)
    for r in (0, 9361, 9362, 37449, 69999):
        assert np.array_equal(big[r], S.family(oracle, f0, f1, a[r:r + 1], b[r:r + 1])[0])


def test_family_mismatch_names_the_first_wrong_word(oracle):
    e0, e1 = oracle.fill_random(6, 11), oracle.fill_random(6, 12)
    a, b = S.scalars(oracle, 40000, 13)
    good = S.family(oracle, e0, e1, a, b)
    assert S.family_mismatch(oracle, good, e0, e1, a, b) is None and S.family_mismatch(oracle, good.reshape(-1), e0, e1, a, b) is None
    bad = good.copy()
    bad[39999, 5] ^= np.uint64(1)
    bad[20000, 2] = good[20001, 2]                                          # a word of the neighbouring row
    assert S.family_mismatch(oracle, bad, e0, e1, a, b) == (20000, 2, int(good[20001, 2]), int(good[20000, 2]))
    swapped = good.copy()
    swapped[[7, 8]] = swapped[[8, 7]]
    assert S.family_mismatch(oracle, swapped, e0, e1, a, b)[:2] == (7, 0)


def _field(width):
    return pyref.Field(width)


def _elems(raw, width):
    return _field(width).group(_vals(raw))


def _words(elems, width):
    return _raw(_field(width).flat(elems))


@pytest.mark.parametrize("width,point_width", [(1, 1), (3, 3), (1, 3)])
def test_evaluation_family_row_by_row_through_pyref(oracle, width, point_width):
    n_coeffs, n_points, rows = 5, 4, 6
    f0, f1 = oracle.fill_random(n_coeffs * width, 21), oracle.fill_random(n_coeffs * width, 22)
    pts = oracle.fill_random(n_points * point_width, 23)
    a, b = S.scalars(oracle, rows, 24)
    fam = S.family(oracle, f0, f1, a, b)
    want = S.family(oracle, S.horner(oracle, f0, pts, width, point_width), S.horner(oracle, f1, pts, width, point_width), a, b)
    F = _field(point_width)
    for r in range(rows):
        coeffs = [c if width == point_width else F.lift(c) for c in _elems(fam[r], width)]
        got = [pyref.poly_eval(F, coeffs, x) for x in _elems(pts, point_width)]
        assert np.array_equal(_words(got, point_width), want[r])


@pytest.mark.parametrize("width", (1, 3))
def test_one_shot_family_is_the_interpolants_family(oracle, width):
    """coset_extrapolate's rows are codewords: the family of the codewords has the family of the interpolants' values"""
    n, rows = 4, 5
    off = oracle.bfe_new(G.OFFSET)
    c0, c1 = oracle.fill_random(n * width, 31), oracle.fill_random(n * width, 32)
    pts = oracle.fill_random(3 * width, 33)
    a, b = S.scalars(oracle, rows, 34)
    fam = S.family(oracle, c0, c1, a, b)
    want = S.family(oracle, *(S.horner(oracle, oracle.coset_interpolate(c, off, width=width), pts, width) for c in (c0, c1)), a, b)
    F = _field(width)
    dom = [F.mul(F.lift(G.OFFSET), F.lift(pow(pyref.root_of_unity(n), i, S.P))) for i in range(n)]
    for r in range(rows):
        coeffs = pyref.lagrange_interpolate(F, dom, _elems(fam[r], width))
        got = [pyref.poly_eval(F, coeffs, x) for x in _elems(pts, width)]
        assert np.array_equal(_words(got, width), want[r])


@pytest.mark.parametrize("width", (1, 3))
def test_interpolation_family_row_by_row_through_pyref(oracle, width):
    n, rows = 5, 4
    dom = oracle.fill_random(n * width, 41)
    v0, v1 = oracle.fill_random(n * width, 42), oracle.fill_random(n * width, 43)
    a, b = S.scalars(oracle, rows, 44)
    fam = S.family(oracle, v0, v1, a, b)
    want = S.family(oracle, oracle.lagrange_interpolate(dom, v0, width=width), oracle.lagrange_interpolate(dom, v1, width=width), a, b)
    F = _field(width)
    for r in range(rows):
        got = pyref.lagrange_interpolate(F, _elems(dom, width), _elems(fam[r], width))
        assert np.array_equal(_words(got, width), want[r])


@pytest.mark.parametrize("width", (1, 3))
def test_division_family_row_by_row(oracle, width):
    """quotient and remainder of every row: pyref's long division over BFieldElement; over XFieldElement the defining identity
    a = q b + r with pyref's products"""
    na, nb, rows = G.E_DIVIDEND, G.E_DIVISOR, 5
    d0, d1 = oracle.fill_random(na * width, 51), oracle.fill_random(na * width, 52)
    div = oracle.fill_random(nb * width, 53)
    a, b = S.scalars(oracle, rows, 54)
    fam = S.family(oracle, d0, d1, a, b)
    (q0, r0), (q1, r1) = (S.long_divide(oracle, d, div, width) for d in (d0, d1))
    assert q0.size == (na - nb + 1) * width and r0.size == (nb - 1) * width
    wq, wr = S.family(oracle, q0, q1, a, b), S.family(oracle, r0, r1, a, b)
    F = _field(width)
    for r in range(rows):
        if width == 1:
            q, rem = pyref.long_divide(_vals(fam[r]), _vals(div))
            assert np.array_equal(_raw(q), wq[r]) and np.array_equal(_raw(rem), wr[r])
        else:
            back = pyref.poly_mul(F, _elems(wq[r], 3), _elems(div, 3))
            for j, e in enumerate(_elems(wr[r], 3)):
                back[j] = F.add(back[j], e)
            assert np.array_equal(_words(back, 3), fam[r])


@pytest.mark.parametrize("width", (1, 3))
def test_barycentric_family_row_by_row_through_pyref(oracle, width):
    n, rows = G.E_BARY_N, 4
    c0, c1 = oracle.fill_random(n * width, 61), oracle.fill_random(n * width, 62)
    x = oracle.fill_random(3, 63)
    a, b = S.scalars(oracle, rows, 64)
    fam = S.family(oracle, c0, c1, a, b)
    want = S.family(oracle, oracle.barycentric_evaluate(c0, x, width=width), oracle.barycentric_evaluate(c1, x, width=width), a, b)
    F = _field(width)
    for r in range(rows):
        got = pyref.barycentric_evaluate(F, _elems(fam[r], width), tuple(_vals(x)))
        assert np.array_equal(_raw(got), want[r])


# ------------------------------------------------------------------ host logic of the library
@pytest.mark.parametrize("width", (1, 3))
def test_router_at_the_unit_limit(tf, width):
    """A3: 65 536 polynomials of two coefficients are 65 536 units, the most the walk indexes: the forced tree route holds.  A4: one
    more, and the router answers Horner even with the tree forced."""
    lib = tf.lib()
    lib.tf_set_batch_eval_route(2)
    try:
        assert lib.tf_batch_eval_plan(2, G.N_POINTS, S.TREE_MAX_UNITS, width) == 2
        assert lib.tf_batch_eval_plan(2, G.N_POINTS, S.TREE_MAX_UNITS + 1, width) == 1
        for name, (n_coeffs, batch, _) in G.A_CASES.items():
            assert lib.tf_batch_eval_plan(n_coeffs, G.N_POINTS, batch, width) == (1 if name == "A4" else 2), name
        # two chunks per polynomial halve the batch the tree takes
        assert lib.tf_batch_eval_plan(G.M_EVAL + 1, G.N_POINTS, S.TREE_MAX_UNITS // 2, width) == 2
        assert lib.tf_batch_eval_plan(G.M_EVAL + 1, G.N_POINTS, S.TREE_MAX_UNITS // 2 + 1, width) == 1
        lib.tf_set_batch_eval_route(1)
        assert lib.tf_batch_eval_plan(2, G.N_POINTS, 4, width) == 1
    finally:
        lib.tf_set_batch_eval_route(0)


def test_one_dividend_more_is_refused_before_any_device_is_asked_for(tf):
    lib = tf.lib()
    a, b, q, r = (np.ones(64, dtype=np.uint64) for _ in range(4))
    st = np.zeros(1, dtype=np.int32)
    # (the device form: the host form uploads its operands first, which needs a device)
    many = lib.tf_poly_clean_divide_many_bfe_dev
    assert many(_p(a), G.E_DIVIDEND, S.CLEAN_DIVIDE_MAX_BATCH + 1, _p(b), G.E_DIVISOR, _p(q), None) == LEN_TOO_LARGE
    for suffix in ("bfe", "xfe"):
        fn = getattr(lib, f"tf_poly_divide_{suffix}_dev")
        assert fn(_p(a), G.E_DIVIDEND, S.DIVIDE_MAX_BATCH + 1, _p(b), G.E_DIVISOR, _p(q), _p(r), None, _p(st)) == LEN_TOO_LARGE
