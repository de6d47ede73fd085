"""The DEEP quotients, the parts that need no GPU: the literal model of tests/deep_ref.py pinned to what the oracle pins (a quotient
by X - z of f - f(z) is a polynomial: low degree with true values, not with a falsified one; times X - z it gives f back); the rows
model against the codeword model; the regrouped model against the literal one; header, exports, plan and work-space rule; the
argument errors in their documented order; the Python wrapper's own checks, which come before any library call; and the absence of
any allocation site in the new unit."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import deep_ref as dr
from tests import pyref
from tests import table_ref
from twenty_first_amd import deep  # the feature under test: collection fails without it

P = pyref.P
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, NOT_POW2, LEN_TOO_LARGE, NULL, NO_DEVICE, INVERSE_OF_ZERO, INVALID = 0, 4, 5, 7, 8, 12, 17
NEW = ("tf_deep_quotient_dev", "tf_deep_quotient_workspace", "tf_deep_quotient_plan", "tf_deep_quotient_rows_dev")
F3 = pyref.Field(3)


def rand_words(rng, count):
    return (rng.integers(0, 1 << 63, count, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, count, dtype=np.uint64)) % np.uint64(P)


def _tables(oracle, rng, n, k1, k3, offset):
    """random polynomials of degree < n / 2 and their codewords on the coset: (main coefficients, aux coefficients, main, aux)"""
    half = n // 2
    fm = [rand_words(rng, half) for _ in range(k1)]
    fa = [rand_words(rng, 3 * half) for _ in range(k3)]
    main = np.concatenate([oracle.coset_evaluate(f, offset, n, width=1) for f in fm]) if k1 else np.zeros(0, np.uint64)
    aux = np.concatenate([oracle.coset_evaluate(f, offset, n, width=3) for f in fa]) if k3 else np.zeros(0, np.uint64)
    return fm, fa, main, aux


def _lifted(f):
    out = np.zeros(3 * f.size, dtype=np.uint64)
    out[0::3] = f
    return out


def _true_values(oracle, fm, fa, points):
    return np.concatenate([oracle.poly_eval_xfe_point(_lifted(f) if w == 1 else f, points[3 * p:3 * p + 3])
                           for p in range(points.size // 3) for fs, w in ((fm, 1), (fa, 3)) for f in fs])


# ------------------------------------------------------------------ the model, pinned to what the oracle pins
@pytest.mark.parametrize("n", [8, 64])
def test_quotient_of_true_values_has_low_degree_and_a_falsified_value_does_not(oracle, n):
    rng = np.random.default_rng(n)
    k1, k3, n_points = 2, 2, 2
    offset = oracle.bfe_new(7)
    fm, fa, main, aux = _tables(oracle, rng, n, k1, k3, offset)
    points, weights = rand_words(rng, 3 * n_points), rand_words(rng, 3 * n_points * (k1 + k3))
    values = _true_values(oracle, fm, fa, points)
    got, bad = dr.codeword(main, k1, n, aux, k3, 3 * n, n, offset, points, weights, values)
    assert not bad
    # (f_c - f_c(z)) / (X - z) has degree < n / 2 - 1, and so has every weighted sum of such quotients
    for interpolate in (lambda cw: oracle.coset_interpolate(cw, offset, width=3),
                        lambda cw: oracle.coset_interpolate_xfe_offset(cw, _lifted(np.array([offset], dtype=np.uint64)))):
        coeffs = interpolate(got).reshape(n, 3)
        assert not coeffs[n // 2 - 1:].any() and coeffs[:n // 2 - 1].any()
    wrong = values.copy()
    wrong[3 * 5] = (int(wrong[3 * 5]) + 1) % P          # one limb of one claimed value, one raw unit off
    got, bad = dr.codeword(main, k1, n, aux, k3, 3 * n, n, offset, points, weights, wrong)
    assert not bad and oracle.coset_interpolate(got, offset, width=3).reshape(n, 3)[n // 2 - 1:].any()


@pytest.mark.parametrize("n", [8, 64])
@pytest.mark.parametrize("width", [1, 3])
def test_one_column_one_point_unit_weight_gives_the_polynomial_back(oracle, n, width):
    rng = np.random.default_rng(10 * n + width)
    offset = oracle.bfe_new(7)
    fm, fa, main, aux = _tables(oracle, rng, n, 1 if width == 1 else 0, 1 if width == 3 else 0, offset)
    z = rand_words(rng, 3)
    one = dr.words([(1, 0, 0)])
    v = _true_values(oracle, fm, fa, z)
    got, bad = dr.codeword(main, len(fm), n, aux, len(fa), 3 * n, n, offset, z, one, v)
    assert not bad
    q = dr.xfes(oracle.coset_interpolate(got, offset, width=3))
    zv, vv = dr.xfes(z)[0], dr.xfes(v)[0]
    back = pyref.poly_mul(F3, q, [pyref.xfe_sub((0, 0, 0), zv), (1, 0, 0)])        # q * (X - z)
    back[0] = pyref.xfe_add(back[0], vv)
    f = dr.xfes(_lifted(fm[0]) if width == 1 else fa[0])
    assert back[:n // 2] == f and all(c == (0, 0, 0) for c in back[n // 2:])


# ------------------------------------------------------------------ the models against each other
@pytest.mark.parametrize("k1,k3", [(3, 2), (2, 0), (0, 1)])
def test_rows_model_on_gathered_rows_is_the_codeword_model_at_those_indices(k1, k3):
    rng = np.random.default_rng(100 * k1 + k3)
    n, n_points = 16, 3
    sm, sa, rsm, rsa = n + 3, 3 * n + 2, k1 + 1, 3 * k3 + 4
    main = dr.strided(rand_words(rng, k1 * n), k1, n, sm, 99)
    aux = dr.strided(rand_words(rng, 3 * k3 * n), k3, 3 * n, sa, 99)
    points, weights, values = rand_words(rng, 3 * n_points), rand_words(rng, 3 * n_points * (k1 + k3)), rand_words(rng, 3 * n_points * (k1 + k3))
    offset = pyref.to_raw(7)
    idx = np.array([0, n - 1, 5, 5, 9, 3], dtype=np.uint32)
    main_rows = table_ref.gather_rows(main, table_ref.COLUMN_MAJOR, n, k1, 1, sm, idx, np.full(idx.size * rsm, 77, np.uint64), rsm)[0] if k1 else np.zeros(0, np.uint64)
    aux_rows = table_ref.gather_rows(aux, table_ref.COLUMN_MAJOR, n, k3, 3, sa, idx, np.full(idx.size * rsa, 77, np.uint64), rsa)[0] if k3 else np.zeros(0, np.uint64)
    want, bad = dr.codeword(main, k1, sm, aux, k3, sa, n, offset, points, weights, values, at=idx)
    got, bad_zero, bad_index = dr.rows(main_rows, k1, rsm, aux_rows, k3, rsa, n, offset, idx, points, weights, values)
    assert not bad and not bad_zero and not bad_index and np.array_equal(got, want)
    # an index beyond the domain and a point on the domain, each flagged on its own row
    idx2 = idx.copy()
    idx2[2] = n
    on_domain = dr.words([pyref.xfe(dr.domain_point(n, offset, 9))])
    got, bad_zero, bad_index = dr.rows(main_rows, k1, rsm, aux_rows, k3, rsa, n, offset, idx2, np.concatenate([points[:3], on_domain]),
                                       weights[:6 * (k1 + k3)], values[:6 * (k1 + k3)])
    assert bad_zero == [4] and bad_index == [2]


def test_regrouped_model_is_the_literal_model():
    rng = np.random.default_rng(5)
    n, k1, k3, n_points = 8, 5, 3, 4
    sm, sa = n + 1, 3 * n + 5
    main = dr.strided(rand_words(rng, k1 * n), k1, n, sm, 99)
    aux = dr.strided(rand_words(rng, 3 * k3 * n), k3, 3 * n, sa, 99)
    points, weights, values = rand_words(rng, 3 * n_points), rand_words(rng, 3 * n_points * (k1 + k3)), rand_words(rng, 3 * n_points * (k1 + k3))
    want, bad = dr.codeword(main, k1, sm, aux, k3, sa, n, pyref.to_raw(3), points, weights, values)
    assert not bad and np.array_equal(dr.codeword_by_sums(main, k1, sm, aux, k3, sa, n, pyref.to_raw(3), points, weights, values), want)
    for a, b in ((k1, 0), (0, k3)):
        k = a + b
        want, _ = dr.codeword(main, a, sm, aux, b, sa, n, pyref.to_raw(3), points[:3], weights[:3 * k], values[:3 * k])
        assert np.array_equal(dr.codeword_by_sums(main, a, sm, aux, b, sa, n, pyref.to_raw(3), points[:3], weights[:3 * k], values[:3 * k]), want)


def test_model_layout_and_domain_on_a_case_small_enough_to_write_down():
    # one main column T = [10, 20], n = 2 (w_2 = -1), offset 3: x = [3, -3]; z = 5, v = 4, w = 2: out[i] = 2 (T[i] - 4) / (x_i - 5)
    main = dr.words([(10, 0, 0), (20, 0, 0)])[0::3]
    got, bad = dr.codeword(main, 1, 2, np.zeros(0, np.uint64), 0, 0, 2, pyref.to_raw(3), dr.words([(5, 0, 0)]), dr.words([(2, 0, 0)]), dr.words([(4, 0, 0)]))
    assert not bad and dr.xfes(got) == [(12 * pow(P - 2, P - 2, P) % P, 0, 0), (32 * pow(P - 8, P - 2, P) % P, 0, 0)]
    got, bad = dr.codeword(main, 1, 2, np.zeros(0, np.uint64), 0, 0, 2, pyref.to_raw(3), dr.words([(P - 3, 0, 0)]), dr.words([(2, 0, 0)]), dr.words([(4, 0, 0)]))
    assert bad == [1] and not got[3:].any()
    assert dr.padding(2, 3, 5).tolist() == [False] * 3 + [True] * 2 + [False] * 3 and dr.strided(np.arange(6), 2, 3, 5, 9).tolist() == [0, 1, 2, 9, 9, 3, 4, 5]


# ------------------------------------------------------------------ the ABI without a device
def _p(a):
    return C.c_void_p(a.ctypes.data)


def test_symbols_declared_and_exported(tf):
    from twenty_first_amd import _lib

    text = open(_lib.HEADER).read()
    exports = open(os.path.join(ROOT, "twenty-first_amd", "csrc", "tf_exports.map")).read()
    assert "global: tf_*;" in exports  # every tf_ symbol of the library is exported, and nothing else
    for name in NEW:
        assert name + "(" in text and name in _lib.SIGNATURES and hasattr(tf.lib(), name), name
        args = text.split(name + "(", 1)[1].split(");", 1)[0]
        assert len(args.split(",")) == len(_lib.SIGNATURES[name][1]), name
    assert "DEEP quotients" in text and tf.deep is deep
    assert _lib.SIGNATURES["tf_deep_quotient_workspace"][0] is C.c_size_t


def test_plan_and_workspace_are_consistent_and_monotone(tf):
    p = deep.plan(1, 1, 0, 1)
    C_, K = p.chunk, p.per_lane
    assert C_ == 64 * K and 1 <= p.points_per_pass <= deep.MAX_POINTS and p.grid_cap >= 1
    assert C_ * 3 * 4 <= 16384, "what a workgroup of four waves moves per column stays inside the guard words of tests/fence.py"
    assert (p.grid_cap + 1) * C_ <= 1 << 24, "the second grid-stride turn can be tested at n <= 2^24"
    last = 0
    for n_points in range(1, deep.MAX_POINTS + 1):
        passes = -(-n_points // p.points_per_pass)
        for n in (1, 2, 64, C_, 8 * C_, 1 << 20, 1 << 32):
            for k1, k3 in ((1, 0), (0, 1), (9, 5), (65535, 0), (0, 65535), (65000, 535)):
                q = deep.plan(n, k1, k3, n_points)
                assert q[:3] == p[:3] and q.grid_cap == p.grid_cap and q.passes == passes and q.launches == 1 + passes
                assert deep.workspace(n, k1, k3, n_points) == 24 * n_points
            q = deep.plan(n, 0, 0, n_points)
            assert (q.passes, q.launches) == (1, 1) and deep.workspace(n, 0, 0, n_points) == 0
        assert deep.workspace(8, 1, 1, n_points) >= last      # monotone in the points; constant in n, k1, k3 (above)
        last = deep.workspace(8, 1, 1, n_points)
        assert deep.plan(0, 3, 3, n_points).launches == 0 and deep.workspace(0, 3, 3, n_points) == 0
    # the capacity bounds what is written, not what is returned
    buf = (C.c_int * 6)(9, 9, 9, 9, 9, 9)
    assert tf.lib().tf_deep_quotient_plan(1024, 2, 2, 3, buf, 2) == 3 and list(buf) == [C_, K, 9, 9, 9, 9]
    assert tf.lib().tf_deep_quotient_plan(1024, 2, 2, 3, None, 0) == 3


def test_plan_and_workspace_of_rejected_calls(tf):
    lib = tf.lib()
    buf = (C.c_int * 6)()
    for args, code in (((8, 1, 1, 0), INVALID), ((8, 1, 1, 5), INVALID), ((12, 1, 1, 1), NOT_POW2), ((12, 1, 1, 9), INVALID),
                       ((1 << 33, 1, 1, 1), LEN_TOO_LARGE), ((8, 65535, 1, 1), LEN_TOO_LARGE), ((8, 0, 65536, 2), LEN_TOO_LARGE),
                       (((1 << 32) + 1, 70000, 0, 1), NOT_POW2), ((0, 1, 1, 7), INVALID)):
        assert lib.tf_deep_quotient_plan(*args, buf, 6) == -code, args
        assert lib.tf_deep_quotient_workspace(*args) == 0, args
    with pytest.raises(tf.TwentyFirstError) as e:
        deep.plan(8, 1, 1, 5)
    assert e.value.code == INVALID
    with pytest.raises(ValueError):
        deep.plan(-8, 1, 1, 1)
    with pytest.raises(ValueError):
        deep.workspace(8, 1, -1, 1)


def test_argument_errors_in_the_documented_order_without_device(tf):
    lib = tf.lib()
    no_gpu = lib.tf_device_count() == 0
    n, k1, k3, n_points = 8, 2, 2, 2
    main, aux = np.arange(64, dtype=np.uint64), np.arange(64, dtype=np.uint64)
    pts, wts, vals = (np.arange(64, dtype=np.uint64) for _ in range(3))
    out, work, status = np.full(64, 7, dtype=np.uint64), np.full(8, 5, dtype=np.uint64), np.zeros(1, dtype=np.int32)
    idx = np.zeros(4, dtype=np.uint32)
    ptrs = {"main": main, "aux": aux, "points": pts, "weights": wts, "values": vals, "out": out, "work": work, "status": status, "indices": idx}

    def both(code, null=(), forms=("codeword", "rows"), **kw):
        a = dict(n=n, k1=k1, k3=k3, n_points=n_points, offset=7, stride_main=None, stride_aux=None, work_bytes=48, n_rows=4)
        a.update(kw)
        p = {name: (None if name in null else _p(arr)) for name, arr in ptrs.items()}
        if "codeword" in forms:
            sm = a["n"] if a["stride_main"] is None else a["stride_main"]
            sa = 3 * a["n"] if a["stride_aux"] is None else a["stride_aux"]
            rc = lib.tf_deep_quotient_dev(p["main"], a["k1"], sm, p["aux"], a["k3"], sa, a["n"], a["offset"], p["points"], a["n_points"], p["weights"],
                                          p["values"], p["out"], p["work"], a["work_bytes"], None, p["status"])
            assert rc == code, ("codeword", code, rc, null, kw)
        if "rows" in forms:
            sm = a["k1"] if a["stride_main"] is None else a["stride_main"]
            sa = 3 * a["k3"] if a["stride_aux"] is None else a["stride_aux"]
            rc = lib.tf_deep_quotient_rows_dev(p["main"], a["k1"], sm, p["aux"], a["k3"], sa, a["n"], a["offset"], p["indices"], a["n_rows"], p["points"],
                                               a["n_points"], p["weights"], p["values"], p["out"], None, p["status"])
            assert rc == code, ("rows", code, rc, null, kw)

    everything = tuple(ptrs)
    # 0. the empty call: TF_OK whatever else is wrong, NULL pointers allowed
    both(OK, null=everything, n=0, n_points=9, offset=0, forms=("codeword",))
    both(OK, null=everything, n_rows=0, n=12, n_points=9, offset=0, forms=("rows",))
    # 1. a NULL pointer, whichever it is -- also when everything behind it is wrong too
    for name in ("main", "aux", "points", "weights", "values", "out", "status"):
        both(NULL, null=(name,))
        both(NULL, null=(name,), n_points=9, n=12, offset=0, stride_main=0, stride_aux=0, k1=70000, k3=70000)
    both(NULL, null=("indices",), forms=("rows",))
    both(NULL, null=("work",), forms=("codeword",))
    both(NULL, null=("main",), k3=0)
    both(NULL, null=("aux",), k1=0)
    # 2. n_points, strides, a short work space -- before the lengths are looked at
    for bad_points in (0, 5, 1 << 40):
        both(INVALID, n_points=bad_points)
        both(INVALID, n_points=bad_points, n=12, k1=70000, offset=0)
    both(INVALID, stride_main=n - 1, forms=("codeword",))
    both(INVALID, stride_aux=3 * n - 1, forms=("codeword",))
    both(INVALID, stride_main=k1 - 1, forms=("rows",))
    both(INVALID, stride_aux=3 * k3 - 1, forms=("rows",))
    both(INVALID, stride_main=0, n=12, offset=0)
    both(INVALID, work_bytes=47, forms=("codeword",))
    both(INVALID, work_bytes=0, forms=("codeword",))
    both(INVALID, work_bytes=47, null=("main",), k1=0, forms=("codeword",))
    # 3. the domain and the limits
    both(NOT_POW2, n=12, stride_main=12, stride_aux=36, offset=0)
    both(NOT_POW2, n=(1 << 33) + 1, stride_main=1 << 34, stride_aux=1 << 36, k1=40000, k3=40000)
    both(NOT_POW2, n=0, forms=("rows",))
    both(LEN_TOO_LARGE, n=1 << 33, stride_main=1 << 33, stride_aux=3 << 33, offset=0)
    both(LEN_TOO_LARGE, k1=65535, k3=1, stride_main=65535, stride_aux=3, offset=0, forms=("rows",))
    both(LEN_TOO_LARGE, k1=65535, k3=1, offset=0, forms=("codeword",))
    both(LEN_TOO_LARGE, k1=65536, k3=0, null=("aux",), offset=0, forms=("codeword",))
    both(LEN_TOO_LARGE, n_rows=(1 << 30) + 1, offset=0, forms=("rows",))
    both(LEN_TOO_LARGE, stride_main=1 << 41, stride_aux=1 << 41, offset=0)
    both(INVERSE_OF_ZERO, offset=0)
    both(INVERSE_OF_ZERO, offset=0, k1=0, k3=0, null=("main", "aux", "weights", "values", "work"), work_bytes=0)
    assert (out == 7).all() and (work == 5).all() and status[0] == 0
    # 4. valid calls: TF_ERR_NO_DEVICE on a machine without a GPU
    if no_gpu:
        both(NO_DEVICE)
        both(NO_DEVICE, k1=0, null=("main",), stride_main=0)
        both(NO_DEVICE, k3=0, null=("aux",), stride_aux=0)
        both(NO_DEVICE, k1=0, k3=0, null=("main", "aux", "weights", "values", "work"), work_bytes=0)
        both(NO_DEVICE, n=1 << 32, stride_main=1 << 32, stride_aux=3 << 32, forms=("codeword",))
        both(NO_DEVICE, n=1 << 32, forms=("rows",))
        both(NO_DEVICE, n=1, n_points=4, work_bytes=96, k1=65000, k3=535, forms=("codeword",))
        assert (out == 7).all() and (work == 5).all() and status[0] == 0


# ------------------------------------------------------------------ the wrapper's own checks come before any library call
class _NoLaunch:
    """the library with the two launches replaced by a tripwire; the host arithmetic stays"""

    def __init__(self, lib):
        self.tf_deep_quotient_workspace, self.tf_deep_quotient_plan = lib.tf_deep_quotient_workspace, lib.tf_deep_quotient_plan
        self.calls = []

    def _trip(self, *args):
        self.calls.append(args)
        return 0

    tf_deep_quotient_dev = tf_deep_quotient_rows_dev = _trip


@pytest.fixture()
def cpu_tensors_pass(tf, monkeypatch):
    """deep.py with the CUDA requirement of its tensors lifted and the launches counted, so that the checks that follow it run here"""
    import torch

    stub = _NoLaunch(tf.lib())
    monkeypatch.setattr(deep, "_t", lambda t, name="tensor": t)
    monkeypatch.setattr(deep, "_status", lambda s: None)
    monkeypatch.setattr(deep, "_indices", lambda t: deep._need(t.dtype == torch.int32, "indices must hold 32-bit words") or t)
    monkeypatch.setattr(deep, "_stream", lambda s: None)
    monkeypatch.setattr(deep._lib, "lib", lambda: stub)
    return stub


def test_python_checks_raise_before_any_library_call(tf, cpu_tensors_pass):
    import torch

    stub = cpu_tensors_pass
    z = lambda k: torch.zeros(k, dtype=torch.int64)  # noqa: E731
    n, k1, k3 = 8, 2, 1
    main, aux, pts, wts, vals, out, work = z(2 * n), z(3 * n), z(6), z(18), z(18), z(3 * n), z(6)
    status = torch.zeros(1, dtype=torch.int32)
    deep.quotient(main, aux, n, k1, k3, 7, pts, wts, vals, out, status, work)
    deep.quotient(main, None, n, k1, 0, 7, pts, wts[:12], vals[:12], out, status, work)
    deep.quotient(None, None, n, 0, 0, 7, pts, None, None, out, status)                       # no column: no weights, no work space
    deep.quotient(z(2 * n + 3), aux, n, k1, k3, 7, pts, wts, vals, out, status, work, stride_main=n + 3)
    assert len(stub.calls) == 4 and stub.calls[-1][2] == n + 3
    big = z(64)
    bad = [
        lambda: deep.quotient(main[:-1], aux, n, k1, k3, 7, pts, wts, vals, out, status, work),           # a short table
        lambda: deep.quotient(main, aux, n, k1, k3, 7, pts, wts, vals, out, status, work, stride_main=n - 1),
        lambda: deep.quotient(main, aux, n, k1, k3, 7, pts, wts, vals, out, status, work, stride_main=n + 1),   # main too short at that stride
        lambda: deep.quotient(None, aux, n, k1, k3, 7, pts, wts, vals, out, status, work),                # a missing table
        lambda: deep.quotient(main, aux, n, k1, k3, 7, z(15), wts, vals, out, status, work),              # five points
        lambda: deep.quotient(main, aux, n, k1, k3, 7, z(0), wts, vals, out, status, work),
        lambda: deep.quotient(main, aux, n, k1, k3, 7, z(4), wts, vals, out, status, work),
        lambda: deep.quotient(main, aux, n, k1, k3, 7, pts, wts[:-3], vals, out, status, work),
        lambda: deep.quotient(main, aux, n, k1, k3, 7, pts, wts, z(21), out, status, work),
        lambda: deep.quotient(main, aux, n, k1, k3, 7, pts, wts, vals, out[:-3], status, work),
        lambda: deep.quotient(main, aux, n, k1, k3, 7, pts, wts, vals, out, status),                      # no work space
        lambda: deep.quotient(main, aux, n, k1, k3, 7, pts, wts, vals, out, status, work[:-1]),           # one word short
        lambda: deep.quotient(big[:16], aux, n, k1, k3, 7, pts, wts, vals, big[8:32], status, work),      # out on an input
        lambda: deep.quotient(main, aux, n, k1, k3, 7, pts, wts, vals, big[:24], status, big[20:26]),     # the work space on out
        lambda: deep.quotient(main, aux, n, k1, k3, 7, big[:6], wts, vals, out, status, big[3:9]),        # the work space on the points
        lambda: deep.quotient(main, aux, -8, k1, k3, 7, pts, wts, vals, out, status, work),
        lambda: deep.quotient(main, aux, n, 65535, 1, 7, pts, wts, vals, out, status, work),
    ]
    for k, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f"bad call {k} was accepted")
        assert len(stub.calls) == 4, k
    # the rows form
    idx = torch.zeros(5, dtype=torch.int32)
    rows_m, rows_a, out_r = z(5 * k1), z(5 * 3 * k3), z(15)
    deep.quotient_rows(rows_m, rows_a, n, k1, k3, 7, idx, pts, wts, vals, out_r, status)
    deep.quotient_rows(z(4 * 7 + k1), rows_a, n, k1, k3, 7, idx, pts, wts, vals, out_r, status, row_stride_main=7)
    assert len(stub.calls) == 6 and stub.calls[-1][2] == 7 and stub.calls[-1][9] == 5
    bad = [
        lambda: deep.quotient_rows(rows_m[:-1], rows_a, n, k1, k3, 7, idx, pts, wts, vals, out_r, status),
        lambda: deep.quotient_rows(rows_m, rows_a, n, k1, k3, 7, idx, pts, wts, vals, out_r, status, row_stride_aux=3 * k3 - 1),
        lambda: deep.quotient_rows(rows_m, rows_a, n, k1, k3, 7, idx.to(torch.int64), pts, wts, vals, out_r, status),
        lambda: deep.quotient_rows(rows_m, rows_a, n, k1, k3, 7, idx, pts, wts, vals, z(12), status),
        lambda: deep.quotient_rows(big[:10], rows_a, n, k1, k3, 7, idx, pts, wts, vals, big[5:20], status),
    ]
    for k, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
        assert len(stub.calls) == 6, k


def test_tensors_must_be_cuda_words(tf):
    import torch

    x = torch.zeros(24, dtype=torch.int64)
    with pytest.raises(TypeError):
        deep.quotient(x[:8], None, 8, 1, 0, 7, x[:3], x[:3], x[:3], x, torch.zeros(1, dtype=torch.int32), x[:3])
    with pytest.raises(TypeError):
        deep.quotient(np.zeros(8, np.uint64), None, 8, 1, 0, 7, x[:3], x[:3], x[:3], x, torch.zeros(1, dtype=torch.int32), x[:3])


# ------------------------------------------------------------------ the unit takes no memory of its own
def test_the_new_unit_has_no_allocation_site():
    from tests import test_temp_guard_cpu as tg

    csrc = os.path.join(ROOT, "twenty-first_amd", "csrc")
    for name in ("tf_deep.hip", "deep_kernels.h", "acc_cols.h"):
        text = open(os.path.join(csrc, name)).read()
        for pattern in tg.SITES + tg.FORWARDERS + ("DevTemp", "StagedUpload", "hipMalloc", "hipHostMalloc", "tf_temp.h"):
            assert pattern not in text, (name, pattern)
    assert not [s for s in tg.sites() if s[0] in ("tf_deep.hip", "deep_kernels.h", "acc_cols.h")]
