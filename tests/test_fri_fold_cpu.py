"""The FRI fold, the parts that need no GPU: the expected-value model the GPU tests compare against (tests/fri_ref.py) pinned to the
reference's get_colinear_y (tests/points_ref.py), to polynomials (tests/pyref.py) and to the oracle; the facts about roots of unity
the kernel rests on; the argument errors every flavour returns before any HIP call, and their order; the plan of passes and the
work-space rule."""
import ctypes as C

import numpy as np
import pytest

from tests import fri_ref
from tests import points_ref as pr
from tests import pyref

P = pyref.P
PAIRS = pr.PAIRS  # (width_c, width_a)
OK, NOT_POW2, LEN_TOO_LARGE, NULL, NO_DEVICE, INVERSE_OF_ZERO, INVALID = 0, 4, 5, 7, 8, 12, 17
NEW = ("tf_fri_fold", "tf_fri_fold_dev", "tf_fri_fold_workspace", "tf_fri_fold_plan")


def _rand_elems(rng, count, w):
    v = [int(x) % P for x in rng.integers(0, 1 << 63, count * w, dtype=np.uint64) * 2 + rng.integers(0, 2, count * w, dtype=np.uint64)]
    return v if w == 1 else [tuple(v[3 * i:3 * i + 3]) for i in range(count)]


def _offsets(rng):
    return [1, 7, P - 1, _rand_elems(rng, 1, 1)[0] or 1]


# ------------------------------------------------------------------ the facts the kernel rests on
def test_roots_of_unity_are_powers_of_two_and_square_down():
    for l in range(1, 7):
        assert pyref.root_of_unity(1 << l) == pow(2, 39 * (1 << (6 - l)), P)
    assert 2 * pow(2, 191, P) % P == 1 and pow(2, 192, P) == 1
    for k in range(1, 31):
        assert pow(pyref.root_of_unity(1 << k), 2, P) == pyref.root_of_unity(1 << (k - 1))


# ------------------------------------------------------------------ the model, pinned to the reference's function
@pytest.mark.parametrize("wc,wa", PAIRS)
@pytest.mark.parametrize("n", [2, 4, 8, 64])
def test_model_equals_get_colinear_y_element_by_element(wc, wa, n):
    rng = np.random.default_rng(1000 * n + 10 * wc + wa)
    for g in _offsets(rng):
        c, alpha = _rand_elems(rng, n, wc), _rand_elems(rng, 1, wa)[0]
        xs = fri_ref.domain(g, n)
        got = fri_ref.fold_level(c, n, wc, g, alpha, wa)
        assert len(got) == n // 2
        for i in range(n // 2):
            assert xs[i + n // 2] == (P - xs[i]) % P
            want = pr.colinear_y_elem((xs[i], pr.lift(c[i], wc, wa)), (xs[i + n // 2], pr.lift(c[i + n // 2], wc, wa)), alpha, 1, wa)
            assert want is not None and got[i] == want, (g, i)


# ------------------------------------------------------------------ the model, pinned to polynomials
def _even_plus_alpha_odd(F, p, alpha):
    return [F.add(p[2 * i], F.mul(alpha, p[2 * i + 1])) for i in range(len(p) // 2)]


@pytest.mark.parametrize("w", [1, 3])
@pytest.mark.parametrize("n", [2, 8, 32])
def test_model_folds_a_polynomial_into_even_plus_alpha_odd(w, n):
    rng = np.random.default_rng(77 * n + w)
    F = pyref.Field(w)
    for g in _offsets(rng):
        p, alpha = _rand_elems(rng, n, w), _rand_elems(rng, 1, w)[0]
        c = pyref.coset_evaluate(F, p, F.lift(g), n)
        want = pyref.coset_evaluate(F, _even_plus_alpha_odd(F, p, alpha), F.lift(g * g % P), n // 2)
        assert fri_ref.fold_level(c, n, w, g, alpha, w) == want


def test_model_folds_the_oracles_coset_evaluation(oracle):
    n, g = 1 << 10, 7
    rng = np.random.default_rng(2025)
    F = pyref.Field(3)
    p, alpha = _rand_elems(rng, n, 3), _rand_elems(rng, 1, 3)[0]
    c = oracle.coset_evaluate(pr.words(p, 3), pyref.to_raw(g), n, width=3)
    want = oracle.coset_evaluate(pr.words(_even_plus_alpha_odd(F, p, alpha), 3), pyref.to_raw(g * g % P), n // 2, width=3)
    got = fri_ref.fold(c, n, 1, 3, pyref.to_raw(g), pr.words([alpha], 3), 1, 1, 3)
    assert np.array_equal(got, want)


# ------------------------------------------------------------------ levels, sets and special challenges
@pytest.mark.parametrize("wc,wa", PAIRS)
def test_model_levels_are_chained_single_folds(wc, wa):
    n, batch = 64, 2
    rng = np.random.default_rng(64 + wc + wa)
    g = _rand_elems(rng, 1, 1)[0] or 1
    cw = pr.words(_rand_elems(rng, batch * n, wc), wc)
    for r in range(1, 7):
        sets = _rand_elems(rng, batch * r, wa)
        got = fri_ref.fold(cw, n, batch, wc, pyref.to_raw(g), pr.words(sets, wa), r, batch, wa)
        cur, w, m, off = cw, wc, n, g
        for j in range(r):
            level = pr.words([sets[b * r + j] for b in range(batch)], wa)
            cur = fri_ref.fold(cur, m, batch, w, pyref.to_raw(off), level, 1, batch, wa)
            w, m, off = wa, m // 2, off * off % P
        assert got.size == batch * (n >> r) * wa and np.array_equal(got, cur), r
        # one set for every codeword: codeword 0 is unchanged, codeword 1 follows set 0
        one = fri_ref.fold(cw, n, batch, wc, pyref.to_raw(g), pr.words(sets[:r], wa), r, 1, wa)
        half = one.size // 2
        assert np.array_equal(one[:half], got[:half])
        assert np.array_equal(one[half:], fri_ref.fold(cw[n * wc:], n, 1, wc, pyref.to_raw(g), pr.words(sets[:r], wa), r, 1, wa))


@pytest.mark.parametrize("wc,wa", PAIRS)
def test_model_challenge_on_a_domain_point_returns_that_value(wc, wa):
    n, g = 16, 7
    rng = np.random.default_rng(16 + wc)
    c = _rand_elems(rng, n, wc)
    xs = fri_ref.domain(g, n)
    for j in (0, 3, n // 2 - 1):
        assert fri_ref.fold_level(c, n, wc, g, pr.lift(xs[j], 1, wa), wa)[j] == pr.lift(c[j], wc, wa)
        assert fri_ref.fold_level(c, n, wc, g, pr.lift((P - xs[j]) % P, 1, wa), wa)[j] == pr.lift(c[j + n // 2], wc, wa)


# ------------------------------------------------------------------ the ABI without a device
def _p(a):
    return C.c_void_p(a.ctypes.data)


def test_symbols_declared_and_exported(tf):
    from twenty_first_amd import _lib

    text = open(_lib.HEADER).read()
    for name in NEW:
        assert name + "(" in text and name in _lib.SIGNATURES and hasattr(tf.lib(), name), name
    assert tf.fri_fold is tf.fri.fold_host


@pytest.fixture()
def bufs():
    cw = pr.words(_rand_elems(np.random.default_rng(5), 3 * 8, 3), 3)  # three codewords of n = 8 at the most, any width
    ch = pr.words(_rand_elems(np.random.default_rng(6), 3 * 3, 3), 3)  # three sets of three levels at the most
    return cw, ch, np.full(3 * 4 * 3, 7, dtype=np.uint64)


def _forms(lib, cw, ch, out, n=8, batch=3, wc=3, g=pyref.to_raw(7), levels=1, n_sets=1, wa=3, null=None):
    ptr = [None if null == i else _p(a) for i, a in enumerate((cw, ch, out))]
    yield "tf_fri_fold", lambda: lib.tf_fri_fold(ptr[0], n, batch, wc, g, ptr[1], levels, n_sets, wa, ptr[2])
    yield "tf_fri_fold_dev", lambda: lib.tf_fri_fold_dev(ptr[0], n, batch, wc, g, ptr[1], levels, n_sets, wa, ptr[2], None)


def test_argument_errors_in_the_documented_order_without_device(tf, bufs):
    lib = tf.lib()
    cw, ch, out = bufs
    no_gpu = lib.tf_device_count() == 0

    def expect(code, **kw):
        for name, call in _forms(lib, cw, ch, out, **kw):
            assert call() == code, (name, code, kw)

    # 1. a NULL pointer, whichever it is -- also when everything behind it is wrong too
    for null in range(3):
        expect(NULL, null=null)
        expect(NULL, null=null, wc=3, wa=1, levels=0, n=6, g=0)
    # 2. a width pair not listed, no level, a number of sets that is neither 1 nor batch -- before the length is looked at
    for wc, wa in ((3, 1), (2, 2), (0, 1), (1, 2)):
        expect(INVALID, wc=wc, wa=wa, n=6, g=0)
    expect(INVALID, levels=0, n=6, g=0)
    expect(INVALID, n_sets=2, n=6, g=0)
    expect(INVALID, n_sets=0, n=0, g=0)
    # 3. a length that is no power of two, 0 included -- before the levels are compared with it
    for n in (0, 3, 6, (1 << 31) - 1):
        expect(NOT_POW2, n=n, levels=40, g=0)
    # 4. more levels than the length has -- before the length is found too large
    expect(INVALID, n=8, levels=4, g=0)
    expect(INVALID, n=1, levels=1, g=0)
    expect(INVALID, n=1 << 31, levels=32, g=0)
    expect(INVALID, n=8, levels=64, g=0)
    expect(INVALID, n=8, levels=1 << 40, g=0)
    # 5. a length above 2^30, more than 2^35 words read -- before the offset is looked at
    expect(LEN_TOO_LARGE, n=1 << 31, levels=1, g=0)
    expect(LEN_TOO_LARGE, n=1 << 30, batch=33, n_sets=1, wc=1, wa=1, g=0)
    expect(LEN_TOO_LARGE, n=1 << 30, batch=11, n_sets=1, wc=3, wa=3, g=0)
    expect(LEN_TOO_LARGE, n=2, batch=(1 << 34) + 1, wc=1, wa=3, g=0)
    # 6. the offset zero, with everything else in order (the largest calls that pass 5 among them)
    expect(INVERSE_OF_ZERO, g=0)
    expect(INVERSE_OF_ZERO, n=1 << 30, batch=32, wc=1, wa=1, levels=30, g=0)
    expect(INVERSE_OF_ZERO, n=1 << 30, batch=10, wc=3, wa=3, g=0)
    assert (out == 7).all()
    # 7. a valid call, every width pair and both kinds of sets: TF_ERR_NO_DEVICE without a GPU; with one, the host form runs
    for wc, wa in PAIRS:
        for levels, n_sets in ((1, 1), (3, 1), (2, 3)):
            for name, call in _forms(lib, cw, ch, out, wc=wc, wa=wa, levels=levels, n_sets=n_sets):
                if no_gpu:
                    assert call() == NO_DEVICE, (name, wc, wa)
                elif name == "tf_fri_fold":
                    out[:] = 7
                    assert call() == OK, (name, wc, wa)
                    want = fri_ref.fold(cw[:3 * 8 * wc], 8, 3, wc, pyref.to_raw(7), ch[:n_sets * levels * wa], levels, n_sets, wa)
                    assert np.array_equal(out[:want.size], want) and (out[want.size:] == 7).all()
    if no_gpu:
        assert (out == 7).all()


def test_the_empty_call_is_ok_with_null_pointers(tf, bufs):
    lib = tf.lib()
    cw, ch, out = bufs
    assert lib.tf_fri_fold(None, 8, 0, 3, pyref.to_raw(7), None, 1, 1, 3, None) == OK
    assert lib.tf_fri_fold_dev(None, 8, 0, 3, pyref.to_raw(7), None, 1, 1, 3, None, None) == OK
    # (before every other check: nothing of an empty call is looked at)
    assert lib.tf_fri_fold(None, 6, 0, 2, 0, None, 0, 5, 2, None) == OK
    for name, call in _forms(lib, cw, ch, out, batch=0, n_sets=0):
        assert call() == OK, name
    assert (out == 7).all()
    assert tf.fri.fold_host(np.zeros(0, np.uint64), 8, pyref.to_raw(7), np.zeros(3, np.uint64), batch=0).size == 0


def test_python_shapes_are_checked_on_the_host(tf):
    g = pyref.to_raw(7)
    cw, ch = np.zeros(8 * 3, np.uint64), np.zeros(3, np.uint64)
    with pytest.raises(ValueError):
        tf.fri.fold_host(cw[:-1], 8, g, ch)
    with pytest.raises(ValueError):
        tf.fri.fold_host(cw, 8, g, ch, levels=2)
    with pytest.raises(ValueError):
        tf.fri.fold_host(cw, 8, g, ch, width_c=3, width_a=1)
    with pytest.raises(ValueError):
        tf.fri.fold_host(cw, 8, g, ch, batch=-1)
    with pytest.raises(tf.TwentyFirstError) as e:
        tf.fri.plan(8, 4)
    assert e.value.code == INVALID
    with pytest.raises(tf.NttPanic) as e:
        tf.fri.plan(6, 1)
    assert e.value.code == NOT_POW2


# ------------------------------------------------------------------ the plan of passes and the work space
def test_plan_and_workspace(tf):
    fri = tf.fri
    rmax = max(fri.plan(1 << 12, 12))
    assert rmax in (2, 3, 4)
    for k in range(1, 13):
        n = 1 << k
        for levels in range(1, k + 1):
            for wc, wa in PAIRS:
                plan = fri.plan(n, levels, wc, wa)
                assert sum(plan) == levels and all(1 <= r <= rmax for r in plan) and all(r == rmax for r in plan[:-1]), (n, levels, plan)
                assert len(plan) == -(-levels // rmax)
                for batch in (1, 3):
                    ws = fri.workspace(n, batch, levels, wc, wa)
                    assert (ws == 0) == (len(plan) == 1), (n, levels, batch)
                    # the first intermediate, and from three passes on the second one next to it
                    live = [batch * (n >> sum(plan[:p + 1])) * wa * 8 for p in range(len(plan) - 1)]
                    assert ws == sum(live[:2]), (n, levels, batch, wc, wa)
    # the capacity bounds what is written, not what is returned
    buf = (C.c_int * 4)(9, 9, 9, 9)
    assert tf.lib().tf_fri_fold_plan(1 << 12, 12, 3, 3, buf, 2) == -(-12 // rmax) and list(buf) == [rmax, rmax, 9, 9]
    assert tf.lib().tf_fri_fold_plan(1 << 12, 12, 3, 3, None, 0) == -(-12 // rmax)


def test_plan_and_workspace_of_rejected_calls(tf):
    lib = tf.lib()
    buf = (C.c_int * 64)()
    # (n, levels, wc, wa) -> minus the status of the fold, in its order
    for args, code in (((8, 1, 3, 1), INVALID), ((8, 0, 3, 3), INVALID), ((6, 0, 3, 3), INVALID), ((0, 1, 1, 1), NOT_POW2), ((6, 9, 1, 3), NOT_POW2),
                       ((8, 4, 1, 1), INVALID), ((1 << 31, 32, 1, 1), INVALID), ((1 << 31, 31, 1, 1), LEN_TOO_LARGE)):
        assert lib.tf_fri_fold_plan(*args, buf, 64) == -code, args
    assert lib.tf_fri_fold_plan(1 << 30, 30, 1, 3, buf, 64) > 0
    # (n, batch, wc, wa, levels): rejected or empty -> 0, whatever the number of passes would be
    for args in ((1 << 12, 1, 3, 1, 12), (1 << 12, 1, 2, 2, 12), (1 << 12, 1, 3, 3, 0), (3 << 10, 1, 3, 3, 10), (0, 1, 3, 3, 10), (1 << 12, 1, 3, 3, 13),
                 (1 << 31, 1, 1, 1, 12), (1 << 30, 33, 1, 1, 12), (1 << 30, 11, 3, 3, 12), (1 << 12, 0, 3, 3, 12)):
        assert lib.tf_fri_fold_workspace(*args) == 0, args
    assert lib.tf_fri_fold_workspace(1 << 30, 32, 1, 1, 12) > 0 and lib.tf_fri_fold_workspace(1 << 30, 10, 3, 3, 12) > 0
