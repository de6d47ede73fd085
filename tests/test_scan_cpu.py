"""The prefix scans, the parts that need no GPU: the blocked model the kernels follow (tests/scan_ref.py: aggregate, spine, apply)
proved equal to the sequential loop; the loop pinned to what the oracle and tests/points_ref already pin (Horner evaluation,
geometric sequences, multiples); the plan and the work-space rule; the argument errors in their documented order; the Python
wrapper's own checks, which come before any library call."""
import ctypes as C

import numpy as np
import pytest

from tests import points_ref as pr
from tests import pyref
from tests import scan_ref as sr
from twenty_first_amd import scan  # the feature under test: collection fails without it

P = pyref.P
SUM, PRODUCT, AFFINE = sr.SUM, sr.PRODUCT, sr.AFFINE
OK, LEN_TOO_LARGE, NULL, NO_DEVICE, INVALID = 0, 5, 7, 8, 17
NEW = ("tf_scan_sum_dev", "tf_scan_product_dev", "tf_scan_affine_dev", "tf_scan_workspace", "tf_scan_plan")


def _rand_elems(rng, count, w):
    v = [int(x) % P for x in rng.integers(0, 1 << 63, count * w, dtype=np.uint64) * 2 + rng.integers(0, 2, count * w, dtype=np.uint64)]
    return v if w == 1 else [tuple(v[3 * i:3 * i + 3]) for i in range(count)]


# ------------------------------------------------------------------ the blocked model is the loop
@pytest.mark.parametrize("w", [1, 3])
@pytest.mark.parametrize("tile,turn", [(1, 1), (1, 2), (2, 1), (2, 37), (37, 2), (37, 37), (37, 1)])
def test_blocked_model_equals_the_loop(w, tile, turn):
    rng = np.random.default_rng(100 * tile + 10 * turn + w)
    for n in sorted({1, 2, tile - 1, tile, tile + 1, 2 * tile + 1, turn * tile + tile + 1, 3 * turn * tile + 5} - {0}):
        a, b, init = _rand_elems(rng, n, w), _rand_elems(rng, n, w), _rand_elems(rng, 1, w)[0]
        for ea, eb in ((a, b), (None, b), (a, None)):
            want = sr.loop(ea, eb, init, w)
            got, maps, starts = sr.blocked(ea, eb, init, w, tile, turn)
            assert got == want, (n, ea is None, eb is None)
            tiles = -(-n // tile)
            assert len(maps) == tiles and maps[-1] is None and all(m is not None for m in maps[:-1])
            assert starts == [init] + [want[t * tile - 1] for t in range(1, tiles)]


def test_the_monoid_is_associative_and_not_commutative():
    rng = np.random.default_rng(3)
    for w in (1, 3):
        f, g, h = [tuple(_rand_elems(rng, 2, w)) for _ in range(3)]
        assert sr.then(sr.then(f, g, w), h, w) == sr.then(f, sr.then(g, h, w), w)
        assert sr.then(f, g, w) != sr.then(g, f, w)
        ident = (pr.one(w), pr.zero(w))
        assert sr.then(ident, f, w) == f and sr.then(f, ident, w) == f
        y = _rand_elems(rng, 1, w)[0]
        assert sr.apply(sr.then(f, g, w), y, w) == sr.apply(g, sr.apply(f, y, w), w)


# ------------------------------------------------------------------ the loop, pinned to what is pinned already
@pytest.mark.parametrize("n", [1, 2, 17, 100])
def test_affine_with_a_constant_multiplier_is_horner(oracle, n):
    rng = np.random.default_rng(n)
    coeffs = _rand_elems(rng, n, 1)
    x = _rand_elems(rng, 1, 1)[0]
    # BFieldElement polynomial at a BFieldElement point, (1, 1)
    got, _ = sr.scan(AFFINE, n, 1, a=pr.words([x], 1), b=pr.words(coeffs[::-1], 1), wa=1, wb=1, a_len=1)
    assert np.array_equal(got[-1:], oracle.poly_eval(pr.words(coeffs, 1), pyref.to_raw(x), width=1))
    # XFieldElement polynomial at an XFieldElement point, (3, 3); the lifted BFieldElement polynomial, (3, 1)
    xc, xp = _rand_elems(rng, n, 3), _rand_elems(rng, 1, 3)[0]
    got, _ = sr.scan(AFFINE, n, 1, a=pr.words([xp], 3), b=pr.words(xc[::-1], 3), wa=3, wb=3, a_len=1)
    assert np.array_equal(got[-3:], oracle.poly_eval_xfe_point(pr.words(xc, 3), pr.words([xp], 3)))
    got, _ = sr.scan(AFFINE, n, 1, a=pr.words([xp], 3), b=pr.words(coeffs[::-1], 1), wa=3, wb=1, a_len=1)
    lifted = pr.words([pr.lift(c, 1, 3) for c in coeffs], 3)
    assert np.array_equal(got[-3:], oracle.poly_eval_xfe_point(lifted, pr.words([xp], 3)))
    # and a_len = n with the same multiplier in every row is the same thing
    rows, _ = sr.scan(AFFINE, n, 1, a=pr.words([xp] * n, 3), b=pr.words(coeffs[::-1], 1), wa=3, wb=1)
    assert np.array_equal(rows, got)


@pytest.mark.parametrize("w", [1, 3])
def test_product_of_a_constant_column_is_the_geometric_sequence(w):
    rng = np.random.default_rng(40 + w)
    r, first = _rand_elems(rng, 1, w)[0], _rand_elems(rng, 1, w)[0]
    n = 50
    got, _ = sr.scan(PRODUCT, n, 1, a=pr.words([r] * n, w), wa=w, wb=w, init=pr.words([first], w))
    # powers: first, first r, ...; the scan starts one step further
    assert np.array_equal(got, pr.powers(pr.words([first], w), pr.words([r], w), w, n + 1)[w:])


@pytest.mark.parametrize("w", [1, 3])
def test_sum_of_a_constant_column_is_its_multiples(w):
    rng = np.random.default_rng(50 + w)
    c = _rand_elems(rng, 1, w)[0]
    n = 70
    got, _ = sr.scan(SUM, n, 1, b=pr.words([c] * n, w), wa=w, wb=w)
    assert np.array_equal(got, pr.words([pr.f_mul(pr.lift(i + 1, 1, w), c, w) for i in range(n)], w))


def test_words_layout_of_the_model():
    """strides, the packed multiplier sets and the start values, on a case small enough to write down"""
    b = np.array([pyref.to_raw(v) for v in (1, 2, 3, 99, 10, 20, 30)], dtype=np.uint64)  # two columns of 3 at stride 4
    got, _ = sr.scan(SUM, 3, 2, b=b, stride_b=4)
    assert [pyref.to_val(int(x)) for x in got] == [1, 3, 6, 10, 30, 60]
    got, _ = sr.scan(SUM, 3, 2, b=b, stride_b=4, init=pr.words([5, 7], 1))
    assert [pyref.to_val(int(x)) for x in got] == [6, 8, 11, 17, 37, 67]
    got, _ = sr.scan(AFFINE, 3, 2, a=pr.words([2, 3], 1), b=b, stride_b=4, a_len=1, a_sets=2, init=pr.words([1], 1))
    assert [pyref.to_val(int(x)) for x in got] == [3, 8, 19, 13, 59, 207]
    assert np.array_equal(sr.strided(got, 3, 2, 1, 5, fill=9)[[3, 4]], [9, 9]) and sr.padding(3, 2, 1, 5).tolist() == [False] * 3 + [True] * 2 + [False] * 3


# ------------------------------------------------------------------ the ABI without a device
def _p(a):
    return C.c_void_p(a.ctypes.data)


def test_symbols_declared_and_exported(tf):
    from twenty_first_amd import _lib

    text = open(_lib.HEADER).read()
    for name in NEW:
        assert name + "(" in text and name in _lib.SIGNATURES and hasattr(tf.lib(), name), name
    assert tf.scan is scan and (scan.SUM, scan.PRODUCT, scan.AFFINE) == (SUM, PRODUCT, AFFINE)
    for macro, value in (("TF_SCAN_SUM", SUM), ("TF_SCAN_PRODUCT", PRODUCT), ("TF_SCAN_AFFINE", AFFINE)):
        assert f"#define {macro} {value}\n" in text


def test_plan_and_workspace_are_consistent_and_monotone(tf):
    for mode in (SUM, PRODUCT, AFFINE):
        for w in (1, 3):
            T, tiles1, S, launches, wave, m_words = scan.plan(mode, 1, 1, w)
            assert (tiles1, launches) == (1, 1) and T % wave == 0 and wave % 64 == 0 and S >= 2
            assert m_words == (2 * w if mode == AFFINE else w)
            assert T * w <= 16384, "a tile of one operand stays inside the guard words of tests/fence.py"
            last = (0, 0)
            for n in (1, 2, 63, 64, 65, wave, wave + 1, T - 1, T, T + 1, 2 * T, 2 * T + 1, S * T, S * T + 1, S * T + T + 1, 1 << 24):
                for batch in (1, 3):
                    p = scan.plan(mode, n, batch, w)
                    assert p.tile == T and p.turn == S and p.tiles == -(-n // T) and p.launches == (1 if n <= T else 3)
                    ws = scan.workspace(mode, n, batch, w)
                    # tile maps and tile start values, nothing for a single launch
                    assert ws == (0 if p.tiles == 1 else p.tiles * batch * (m_words + w) * 8), (mode, w, n, batch)
                p1 = scan.plan(mode, n, 1, w)
                assert (p1.tiles, scan.workspace(mode, n, 1, w)) >= last
                last = (p1.tiles, scan.workspace(mode, n, 1, w))
    # the capacity bounds what is written, not what is returned
    buf = (C.c_int * 4)(9, 9, 9, 9)
    assert tf.lib().tf_scan_plan(SUM, 10000, 1, 1, buf, 2) == 3 and list(buf)[2:] == [9, 9] and buf[1] == -(-10000 // buf[0])
    assert tf.lib().tf_scan_plan(SUM, 10000, 1, 1, None, 0) == 3
    assert tf.lib().tf_scan_plan(SUM, 0, 1, 1, buf, 4) == 0 and tf.lib().tf_scan_plan(AFFINE, 5, 0, 3, buf, 4) == 0


def test_plan_and_workspace_of_rejected_and_empty_calls(tf):
    lib = tf.lib()
    buf = (C.c_int * 6)()
    big = 1 << 24
    for args, code in (((3, big, 1, 1), INVALID), ((-1, big, 1, 1), INVALID), ((SUM, big, 1, 2), INVALID), ((AFFINE, big, 1, 0), INVALID),
                       ((SUM, (1 << 30) + 1, 1, 1), LEN_TOO_LARGE), ((SUM, 1 << 30, 33, 1), LEN_TOO_LARGE), ((PRODUCT, 1 << 30, 11, 3), LEN_TOO_LARGE),
                       ((AFFINE, 1 << 30, 17, 1), LEN_TOO_LARGE), ((AFFINE, 3, (1 << 34) // 9 + 1, 3), LEN_TOO_LARGE),
                       # one workgroup per (column, tile) above a wave's elements, fewer than 2^24 of them in a launch
                       ((SUM, 1025, 1 << 24, 1), LEN_TOO_LARGE), ((PRODUCT, 513, 1 << 24, 3), LEN_TOO_LARGE), ((SUM, 2048, 1 << 24, 1), LEN_TOO_LARGE)):
        assert lib.tf_scan_plan(*args, buf, 6) == -code, args
        assert lib.tf_scan_workspace(*args) == 0, args
    for args in ((SUM, 1 << 30, 32, 1), (PRODUCT, 1 << 30, 10, 3), (AFFINE, 1 << 30, 16, 1), (AFFINE, 3, (1 << 34) // 9, 3),
                 (SUM, 1025, (1 << 24) - 1, 1), (SUM, 1024, 1 << 25, 1), (PRODUCT, 512, 1 << 24, 3), (PRODUCT, 682, (1 << 24) - 1, 3)):
        assert lib.tf_scan_plan(*args, buf, 6) > 0, args
    assert lib.tf_scan_workspace(SUM, 1 << 30, 32, 1) > 0 and lib.tf_scan_workspace(AFFINE, 3, (1 << 34) // 9, 3) == 0
    for args in ((SUM, 0, 5, 1), (AFFINE, big, 0, 3)):
        assert lib.tf_scan_workspace(*args) == 0 and lib.tf_scan_plan(*args, buf, 6) == 0
    with pytest.raises(tf.TwentyFirstError) as e:
        scan.plan(7, 100)
    assert e.value.code == INVALID
    with pytest.raises(ValueError):
        scan.plan(SUM, -1)
    with pytest.raises(ValueError):
        scan.workspace(SUM, 10, batch=-1)


@pytest.fixture()
def bufs():
    words = np.arange(64, dtype=np.uint64)
    return words.copy(), words.copy(), np.full(64, 7, dtype=np.uint64), np.full(8, 3, dtype=np.uint64), np.full(64, 5, dtype=np.uint64)


def _forms(lib, a, b, out, init, work, n=4, batch=2, wa=3, wb=3, a_len=None, a_sets=1, stride_a=None, stride_b=None, stride_out=None, n_init=0,
           work_bytes=None, null=(), modes=(SUM, PRODUCT, AFFINE)):
    """the three entry points on the same arguments; `null`: names of the pointers passed as NULL"""
    ptr = {name: (None if name in null else _p(arr)) for name, arr in (("a", a), ("b", b), ("out", out), ("init", init), ("work", work))}
    if n_init == 0 and "init" not in null and init is None:
        ptr["init"] = None
    wb_bytes = work.size * 8 if work_bytes is None else work_bytes
    sa = n * wa if stride_a is None else stride_a
    sb = n * wb if stride_b is None else stride_b
    so = n * wa if stride_out is None else stride_out
    if SUM in modes:
        yield "sum", lambda: lib.tf_scan_sum_dev(ptr["b"], n, batch, wb, sb, ptr["init"], n_init, ptr["out"], n * wb if stride_out is None else so, ptr["work"],
                                                 wb_bytes, None)
    if PRODUCT in modes:
        yield "product", lambda: lib.tf_scan_product_dev(ptr["a"], n, batch, wa, sa, ptr["init"], n_init, ptr["out"], so, ptr["work"], wb_bytes, None)
    if AFFINE in modes:
        yield "affine", lambda: lib.tf_scan_affine_dev(ptr["a"], n if a_len is None else a_len, a_sets, wa, sa, ptr["b"], wb, sb, n, batch, ptr["init"],
                                                        n_init, ptr["out"], so, ptr["work"], wb_bytes, None)


def test_argument_errors_in_the_documented_order_without_device(tf, bufs):
    lib = tf.lib()
    a, b, out, init, work = bufs
    no_gpu = lib.tf_device_count() == 0
    T3 = scan.plan(SUM, 1, 1, 3).tile

    def expect(code, **kw):
        for name, call in _forms(lib, a, b, out, init, work, **kw):
            assert call() == code, (name, code, kw)

    # 0. the empty call: TF_OK whatever else is wrong, NULL pointers allowed
    expect(OK, n=0, null=("a", "b", "out", "init", "work"), wa=2, wb=5, n_init=9)
    expect(OK, batch=0, null=("a", "b", "out", "init", "work"), stride_a=0, stride_b=0, stride_out=0)
    # 1. a NULL pointer, whichever it is -- also when everything behind it is wrong too
    expect(NULL, null=("a",), modes=(PRODUCT, AFFINE))
    expect(NULL, null=("b",), modes=(SUM, AFFINE))
    expect(NULL, null=("out",))
    expect(NULL, null=("init",), n_init=1)
    expect(NULL, null=("out",), wa=2, wb=2, stride_a=0, stride_b=0, n_init=5, n=1 << 40)
    expect(NULL, null=("init",), n_init=7, stride_out=1)
    expect(NULL, null=("work",), n=T3 + 1, batch=1)                     # a valid call of two tiles needs its work space
    # 2. widths, a_len, a_sets, strides, n_init, a short work space -- before the length is looked at
    for wa, wb in ((2, 2), (0, 0), (5, 5)):
        expect(INVALID, wa=wa, wb=wb, n=1 << 40)
    for wa, wb in ((1, 3), (3, 2), (1, 0)):
        expect(INVALID, wa=wa, wb=wb, modes=(AFFINE,), n=1 << 40)
    expect(INVALID, a_len=2, modes=(AFFINE,), n=1 << 40)
    expect(INVALID, a_len=0, modes=(AFFINE,))
    expect(INVALID, a_len=1, a_sets=3, modes=(AFFINE,))
    expect(INVALID, a_len=1, a_sets=0, modes=(AFFINE,), n=1 << 40, stride_b=3 << 40, stride_out=3 << 40)
    expect(INVALID, stride_a=11, modes=(PRODUCT, AFFINE))
    expect(INVALID, n=1, a_len=1, stride_a=2, modes=(AFFINE,))            # n = 1, a stride that is not 0: a table of one row
    expect(INVALID, n=1, a_len=1, stride_a=0, a_sets=3, modes=(AFFINE,))  # n = 1, stride_a = 0: the packed form, a_sets counts
    expect(LEN_TOO_LARGE, n=2048, batch=1 << 24, wa=1, wb=1, n_init=1, work_bytes=0)   # more workgroups than a launch holds
    expect(INVALID, stride_b=11, modes=(SUM, AFFINE))
    expect(INVALID, stride_b=3, wb=1, modes=(AFFINE,))
    expect(INVALID, stride_out=11)
    expect(INVALID, n=1 << 40, stride_out=12)                            # (a stride is compared with the length before the length with its bound)
    expect(INVALID, n_init=3)
    expect(INVALID, n_init=3, n=1 << 31, stride_a=3 << 31, stride_b=3 << 31, stride_out=3 << 31)
    expect(INVALID, n=T3 + 1, batch=1, work_bytes=scan.workspace(AFFINE, T3 + 1, 1, 3) - 1, modes=(AFFINE,))
    expect(INVALID, n=T3 + 1, batch=1, work_bytes=scan.workspace(SUM, T3 + 1, 1, 3) - 8, modes=(SUM, PRODUCT))
    # 3. a length above 2^30, too many words -- with everything else in order
    expect(LEN_TOO_LARGE, n=(1 << 30) + 1, stride_a=3 << 31, stride_b=3 << 31, stride_out=3 << 31, work_bytes=1 << 62)
    expect(LEN_TOO_LARGE, n=1 << 30, batch=11, stride_a=3 << 30, stride_b=3 << 30, stride_out=3 << 30, work_bytes=1 << 62, modes=(SUM, PRODUCT))
    expect(LEN_TOO_LARGE, n=1 << 30, batch=6, stride_a=3 << 30, stride_b=3 << 30, stride_out=3 << 30, work_bytes=1 << 62, modes=(AFFINE,))
    expect(LEN_TOO_LARGE, n=1 << 30, batch=6, a_len=1, stride_b=1 << 30, wb=1, stride_out=3 << 30, work_bytes=1 << 62, modes=(AFFINE,))
    assert (out == 7).all() and (work == 5).all()
    # 4. valid calls of every mode, width pair and multiplier form: TF_ERR_NO_DEVICE on a machine without a GPU
    if no_gpu:
        for wa, wb in ((1, 1), (3, 3)):
            expect(NO_DEVICE, wa=wa, wb=wb, n_init=2)
            expect(NO_DEVICE, wa=wa, wb=wb, null=("work", "init"), work_bytes=0)
        for a_len, a_sets in ((None, 1), (None, 77), (1, 1), (1, 2)):
            expect(NO_DEVICE, wa=3, wb=1, a_len=a_len, a_sets=a_sets, n_init=1, modes=(AFFINE,))
        expect(NO_DEVICE, n=1, a_len=1, a_sets=77, modes=(AFFINE,))            # a table of one row at its stride: a_sets not looked at
        for a_sets in (1, 2):
            expect(NO_DEVICE, n=1, a_len=1, a_sets=a_sets, stride_a=0, modes=(AFFINE,))   # one row under packed multipliers
        assert (out == 7).all() and (work == 5).all()


# ------------------------------------------------------------------ the wrapper's own checks come before any library call
class _NoLaunch:
    """the library with the three scans replaced by a tripwire; the host arithmetic stays"""

    def __init__(self, lib):
        self.tf_scan_workspace, self.tf_scan_plan = lib.tf_scan_workspace, lib.tf_scan_plan
        self.calls = []

    def _trip(self, *args):
        self.calls.append(args)
        return 0

    tf_scan_sum_dev = tf_scan_product_dev = tf_scan_affine_dev = _trip


@pytest.fixture()
def cpu_tensors_pass(tf, monkeypatch):
    """scan.py with the CUDA requirement of its tensors lifted and the launches counted, so that the checks that follow it run here"""
    stub = _NoLaunch(tf.lib())
    monkeypatch.setattr(scan, "_t", lambda t, name="tensor": t)
    monkeypatch.setattr(scan, "_stream", lambda s: None)
    monkeypatch.setattr(scan._lib, "lib", lambda: stub)
    return stub


def test_python_checks_raise_before_any_library_call(tf, cpu_tensors_pass):
    import torch

    stub = cpu_tensors_pass
    T = scan.plan(SUM, 1, 1, 1).tile
    z = lambda k: torch.zeros(k, dtype=torch.int64)  # noqa: E731
    x, out = z(24), z(24)
    scan.sum_(x, 8, out, batch=3)
    scan.sum_(x, 8, x, batch=3)                                             # exactly in place
    scan.product(x, 7, x, batch=3, stride_in=8, stride_out=8)
    scan.affine(z(3), x, 8, x, a_len=1)                                     # in place on b, one packed multiplier
    scan.affine(z(3), z(8), 8, out, width_b=1, a_len=1, init=z(3))          # an XFieldElement multiplier over a BFieldElement column
    assert len(stub.calls) == 5
    # one row: a_len = 1 said aloud is the packed form and reaches the library with stride_a = 0; left at its default it is a table
    scan.affine(z(3), z(6), 1, z(6), batch=2, a_len=1)
    assert stub.calls[-1][1:5] == (1, 1, 3, 0)
    scan.affine(z(7), z(6), 1, z(6), batch=2, stride_a=4)
    assert stub.calls[-1][1:5] == (1, 1, 3, 4)
    with pytest.raises(ValueError):
        scan.affine(z(3), z(6), 1, z(6), batch=2)                           # a table of two rows' worth does not fit one element
    del stub.calls[5:]
    bad = [
        lambda: scan.sum_(x, 8, out, batch=4),                              # short operands
        lambda: scan.sum_(x, 8, out[:23], batch=3),
        lambda: scan.sum_(x, 8, out, batch=3, width=2),
        lambda: scan.sum_(x, 8, out, batch=3, stride_in=7),
        lambda: scan.sum_(x, 8, out, batch=-3),
        lambda: scan.sum_(x, 8, x[1:], batch=2),                            # overlapping, not in place
        lambda: scan.sum_(x, 7, x, batch=3, stride_in=8, stride_out=7),     # the same pointer under another stride
        lambda: scan.product(x[:16], 8, x[8:], batch=2),
        lambda: scan.sum_(x, 8, out, batch=3, init=z(2)),                   # init: one element or one per column
        lambda: scan.sum_(x, 8, out, batch=3, init=out[:1]),                # init inside out
        lambda: scan.sum_(z(T + 1), T + 1, z(T + 1)),                       # two tiles and no work space
        lambda: scan.sum_(z(T + 1), T + 1, z(T + 1), work=z(scan.workspace(SUM, T + 1) // 8 - 1)),
        lambda: scan.affine(x, x, 8, out, width_a=1, width_b=3),            # a pair not listed
        lambda: scan.affine(x, x, 8, out, a_len=2),
        lambda: scan.affine(z(6), x, 8, out, a_len=1, a_sets=2),            # a_sets neither 1 nor batch
        lambda: scan.affine(z(6), x, 8, out, a_len=1),                      # a holds more than a_sets elements
        lambda: scan.affine(z(24), x, 8, x, width_a=3, width_b=1),              # in place needs equal widths
        lambda: scan.affine(out, x, 8, out),                                # out on a
        lambda: scan.affine(out[:3], x, 8, out, a_len=1),
    ]
    for k, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
        assert len(stub.calls) == 5, k
    work = z(scan.workspace(SUM, T + 1) // 8)
    with pytest.raises(ValueError):                                         # the work space on an operand
        big = z(T + 1 + work.numel())
        scan.sum_(big[:T + 1], T + 1, z(T + 1), work=big[T:T + work.numel()])
    scan.sum_(z(T + 1), T + 1, z(T + 1), work=work)
    assert len(stub.calls) == 6


def test_tensors_must_be_cuda_words(tf):
    import torch

    x = torch.zeros(8, dtype=torch.int64)
    with pytest.raises(TypeError):
        scan.sum_(x, 8, x)
    with pytest.raises(TypeError):
        scan.affine(np.zeros(3, np.uint64), x, 8, x, a_len=1)
