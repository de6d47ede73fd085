"""Every loop that is keyed by the BATCH, taken past its first turn, and every hard batch limit on both of its sides.

The rest of the GPU suite wraps the x direction of the grid-stride kernels; its largest batches (300 columns, 7 dividends, 5 codewords,
4 rows) leave these loops at one turn each:

  A  tree_batch_evaluate (tf_poly.hip): the walk in slabs of 2^25 / M units, chunk_combine launches of 65 535 polynomials, the unit
     limit of 65 536 and the fall-back to Horner beyond it -- through the ZerofierTree handle and one-shot through coset_extrapolate
     with the tree route forced;
  B  batch_evaluate_horner: launches of 65 535 polynomials, lane kernel and split kernel, BFieldElement, XFieldElement and base-field
     polynomials at extension-field points;
  C  tree_interpolate_rows: turns of min(rows, 32 768, 2^26 / (M L)) rows;
  D  the rows of the algebra kernels (`r += gridDim.y`): add, sub, scale, formal_derivative, degree;
  E  the limits: 65 535 dividends (divide, clean_divide_many), 131 069 codewords (barycentric_evaluate); one more is
     TF_ERR_LEN_TOO_LARGE.

Expected values: A, B, C, E are rank-2 families (tests/slab_ref.py: row r = a_r F0 + b_r F1, expected a_r E0 + b_r E1 with E0, E1 the
oracle's plain results for the two base rows), so every row differs from every other and a row read from a wrong base offset shows; D
is tests/algebra_ref.py on every row.  Every output word is compared, outputs start as words no field element has.

That a loop really turned is shown twice: the shape arithmetic is asserted from the constants mirrored in tests/slab_ref.py (pinned to
their sites in csrc/ by tests/test_slab_edges_cpu.py, which also checks the tables below), and for A and C the slab is read back from
the bytes the call requested under its own label (the per-label counters of tf_debug_temp_guard)."""
import numpy as np
import pytest

from tests import algebra_ref, fence
from tests import slab_ref as S

pytestmark = pytest.mark.gpu

LEN_TOO_LARGE = 5   # TF_ERR_LEN_TOO_LARGE
OFFSET = 7          # the coset of the one-shot extrapolations
NO_ELEMENT = -1     # 0xFFFF...: above p, what every output holds before the call

# ------------------------------------------------------------------ the shapes (tests/test_slab_edges_cpu.py checks their arithmetic too)
N_POINTS = 600                                                       # M = 1024: 32 768 units per walk
M_EVAL = S.padded_points(N_POINTS, S.INTERP_LEAF)                    # the handle's tree; the one-shot tree pads to the same M
# name -> (n_coeffs, batch, one-shot too).  A2's slab edge lies between two polynomials (two chunks each, an even slab); A2x has
# three chunks per polynomial, so the edge falls inside polynomial 10 922 and chunk_combine joins across it.
A_CASES = {"A1": (2, 32771, True), "A2": (M_EVAL + 5, 16386, False), "A2x": (2 * M_EVAL + 5, 10924, False), "A3": (2, 65536, True),
           "A4": (2, 65537, True)}
B_POINTS = 3
B_LANE = [(5, b) for b in (65535, 65536, 65538)]
B_SPLIT = [(S.HORNER_SPLIT, 65537)]
B_ONE_SHOT = [(4, b) for b in (65535, 65536, 65538)] + B_SPLIT       # a codeword has a power of two of elements: 4 stands in for 5
# name -> (n, rows, widths)
C_CASES = {"C1": (3, 32773, (1, 3)), "C2": (100, 32773, (1, 3)), "C3": (5000, 8195, (1,)), "C4": (5000, 2733, (3,))}
D_BATCHES = (65535, 65536, 131071)
D_NA, D_NB = 3, 2
E_DIVIDEND, E_DIVISOR = 5, 3
E_BARY_N = 4
E_BARY_BATCHES = (S.BARY_MAX_BATCH - 1, S.BARY_MAX_BATCH)            # 131 068: the last row group holds the denominator alone


def a_arithmetic(name):
    """what case `name` of A must cross, from the mirrored constants: (chunks, units, slab)"""
    n_coeffs, batch, _ = A_CASES[name]
    for leaf in (S.INTERP_LEAF, S.TREE_LEAF[1], S.TREE_LEAF[3]):
        assert S.padded_points(N_POINTS, leaf) == M_EVAL and N_POINTS >= 2 * leaf     # one M for every tree; the router admits the tree
    chunks, units, slab = S.tree_units(n_coeffs, batch, M_EVAL)
    if name == "A1":
        assert chunks == 1 and units <= S.TREE_MAX_UNITS and S.turns(units, slab) == 2 and units - slab == 3
    elif name == "A2":
        assert chunks == 2 and units <= S.TREE_MAX_UNITS and S.turns(units, slab) == 2 and slab % chunks == 0
    elif name == "A2x":
        assert chunks == 3 and units <= S.TREE_MAX_UNITS and S.turns(units, slab) == 2 and slab % chunks != 0
    elif name == "A3":
        assert units == S.TREE_MAX_UNITS == 2 * slab and S.turns(batch, S.GRID_Y) == 2 and batch - S.GRID_Y == 1
    else:
        assert units > S.TREE_MAX_UNITS and S.turns(batch, S.GRID_Y) == 2 and batch - S.GRID_Y == 2   # Horner, whose own loop turns
    return chunks, units, slab


def c_arithmetic(name, width):
    n, rows, _ = C_CASES[name]
    m = S.padded_points(n, S.INTERP_LEAF)
    slab = S.interp_slab(rows, m, width)
    assert slab < rows and S.turns(rows, slab) == 2 and rows <= S.GRID_Y
    if name in ("C1", "C2"):
        assert slab == S.INTERP_SLAB_ROWS and (m == S.INTERP_LEAF) == (name == "C1")                   # the row bound; one leaf / one level
    else:
        assert slab == S.INTERP_SLAB_ELEMS // (m * width) < S.INTERP_SLAB_ROWS and slab == {1: 8192, 3: 2730}[width]   # the byte bound
    return m, slab


# ------------------------------------------------------------------ plumbing
@pytest.fixture(scope="module", autouse=True)
def _need_gpu(tf):
    assert tf.lib().tf_device_count() > 0, "no HIP device visible: the product has no CPU fallback"
    yield
    _CACHE.clear()
    _release(tf)


def _release(tf):
    """give back what the pools hold: the work space of the largest cases is 8 - 10 GB, and two of them must not add up"""
    import torch

    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    assert tf.lib().tf_release_caches() == 0


def _dev(a):
    import warnings

    import torch

    with warnings.catch_warnings():   # the shared operands are read-only arrays; the tensor made of one is uploaded, never written
        warnings.filterwarnings("ignore", message="The given NumPy array is not writable")
        return torch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.int64)).cuda()


def _blank(words, dtype=None):
    import torch

    return torch.full((words,), NO_ELEMENT, dtype=dtype or torch.int64, device="cuda")


def _host(t):
    return t.cpu().numpy().view(np.uint64)


_CACHE = {}


def _once(key, make):
    """a reference or an operand computed once, shared by the tests that need it, read-only"""
    if key not in _CACHE:
        v = make()
        for a in (v if isinstance(v, tuple) else (v,)):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _CACHE[key] = v
    return _CACHE[key]


def _rows(oracle, key, words, batch, seed):
    """(f0, f1, a, b, the family's rows) for base rows of `words` words"""
    def make():
        f0, f1 = oracle.fill_random(words, seed), oracle.fill_random(words, seed + 1)
        a, b = S.scalars(oracle, batch, seed + 2)
        return f0, f1, a, b, S.family(oracle, f0, f1, a, b)

    return _once(("rows", key, words, batch, seed), make)


def _points(oracle, count, width, seed):
    def make():
        p = oracle.fill_random(count * width, seed)
        assert len({tuple(e) for e in p.reshape(-1, width).tolist()}) == count
        return p

    return _once(("points", count, width, seed), make)


def _same(oracle, got, e0, e1, a, b, what):
    bad = S.family_mismatch(oracle, got, e0, e1, a, b)
    assert bad is None, f"{what}: row {bad[0]} word {bad[1]}: got {bad[2]:#x}, expected {bad[3]:#x}"


class _route:
    """tf_set_batch_eval_route(route) around a call, automatic again afterwards"""

    def __init__(self, tf, route):
        self.lib, self.route = tf.lib(), route

    def __enter__(self):
        self.lib.tf_set_batch_eval_route(self.route)

    def __exit__(self, *exc):
        self.lib.tf_set_batch_eval_route(0)


# ------------------------------------------------------------------ A. batch evaluation on the zerofier tree
def _a_operands(oracle, name, width):
    n_coeffs, batch, _ = A_CASES[name]
    pts = _points(oracle, N_POINTS, width, 0xA0 + width)
    f0, f1, a, b, rows = _rows(oracle, "A", n_coeffs * width, batch, 0xA100 + width)
    e0, e1 = _once(("A", name, width), lambda: (S.horner(oracle, f0, pts, width), S.horner(oracle, f1, pts, width)))
    return n_coeffs, batch, pts, rows, a, b, e0, e1


def _handle_evaluate(tf, pts, width, rows, n_coeffs, batch):
    out = _blank(batch * (pts.size // width) * width)
    with tf.device.ZerofierTree(_dev(pts), width=width) as tree:
        tree.batch_evaluate(_dev(rows), n_coeffs, out, batch=batch)
        got = _host(out)
    return got


@pytest.mark.parametrize("width", (1, 3))
@pytest.mark.parametrize("name", sorted(A_CASES))
def test_tree_handle_batch_evaluate_past_one_walk(tf, oracle, name, width):
    a_arithmetic(name)
    n_coeffs, batch, pts, rows, a, b, e0, e1 = _a_operands(oracle, name, width)
    try:
        got = _handle_evaluate(tf, pts, width, rows, n_coeffs, batch)
        _same(oracle, got, e0, e1, a, b, f"{name} width {width} through the handle")
    finally:
        _release(tf)


@pytest.mark.parametrize("width", (1, 3))
@pytest.mark.parametrize("name", [n for n in sorted(A_CASES) if A_CASES[n][2]])
def test_one_shot_tree_route_past_one_walk(tf, oracle, name, width):
    """coset_extrapolate of codewords of length 2 with the tree forced: the interpolants are the polynomials of two coefficients"""
    _, units, _ = a_arithmetic(name)
    n, batch, _ = A_CASES[name]
    assert n == 2
    pts = _points(oracle, N_POINTS, width, 0xA0 + width)
    c0, c1, a, b, rows = _rows(oracle, "A", n * width, batch, 0xA100 + width)
    e0, e1 = _once(("A one-shot", width), lambda: tuple(S.horner(oracle, oracle.coset_interpolate(c, oracle.bfe_new(OFFSET), width=width), pts, width)
                                                         for c in (c0, c1)))
    out = _blank(batch * N_POINTS * width)
    try:
        with _route(tf, 2):
            assert tf.lib().tf_batch_eval_plan(n, N_POINTS, batch, width) == (2 if units <= S.TREE_MAX_UNITS else 1)
            tf.device.coset_extrapolate(oracle.bfe_new(OFFSET), _dev(rows), n, _dev(pts), out, batch=batch, width=width)
        _same(oracle, _host(out), e0, e1, a, b, f"{name} width {width} one-shot")
    finally:
        del out
        _release(tf)


@pytest.mark.parametrize("width", (1, 3))
def test_the_walk_asked_for_a_slab_smaller_than_its_units(tf, oracle, width):
    """A1 again with the library's memory guarded: the bytes requested under "zerofier tree walk" are
    (2 units + kTreeWorkArrays slab) M L words, which gives the slab the code really used"""
    _, units, slab = a_arithmetic("A1")
    n_coeffs, batch, pts, rows, a, b, e0, e1 = _a_operands(oracle, "A1", width)
    try:
        with fence.temp_guarded(tf.lib(), 1, must_see=["zerofier tree walk"]) as box:
            got = _handle_evaluate(tf, pts, width, rows, n_coeffs, batch)
        blocks, nbytes = box[0].labels["zerofier tree walk"]
        per_unit = 8 * M_EVAL * width
        assert blocks == 1 and nbytes % per_unit == 0 and (nbytes // per_unit - 2 * units) % S.TREE_WORK_ARRAYS == 0
        used = (nbytes // per_unit - 2 * units) // S.TREE_WORK_ARRAYS
        assert used == slab == S.TREE_SLAB_ELEMS // M_EVAL and used < units
        _same(oracle, got, e0, e1, a, b, f"A1 width {width}, guarded")
    finally:
        _release(tf)


# ------------------------------------------------------------------ B. Horner's launches of 65 535 polynomials
def _b_arithmetic(n_coeffs, batch):
    assert (n_coeffs >= S.HORNER_SPLIT) == ((n_coeffs, batch) in B_SPLIT) and B_POINTS <= S.INTERP_LEAF
    assert S.turns(batch, S.GRID_Y) == (1 if batch == S.GRID_Y else 2)


def _b_operands(oracle, n_coeffs, batch, width, point_width):
    pts = _points(oracle, B_POINTS, point_width, 0xB0 + point_width)
    f0, f1, a, b, rows = _rows(oracle, "B", n_coeffs * width, batch, 0xB100 + width)
    e0, e1 = _once(("B", n_coeffs, width, point_width), lambda: (S.horner(oracle, f0, pts, width, point_width), S.horner(oracle, f1, pts, width, point_width)))
    return pts, rows, a, b, e0, e1


@pytest.mark.parametrize("width", (1, 3))
@pytest.mark.parametrize("n_coeffs,batch", B_LANE + B_SPLIT)
def test_horner_batches_through_a_single_leaf_handle(tf, oracle, n_coeffs, batch, width):
    _b_arithmetic(n_coeffs, batch)
    pts, rows, a, b, e0, e1 = _b_operands(oracle, n_coeffs, batch, width, width)
    got = _handle_evaluate(tf, pts, width, rows, n_coeffs, batch)
    _same(oracle, got, e0, e1, a, b, f"{batch} polynomials of {n_coeffs}, width {width}")


@pytest.mark.parametrize("n_coeffs,batch", B_LANE + B_SPLIT)
def test_horner_batches_of_base_field_polynomials_at_extension_points(tf, oracle, n_coeffs, batch):
    _b_arithmetic(n_coeffs, batch)
    pts, rows, a, b, e0, e1 = _b_operands(oracle, n_coeffs, batch, 1, 3)
    out = _blank(batch * B_POINTS * 3)
    tf.device.evaluate_bfe_at_xfe(_dev(rows), n_coeffs, _dev(pts), out, batch=batch)
    _same(oracle, _host(out), e0, e1, a, b, f"{batch} base-field polynomials of {n_coeffs} at extension-field points")


@pytest.mark.parametrize("width", (1, 3))
@pytest.mark.parametrize("n,batch", B_ONE_SHOT)
def test_horner_batches_one_shot_on_route_1(tf, oracle, n, batch, width):
    _b_arithmetic(n, batch)
    pts = _points(oracle, B_POINTS, width, 0xB0 + width)
    c0, c1, a, b, rows = _rows(oracle, "B", n * width, batch, 0xB100 + width)
    e0, e1 = _once(("B one-shot", n, width), lambda: tuple(S.horner(oracle, oracle.coset_interpolate(c, oracle.bfe_new(OFFSET), width=width), pts, width)
                                                            for c in (c0, c1)))
    out = _blank(batch * B_POINTS * width)
    with _route(tf, 1):
        assert tf.lib().tf_batch_eval_plan(n, B_POINTS, batch, width) == 1
        tf.device.coset_extrapolate(oracle.bfe_new(OFFSET), _dev(rows), n, _dev(pts), out, batch=batch, width=width)
    _same(oracle, _host(out), e0, e1, a, b, f"{batch} codewords of {n}, width {width}, route 1")


# ------------------------------------------------------------------ C. interpolation rows
def _c_operands(oracle, name, width):
    n, rows, _ = C_CASES[name]
    dom = _points(oracle, n, width, 0xC0 + width)
    v0, v1, a, b, values = _rows(oracle, "C", n * width, rows, 0xC100 + width)
    e0, e1 = _once(("C", n, width), lambda: (oracle.lagrange_interpolate(dom, v0, width=width), oracle.lagrange_interpolate(dom, v1, width=width)))
    return n, rows, dom, values, a, b, e0, e1


def _interpolate(tf, entry, dom, values, rows, width):
    out = _blank(values.size)
    if entry == "one-shot":
        tf.device.interpolate(_dev(dom), _dev(values), out, rows=rows, width=width)
        return _host(out)
    with tf.device.ZerofierTree(_dev(dom), width=width) as tree:
        tree.interpolate(_dev(values), out, rows=rows)
        return _host(out)


@pytest.mark.parametrize("entry", ("one-shot", "handle"))
@pytest.mark.parametrize("name,width", [(n, w) for n in sorted(C_CASES) for w in C_CASES[n][2]])
def test_interpolation_rows_past_one_turn(tf, oracle, name, width, entry):
    c_arithmetic(name, width)
    n, rows, dom, values, a, b, e0, e1 = _c_operands(oracle, name, width)
    try:
        got = _interpolate(tf, entry, dom, values, rows, width)
        _same(oracle, got, e0, e1, a, b, f"{name} width {width}, {entry}")
    finally:
        _release(tf)


@pytest.mark.parametrize("name,width", [("C1", 1), ("C2", 3), ("C3", 1), ("C4", 3)])
def test_the_walk_up_asked_for_fewer_rows_than_it_was_given(tf, oracle, name, width):
    """with the library's memory guarded: "interpolation rows" is 5 slab M L words, which gives the rows of one turn"""
    m, slab = c_arithmetic(name, width)
    n, rows, dom, values, a, b, e0, e1 = _c_operands(oracle, name, width)
    try:
        with fence.temp_guarded(tf.lib(), 1, must_see=["interpolation rows"]) as box:
            got = _interpolate(tf, "handle", dom, values, rows, width)
        blocks, nbytes = box[0].labels["interpolation rows"]
        per_row = 8 * S.INTERP_ROW_ARRAYS * m * width
        assert blocks == 1 and nbytes % per_row == 0 and nbytes // per_row == slab < rows
        _same(oracle, got, e0, e1, a, b, f"{name} width {width}, guarded")
    finally:
        _release(tf)


# ------------------------------------------------------------------ D. rows of the algebra kernels
D_MAX = max(D_BATCHES)


def _d_words(oracle, count, seed):
    return _once(("D words", count, seed), lambda: oracle.fill_random(count, seed))


def _d_arithmetic(batch):
    assert S.turns(batch, S.GRID_Y) == {65535: 1, 65536: 2, 131071: 3}[batch]   # 131 071: the loop turns twice


def _d_prefix(t, words):
    return t[:words].clone()


@pytest.mark.parametrize("batch", D_BATCHES)
@pytest.mark.parametrize("width", (1, 3))
@pytest.mark.parametrize("op", ("add", "sub"))
def test_add_sub_rows_wrap(tf, oracle, op, width, batch):
    """unequal lengths keep the row dimension; the expected rows of the largest batch are computed once, a smaller batch is their prefix"""
    _d_arithmetic(batch)
    assert D_NA != D_NB
    x, y = _d_words(oracle, D_MAX * D_NA * width, 0xD1 + width), _d_words(oracle, D_MAX * D_NB * width, 0xD2 + width)
    want = _once(("D", op, width), lambda: getattr(algebra_ref, op)(x, D_NA, y, D_NB, width, D_MAX))
    out = _blank(batch * D_NA * width)
    fn = tf.device.poly_add if op == "add" else tf.device.poly_sub
    fn(_dev(x[:batch * D_NA * width]), D_NA, _dev(y[:batch * D_NB * width]), D_NB, out, batch=batch, width=width)
    assert np.array_equal(_host(out), want[:batch * D_NA * width])


@pytest.mark.parametrize("batch", D_BATCHES)
@pytest.mark.parametrize("width", (1, 3))
def test_scale_rows_wrap(tf, oracle, width, batch):
    _d_arithmetic(batch)
    x, alpha = _d_words(oracle, D_MAX * D_NA * width, 0xD1 + width), _d_words(oracle, width, 0xD3 + width)
    want = _once(("D", "scale", width), lambda: algebra_ref.scale(x, D_NA, width, alpha, width, D_MAX))
    out = _blank(batch * D_NA * width)
    tf.device.poly_scale(_dev(x[:batch * D_NA * width]), D_NA, alpha, out, batch=batch, width=width, width_alpha=width)
    assert np.array_equal(_host(out), want[:batch * D_NA * width])


@pytest.mark.parametrize("batch", D_BATCHES)
@pytest.mark.parametrize("width", (1, 3))
def test_formal_derivative_rows_wrap(tf, oracle, width, batch):
    _d_arithmetic(batch)
    x = _d_words(oracle, D_MAX * D_NA * width, 0xD1 + width)
    want = _once(("D", "derivative", width), lambda: algebra_ref.formal_derivative(x, D_NA, width, D_MAX))
    out = _blank(batch * (D_NA - 1) * width)
    tf.device.poly_formal_derivative(_dev(x[:batch * D_NA * width]), D_NA, out, batch=batch, width=width)
    assert np.array_equal(_host(out), want[:batch * (D_NA - 1) * width])


@pytest.mark.parametrize("first", ("full", "zero"))
@pytest.mark.parametrize("batch", D_BATCHES)
@pytest.mark.parametrize("width", (1, 3))
def test_degree_rows_wrap(tf, oracle, width, batch, first):
    """every row has a zero leading coefficient (degree 1, 0 or -1 by turns) but one, and one row is zero: the two stand in the first
    row past the launch's 65 535 (or the last row but one, when nothing wraps) and in the last row, either way round"""
    import torch

    _d_arithmetic(batch)
    x = _d_words(oracle, batch * D_NA * width, 0xD4 + width).copy().reshape(batch, D_NA, width)
    x[:, D_NA - 1] = 0
    x[1::3, 1] = 0
    x[2::3, 0] = 0
    x[2::3, 1] = 0
    x[5::6, 0, width - 1] = oracle.bfe_new(1)
    p1, p2 = min(S.GRID_Y, batch - 2), batch - 1
    full, zero = (p1, p2) if first == "full" else (p2, p1)
    x[zero] = 0
    x[full, D_NA - 1, width - 1] = oracle.bfe_new(1)                 # the only full-degree row; over XFE its last limb alone
    assert batch == S.GRID_Y or p2 >= S.GRID_Y
    want = algebra_ref.degree(x.reshape(-1), D_NA, width, batch)
    assert want[full] == D_NA - 1 and want[zero] == -1 and (want == D_NA - 1).sum() == 1 and set(want.tolist()) == {-1, 0, 1, 2}
    deg = _blank(batch, torch.int64)
    deg.fill_(7)
    tf.device.poly_degree(_dev(x), D_NA, deg, batch=batch, width=width)
    assert np.array_equal(deg.cpu().numpy(), want)


# ------------------------------------------------------------------ E. the hard limits, both sides
def _panics_too_large(tf, call):
    with pytest.raises(tf.TwentyFirstError) as e:
        call()
    assert e.value.code == LEN_TOO_LARGE


@pytest.mark.parametrize("width", (1, 3))
def test_divide_at_its_limit_of_dividends(tf, oracle, width):
    import torch

    batch = S.DIVIDE_MAX_BATCH
    assert batch == S.GRID_Y
    d0, d1, a, b, rows = _rows(oracle, "E1", E_DIVIDEND * width, batch, 0xE100 + width)
    div = oracle.fill_random(E_DIVISOR * width, 0xE1 + width)
    assert div[(E_DIVISOR - 1) * width:].any()
    (q0, r0), (q1, r1) = (S.long_divide(oracle, d, div, width) for d in (d0, d1))
    nq, nr = E_DIVIDEND - E_DIVISOR + 1, E_DIVISOR - 1
    q, r = _blank(batch * nq * width), _blank(batch * nr * width)
    tf.device.divide(_dev(rows), E_DIVIDEND, _dev(div), q, r, batch=batch, width=width)
    _same(oracle, _host(q), q0, q1, a, b, f"quotients, width {width}")
    _same(oracle, _host(r), r0, r1, a, b, f"remainders, width {width}")
    more = torch.zeros((batch + 1) * E_DIVIDEND * width, dtype=torch.int64, device="cuda")
    _panics_too_large(tf, lambda: tf.device.divide(more, E_DIVIDEND, _dev(div), _blank((batch + 1) * nq * width), _blank((batch + 1) * nr * width),
                                                   batch=batch + 1, width=width))


def test_clean_divide_many_at_its_limit_of_dividends(tf, oracle):
    import torch

    batch = S.CLEAN_DIVIDE_MAX_BATCH
    assert batch == S.GRID_Y
    nq = E_DIVIDEND - E_DIVISOR + 1
    div = oracle.fill_random(E_DIVISOR, 0xE2)
    assert div[-1]
    # clean dividends: the products of two base quotients with the divisor, and their combinations
    d0, d1 = (oracle.poly_mul(oracle.fill_random(nq, 0xE20 + k), div) for k in (0, 1))
    a, b = S.scalars(oracle, batch, 0xE22)
    rows = S.family(oracle, d0, d1, a, b)
    assert rows[:, -1].all()                                         # normalised dividends
    (q0, r0), (q1, r1) = (S.long_divide(oracle, d, div, 1) for d in (d0, d1))
    assert not r0.any() and not r1.any()
    q = _blank(batch * nq)
    tf.device.clean_divide_many(_dev(rows), E_DIVIDEND, _dev(div), q, batch)
    torch.cuda.synchronize()
    _same(oracle, _host(q), q0, q1, a, b, "clean quotients")
    more = torch.zeros((batch + 1) * E_DIVIDEND, dtype=torch.int64, device="cuda")
    _panics_too_large(tf, lambda: tf.device.clean_divide_many(more, E_DIVIDEND, _dev(div), _blank((batch + 1) * nq), batch + 1))


@pytest.mark.parametrize("width", (1, 3))
@pytest.mark.parametrize("batch", E_BARY_BATCHES)
def test_barycentric_evaluate_up_to_its_limit_of_codewords(tf, oracle, batch, width):
    groups = S.turns(batch + 1, S.BARY_ROWS_PER_BLOCK)                # the denominator is row `batch`
    assert groups == S.GRID_Y and batch <= S.BARY_MAX_BATCH
    assert ((batch + 1) % S.BARY_ROWS_PER_BLOCK == 1) == (batch == S.BARY_MAX_BATCH - 1)   # the last group: the denominator alone, or full
    x = oracle.fill_random(3, 0xE3)
    c0, c1, a, b, rows = _rows(oracle, "E3", E_BARY_N * width, batch, 0xE300 + width)
    e0, e1 = (oracle.barycentric_evaluate(c, x, width=width) for c in (c0, c1))
    out = _blank(3 * batch)
    tf.device.barycentric_evaluate(_dev(rows), E_BARY_N, x, out, batch=batch, width=width)
    _same(oracle, _host(out), e0, e1, a, b, f"{batch} codewords, width {width}")


@pytest.mark.parametrize("width", (1, 3))
def test_barycentric_evaluate_refuses_one_codeword_more(tf, oracle, width):
    """include/tf_hip.h: at most 131 069 codewords per call"""
    import torch

    batch = S.BARY_MAX_BATCH + 1
    assert batch == 131070 and S.turns(batch + 1, S.BARY_ROWS_PER_BLOCK) == S.GRID_Y + 1
    cw = torch.zeros(batch * E_BARY_N * width, dtype=torch.int64, device="cuda")
    _panics_too_large(tf, lambda: tf.device.barycentric_evaluate(cw, E_BARY_N, oracle.fill_random(3, 0xE3), _blank(3 * batch), batch=batch, width=width))
