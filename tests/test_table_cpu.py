"""Table transposes, row opening and the row-major LDE: the parts that need no GPU -- the numpy models the GPU tests compare against
(tests/table_ref.py) on hand-written tables; the exported symbols; the argument errors every flavour returns before any HIP call,
and their order; the work-space rule of the LDE; and that every public callable of twenty_first_amd/table.py has a fence row in
tests/test_gpu_table.py."""
import ctypes as C
import inspect
import os

import numpy as np
import pytest

from tests import table_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("tf_table_transpose", "tf_table_transpose_dev", "tf_table_gather_rows", "tf_table_gather_rows_dev", "tf_table_lde_rows_bfe_dev",
       "tf_table_lde_rows_xfe_dev", "tf_table_lde_rows_workspace")
PYTHON = ("transpose", "columns_to_rows", "rows_to_columns", "gather_rows", "lde_rows", "lde_rows_workspace")
OK, NOT_POW2, LEN_TOO_LARGE, NOT_ABOVE, NULL, NO_DEVICE, INVERSE_OF_ZERO, INVALID = 0, 4, 5, 6, 7, 8, 12, 17
BIG = (1 << 30) + 1
X = 77  # padding / canary words of the hand-written tables


def _p(a):
    return C.c_void_p(a.ctypes.data)


def u(*v):
    return np.array(v, dtype=np.uint64)


# ------------------------------------------------------------------ the models on hand-written 2 x 3 tables
def test_model_transpose_2x3():
    # two lines of three BFieldElements, one padding word per line -> three lines of two, two padding words per line
    src = u(1, 2, 3, X, 4, 5, 6, X)
    assert ref.transpose(src, 2, 3, 1, 4, np.full(12, 9, np.uint64), 4).tolist() == [1, 4, 9, 9, 2, 5, 9, 9, 3, 6, 9, 9]
    # exact strides; the last line may end the buffer
    assert ref.transpose(u(1, 2, 3, 4, 5, 6), 2, 3, 1, 3, np.zeros(6, np.uint64), 2).tolist() == [1, 4, 2, 5, 3, 6]
    # XFieldElements move as three words: 2 lines of 3 elements -> 3 lines of 2 elements
    src = np.arange(18, dtype=np.uint64)
    assert ref.transpose(src, 2, 3, 3, 9, np.zeros(18, np.uint64), 6).tolist() == [0, 1, 2, 9, 10, 11, 3, 4, 5, 12, 13, 14, 6, 7, 8, 15, 16, 17]
    # two matrices, n_outer * src_stride and n_inner * dst_stride apart
    src = u(1, 2, 3, 4, 5, 6, 11, 12, 13, 14, 15, 16)
    assert ref.transpose(src, 2, 3, 1, 3, np.zeros(12, np.uint64), 2, batch=2).tolist() == [1, 4, 2, 5, 3, 6, 11, 14, 12, 15, 13, 16]
    # there and back is the identity on the lines, and the padding of the first buffer is never looked at
    src = u(1, 2, 3, X, 4, 5, 6, X)
    back = ref.transpose(ref.transpose(src, 2, 3, 1, 4, np.zeros(8, np.uint64), 2), 3, 2, 1, 2, np.full(8, 9, np.uint64), 4)
    assert back.tolist() == [1, 2, 3, 9, 4, 5, 6, 9]


def test_model_fast_transpose_agrees_with_the_loops():
    rng = np.random.default_rng(5)
    for w in (1, 3):
        for n_outer, n_inner, ps, pd, batch in ((2, 3, 0, 0, 1), (5, 4, 1, 5, 2), (1, 7, 5, 1, 3), (7, 1, 0, 1, 1)):
            ss, ds = n_inner * w + ps, n_outer * w + pd
            src = rng.integers(0, 1 << 63, batch * n_outer * ss, dtype=np.uint64)
            before = rng.integers(0, 1 << 63, batch * n_inner * ds, dtype=np.uint64)
            assert np.array_equal(ref.transpose(src, n_outer, n_inner, w, ss, before, ds, batch), ref.transpose_fast(src, n_outer, n_inner, w, ss, before, ds, batch))


def test_model_gather_rows_2x3():
    # the 2 x 3 table [[1, 2, 3], [4, 5, 6]] in both layouts, one padding word per line
    cols = u(1, 4, X, 2, 5, X, 3, 6, X)
    rows = u(1, 2, 3, X, 4, 5, 6, X)
    before = np.full(16, 9, np.uint64)
    want = [4, 5, 6, 9, 1, 2, 3, 9, 4, 5, 6, 9, 9, 9, 9, 9]
    got, bad = ref.gather_rows(cols, ref.COLUMN_MAJOR, 2, 3, 1, 3, [1, 0, 1, 2], before, 4)
    assert got.tolist() == want and bad == [3]
    got, bad = ref.gather_rows(rows, ref.ROW_MAJOR, 2, 3, 1, 4, [1, 0, 1, 2], before, 4)
    assert got.tolist() == want and bad == [3]
    # 2^32 - 1 is an index like any other, and a bad row stays as it was in EVERY table
    two = np.concatenate([rows, rows + u(10)])
    got, bad = ref.gather_rows(two, ref.ROW_MAJOR, 2, 3, 1, 4, np.array([0xFFFFFFFF, 1], dtype=np.uint32), np.full(12, 9, np.uint64), 3, batch=2)
    assert got.tolist() == [9, 9, 9, 4, 5, 6, 9, 9, 9, 14, 15, 16] and bad == [0]
    # XFieldElements: the column-major source is one scattered element per output element
    xcols = np.arange(12, dtype=np.uint64)  # 2 columns of 2 elements of 3 words
    got, bad = ref.gather_rows(xcols, ref.COLUMN_MAJOR, 2, 2, 3, 6, [1], np.zeros(6, np.uint64), 6)
    assert got.tolist() == [3, 4, 5, 9, 10, 11] and bad == []


def test_model_lde_rows_2x3():
    # "extension" by repeating every value twice: columns of [[1, 2, 3], [4, 5, 6]] with a padding word on either side
    rows = u(1, 2, 3, X, 4, 5, 6, X)
    got = ref.lde_rows(lambda col: np.repeat(col, 2), rows, 2, 3, 1, 4, np.full(20, 9, np.uint64), 4, 5)
    assert got.tolist() == [1, 2, 3, 9, 9, 1, 2, 3, 9, 9, 4, 5, 6, 9, 9, 4, 5, 6, 9, 9]


def test_model_masks_and_spans():
    assert ref.span(3, 5, 2) == 12 and ref.span(0, 5, 2) == 0 and ref.span(3, 5, 0) == 0
    assert ref.line_mask(2, 3, 2).tolist() == [True, True, False, True, True]
    assert ref.line_mask(2, 3, 2, size=6).tolist() == [True, True, False, True, True, False]


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
    assert "#define TF_TABLE_COLUMN_MAJOR 0" in header and "#define TF_TABLE_ROW_MAJOR 1" in header
    assert lib.tf_version() == 1002  # new entry points are found by their symbols, not by a version bump
    assert "table" in tf.__all__ and "Table" in tf.__all__
    for name in PYTHON:
        assert callable(getattr(tf.table, name)), name
    for name in ("columns_to_rows", "rows_to_columns", "gather_rows"):
        assert callable(getattr(tf.Table, name)), name
    assert (tf.table.COLUMN_MAJOR, tf.table.ROW_MAJOR) == (0, 1) == (tf.Table.COLUMN_MAJOR, tf.Table.ROW_MAJOR)


@pytest.fixture
def bufs():
    return np.arange(1, 65, dtype=np.uint64), np.zeros(64, dtype=np.uint64), np.zeros(4, dtype=np.uint32), np.zeros(1, dtype=np.int32)


def _calls(lib, bufs, null=None, width=1, short=None, layout=0, n=4, cols=3, k=4, batch=1, off_in=7):
    """One call of every status-returning entry point as (name, number of pointers, thunk): a 4 x 3 table with valid arguments except
    for what is asked for.  null = index of the pointer argument to replace by NULL; short = index of the stride argument to make one
    word too short."""
    src, dst, idx, st = bufs

    def ptrs(*ps):
        return [None if null is not None and i == null else _p(p) for i, p in enumerate(ps)]

    def strides(*ss):
        return [s - 1 if short is not None and i == short else s for i, s in enumerate(ss)]

    w = width
    calls = []
    a, b = ptrs(src, dst)
    s1, s2 = strides(cols * w, n * w)
    calls.append(("tf_table_transpose", 2, lambda: lib.tf_table_transpose(a, n, cols, w, s1, b, s2, batch)))
    calls.append(("tf_table_transpose_dev", 2, lambda: lib.tf_table_transpose_dev(a, n, cols, w, s1, b, s2, batch, None)))
    t, ix, o, status = ptrs(src, idx, dst, st)
    g1, g2 = strides((cols if layout == 1 else n) * w, cols * w)
    calls.append(("tf_table_gather_rows", 3, lambda: lib.tf_table_gather_rows(t, layout, n, cols, w, g1, ix, k, o, g2, batch)))
    calls.append(("tf_table_gather_rows_dev", 4, lambda: lib.tf_table_gather_rows_dev(t, layout, n, cols, w, g1, ix, k, o, g2, batch, None, status)))
    r, lo = ptrs(src, dst)
    l1, l2 = strides(cols * w, cols * w)
    fn = {1: lib.tf_table_lde_rows_bfe_dev, 3: lib.tf_table_lde_rows_xfe_dev}.get(w)
    if fn is not None and layout in (0, 1) and batch == 1 and k == 4:  # (no width argument, no layout, one table, no index list)
        calls.append((fn.__name__, 2, lambda: fn(r, n, cols, l1, off_in, lo, 2 * n, l2, 7, 0, None)))
    return calls


def test_argument_errors_in_the_documented_order_without_device(tf, bufs):
    lib = tf.lib()
    no_gpu = lib.tf_device_count() == 0
    # 1. a NULL pointer, whichever it is -- also when a width, a stride or the layout is wrong and a length too large
    for null in range(4):
        for kw in ({}, {"width": 2}, {"short": 0}, {"short": 1}, {"layout": 2}, {"cols": BIG}, {"width": 4, "layout": 2, "short": 0, "cols": BIG}):
            for name, n_ptrs, call in _calls(lib, bufs, null=null, **kw):
                if null < n_ptrs:
                    assert call() == NULL, (name, null, kw)
    # 2. widths 0 / 2 / 4, strides one word short, layout 2 -- also when a length is too large
    for big in ({}, {"cols": BIG}, {"k": BIG}, {"batch": 1 << 36}):
        for width in (0, 2, 4, -1):
            for name, _, call in _calls(lib, bufs, width=width, **big):
                assert call() == INVALID, (name, width, big)
        for width in (1, 3):
            for short in (0, 1):
                for layout in (0, 1):
                    for name, _, call in _calls(lib, bufs, width=width, short=short, layout=layout, **big):
                        if not (name.startswith("tf_table_lde") and "cols" in big):  # (the LDE: its own order, below)
                            assert call() == INVALID, (name, width, short, layout, big)
        for layout in (2, -1, 3):
            for name, _, call in _calls(lib, bufs, layout=layout, **big):
                if "gather" in name:
                    assert call() == INVALID, (name, layout, big)
    # 3. lengths: 2^30 + 1 lines, elements, rows, columns or indices; more than 2^35 words moved
    src, dst, idx, st = (_p(b) for b in bufs)
    for fn, extra in ((lib.tf_table_transpose, ()), (lib.tf_table_transpose_dev, (None,))):
        assert fn(src, BIG, 3, 1, 3, dst, BIG, 1, *extra) == LEN_TOO_LARGE
        assert fn(src, 3, BIG, 1, BIG, dst, 3, 1, *extra) == LEN_TOO_LARGE
        if no_gpu:  # exactly 2^35 words are allowed
            assert fn(src, 1 << 18, 1 << 17, 1, 1 << 17, dst, 1 << 18, 1, *extra) == NO_DEVICE
        assert fn(src, 1 << 18, 1 << 17, 1, 1 << 17, dst, 1 << 18, 2, *extra) == LEN_TOO_LARGE                      # 2^36
        assert fn(src, 1 << 18, 1 << 17, 3, 3 << 17, dst, 3 << 18, 1, *extra) == LEN_TOO_LARGE                      # 3 * 2^35
        assert fn(src, 4, 3, 1, 3, dst, 4, (1 << 35) // 12 + 1, *extra) == LEN_TOO_LARGE
        assert fn(src, 4, 3, 1, 3, dst, 4, (1 << 64) - 1, *extra) == LEN_TOO_LARGE                                  # (no wrap-around)
        for huge in (1 << 39, 1 << 62, (1 << 64) - 1):  # an operand spanning more than 2^40 words: no wrap of span() or of the kernels' offsets
            assert fn(src, 4, 3, 1, huge, dst, 4, 1, *extra) == LEN_TOO_LARGE and fn(src, 4, 3, 1, 3, dst, huge, 1, *extra) == LEN_TOO_LARGE
        assert fn(src, 4, 3, 1, 1 << 20, dst, 4, 1 << 19, *extra) == LEN_TOO_LARGE       # batch * lines * stride
        if no_gpu:
            assert fn(src, 4, 3, 1, 1 << 38, dst, 1 << 38, 1, *extra) == NO_DEVICE       # exactly 2^40 and below are allowed
    for fn, extra in ((lib.tf_table_gather_rows, ()), (lib.tf_table_gather_rows_dev, (None, st))):
        for layout in (0, 1):
            for huge in (1 << 39, 1 << 62, (1 << 64) - 1):
                assert fn(src, layout, 4, 3, 1, huge, idx, 4, dst, 3, 1, *extra) == LEN_TOO_LARGE
                assert fn(src, layout, 4, 3, 1, 4, idx, 4, dst, huge, 1, *extra) == LEN_TOO_LARGE
            assert fn(src, layout, 4, 3, 1, 4, idx, 4, dst, 3, (1 << 38) + 1, *extra) == LEN_TOO_LARGE  # batch * lines wraps nothing either
            assert fn(src, layout, BIG, 3, 1, BIG if layout == 0 else 3, idx, 4, dst, 3, 1, *extra) == LEN_TOO_LARGE
            assert fn(src, layout, 4, BIG, 1, 4 if layout == 0 else BIG, idx, 4, dst, BIG, 1, *extra) == LEN_TOO_LARGE
            assert fn(src, layout, 4, 3, 1, 4 if layout == 0 else 3, idx, BIG, dst, 3, 1, *extra) == LEN_TOO_LARGE
            assert fn(src, layout, 4, 1 << 17, 1, 4 if layout == 0 else 1 << 17, idx, 1 << 18, dst, 1 << 17, 2, *extra) == LEN_TOO_LARGE
    # 4. a valid call, both widths and layouts: TF_ERR_NO_DEVICE without a GPU; with one, the host forms run
    for width in (1, 3):
        for layout in (0, 1):
            for name, _, call in _calls(lib, bufs, width=width, layout=layout):
                if no_gpu:
                    assert call() == NO_DEVICE, (name, width, layout)
                elif not name.endswith("_dev"):
                    assert call() == OK, (name, width, layout)
    if no_gpu:
        assert not bufs[1].any() and not bufs[3].any()


def test_lde_rows_keeps_the_argument_errors_of_lde_without_device(tf, bufs):
    lib = tf.lib()
    src, dst = _p(bufs[0]), _p(bufs[1])
    for fn, w in ((lib.tf_table_lde_rows_bfe_dev, 1), (lib.tf_table_lde_rows_xfe_dev, 3)):
        rs = 3 * w
        assert fn(src, 8, 3, rs, 7, dst, 4, rs, 7, 0, None) == NOT_ABOVE                      # m < n, before anything else
        assert fn(None, 8, 3, 0, 0, None, 4, 0, 7, 0, None) == NOT_ABOVE
        assert fn(src, 3, 3, rs, 7, dst, 8, rs, 7, 0, None) == NOT_POW2                       # n
        assert fn(src, 4, 3, rs, 7, dst, 12, rs, 7, 0, None) == NOT_POW2                      # m
        assert fn(src, 4, 3, rs, 7, dst, 1 << 32, rs, 7, 0, None) == LEN_TOO_LARGE            # the lengths of ntt.rs:134-139
        assert fn(None, 4, 3, rs, 7, dst, 8, rs, 7, 0, None) == NULL and fn(src, 4, 3, rs, 7, None, 8, rs, 7, 0, None) == NULL
        assert fn(src, 4, 3, rs, 0, dst, 8, rs, 7, 0, None) == INVERSE_OF_ZERO                # offset_in: its inverse scales the coefficients
        assert fn(src, 4, 3, rs - 1, 0, dst, 8, rs, 7, 0, None) == INVERSE_OF_ZERO            # ... before the table's own checks
        assert fn(src, 4, BIG, rs, 7, dst, 8, rs, 7, 0, None) == LEN_TOO_LARGE
        assert fn(src, 1 << 20, (1 << 15) + 1, rs << 15, 7, dst, 1 << 20, rs << 15, 7, 0, None) == LEN_TOO_LARGE   # more than 2^35 words of output
        for huge in (1 << 39, 1 << 62, (1 << 64) - 1):  # a stride whose lines span more than 2^40 words may not wrap the offsets
            assert fn(src, 4, 3, huge, 7, dst, 8, rs, 7, 0, None) == LEN_TOO_LARGE and fn(src, 4, 3, rs, 7, dst, 8, huge, 7, 0, None) == LEN_TOO_LARGE
        assert fn(src, 4, 3, rs - 1, 7, dst, 8, rs, 7, 0, None) == INVALID and fn(src, 4, 3, rs, 7, dst, 8, rs - 1, 7, 0, None) == INVALID
        # empty: no columns, or no output rows
        assert fn(None, 4, 0, 0, 0, None, 8, 0, 0, 0, None) == OK and fn(None, 0, 3, 0, 0, None, 0, 0, 0, 5, None) == OK
        if lib.tf_device_count() == 0:
            assert fn(src, 4, 3, rs, 7, dst, 8, rs, 0, 2, None) == NO_DEVICE                  # (offset_out may be zero, as for tf_lde_*_dev)
    assert not bufs[1].any()


def test_empty_calls_return_ok_and_touch_nothing(tf, bufs):
    lib = tf.lib()
    src, dst, idx, st = (_p(b) for b in bufs)
    for w in (1, 3, 2):  # (nothing is looked at when there is nothing to do)
        for n_outer, n_inner, batch in ((0, 3, 1), (4, 0, 1), (4, 3, 0), (0, 0, 0)):
            assert lib.tf_table_transpose(None, n_outer, n_inner, w, 0, None, 0, batch) == OK
            assert lib.tf_table_transpose_dev(None, n_outer, n_inner, w, 0, None, 0, batch, None) == OK
            assert lib.tf_table_transpose(src, n_outer, n_inner, w, 0, dst, 0, batch) == OK
        for layout in (0, 1, 2):
            for n_cols, k, batch in ((0, 4, 1), (3, 0, 1), (3, 4, 0)):
                assert lib.tf_table_gather_rows(None, layout, 4, n_cols, w, 0, None, k, None, 0, batch) == OK
                assert lib.tf_table_gather_rows_dev(None, layout, 4, n_cols, w, 0, None, k, None, 0, batch, None, None) == OK
                assert lib.tf_table_gather_rows_dev(src, layout, 4, n_cols, w, 0, idx, k, dst, 0, batch, None, st) == OK
    assert not bufs[1].any() and not bufs[3].any()


def test_lde_rows_workspace_rule(tf):
    ws = tf.lib().tf_table_lde_rows_workspace
    for n, m, n_cols, w, c in ((32, 128, 5, 1, 0), (32, 128, 5, 3, 2), (32, 128, 5, 3, 7), (1 << 18, 1 << 20, 64, 1, 0), (1 << 18, 1 << 20, 64, 3, 0),
                               (1 << 18, 1 << 20, 64, 1, 64), (1 << 18, 1 << 20, 64, 1, 1), (1 << 10, 1 << 10, 1 << 20, 1, 0), (0, 8, 3, 1, 0)):
        assert ws(n, m, n_cols, w, c) == ref.lde_workspace(n, m, n_cols, w, c) == tf.table.lde_rows_workspace(n, m, n_cols, w, c), (n, m, n_cols, w, c)
    # an empty table (no output rows) is an accepted call that takes nothing, whatever the block size asked for
    for w in (1, 3):
        for c in (0, 1, 3, 7):
            assert ws(0, 0, 3, w, c) == 0 == ref.lde_workspace(0, 0, 3, w, c) == tf.table.lde_rows_workspace(0, 0, 3, w, c), (w, c)
    # more than 2^35 words of output are rejected, so the product behind the result cannot wrap
    assert ws(1 << 20, 1 << 20, 1 << 15, 1, 1 << 15) == (1 << 15) * (2 << 20) * 8 and ws(1 << 20, 1 << 20, (1 << 15) + 1, 1, 0) == 0
    assert ws(1 << 31, 1 << 31, 1 << 30, 3, 1 << 30) == 0
    per = lambda n, m, w: (n + m) * w * 8  # noqa: E731  bytes of the two temporaries per column
    # below the 256 MiB bound every column fits in one block; a request above n_cols means n_cols
    assert ws(32, 128, 5, 1, 0) == 5 * per(32, 128, 1) == ws(32, 128, 5, 1, 5) == ws(32, 128, 5, 1, 7) == ws(32, 128, 5, 1, 1 << 40)
    assert ws(32, 128, 5, 3, 2) == 2 * per(32, 128, 3)
    # above it: 2^18 -> 2^20 is 10 MiB per BFieldElement column, so 25 columns (250 MiB; 26 would be 260), 8 XFieldElement columns
    assert ws(1 << 18, 1 << 20, 64, 1, 0) == 25 * per(1 << 18, 1 << 20, 1) <= 256 << 20 < 26 * per(1 << 18, 1 << 20, 1)
    assert ws(1 << 18, 1 << 20, 64, 3, 0) == 8 * per(1 << 18, 1 << 20, 3)
    assert ws(1 << 18, 1 << 20, 25, 1, 0) == ws(1 << 18, 1 << 20, 26, 1, 0) == 25 * per(1 << 18, 1 << 20, 1) and ws(1 << 18, 1 << 20, 24, 1, 0) == 24 * per(1 << 18, 1 << 20, 1)
    # exactly at the bound: 2^22 -> 2^22 is 64 MiB per column, four columns are 256 MiB
    assert ws(1 << 22, 1 << 22, 9, 1, 0) == 256 << 20
    # one column is taken even when it alone exceeds the bound
    assert ws(1 << 25, 1 << 25, 9, 1, 0) == per(1 << 25, 1 << 25, 1) > 256 << 20
    # an explicit request is not bounded
    assert ws(1 << 18, 1 << 20, 64, 1, 64) == 64 * per(1 << 18, 1 << 20, 1)
    # 0 for arguments the call rejects
    for args in ((32, 128, 5, 2, 0), (32, 128, 5, 0, 0), (128, 32, 5, 1, 0), (3, 8, 5, 1, 0), (4, 12, 5, 1, 0), (4, 1 << 32, 5, 1, 0), (32, 128, BIG, 1, 0), (32, 128, 0, 1, 0)):
        assert ws(*args) == 0, args


def test_python_shapes_are_checked_on_the_host(tf):
    z = np.zeros(12, dtype=np.uint64)
    with pytest.raises(ValueError):
        tf.Table.columns_to_rows(z, 4, 3, width=2)
    with pytest.raises(ValueError):
        tf.Table.columns_to_rows(z, 4, 3, col_stride=3)
    with pytest.raises(ValueError):
        tf.Table.rows_to_columns(z, 4, 3, col_stride=3)
    with pytest.raises(ValueError):
        tf.Table.columns_to_rows(z, 4, 4)          # the table holds 12 words
    with pytest.raises(ValueError):
        tf.Table.gather_rows(z, 4, 3, [0], layout=2)
    with pytest.raises(ValueError):
        tf.Table.gather_rows(z, 4, 3, [0], stride=3)  # column-major: a column is 4 words
    with pytest.raises(ValueError):
        tf.Table.gather_rows(z, 4, 3, [0], batch=2)
    with pytest.raises(TypeError):
        tf.Table.columns_to_rows(z.astype(np.int64), 4, 3)
    # empty tables never reach a device
    e = np.zeros(0, dtype=np.uint64)
    assert tf.Table.columns_to_rows(e, 0, 3).size == 0 and tf.Table.rows_to_columns(e, 4, 0).size == 0
    assert tf.Table.gather_rows(z, 4, 3, []).shape == (1, 0, 3) and tf.Table.gather_rows(e, 4, 0, [1, 2]).shape == (1, 2, 0)


# ------------------------------------------------------------------ the fence rows of tests/test_gpu_table.py are complete
# public callables of table.py that need no row, each with its reason
NOT_FENCED = {"lde_rows_workspace": "host arithmetic: no tensor"}


def test_every_public_callable_of_table_py_has_a_fence_row(tf):
    from tests import test_gpu_table

    names = [n for n, f in vars(tf.table).items() if not n.startswith("_") and inspect.isfunction(f) and f.__module__ == tf.table.__name__]
    assert sorted(names) == sorted(PYTHON)
    rows = set(test_gpu_table.ROWS)
    missing = [n for n in names if n not in rows and n not in NOT_FENCED]
    assert not missing, f"table.py callables without a fence row in tests/test_gpu_table.py (or a reasoned exclusion here): {missing}"
    assert not rows & set(NOT_FENCED), "a callable is both fenced and excluded"
    stale = [n for n in list(rows) + list(NOT_FENCED) if n not in names]
    assert not stale, f"rows or exclusions that name nothing in table.py: {stale}"
