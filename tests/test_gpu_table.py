"""Table transposes, row opening and the row-major LDE on the GPU (twenty_first_amd/table.py, tf_table_*), compared word for word
with tests/table_ref (pinned to hand-written tables by tests/test_table_cpu.py) or with the oracle.

Whole buffers are compared: every destination starts as canary words, the models carry the words between a line's end and its stride
through untouched, so a store into padding shows as a mismatch like any wrong word.

The transpose stages TILE x TILE elements per step (csrc/table_kernels.h): TILE = 64 for width 1 and 32 for width 3.  The issue's
sizes {1, 2, 63, 64, 65, 129} are one below, at and one above the tile edge and two tiles plus one for width 1; for width 3 they are
adjusted to its tile: {1, 2, 31, 32, 33, 65}.  One more shape has more tiles than the launch has workgroups (eight per compute unit),
so that the grid-stride loop wraps."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import fence, table_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE = {1: 64, 3: 32}  # tfk::TableTile<W>::TILE
SIZES = {w: (1, 2, t - 1, t, t + 1, 2 * t + 1) for w, t in TILE.items()}
PADS = (0, 1, 5)
CANARY = np.uint64(0xC0FFEE0000C0FFEE)
INVALID = 17
ROWS = {}  # the fence rows: callable of table.py -> (cases, generator of (shape, operands, call)), as tests/test_gpu_fences.py


def _need_gpu(tf):
    assert tf.lib().tf_device_count() > 0, "no HIP device visible: the product has no CPU fallback"


def _to_dev(a):
    import torch

    a = np.ascontiguousarray(a) if a.flags.writeable else np.array(a)  # (torch wants a writable array; the pool of words is read-only)
    return torch.from_numpy(a.view(np.int64 if a.dtype == np.uint64 else np.int32)).cuda()


def _to_host(t):
    return t.cpu().numpy().view(np.uint64)


def _p(a):
    return C.c_void_p(a.ctypes.data)


def _status(v=0):
    import torch

    return torch.full((1,), v, dtype=torch.int32, device="cuda")


def _canary(words):
    return np.full(words, CANARY, dtype=np.uint64)


def _cus():
    import torch

    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.fixture(scope="module")
def words(oracle):
    """one pool of canonical random words, computed once and only read: every test cuts its tables out of it"""
    w = oracle.fill_random(1 << 20, 0x7AB1E)
    w.setflags(write=False)
    return w


# ------------------------------------------------------------------ 1. transpose
def _transpose_both_forms(tf, src, n_outer, n_inner, w, ss, ds, batch):
    """the _dev form and the host form on one source: each must leave exactly the model's buffer"""
    before = _canary(batch * n_inner * ds)
    want = ref.transpose_fast(src, n_outer, n_inner, w, ss, before, ds, batch)
    d_dst = _to_dev(before)
    tf.table.transpose(_to_dev(src), n_outer, n_inner, d_dst, width=w, src_stride=ss, dst_stride=ds, batch=batch)
    got = _to_host(d_dst)
    assert np.array_equal(got, want), ("dev", n_outer, n_inner, w, ss, ds, batch, int(np.flatnonzero(got != want)[0]))
    host = before.copy()
    src = np.ascontiguousarray(src)
    assert tf.lib().tf_table_transpose(_p(src), n_outer, n_inner, w, ss, _p(host), ds, batch) == 0
    assert np.array_equal(host, want), ("host", n_outer, n_inner, w, ss, ds, batch, int(np.flatnonzero(host != want)[0]))
    return want


@pytest.mark.gpu
@pytest.mark.parametrize("w,n_outer", [(w, n) for w in (1, 3) for n in SIZES[w]])
def test_transpose_tile_edges_strides_and_batches(tf, words, w, n_outer):
    _need_gpu(tf)
    for n_inner in SIZES[w]:
        for ps in PADS:
            for pd in PADS:
                for batch in (1, 3):
                    ss, ds = n_inner * w + ps, n_outer * w + pd
                    _transpose_both_forms(tf, words[:batch * n_outer * ss], n_outer, n_inner, w, ss, ds, batch)


@pytest.mark.gpu
@pytest.mark.parametrize("w", [1, 3])
def test_transpose_round_trip_is_the_identity(tf, words, w):
    _need_gpu(tf)
    t = TILE[w]
    for n_rows, n_cols, pc, pr, batch in ((2 * t + 1, t + 1, 5, 1, 3), (t - 1, 7, 0, 0, 1), (5, 3 * t + 2, 1, 5, 2)):
        cs, rs = n_rows * w + pc, n_cols * w + pr
        table = words[:batch * n_cols * cs]
        d_table, d_rows, d_back = _to_dev(table), _to_dev(_canary(batch * n_rows * rs)), _to_dev(_canary(batch * n_cols * cs))
        tf.table.columns_to_rows(d_table, n_rows, n_cols, d_rows, width=w, col_stride=cs, row_stride=rs, batch=batch)
        tf.table.rows_to_columns(d_rows, n_rows, n_cols, d_back, width=w, row_stride=rs, col_stride=cs, batch=batch)
        lines = ref.line_mask(batch * n_cols, cs, n_rows * w, size=table.size)
        back = _to_host(d_back)
        assert np.array_equal(back[lines], table[lines]) and (back[~lines] == CANARY).all()
        assert np.array_equal(_to_host(d_rows), ref.transpose_fast(table, n_cols, n_rows, w, cs, _canary(batch * n_rows * rs), rs, batch))
        # the numpy host API: exact strides out, zero padding where a stride is asked for
        rows = tf.Table.columns_to_rows(np.ascontiguousarray(table), n_rows, n_cols, width=w, col_stride=cs, batch=batch)
        assert np.array_equal(rows, ref.transpose_fast(table, n_cols, n_rows, w, cs, np.zeros(batch * n_rows * n_cols * w, np.uint64), n_cols * w, batch))
        cols = tf.Table.rows_to_columns(rows, n_rows, n_cols, width=w, col_stride=cs, batch=batch)
        assert np.array_equal(cols[lines], table[lines]) and not cols[~lines].any()


@pytest.mark.gpu
@pytest.mark.parametrize("w", [1, 3])
def test_transpose_more_tiles_than_workgroups(tf, words, w):
    """the grid-stride loop over (tile, matrix): a launch has at most eight workgroups per compute unit"""
    _need_gpu(tf)
    tiles = 8 * _cus() + 3
    n_inner, n_outer = (tiles // 2) * TILE[w] + 5, 2
    assert (tiles // 2) * 2 > 8 * _cus() and 4 * (n_inner * w + 1) <= words.size
    _transpose_both_forms(tf, words[:4 * (n_inner * w + 1)], n_outer, n_inner, w, n_inner * w + 1, n_outer * w + 1, 2)
    _transpose_both_forms(tf, words[:2 * n_inner * (n_outer * w + 1)], n_inner, n_outer, w, n_outer * w + 1, n_inner * w + 1, 2)


@pytest.mark.gpu
def test_python_wrapper_checks_shapes_and_overlap(tf):
    import torch

    _need_gpu(tf)
    z = torch.zeros(24, dtype=torch.int64, device="cuda")
    o = torch.zeros(24, dtype=torch.int64, device="cuda")
    with pytest.raises(ValueError):
        tf.table.transpose(z, 4, 3, o, width=2)
    with pytest.raises(ValueError):
        tf.table.transpose(z, 4, 3, o, src_stride=2)
    with pytest.raises(ValueError):
        tf.table.transpose(z, 4, 7, o)            # src holds 24 words
    with pytest.raises(ValueError):
        tf.table.transpose(z, 4, 3, z[12:])       # dst overlaps src
    with pytest.raises(ValueError):
        tf.table.transpose(z, 4, 3, z)
    with pytest.raises(ValueError):
        tf.table.gather_rows(z, 4, 3, torch.zeros(2, dtype=torch.int32, device="cuda"), o, layout=2)
    with pytest.raises(ValueError):
        tf.table.gather_rows(z, 4, 3, torch.zeros(9, dtype=torch.int32, device="cuda"), o)  # out holds 8 rows
    idx = torch.zeros(2, dtype=torch.int32, device="cuda")
    st = torch.zeros(1, dtype=torch.int32, device="cuda")
    with pytest.raises(ValueError):
        tf.table.gather_rows(z, 4, 3, o.view(torch.int32)[4:6], o)           # the index list lies inside out
    with pytest.raises(ValueError):
        tf.table.gather_rows(z, 4, 3, idx, o, status=o.view(torch.int32)[7:8])  # ... the status word inside out
    with pytest.raises(ValueError):
        tf.table.gather_rows(z, 4, 3, idx, o, status=z.view(torch.int32)[0:1])  # ... inside the table
    with pytest.raises(ValueError):
        tf.table.gather_rows(z, 4, 3, idx, o, status=idx[1:2])                  # ... inside the index list
    tf.table.gather_rows(z, 4, 3, idx, o, status=st)                            # apart: accepted
    torch.cuda.synchronize()
    assert int(st.item()) == 0
    with pytest.raises(ValueError):
        tf.table.lde_rows(z, 4, 3, 7, o, 16, 7)   # out holds 8 rows of 3
    with pytest.raises(ValueError):
        tf.table.lde_rows(z, 4, 3, 7, z, 8, 7)


# ------------------------------------------------------------------ 2. gather_rows
N_ROWS = 301  # odd, and not a multiple of anything the kernel counts in


def _table(words, layout, n_rows, n_cols, w, pad, batch):
    lines, line = (n_rows, n_cols * w) if layout == ref.ROW_MAJOR else (n_cols, n_rows * w)
    stride = line + pad
    return words[:batch * lines * stride], stride


@pytest.mark.gpu
@pytest.mark.parametrize("layout,w", [(layout, w) for layout in (ref.COLUMN_MAJOR, ref.ROW_MAJOR) for w in (1, 3)])
def test_gather_rows_both_layouts(tf, words, layout, w):
    _need_gpu(tf)
    rng = np.random.default_rng(100 * layout + w)
    for n_cols in (1, 17, 200):  # 200 elements: far beyond the 16 words of gather_elements
        for k in (1, 64, 257):
            for batch in (1, 2):
                table, stride = _table(words, layout, N_ROWS, n_cols, w, 3, batch)
                idx = rng.integers(0, N_ROWS, size=k).astype(np.uint32)
                idx[k // 2] = idx[0]  # a repeat
                os_ = n_cols * w + 2
                before = _canary(batch * k * os_)
                want, bad = ref.gather_rows(table, layout, N_ROWS, n_cols, w, stride, idx, before, os_, batch)
                assert not bad
                d_out, st = _to_dev(before), _status()
                tf.table.gather_rows(_to_dev(table), N_ROWS, n_cols, _to_dev(idx.view(np.int32)), d_out, layout=layout, width=w, stride=stride,
                                     out_stride=os_, batch=batch, status=st)
                assert np.array_equal(_to_host(d_out), want) and int(st.item()) == 0, (n_cols, k, batch)
                host = before.copy()
                t = np.ascontiguousarray(table)
                assert tf.lib().tf_table_gather_rows(_p(t), layout, N_ROWS, n_cols, w, stride, _p(idx), k, _p(host), os_, batch) == 0
                assert np.array_equal(host, want), (n_cols, k, batch)
                got = tf.Table.gather_rows(t, N_ROWS, n_cols, idx, layout=layout, width=w, stride=stride, batch=batch)
                assert np.array_equal(got.reshape(-1), want.reshape(batch * k, os_)[:, :n_cols * w].reshape(-1))


@pytest.mark.gpu
@pytest.mark.parametrize("layout,w", [(layout, w) for layout in (ref.COLUMN_MAJOR, ref.ROW_MAJOR) for w in (1, 3)])
def test_gather_rows_bad_indices_leave_their_slots_and_raise_17(tf, words, layout, w):
    _need_gpu(tf)
    n_cols, k, batch = 17, 64, 2
    table, stride = _table(words, layout, N_ROWS, n_cols, w, 3, batch)
    idx = np.random.default_rng(7).integers(0, N_ROWS, size=k).astype(np.uint32)
    idx[5], idx[40] = N_ROWS, 0xFFFFFFFF
    os_ = n_cols * w + 2
    before = _canary(batch * k * os_)
    want, bad = ref.gather_rows(table, layout, N_ROWS, n_cols, w, stride, idx, before, os_, batch)
    assert bad == [5, 40]
    for t in range(batch):
        for q in bad:
            assert (want[(t * k + q) * os_:(t * k + q + 1) * os_] == CANARY).all()  # as it was, in every table
    d_table, d_idx, d_out, st = _to_dev(table), _to_dev(idx.view(np.int32)), _to_dev(before), _status()
    kw = dict(layout=layout, width=w, stride=stride, out_stride=os_, batch=batch)
    tf.table.gather_rows(d_table, N_ROWS, n_cols, d_idx, d_out, status=st, **kw)
    assert np.array_equal(_to_host(d_out), want) and int(st.item()) == INVALID
    # the status word is never cleared: a later good call leaves the 17
    good = _to_dev((idx % N_ROWS).astype(np.uint32).view(np.int32))
    tf.table.gather_rows(d_table, N_ROWS, n_cols, good, d_out, status=st, **kw)
    assert int(st.item()) == INVALID
    assert np.array_equal(_to_host(d_out), ref.gather_rows(table, layout, N_ROWS, n_cols, w, stride, idx % N_ROWS, before, os_, batch)[0])
    # the first non-zero code stays
    other = _status(12)
    tf.table.gather_rows(d_table, N_ROWS, n_cols, d_idx, _to_dev(before), status=other, **kw)
    assert int(other.item()) == 12
    # without a status word the wrapper raises after one synchronisation; the rows are written all the same
    d_out2 = _to_dev(before)
    with pytest.raises(tf.TwentyFirstError) as e:
        tf.table.gather_rows(d_table, N_ROWS, n_cols, d_idx, d_out2, **kw)
    assert e.value.code == INVALID and np.array_equal(_to_host(d_out2), want)
    # the host form returns the code; its other rows are correct too
    host = before.copy()
    t = np.ascontiguousarray(table)
    assert tf.lib().tf_table_gather_rows(_p(t), layout, N_ROWS, n_cols, w, stride, _p(idx), k, _p(host), os_, batch) == INVALID
    assert np.array_equal(host, want)
    with pytest.raises(tf.TwentyFirstError):
        tf.Table.gather_rows(t, N_ROWS, n_cols, idx, layout=layout, width=w, stride=stride, batch=batch)


@pytest.mark.gpu
def test_gather_rows_more_words_than_threads_in_the_launch(tf, words):
    """the grid-stride loop over the words of out: a launch has at most eight workgroups of 256 threads per compute unit"""
    _need_gpu(tf)
    n_rows, n_cols = 1000, 200
    k = 8 * _cus() * 256 // n_cols + 77
    idx = np.random.default_rng(9).integers(0, n_rows, size=k).astype(np.uint32)
    for layout in (ref.COLUMN_MAJOR, ref.ROW_MAJOR):
        table = words[:n_rows * n_cols]
        rows = table.reshape(n_rows, n_cols) if layout == ref.ROW_MAJOR else table.reshape(n_cols, n_rows).T
        d_out = _to_dev(_canary(k * n_cols))
        tf.table.gather_rows(_to_dev(table), n_rows, n_cols, _to_dev(idx.view(np.int32)), d_out, layout=layout)
        assert np.array_equal(_to_host(d_out).reshape(k, n_cols), rows[idx.astype(np.int64)])


@pytest.mark.gpu
@pytest.mark.parametrize("layout", [ref.COLUMN_MAJOR, ref.ROW_MAJOR])
def test_gather_rows_takes_a_sponge_s_sampled_indices(tf, oracle, words, layout):
    _need_gpu(tf)
    import torch

    n_rows, n_cols, w, k = 256, 17, 3, 40
    table, stride = _table(words, layout, n_rows, n_cols, w, 3, 1)
    states = _to_dev(oracle.fill_random(16, 0x5B0))
    d_idx = torch.zeros(k, dtype=torch.int32, device="cuda")
    tf.device.tip5_sponge_sample_indices(states, n_rows, d_idx)  # straight from the sampler: never through the host
    d_out = _to_dev(_canary(k * n_cols * w))
    tf.table.gather_rows(_to_dev(table), n_rows, n_cols, d_idx, d_out, layout=layout, width=w, stride=stride)
    idx = d_idx.cpu().numpy()
    assert len(set(idx.tolist())) > 1 and (idx >= 0).all() and (idx < n_rows).all()
    want, bad = ref.gather_rows(table, layout, n_rows, n_cols, w, stride, idx, _canary(k * n_cols * w), n_cols * w)
    assert not bad and np.array_equal(_to_host(d_out), want)


# ------------------------------------------------------------------ 3. the chain through the existing entry points
@pytest.mark.gpu
@pytest.mark.parametrize("w", [1, 3])
def test_commit_and_open_chain(tf, oracle, words, w):
    """64 rows x 7 columns, padded col_stride: the row-major rows commit to the tree the column-major table commits to, and the rows
    opened from the column-major table hash to that tree's leafs"""
    _need_gpu(tf)
    d = tf.device
    n_rows, n_cols = 64, 7
    cs = n_rows * w + 5
    table = words[:n_cols * cs]
    d_table = _to_dev(table)
    nodes_cols, nodes_rows = _to_dev(_canary(n_rows * 10)), _to_dev(_canary(n_rows * 10))
    d.merkle_from_columns(d_table, n_rows, n_cols, nodes_cols, width=w, col_stride=cs)
    d_rows = _to_dev(_canary(n_rows * n_cols * w))
    tf.table.columns_to_rows(d_table, n_rows, n_cols, d_rows, width=w, col_stride=cs)
    d.merkle_from_rows(d_rows, n_cols * w, n_rows, nodes_rows)
    rows = ref.transpose(table, n_cols, n_rows, w, cs, np.zeros(n_rows * n_cols * w, np.uint64), n_cols * w)
    assert np.array_equal(_to_host(d_rows), rows)
    nodes = _to_host(nodes_cols)
    assert np.array_equal(_to_host(nodes_rows)[5:], nodes[5:])  # (node 0 of the heap is not part of the tree)
    leafs = oracle.hash_varlen_rows(rows, n_cols * w).reshape(n_rows, 5)
    assert np.array_equal(nodes.reshape(2 * n_rows, 5)[n_rows:], leafs)
    idx = np.array([63, 0, 17, 17, 32, 1], dtype=np.uint32)
    d_open, d_digests = _to_dev(_canary(idx.size * n_cols * w)), _to_dev(_canary(idx.size * 5))
    tf.table.gather_rows(d_table, n_rows, n_cols, _to_dev(idx.view(np.int32)), d_open, width=w, stride=cs)
    d.tip5_hash_varlen_rows(d_open, n_cols * w, d_digests)
    assert np.array_equal(_to_host(d_digests).reshape(-1, 5), nodes.reshape(2 * n_rows, 5)[n_rows + idx.astype(np.int64)])


# ------------------------------------------------------------------ 4. lde_rows
LDE = dict(n=32, m=128, n_cols=5)


@pytest.fixture(scope="module")
def lde_cases(oracle, words):
    """(rows, strides, expected buffer) per width, from oracle.coset_interpolate + oracle.coset_evaluate column by column: computed once"""
    n, m, n_cols = LDE["n"], LDE["m"], LDE["n_cols"]
    off_in, off_out = oracle.bfe_new(7), oracle.bfe_new(49)
    cases = {}
    for w in (1, 3):
        si, so = n_cols * w + 1, n_cols * w + 5
        rows = words[1000:1000 + n * si]
        column = lambda v, w=w: oracle.coset_evaluate(oracle.coset_interpolate(v, off_in, width=w), off_out, m, width=w)  # noqa: E731
        want = ref.lde_rows(column, rows, n, n_cols, w, si, _canary(m * so), m, so)
        want.setflags(write=False)
        cases[w] = (rows, si, so, off_in, off_out, want)
    return cases


@pytest.mark.gpu
@pytest.mark.parametrize("w", [1, 3])
def test_lde_rows_every_block_size_gives_the_oracle_s_words(tf, lde_cases, w):
    _need_gpu(tf)
    n, m, n_cols = LDE["n"], LDE["m"], LDE["n_cols"]
    rows, si, so, off_in, off_out, want = lde_cases[w]
    d_rows = _to_dev(rows)
    for c in (0, 1, 2, 5, 7):
        d_out = _to_dev(_canary(m * so))
        tf.table.lde_rows(d_rows, n, n_cols, off_in, d_out, m, off_out, width=w, row_stride_in=si, row_stride_out=so, cols_per_block=c)
        got = _to_host(d_out)
        assert np.array_equal(got, want), (w, c, int(np.flatnonzero(got != want)[0]))
    assert np.array_equal(_to_host(d_rows), rows)


# ------------------------------------------------------------------ 5. fence rows: one per callable of table.py
def row(name, cases):
    def register(gen):
        assert name not in ROWS, name
        ROWS[name] = (list(cases), gen)
        return gen
    return register


def _rnd(oracle, count, seed):
    return oracle.fill_random(count, seed)


def _transpose_ops(oracle, n_outer, n_inner, w, ps, pd, batch, names=("src", "dst")):
    ss, ds = n_inner * w + ps, n_outer * w + pd
    src = _rnd(oracle, batch * n_outer * ss, 0x7A00 + n_outer + n_inner)
    want = ref.transpose_fast(src, n_outer, n_inner, w, ss, np.zeros(batch * n_inner * ds, np.uint64), ds, batch)
    ops = [fence.inp(names[0], src, padding=~ref.line_mask(batch * n_outer, ss, n_inner * w, size=src.size)),
           fence.out(names[1], want, kept=~ref.line_mask(batch * n_inner, ds, n_outer * w, size=want.size))]
    return ops, ss, ds


def _fence_shapes(w):
    t = TILE[w]
    return [(1, 1), (t - 1, t + 1), (t, t), (2 * t + 1, 3), (7, 2 * t + 1)]


@row("transpose", cases=[(w, ps, pd, batch) for w in (1, 3) for ps, pd, batch in ((0, 0, 1), (1, 5, 2), (5, 1, 3))])
def _fence_transpose(tf, oracle, t, w, ps, pd, batch):
    for n_outer, n_inner in _fence_shapes(w):
        ops, ss, ds = _transpose_ops(oracle, n_outer, n_inner, w, ps, pd, batch)
        yield (f"w={w} {n_outer}x{n_inner} pads=({ps},{pd}) batch={batch}", ops,
               lambda src, dst, a=(n_outer, n_inner, ss, ds): t.transpose(src, a[0], a[1], dst, width=w, src_stride=a[2], dst_stride=a[3], batch=batch))


@row("columns_to_rows", cases=[(w, ps, pd, batch) for w in (1, 3) for ps, pd, batch in ((0, 0, 1), (5, 1, 2))])
def _fence_columns_to_rows(tf, oracle, t, w, ps, pd, batch):
    for n_cols, n_rows in _fence_shapes(w):
        ops, cs, rs = _transpose_ops(oracle, n_cols, n_rows, w, ps, pd, batch, names=("table", "rows_out"))
        yield (f"w={w} rows={n_rows} cols={n_cols} pads=({ps},{pd}) batch={batch}", ops,
               lambda table, rows_out, a=(n_rows, n_cols, cs, rs): t.columns_to_rows(table, a[0], a[1], rows_out, width=w, col_stride=a[2], row_stride=a[3], batch=batch))


@row("rows_to_columns", cases=[(w, ps, pd, batch) for w in (1, 3) for ps, pd, batch in ((0, 0, 1), (1, 5, 2))])
def _fence_rows_to_columns(tf, oracle, t, w, ps, pd, batch):
    for n_rows, n_cols in _fence_shapes(w):
        ops, rs, cs = _transpose_ops(oracle, n_rows, n_cols, w, ps, pd, batch, names=("rows", "table_out"))
        yield (f"w={w} rows={n_rows} cols={n_cols} pads=({ps},{pd}) batch={batch}", ops,
               lambda rows, table_out, a=(n_rows, n_cols, rs, cs): t.rows_to_columns(rows, a[0], a[1], table_out, width=w, row_stride=a[2], col_stride=a[3], batch=batch))


@row("gather_rows", cases=[(layout, w, batch) for layout in (ref.COLUMN_MAJOR, ref.ROW_MAJOR) for w in (1, 3) for batch in (1, 2)])
def _fence_gather_rows(tf, oracle, t, layout, w, batch):
    n_rows = 40
    for n_cols, k, pad in ((1, 1, 0), (17, 65, 3), (200, 9, 1)):
        lines, line = (n_rows, n_cols * w) if layout == ref.ROW_MAJOR else (n_cols, n_rows * w)
        stride, os_ = line + pad, n_cols * w + pad
        table = _rnd(oracle, batch * lines * stride, 0x7B00 + n_cols)
        idx = np.random.default_rng(k).integers(0, n_rows, size=k).astype(np.uint32)
        zeros = np.zeros(batch * k * os_, np.uint64)
        tab = fence.inp("table", table, padding=~ref.line_mask(batch * lines, stride, line, size=table.size))
        pad_mask = ~ref.line_mask(batch * k, os_, n_cols * w, size=zeros.size)
        call = lambda table, indices, out, status, a=(n_cols, stride, os_): t.gather_rows(  # noqa: E731
            table, n_rows, a[0], indices, out, layout=layout, width=w, stride=a[1], out_stride=a[2], batch=batch, status=status)
        want, bad = ref.gather_rows(table, layout, n_rows, n_cols, w, stride, idx, zeros, os_, batch)
        assert not bad
        yield (f"layout={layout} w={w} cols={n_cols} k={k} batch={batch}",
               [tab, fence.inp("indices", idx, dtype="int32"), fence.out("out", want, kept=pad_mask),
                fence.out("status", np.zeros(1, np.int32), dtype="int32", kept=[True])], call)
        # one index == n_rows: 17 in the status, and its row stays as it was in every table
        idx = idx.copy()
        idx[k // 2] = n_rows
        want, bad = ref.gather_rows(table, layout, n_rows, n_cols, w, stride, idx, zeros, os_, batch)
        kept = pad_mask.copy()
        for tb in range(batch):
            kept[(tb * k + bad[0]) * os_:(tb * k + bad[0] + 1) * os_] = True
        yield (f"layout={layout} w={w} cols={n_cols} k={k} batch={batch} index {k // 2} out of range",
               [tab, fence.inp("indices", idx, dtype="int32"), fence.out("out", want, kept=kept),
                fence.inout("status", np.zeros(1, np.int32), np.array([INVALID], np.int32), dtype="int32")], call)


@row("lde_rows", cases=[(w, c) for w in (1, 3) for c in (0, 2)])
def _fence_lde_rows(tf, oracle, t, w, c):
    n, m, n_cols = 8, 32, 5
    off_in, off_out = oracle.bfe_new(7), oracle.bfe_new(3)
    column = lambda v: oracle.coset_evaluate(oracle.coset_interpolate(v, off_in, width=w), off_out, m, width=w)  # noqa: E731
    for pi, po in ((0, 0), (1, 5)):
        si, so = n_cols * w + pi, n_cols * w + po
        rows = _rnd(oracle, n * si, 0x7C00 + w)
        want = ref.lde_rows(column, rows, n, n_cols, w, si, np.zeros(m * so, np.uint64), m, so)
        yield (f"w={w} cols_per_block={c} pads=({pi},{po})",
               [fence.inp("rows", rows, padding=~ref.line_mask(n, si, n_cols * w, size=rows.size)),
                fence.out("out", want, kept=~ref.line_mask(m, so, n_cols * w, size=want.size))],
               lambda rows, out, a=(si, so): t.lde_rows(rows, n, n_cols, off_in, out, m, off_out, width=w, row_stride_in=a[0], row_stride_out=a[1],
                                                        cols_per_block=c))


def _ids():
    return [pytest.param(name, case, id=f"{name}-{k}") for name in ROWS for k, case in enumerate(ROWS[name][0])]


@pytest.mark.gpu
@pytest.mark.parametrize("name,case", _ids())
def test_fenced(tf, oracle, name, case):
    _need_gpu(tf)
    _, gen = ROWS[name]
    for shape, operands, call in gen(tf, oracle, tf.table, *case):
        fence.run(name, shape, operands, call)


# ------------------------------------------------------------------ 6. the C++ mirror
@pytest.mark.gpu
def test_cpp_mirror_table_selftest_runs():
    host = os.path.join(ROOT, "twenty-first_amd", "host")
    subprocess.check_call(["make", "-C", host, "table_selftest"], stdout=subprocess.DEVNULL)
    r = subprocess.run(["timeout", "-k", "10", "120", os.path.join(host, "table_selftest")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("PASS") >= 4 and "FAIL" not in r.stdout, r.stdout
