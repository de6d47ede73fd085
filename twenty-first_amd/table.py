"""Tables on the device: the transposes between the column-major and the row-major layout, row opening and the row-major
low-degree extension (include/tf_hip.h, "Tables").

The device-pointer API of device.py for whole tables: 1-D contiguous int64 / uint64 CUDA tensors of raw Montgomery words, work
enqueued on torch's current stream (or the given one) and NOT synchronised here.  An element is `width` words; strides count words.

    column-major   column j = n_rows elements at table[j * col_stride:], col_stride >= n_rows * width; tables n_cols * col_stride apart
    row-major      row i = n_cols elements at rows[i * row_stride:], row_stride >= n_cols * width; tables n_rows * row_stride apart

A stride left as None is the exact one.  Words between the end of a line and its stride are never read in a source and never written
in a destination; a tensor may end with the last line (the padding behind it need not exist).
"""
from __future__ import annotations

import ctypes as C

from . import _lib
from .device import _apart, _chk, _need, _own_status, _p, _raise_own_status, _status, _stream, _t, _width

COLUMN_MAJOR = 0
ROW_MAJOR = 1


def _span(lines: int, stride: int, line_words: int) -> int:
    """words from the first word of the first line to the last word of the last line"""
    return (lines - 1) * stride + line_words if lines and line_words else 0


def _stride(stride, elements: int, width: int, name: str) -> int:
    s = elements * width if stride is None else int(stride)
    _need(s >= elements * width, f"{name} must be at least {elements} elements of {width} word(s)")
    return s


def _apart_bytes(a, b, what: str) -> None:
    """device._apart for tensors of different element sizes (an index list or a status word against a table of words)"""
    a0, b0 = a.data_ptr(), b.data_ptr()
    _need(a.numel() == 0 or b.numel() == 0 or b0 >= a0 + a.numel() * a.element_size() or a0 >= b0 + b.numel() * b.element_size(), what)


def _counts(**counts) -> None:
    for name, v in counts.items():
        _need(isinstance(v, int) and v >= 0, f"{name} must be a non-negative integer")


def transpose(src, n_outer: int, n_inner: int, dst, width: int = 1, src_stride=None, dst_stride=None, batch: int = 1, stream=None) -> None:
    """dst line i, element o = src line o, element i (tf_table_transpose_dev).  src holds `batch` matrices of n_outer lines of n_inner
    elements, line o at src_stride * o, matrices n_outer * src_stride apart; dst n_inner lines of n_outer elements at dst_stride,
    matrices n_inner * dst_stride apart.  dst may not overlap src.  Only enqueues."""
    src, dst = _t(src, "src"), _t(dst, "dst")
    w = _width(width)
    _counts(n_outer=n_outer, n_inner=n_inner, batch=batch)
    ss, ds = _stride(src_stride, n_inner, w, "src_stride"), _stride(dst_stride, n_outer, w, "dst_stride")
    _need(src.numel() >= _span(batch * n_outer, ss, n_inner * w), "src is smaller than batch * n_outer lines at src_stride")
    _need(dst.numel() >= _span(batch * n_inner, ds, n_outer * w), "dst is smaller than batch * n_inner lines at dst_stride")
    _apart(src, dst, "dst must not overlap src")
    _chk(_lib.lib().tf_table_transpose_dev(_p(src), n_outer, n_inner, w, ss, _p(dst), ds, batch, _stream(stream)), "table_transpose")


def columns_to_rows(table, n_rows: int, n_cols: int, rows_out, width: int = 1, col_stride=None, row_stride=None, batch: int = 1, stream=None) -> None:
    """Column-major tables (what a batch of coset evaluations leaves) -> row-major rows (what tip5_hash_varlen_rows and
    merkle_from_rows read, and what a prover reveals).  Only enqueues."""
    transpose(table, n_cols, n_rows, rows_out, width=width, src_stride=col_stride, dst_stride=row_stride, batch=batch, stream=stream)


def rows_to_columns(rows, n_rows: int, n_cols: int, table_out, width: int = 1, row_stride=None, col_stride=None, batch: int = 1, stream=None) -> None:
    """Row-major rows (a trace, one row per cycle) -> column-major tables (what lde, merkle_from_columns and poly_linear_combination
    read).  Only enqueues."""
    transpose(rows, n_rows, n_cols, table_out, width=width, src_stride=row_stride, dst_stride=col_stride, batch=batch, stream=stream)


def gather_rows(table, n_rows: int, n_cols: int, indices, out, layout: int = COLUMN_MAJOR, width: int = 1, stride=None, out_stride=None,
                batch: int = 1, stream=None, status=None) -> None:
    """out row q of table t (at out[(t * k + q) * out_stride:], n_cols elements) = row indices[q] of table t, from either layout
    (tf_table_gather_rows_dev): one index list for all `batch` tables, repeats allowed; indices is a CUDA tensor of 32-bit words, as
    Tip5 sponges sample them.  Without status an index >= n_rows raises TwentyFirstError (code 17) after the call has synchronised
    once; with status (see device._status) nothing is synchronised and such an index writes 17 there.  Such a row is never read and
    leaves its slot of out as it was, in every table; every other row is correct."""
    import torch

    table, out = _t(table, "table"), _t(out, "out")
    w = _width(width)
    _need(layout in (COLUMN_MAJOR, ROW_MAJOR), "layout must be COLUMN_MAJOR or ROW_MAJOR")
    _need(isinstance(indices, torch.Tensor) and indices.is_cuda and indices.is_contiguous() and indices.dtype in (torch.int32, torch.uint32),
          "indices must be a contiguous CUDA tensor of 32-bit words")
    _counts(n_rows=n_rows, n_cols=n_cols, batch=batch)
    k = indices.numel()
    if layout == ROW_MAJOR:
        st = _stride(stride, n_cols, w, "stride (row_stride)")
        need = _span(batch * n_rows, st, n_cols * w)
    else:
        st = _stride(stride, n_rows, w, "stride (col_stride)")
        need = _span(batch * n_cols, st, n_rows * w)
    os_ = _stride(out_stride, n_cols, w, "out_stride")
    _need(table.numel() >= need, "table is smaller than batch tables at this stride")
    _need(out.numel() >= _span(batch * k, os_, n_cols * w), "out is smaller than batch * k rows at out_stride")
    _apart(table, out, "out must not overlap table")
    _apart_bytes(indices, out, "out must not overlap indices")
    own = _own_status(status, out)
    _status(own)  # (its type, before its address is compared)
    for other, name in ((table, "table"), (indices, "indices"), (out, "out")):
        _apart_bytes(own, other, f"status must not overlap {name}")
    _chk(_lib.lib().tf_table_gather_rows_dev(_p(table), layout, n_rows, n_cols, w, st, _p(indices), k, _p(out), os_, batch, _stream(stream),
                                             _status(own)), "table_gather_rows")
    if status is None and k and n_cols and batch:
        _raise_own_status(own, stream, "table_gather_rows")


def lde_rows_workspace(n: int, m: int, n_cols: int, width: int = 1, cols_per_block: int = 0) -> int:
    """Bytes of the two column-major temporaries lde_rows takes for these arguments (tf_table_lde_rows_workspace: host arithmetic,
    no device needed; what lde itself takes comes on top); 0 for arguments the call rejects."""
    return int(_lib.lib().tf_table_lde_rows_workspace(n, m, n_cols, width, cols_per_block))


def lde_rows(rows, n: int, n_cols: int, offset_in_raw: int, out, m: int, offset_out_raw: int, width: int = 1, row_stride_in=None,
             row_stride_out=None, cols_per_block: int = 0, stream=None) -> None:
    """device.lde of every column of ONE row-major table without a transpose of the caller's own: rows = n x n_cols values on
    {offset_in w_n^i}, out = m x n_cols values on {offset_out w_m^i}.  Works through blocks of cols_per_block columns (0: as many
    as keep the two temporaries within 256 MiB; more than n_cols: n_cols).  Blocking bounds memory and costs time: pass
    cols_per_block=n_cols when lde_rows_workspace(n, m, n_cols, width, n_cols) bytes are to spare.  Only enqueues."""
    rows, out = _t(rows, "rows"), _t(out, "out")
    w = _width(width)
    _counts(n=n, m=m, n_cols=n_cols, cols_per_block=cols_per_block)
    si, so = _stride(row_stride_in, n_cols, w, "row_stride_in"), _stride(row_stride_out, n_cols, w, "row_stride_out")
    _need(rows.numel() >= _span(n, si, n_cols * w) and out.numel() >= _span(m, so, n_cols * w), "buffer sizes do not match n/m/n_cols/width and the strides")
    _apart(rows, out, "out must not overlap rows")
    fn = _lib.lib().tf_table_lde_rows_bfe_dev if w == 1 else _lib.lib().tf_table_lde_rows_xfe_dev
    _chk(fn(_p(rows), n, n_cols, si, C.c_uint64(offset_in_raw), _p(out), m, so, C.c_uint64(offset_out_raw), cols_per_block, _stream(stream)),
         "table_lde_rows")
