"""Expected values of the table calls (tf_table_transpose, tf_table_gather_rows, tf_table_lde_rows_*) on the strided layouts of
include/tf_hip.h ("Tables") -- plain numpy loops over lines, independent of the library.  An element is `width` words; strides
count words.  Every model takes the destination as it was before the call and returns what it must be afterwards: the words between
the end of a line and its stride (and the rows of a bad index) are carried through untouched, so a test can compare WHOLE buffers.
"""
import numpy as np

COLUMN_MAJOR = 0
ROW_MAJOR = 1


def span(lines, stride, line_words):
    """words from the first word of the first line to the last word of the last line"""
    return (lines - 1) * stride + line_words if lines and line_words else 0


def line_mask(lines, stride, line_words, size=None):
    """bool mask over a buffer of `size` words (default: the span): True on the words of the lines, False on the padding"""
    m = np.zeros(span(lines, stride, line_words) if size is None else size, dtype=bool)
    for i in range(lines):
        m[i * stride:i * stride + line_words] = True
    return m


def transpose(src, n_outer, n_inner, width, src_stride, dst_before, dst_stride, batch=1):
    """dst line i, element o = src line o, element i, for `batch` matrices (src matrices n_outer * src_stride apart, dst matrices
    n_inner * dst_stride apart)."""
    src = np.asarray(src, dtype=np.uint64).reshape(-1)
    dst = np.array(dst_before, dtype=np.uint64).reshape(-1)
    assert src_stride >= n_inner * width and dst_stride >= n_outer * width
    for b in range(batch):
        for o in range(n_outer):
            s0 = (b * n_outer + o) * src_stride
            for i in range(n_inner):
                d0 = (b * n_inner + i) * dst_stride + o * width
                dst[d0:d0 + width] = src[s0 + i * width:s0 + (i + 1) * width]
    return dst


def transpose_fast(src, n_outer, n_inner, width, src_stride, dst_before, dst_stride, batch=1):
    """transpose() through numpy views: the same words for the shapes where the loops above would take seconds (the two agree on
    the small shapes, tests/test_table_cpu.py)"""
    src = np.asarray(src, dtype=np.uint64).reshape(-1)
    dst = np.array(dst_before, dtype=np.uint64).reshape(-1)
    for b in range(batch):
        for o in range(n_outer):
            s0 = (b * n_outer + o) * src_stride
            line = src[s0:s0 + n_inner * width].reshape(n_inner, width)
            base = b * n_inner * dst_stride + o * width
            for k in range(width):
                dst[base + k:base + k + (n_inner - 1) * dst_stride + 1:dst_stride] = line[:, k]
    return dst


def row_of(table, layout, n_rows, n_cols, width, stride, t, i):
    """the n_cols * width words of row i of table t"""
    table = np.asarray(table, dtype=np.uint64).reshape(-1)
    if layout == ROW_MAJOR:
        r0 = (t * n_rows + i) * stride
        return table[r0:r0 + n_cols * width].copy()
    at = ((t * n_cols + np.arange(n_cols, dtype=np.int64)) * stride + i * width)[:, None] + np.arange(width, dtype=np.int64)[None, :]
    return table[at.reshape(-1)]


def gather_rows(table, layout, n_rows, n_cols, width, stride, indices, out_before, out_stride, batch=1):
    """out row q of table t (at (t * k + q) * out_stride) = row indices[q] of table t.  Returns (out, bad): bad lists the positions
    q whose index is >= n_rows; their rows of out stay as they were, in every table."""
    assert layout in (COLUMN_MAJOR, ROW_MAJOR) and out_stride >= n_cols * width
    idx = np.asarray(indices).reshape(-1)
    idx = [int(v) for v in (idx.view(np.uint32) if idx.dtype == np.int32 else idx.astype(np.uint32))]  # (int32 tensors carry u32 bits)
    out = np.array(out_before, dtype=np.uint64).reshape(-1)
    bad = [q for q, v in enumerate(idx) if v >= n_rows]
    for t in range(batch):
        for q, v in enumerate(idx):
            if v < n_rows:
                o0 = (t * len(idx) + q) * out_stride
                out[o0:o0 + n_cols * width] = row_of(table, layout, n_rows, n_cols, width, stride, t, v)
    return out, bad


def lde_rows(lde_column, rows, n, n_cols, width, row_stride_in, out_before, m, row_stride_out):
    """lde_column(values of n elements) -> m elements, applied to every column of one row-major table: the m x n_cols rows"""
    rows = np.asarray(rows, dtype=np.uint64).reshape(-1)
    out = np.array(out_before, dtype=np.uint64).reshape(-1)
    for j in range(n_cols):
        col = np.concatenate([rows[i * row_stride_in + j * width:i * row_stride_in + (j + 1) * width] for i in range(n)]) if n else np.zeros(0, np.uint64)
        ext = np.asarray(lde_column(col), dtype=np.uint64).reshape(m, width)
        for i in range(m):
            out[i * row_stride_out + j * width:i * row_stride_out + (j + 1) * width] = ext[i]
    return out


def lde_block_cols(n, m, n_cols, width, cols_per_block):
    """columns per block of tf_table_lde_rows_*: the request clamped to n_cols, or for 0 the largest count whose two temporaries
    stay within 256 MiB, at least 1"""
    if cols_per_block:
        return min(cols_per_block, n_cols)
    if n + m == 0:
        return n_cols  # (an empty table: nothing is taken)
    return max(1, min(n_cols, (256 << 20) // ((n + m) * width * 8)))


def lde_workspace(n, m, n_cols, width, cols_per_block):
    return lde_block_cols(n, m, n_cols, width, cols_per_block) * (n + m) * width * 8
