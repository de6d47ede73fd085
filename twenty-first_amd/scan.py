"""Inclusive prefix scans along the columns of a column-major table (include/tf_hip.h, "Prefix scans"): the auxiliary columns of an AIR.

    y_-1 = init,   y_i = a_i * y_(i-1) + b_i   (0 <= i < n),   out[i] = y_i

sum_ is a = 1 (a log-derivative column), product is b = 0 (the running product of a permutation argument), affine the whole
recurrence (a running evaluation; with one multiplier for the column, Horner's rule).  Column c of an operand starts `stride` WORDS
after column c - 1 (default n * width, packed); words between n * width and the stride are neither read nor written.  (width_a,
width_b) of affine is (1, 1), (3, 3) or (3, 1); out and init have max(width_a, width_b) words per element.

sum_, product and affine are the device-pointer API of device.py: 1-D contiguous int64 / uint64 CUDA tensors of raw Montgomery
words, work enqueued on torch's current stream (or the given one) and NOT synchronised; a multiplier of affine with a_len = 1 is what
device.tip5_sponge_sample_scalars wrote.  The work space is the caller's: a tensor of at least workspace(...) bytes, needed from two
tiles per column on (plan(...).launches == 3).  sum_host, product_host and affine_host are the numpy forms; they stage through
torch tensors here, the library has no host form of a scan.  plan and workspace are host arithmetic and need no device.
"""
from __future__ import annotations

import collections
import ctypes as C

import numpy as np

from . import _lib
from .device import _chk, _need, _p, _stream, _t
from .table import _apart_bytes, _counts

SUM, PRODUCT, AFFINE = 0, 1, 2  # TF_SCAN_SUM, TF_SCAN_PRODUCT, TF_SCAN_AFFINE
PAIRS = ((1, 1), (3, 3), (3, 1))  # (width_a, width_b) of affine

Plan = collections.namedtuple("Plan", "tile tiles turn launches wave map_words")


def _span(batch: int, stride: int, line: int) -> int:
    """words from the start of the first column to the end of the last"""
    return (batch - 1) * stride + line if batch and line else 0


def _stride(stride, n: int, width: int, name: str) -> int:
    s = n * width if stride is None else stride
    _need(isinstance(s, int) and s >= n * width, f"{name} must be at least n * width words")
    return s


def _column_operand(t, name: str, n: int, batch: int, width: int, stride) -> int:
    s = _stride(stride, n, width, f"stride of {name}")
    _need(t.numel() >= _span(batch, s, n * width), f"{name} is smaller than batch columns of n elements at its stride")
    return s


def _init(init, batch: int, width: int):
    """(pointer, n_init) of the start values: None, one element, or one per column"""
    if init is None:
        return C.c_void_p(0), 0
    init = _t(init, "init")
    _need(init.numel() in (width, batch * width), "init must hold one element of the result's width, or one per column")
    return _p(init), init.numel() // width


def _work(work, need: int, others):
    """(pointer, bytes) of the caller's work space, checked against workspace() and against every operand"""
    if need == 0 and work is None:
        return C.c_void_p(0), 0
    _need(work is not None, f"this call needs a work space of {need} bytes (scan.workspace)")
    work = _t(work, "work")
    _need(work.numel() * work.element_size() >= need, f"work is smaller than the {need} bytes this call needs (scan.workspace)")
    for name, t in others:
        _apart_bytes(t, work, f"work must not overlap {name}")
    return _p(work), work.numel() * work.element_size()


def _out_against(out, stride_out: int, operand, stride: int, same_width: bool, name: str) -> None:
    """out is exactly the operand (the same pointer, stride and width: the in-place form) or apart from it"""
    if same_width and out.data_ptr() == operand.data_ptr() and stride_out == stride:
        return
    _apart_bytes(operand, out, f"out must be exactly {name} (the same pointer, stride and width) or not overlap it")


def _one_operand(fn, where: str, mode: int, x, n, out, batch, width, stride_in, stride_out, init, work, stream) -> None:
    x, out = _t(x, "the operand"), _t(out, "out")
    _need(width in (1, 3), "width must be 1 (BFieldElement) or 3 (XFieldElement)")
    _counts(n=n, batch=batch)
    si, so = _column_operand(x, "the operand", n, batch, width, stride_in), _column_operand(out, "out", n, batch, width, stride_out)
    _out_against(out, so, x, si, True, "the operand")
    p_init, n_init = _init(init, batch, width)
    if n_init:
        _apart_bytes(init, out, "out must not overlap init")
    others = [("the operand", x), ("out", out)] + ([("init", init)] if n_init else [])
    p_work, work_bytes = _work(work, workspace(mode, n, batch, width), others)
    _chk(fn(_p(x), n, batch, width, si, p_init, n_init, _p(out), so, p_work, work_bytes, _stream(stream)), where)


def sum_(x, n: int, out, batch: int = 1, width: int = 1, stride_in=None, stride_out=None, init=None, work=None, stream=None) -> None:
    """out[i] = init + x[0] + ... + x[i] along each of `batch` columns of n elements (tf_scan_sum_dev).  out may be exactly x.  Only
    enqueues: nothing is synchronised or copied back."""
    _one_operand(_lib.lib().tf_scan_sum_dev, "scan_sum", SUM, x, n, out, batch, width, stride_in, stride_out, init, work, stream)


def product(x, n: int, out, batch: int = 1, width: int = 1, stride_in=None, stride_out=None, init=None, work=None, stream=None) -> None:
    """out[i] = init * x[0] * ... * x[i] along each of `batch` columns of n elements (tf_scan_product_dev; init None: 1).  out may be
    exactly x.  Only enqueues."""
    _one_operand(_lib.lib().tf_scan_product_dev, "scan_product", PRODUCT, x, n, out, batch, width, stride_in, stride_out, init, work, stream)


def affine(a, b, n: int, out, batch: int = 1, width_a: int = 3, width_b: int = 3, a_len=None, a_sets: int = 1, stride_a=None, stride_b=None,
           stride_out=None, init=None, work=None, stream=None) -> None:
    """out[i] = a[i] * out[i - 1] + b[i], out[-1] = init, along each of `batch` columns (tf_scan_affine_dev).  a_len = n (the default):
    `a` is a table like b, at stride_a.  a_len = 1: one multiplier for the whole column, `a` holds a_sets of them packed, a_sets = 1
    (the same for every column) or batch -- also for n = 1, where only an a_len left at its default means the table.  out may be exactly b when width_a == width_b.  Only enqueues."""
    a, b, out = _t(a, "a"), _t(b, "b"), _t(out, "out")
    _need((width_a, width_b) in PAIRS, "(width_a, width_b) must be (1, 1), (3, 3) or (3, 1)")
    _counts(n=n, batch=batch, a_sets=a_sets)
    packed = a_len == 1  # said so by the caller: with n = 1 the default is still the table, and stride_a = 0 tells the library which
    a_len = n if a_len is None else a_len
    _need(a_len in (1, n), "a_len must be 1 or n")
    w = width_a
    sb, so = _column_operand(b, "b", n, batch, width_b, stride_b), _column_operand(out, "out", n, batch, w, stride_out)
    if packed:
        _need(a_sets in (1, batch), "a_sets must be 1 or batch")
        _need(a.numel() == a_sets * w, "a must hold a_sets elements of width_a words")
        sa = 0
    else:
        sa = _column_operand(a, "a", n, batch, w, stride_a)
    _apart_bytes(a, out, "out must not overlap a")
    _out_against(out, so, b, sb, width_a == width_b, "b")
    p_init, n_init = _init(init, batch, w)
    if n_init:
        _apart_bytes(init, out, "out must not overlap init")
    others = [("a", a), ("b", b), ("out", out)] + ([("init", init)] if n_init else [])
    p_work, work_bytes = _work(work, workspace(AFFINE, n, batch, w), others)
    _chk(_lib.lib().tf_scan_affine_dev(_p(a), a_len, a_sets, width_a, sa, _p(b), width_b, sb, n, batch, p_init, n_init, _p(out), so, p_work, work_bytes,
                                       _stream(stream)), "scan_affine")


def plan(mode: int, n: int, batch: int = 1, width_out: int = 1) -> Plan:
    """How a scan of `batch` columns of n elements runs (tf_scan_plan): elements per tile, tiles per column, tile maps the spine takes
    per turn, launches (0, 1 or 3), elements up to which one wave scans a column, words per tile map.  Raises what the scan would
    raise for these arguments."""
    _counts(n=n, batch=batch)
    buf = (C.c_int * 6)()
    rc = int(_lib.lib().tf_scan_plan(mode, n, batch, width_out, buf, 6))
    if rc < 0:
        _chk(-rc, "scan_plan")
    return Plan(*(int(v) for v in buf))


def workspace(mode: int, n: int, batch: int = 1, width_out: int = 1) -> int:
    """Bytes of work space the scan needs from its caller (tf_scan_workspace): tiles x batch tile maps and as many start values; 0 for
    one tile per column and for arguments the call rejects."""
    _counts(n=n, batch=batch)
    return int(_lib.lib().tf_scan_workspace(mode, n, batch, width_out))


# ----------------------------------------------------------------------------- numpy forms
def _up(x):
    import torch

    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.uint64).reshape(-1).view(np.int64).copy()).cuda()


def _host(call, mode: int, n: int, batch: int, width: int, init) -> np.ndarray:
    """run `call(out, init, work)` on device copies and bring batch x n packed elements back"""
    import torch

    _counts(n=n, batch=batch)
    if n == 0 or batch == 0:
        return np.zeros(0, dtype=np.uint64)
    out = torch.empty(batch * n * width, dtype=torch.int64, device="cuda")
    need = workspace(mode, n, batch, width)
    work = torch.empty(need // 8, dtype=torch.int64, device="cuda") if need else None
    call(out, None if init is None else _up(init), work)
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint64)


def sum_host(x, n: int, batch: int = 1, width: int = 1, stride_in=None, init=None) -> np.ndarray:
    """sum_ on numpy arrays of raw words: returns batch x n elements, packed."""
    return _host(lambda out, d_init, work: sum_(_up(x), n, out, batch, width, stride_in, None, d_init, work), SUM, n, batch, width, init)


def product_host(x, n: int, batch: int = 1, width: int = 1, stride_in=None, init=None) -> np.ndarray:
    """product on numpy arrays of raw words: returns batch x n elements, packed."""
    return _host(lambda out, d_init, work: product(_up(x), n, out, batch, width, stride_in, None, d_init, work), PRODUCT, n, batch, width, init)


def affine_host(a, b, n: int, batch: int = 1, width_a: int = 3, width_b: int = 3, a_len=None, a_sets: int = 1, stride_a=None, stride_b=None,
                init=None) -> np.ndarray:
    """affine on numpy arrays of raw words: returns batch x n elements of width_a words, packed."""
    return _host(lambda out, d_init, work: affine(_up(a), _up(b), n, out, batch, width_a, width_b, a_len, a_sets, stride_a, stride_b, None, d_init, work),
                 AFFINE, n, batch, width_a, init)
