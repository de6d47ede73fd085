"""DEEP quotients of the extended tables (include/tf_hip.h, "DEEP quotients"): the codeword FRI is run on, and the same value at
sampled rows for the verifier.

    out[i] = sum_p ( sum_c w[p][c] * (T_c[i] - v[p][c]) ) / (x_i - z_p),    x_i = offset * w_n^i   (natural order, the domain of fri.fold)

T_c are k1 BFieldElement columns (`main`, column c at c * stride_main words) followed by k3 XFieldElement columns (`aux`, 3 n words
each at stride_aux); points holds n_points (1 to 4) XFieldElements z_p; weights and values hold n_points * (k1 + k3) XFieldElements
each, point-major, main columns first.  Either table may be empty (None).  out holds n XFieldElements and overlaps no input.

quotient and quotient_rows are the device-pointer API of device.py: 1-D contiguous int64 / uint64 CUDA tensors of raw Montgomery
words, work enqueued on torch's current stream (or the given one) and NOT synchronised.  points, weights and values stay where
device.barycentric_evaluate and device.tip5_sponge_sample_scalars left them.  A zero denominator (z_p a lifted point of the domain)
writes 12 to `status`, a one-element int32 CUDA tensor in which the first non-zero code stays; quotient_rows writes 17 there for an
index >= n.  The work space is the caller's: a tensor of at least workspace(...) bytes.  quotient_host and quotient_rows_host are
the numpy forms; they stage through torch tensors here, the library has no host form.  plan and workspace are host arithmetic and
need no device.
"""
from __future__ import annotations

import collections
import ctypes as C

import numpy as np

from . import _lib
from .device import _chk, _need, _p, _status, _stream, _t
from .table import _apart_bytes, _counts

MAX_POINTS = 4
MAX_COLUMNS = 65535

Plan = collections.namedtuple("Plan", "chunk per_lane points_per_pass passes launches grid_cap")


def _span(lines: int, stride: int, line_words: int) -> int:
    """words from the start of the first line to the end of the last"""
    return (lines - 1) * stride + line_words if lines and line_words else 0


def _table(t, name: str, lines: int, line_words: int, stride):
    """(tensor or None, stride) of a table of `lines` lines of line_words words; an empty table needs no tensor"""
    s = line_words if stride is None else stride
    _need(isinstance(s, int) and s >= 0, f"the stride of {name} must be a non-negative integer")
    if lines == 0 or line_words == 0:
        return None, s
    _need(t is not None, f"{name} is missing")
    t = _t(t, name)
    _need(s >= line_words, f"the stride of {name} must be at least {line_words} words")
    _need(t.numel() >= _span(lines, s, line_words), f"{name} is smaller than {lines} lines of {line_words} words at its stride")
    return t, s


def _points(points, weights, values, k: int):
    points = _t(points, "points")
    _need(points.numel() % 3 == 0 and 1 <= points.numel() // 3 <= MAX_POINTS, "points must hold 1 to 4 XFieldElements")
    n_points = points.numel() // 3
    if k == 0:
        return points, n_points, None, None
    weights, values = _t(weights, "weights"), _t(values, "values")
    _need(weights.numel() == n_points * k * 3, "weights must hold n_points * (k1 + k3) XFieldElements")
    _need(values.numel() == n_points * k * 3, "values must hold n_points * (k1 + k3) XFieldElements")
    return points, n_points, weights, values


def _indices(indices):
    import torch

    _need(isinstance(indices, torch.Tensor) and indices.is_cuda and indices.is_contiguous() and indices.dtype in (torch.int32, torch.uint32),
          "indices must be a contiguous CUDA tensor of 32-bit words")
    return indices


def _ptr(t):
    return C.c_void_p(0) if t is None else _p(t)


def _out_apart(out, status, inputs) -> None:
    for name, t in inputs:
        if t is not None:
            _apart_bytes(t, out, f"out must not overlap {name}")
            _apart_bytes(t, status, f"status must not overlap {name}")
    _apart_bytes(out, status, "status must not overlap out")


def quotient(main, aux, n: int, k1: int, k3: int, offset_raw: int, points, weights, values, out, status, work=None, stride_main=None,
             stride_aux=None, stream=None) -> None:
    """The whole codeword (tf_deep_quotient_dev): out[i] for 0 <= i < n.  Only enqueues: nothing is synchronised or copied back."""
    _counts(n=n, k1=k1, k3=k3)
    _need(k1 + k3 <= MAX_COLUMNS, "k1 + k3 must be at most 65 535")
    main, sm = _table(main, "main", k1, n, stride_main)
    aux, sa = _table(aux, "aux", k3, 3 * n, stride_aux)
    points, n_points, weights, values = _points(points, weights, values, k1 + k3)
    out = _t(out, "out")
    _need(out.numel() == 3 * n, "out must hold n XFieldElements")
    st = _status(status)
    inputs = [("main", main), ("aux", aux), ("points", points), ("weights", weights), ("values", values)]
    _out_apart(out, status, inputs)
    need = workspace(n, k1, k3, n_points)
    if need == 0 and work is None:
        p_work, work_bytes = C.c_void_p(0), 0
    else:
        _need(work is not None, f"this call needs a work space of {need} bytes (deep.workspace)")
        work = _t(work, "work")
        work_bytes = work.numel() * work.element_size()
        _need(work_bytes >= need, f"work is smaller than the {need} bytes this call needs (deep.workspace)")
        for name, t in inputs + [("out", out), ("status", status)]:
            if t is not None:
                _apart_bytes(t, work, f"work must not overlap {name}")
        p_work = _p(work)
    _chk(_lib.lib().tf_deep_quotient_dev(_ptr(main), k1, sm, _ptr(aux), k3, sa, n, C.c_uint64(offset_raw), _p(points), n_points, _ptr(weights),
                                         _ptr(values), _p(out), p_work, work_bytes, _stream(stream), st), "deep_quotient")


def quotient_rows(main_rows, aux_rows, n: int, k1: int, k3: int, offset_raw: int, indices, points, weights, values, out, status,
                  row_stride_main=None, row_stride_aux=None, stream=None) -> None:
    """The quotient at sampled indices (tf_deep_quotient_rows_dev), from the rows table.gather_rows opened: row r of main_rows holds k1
    words at r * row_stride_main, row r of aux_rows 3 * k3 words at r * row_stride_aux; indices is a CUDA tensor of 32-bit words, as
    Tip5 sponges sample them.  out holds one XFieldElement per index.  Only enqueues."""
    _counts(n=n, k1=k1, k3=k3)
    _need(k1 + k3 <= MAX_COLUMNS, "k1 + k3 must be at most 65 535")
    n_rows = _indices(indices).numel()
    main_rows, sm = _table(main_rows, "main_rows", n_rows if k1 else 0, k1, row_stride_main)
    aux_rows, sa = _table(aux_rows, "aux_rows", n_rows if k3 else 0, 3 * k3, row_stride_aux)
    points, n_points, weights, values = _points(points, weights, values, k1 + k3)
    out = _t(out, "out")
    _need(out.numel() == 3 * n_rows, "out must hold one XFieldElement per index")
    st = _status(status)
    _out_apart(out, status, [("main_rows", main_rows), ("aux_rows", aux_rows), ("indices", indices), ("points", points), ("weights", weights),
                             ("values", values)])
    _chk(_lib.lib().tf_deep_quotient_rows_dev(_ptr(main_rows), k1, sm, _ptr(aux_rows), k3, sa, n, C.c_uint64(offset_raw), _p(indices), n_rows,
                                              _p(points), n_points, _ptr(weights), _ptr(values), _p(out), _stream(stream), st), "deep_quotient_rows")


def plan(n: int, k1: int, k3: int, n_points: int) -> Plan:
    """How a codeword call runs (tf_deep_quotient_plan): elements per wave and step (the chunk), elements per lane, points per pass,
    passes (each reads the table once), launches, and the number of chunks in flight above which a wave takes a second chunk.
    Raises what the call would raise for these arguments."""
    _counts(n=n, k1=k1, k3=k3, n_points=n_points)
    buf = (C.c_int * 6)()
    rc = int(_lib.lib().tf_deep_quotient_plan(n, k1, k3, n_points, buf, 6))
    if rc < 0:
        _chk(-rc, "deep_quotient_plan")
    return Plan(*(int(v) for v in buf))


def workspace(n: int, k1: int, k3: int, n_points: int) -> int:
    """Bytes of work space a codeword call needs from its caller (tf_deep_quotient_workspace): one XFieldElement per point; 0 for an
    empty call, a call without columns and for arguments the call rejects."""
    _counts(n=n, k1=k1, k3=k3, n_points=n_points)
    return int(_lib.lib().tf_deep_quotient_workspace(n, k1, k3, n_points))


# ----------------------------------------------------------------------------- numpy forms
def _up(x):
    import torch

    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.uint64).reshape(-1).view(np.int64).copy()).cuda()


def _host(count: int, call):
    """run `call(out, status)` on device copies; -> (count XFieldElements, the status word)"""
    import torch

    out = torch.zeros(3 * count, dtype=torch.int64, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    call(out, status)
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint64), int(status.item())


def quotient_host(main, aux, n: int, k1: int, k3: int, offset_raw: int, points, weights, values, stride_main=None, stride_aux=None):
    """quotient on numpy arrays of raw words: returns (n XFieldElements, status code)."""
    import torch

    _counts(n=n, k1=k1, k3=k3)
    k = k1 + k3
    n_points = np.asarray(points).size // 3
    need = workspace(n, k1, k3, n_points)
    work = torch.empty(need // 8, dtype=torch.int64, device="cuda") if need else None
    return _host(n, lambda out, status: quotient(_up(main) if k1 and n else None, _up(aux) if k3 and n else None, n, k1, k3, offset_raw, _up(points),
                                                 _up(weights) if k else None, _up(values) if k else None, out, status, work, stride_main, stride_aux))


def quotient_rows_host(main_rows, aux_rows, n: int, k1: int, k3: int, offset_raw: int, indices, points, weights, values, row_stride_main=None,
                       row_stride_aux=None):
    """quotient_rows on numpy arrays: returns (one XFieldElement per index, status code)."""
    import torch

    _counts(n=n, k1=k1, k3=k3)
    k = k1 + k3
    idx = torch.from_numpy(np.ascontiguousarray(indices, dtype=np.uint32).reshape(-1).view(np.int32).copy()).cuda()
    rows = idx.numel()
    return _host(rows, lambda out, status: quotient_rows(_up(main_rows) if k1 and rows else None, _up(aux_rows) if k3 and rows else None, n, k1, k3,
                                                         offset_raw, idx, _up(points), _up(weights) if k else None, _up(values) if k else None, out,
                                                         status, row_stride_main, row_stride_aux))
