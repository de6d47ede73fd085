"""The FRI split-and-fold of whole codewords, one to many levels per call (include/tf_hip.h, "FRI folding").

A codeword of n = 2^k elements lies on {g w_n^i} in natural order (g = offset_raw, a non-zero raw BFieldElement word).  One level
folds it by a challenge alpha into n/2 elements on {g^2 w_{n/2}^i}:

    out[i] = Polynomial::get_colinear_y((x_i, c[i]), (-x_i, c[i + n/2]), alpha),   x_i = g w_n^i   (math/polynomial.rs:386-394)

and levels = r with r challenges is r such folds in a row.  (width_c, width_a) -- codeword; challenges and result -- is (1, 1),
(3, 3) or (1, 3); the mixed form gives word for word what (3, 3) gives on the lifted codeword.  `challenges` holds n_sets x levels
elements, n_sets = 1 (one set for every codeword) or batch (set b for codeword b).

fold is the device-pointer API of device.py: 1-D contiguous int64 / uint64 CUDA tensors of raw Montgomery words, work enqueued on
torch's current stream (or the given one) and NOT synchronised; `challenges` is what device.tip5_sponge_sample_scalars wrote.
fold_host is the numpy form.  plan and workspace are host arithmetic and need no device.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .device import _chk, _need, _p, _stream, _t
from .table import _apart_bytes, _counts

PAIRS = ((1, 1), (3, 3), (1, 3))


def _shape(n: int, batch: int, levels: int, n_sets: int, width_c: int, width_a: int) -> None:
    """what decides the sizes of the three buffers; everything else is the library's to judge"""
    _need((width_c, width_a) in PAIRS, "(width_c, width_a) must be (1, 1), (3, 3) or (1, 3)")
    _counts(n=n, batch=batch, levels=levels, n_sets=n_sets)
    _need(levels < 64, "levels must be below 64")


def fold(codewords, n: int, offset_raw: int, challenges, out, batch: int = 1, levels: int = 1, n_sets: int = 1, width_c: int = 3,
         width_a: int = 3, stream=None) -> None:
    """`levels` folds of `batch` codewords of n elements on device buffers (tf_fri_fold_dev): out receives batch x n / 2^levels
    elements of width_a words; out may not overlap an input.  Only enqueues: nothing is synchronised or copied back, and a fold has
    no data-dependent error.  More than four levels take work space from the library's pool: workspace()."""
    codewords, challenges, out = _t(codewords, "codewords"), _t(challenges, "challenges"), _t(out, "out")
    _shape(n, batch, levels, n_sets, width_c, width_a)
    _need(codewords.numel() == batch * n * width_c, "codewords must hold batch codewords of n elements of width_c words")
    _need(challenges.numel() == n_sets * levels * width_a, "challenges must hold n_sets x levels elements of width_a words")
    _need(out.numel() == batch * (n >> levels) * width_a, "out must hold batch x n / 2^levels elements of width_a words")
    _apart_bytes(codewords, out, "out must not overlap codewords")
    _apart_bytes(challenges, out, "out must not overlap challenges")
    _chk(_lib.lib().tf_fri_fold_dev(_p(codewords), n, batch, width_c, C.c_uint64(offset_raw), _p(challenges), levels, n_sets, width_a, _p(out),
                                    _stream(stream)), "fri_fold")


def fold_host(codewords, n: int, offset_raw: int, challenges, batch: int = 1, levels: int = 1, n_sets: int = 1, width_c: int = 3,
              width_a: int = 3) -> np.ndarray:
    """The same on numpy arrays of raw words (tf_fri_fold): returns batch x n / 2^levels elements of width_a words."""
    cw = np.ascontiguousarray(codewords, dtype=np.uint64).reshape(-1)
    ch = np.ascontiguousarray(challenges, dtype=np.uint64).reshape(-1)
    _shape(n, batch, levels, n_sets, width_c, width_a)
    _need(cw.size == batch * n * width_c, "codewords must hold batch codewords of n elements of width_c words")
    _need(ch.size == n_sets * levels * width_a, "challenges must hold n_sets x levels elements of width_a words")
    out = np.empty(batch * (n >> levels) * width_a, dtype=np.uint64)
    pad = np.zeros(1, dtype=np.uint64)  # stands for an empty output (never written)
    _chk(_lib.lib().tf_fri_fold(C.c_void_p(cw.ctypes.data), n, batch, width_c, C.c_uint64(offset_raw), C.c_void_p(ch.ctypes.data), levels, n_sets,
                                width_a, C.c_void_p((out if out.size else pad).ctypes.data)), "fri_fold")
    return out


def plan(n: int, levels: int, width_c: int = 3, width_a: int = 3) -> list:
    """The levels each pass of fold(n, levels) takes (tf_fri_fold_plan): at most four per pass, the remainder last.  Raises what
    the fold would raise for these arguments."""
    _counts(n=n, levels=levels)
    buf = (C.c_int * 64)()
    rc = int(_lib.lib().tf_fri_fold_plan(n, levels, width_c, width_a, buf, 64))
    if rc < 0:
        _chk(-rc, "fri_fold_plan")
    return [int(buf[i]) for i in range(rc)]


def workspace(n: int, batch: int = 1, levels: int = 1, width_c: int = 3, width_a: int = 3) -> int:
    """Bytes fold requests from the library's pool for the intermediates between its passes (tf_fri_fold_workspace); 0 for one pass
    and for arguments the call rejects."""
    _counts(n=n, batch=batch, levels=levels)
    return int(_lib.lib().tf_fri_fold_workspace(n, batch, width_c, width_a, levels))
