"""twenty_first_amd -- host-side mirror of the reference's API for the hot path, on top of the
C ABI of libtf_hip.so (include/tf_hip.h).  Python is only the harness language here (tests,
bench); the C++ mirror of the same interface is host/twenty_first.hpp.

Names, argument meaning and error behaviour follow the Rust crate (paths relative to
/root/reference/twenty-first/src/):

    ntt / intt                       math/ntt.rs:67-82, :109-125
    Polynomial.fast_coset_evaluate   math/polynomial.rs:1374-1399
    Tip5.hash_10 / hash_pair / hash_varlen / permutation   tip5/mod.rs:529-623
    MerkleTree.par_new / sequential_new / par_frugal_root / sequential_frugal_root
                                     util_types/merkle_tree.rs:149-364
    MerkleTreeError                  util_types/merkle_tree.rs:933-965

Data are numpy uint64 arrays of RAW Montgomery words exactly as the Rust types lay them out
(BFieldElement 1 word, XFieldElement 3, Digest 5); `BFieldElement.new/value` convert single values.
Every operation runs on the GPU through the C ABI; there is no CPU fallback -- a missing library
or device raises.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib

__all__ = [
    "P", "BFieldElement", "ntt", "intt", "batch_inversion", "inverse_or_zero", "linear_combination", "get_colinear_y", "are_colinear", "mod_pow", "powers", "fri_fold", "Polynomial", "ZerofierTree", "barycentric_evaluate", "fast_coset_evaluate", "fast_coset_interpolate", "fast_multiply", "fast_square", "Tip5", "Tip5Sponge", "Digest", "MerkleTree", "Table",
    "MerkleTreeInclusionProof", "MerkleTreeError", "TwentyFirstError", "NttPanic", "lib", "device", "table", "merkle_sampled", "fri", "scan", "deep", "set_device", "get_device", "shard_range",
]

P = 0xFFFFFFFF00000001  # BFieldElement::P, math/b_field_element.rs:225
_R = 1 << 64
_R_INV = pow(_R, P - 2, P)


def lib():
    return _lib.lib()


# ----------------------------------------------------------------------------- errors
class TwentyFirstError(RuntimeError):
    def __init__(self, code: int, where: str = ""):
        name = lib().tf_status_string(code).decode()
        detail = lib().tf_last_error().decode()
        msg = f"{where}: {name}" if where else name
        if detail and (8 <= code <= 10 or code == 18):  # tf_last_error() is the text of a HIP failure / of an exception caught at the ABI; the other codes carry none
            msg += f" ({detail})"
        super().__init__(msg)
        self.code = code


class NttPanic(TwentyFirstError):
    """Raised where the reference panics (math/ntt.rs:135-140, math/polynomial.rs:1388-1392)."""


class MerkleTreeError(TwentyFirstError):
    """util_types/merkle_tree.rs:933-965; .variant is the Rust variant name."""

    VARIANTS = {1: "TooFewLeafs", 2: "IncorrectNumberOfLeafs", 3: "TreeTooHigh", 11: "LeafIndexInvalid",
                19: "AuthenticationStructureLengthMismatch", 20: "RepeatedLeafDigestMismatch", 21: "RootMismatch"}

    def __init__(self, code: int, where: str = ""):
        super().__init__(code, where)
        self.variant = self.VARIANTS.get(code, "Unknown")


def _check(rc: int, where: str):
    if rc == 0:
        return
    if rc in (1, 2, 3, 11, 19, 20, 21):
        raise MerkleTreeError(rc, where)
    if rc in (4, 5, 6, 12, 14, 15, 16):
        raise NttPanic(rc, where)
    raise TwentyFirstError(rc, where)


# ----------------------------------------------------------------------------- scalars
class BFieldElement:
    """Conversions between canonical values and raw Montgomery words (host-side convenience;
    math/b_field_element.rs:235-237, :248-250)."""

    P = P
    MAX = P - 1
    ZERO_RAW = 0             # :691-693
    ONE_RAW = 0xFFFFFFFF     # :707-709 (2^64 mod p)

    @staticmethod
    def new(value: int) -> int:
        return (value % (1 << 64)) % P * _R % P

    @staticmethod
    def value(raw: int) -> int:
        return int(raw) * _R_INV % P

    @staticmethod
    def generator() -> int:
        return BFieldElement.new(7)  # :312-314

    @staticmethod
    def primitive_root_of_unity(n: int):
        """:814-818; raw word, or None if n is not 0/1/a power of two <= 2^32."""
        if n in (0, 1):
            return BFieldElement.new(1)
        if n & (n - 1) or n > (1 << 32):
            return None
        return BFieldElement.new(pow(7, (P - 1) // n, P))


def _words(x, name="x") -> np.ndarray:
    if not isinstance(x, np.ndarray) or x.dtype != np.uint64 or not x.flags["C_CONTIGUOUS"]:
        raise TypeError(f"{name} must be a C-contiguous numpy uint64 array of raw Montgomery words")
    return x


def _ptr(a: np.ndarray):
    return C.c_void_p(a.ctypes.data) if a.size else C.c_void_p(0)


# ----------------------------------------------------------------------------- devices
def set_device(device: int) -> None:
    """Select the GPU every later call of this host thread runs on (include/tf_hip.h: tf_set_device)."""
    _check(lib().tf_set_device(int(device)), "set_device")


def get_device() -> int:
    d = C.c_int(0)
    _check(lib().tf_get_device(C.byref(d)), "get_device")
    return d.value


def shard_range(total_units: int, n_shards: int, shard: int):
    """[lo, hi) of slice `shard` when `total_units` independent units are split over `n_shards` devices: the rule of the
    multi-device entry points (tf_shard_range), the same as sharding.shard_range."""
    lo, hi = C.c_size_t(0), C.c_size_t(0)
    _check(lib().tf_shard_range(total_units, n_shards, shard, C.byref(lo), C.byref(hi)), "shard_range")
    return lo.value, hi.value


def _devices(devices):
    """devices="all" -> (NULL, 0): every visible GPU; a sequence of indices -> (int array, count).  The same index may repeat."""
    if isinstance(devices, str):
        if devices != "all":
            raise ValueError('devices must be "all" or a sequence of device indices')
        return C.cast(C.c_void_p(0), C.POINTER(C.c_int)), 0
    ids = [int(d) for d in devices]
    if not ids:
        raise ValueError("devices must not be empty")
    return (C.c_int * len(ids))(*ids), len(ids)


# ----------------------------------------------------------------------------- NTT
def ntt(x: np.ndarray, width: int = 1, batch: int = 1, _inverse: bool = False, devices=None) -> None:
    """In-place NTT of `batch` contiguous slices (math/ntt.rs:67-82).  width 1 = BFieldElement slice,
    3 = XFieldElement slice.  Raises NttPanic where the reference panics.
    devices: None = the current GPU; "all" or a list of device indices = the batch split over those GPUs (tf_ntt_*_multi)."""
    x = _words(x)
    if width not in (1, 3):
        raise ValueError("width must be 1 (BFieldElement) or 3 (XFieldElement)")
    if batch < 0 or (batch and x.size % (batch * width)):
        raise ValueError("array size is not batch * n * width")
    n = x.size // (batch * width) if batch else 0
    if devices is not None:
        ids, k = _devices(devices)
        fn = lib().tf_ntt_bfe_multi if width == 1 else lib().tf_ntt_xfe_multi
        _check(fn(_ptr(x), n, batch, int(_inverse), ids, k), "intt" if _inverse else "ntt")
        return
    fn = lib().tf_ntt_bfe if width == 1 else lib().tf_ntt_xfe
    _check(fn(_ptr(x), n, batch, int(_inverse)), "intt" if _inverse else "ntt")


def intt(x: np.ndarray, width: int = 1, batch: int = 1, devices=None) -> None:
    """In-place inverse NTT (math/ntt.rs:109-125)."""
    ntt(x, width=width, batch=batch, _inverse=True, devices=devices)


def _xfe_offset(offset, width: int):
    """None for a BFieldElement offset (one raw word), the 3 raw words for an XFieldElement offset (XFE polynomials only:
    FF: Mul<S, Output = FF>, math/polynomial.rs:1376)."""
    if isinstance(offset, (int, np.integer)):
        return None
    off = np.ascontiguousarray(offset, dtype=np.uint64).reshape(-1)
    if off.size == 1:
        return None
    if off.size != 3 or width != 3:
        raise TypeError("an XFieldElement offset (3 raw words) needs XFieldElement coefficients")
    return off


def fast_coset_evaluate(coeffs: np.ndarray, offset_raw, order: int, width: int = 1, batch: int = 1, devices=None) -> np.ndarray:
    """`batch` polynomials of equal length -> `batch` x `order` evaluations (math/polynomial.rs:1374-1399).
    The reference compares `order` with the DEGREE (:1388): high-order zero coefficients common to the whole batch are
    trimmed here before the length reaches the C ABI, as Polynomial::degree() does for one polynomial."""
    coeffs = _words(coeffs, "coeffs")
    if batch and coeffs.size % (batch * width):
        raise ValueError("coeffs size is not batch * n_coeffs * width")
    n_coeffs = coeffs.size // (batch * width) if batch else 0
    if batch and n_coeffs > order:
        c3 = coeffs.reshape(batch, n_coeffs, width)
        live = np.nonzero(c3.any(axis=(0, 2)))[0]
        keep = int(live[-1]) + 1 if live.size else 0
        if keep < n_coeffs:
            coeffs = np.ascontiguousarray(c3[:, :keep, :]).reshape(-1)
            n_coeffs = keep
    out = np.empty(batch * order * width, dtype=np.uint64)
    xoff = _xfe_offset(offset_raw, width)
    if xoff is not None:  # S = XFieldElement (:1374-1378)
        if devices is not None:  # (this used to run on the current GPU only, without saying so)
            raise NotImplementedError("fast_coset_evaluate with an XFieldElement offset is a single-device call: there is no tf_coset_eval_xfe_xoffset_multi")
        _check(lib().tf_coset_eval_xfe_xoffset(_ptr(coeffs), n_coeffs, _ptr(xoff), _ptr(out), order, batch), "fast_coset_evaluate")
        return out
    offset_raw = int(np.asarray(offset_raw).reshape(-1)[0])
    if devices is not None:  # the polynomials of the batch split over several GPUs (tf_coset_eval_*_multi)
        ids, k = _devices(devices)
        fn = lib().tf_coset_eval_bfe_multi if width == 1 else lib().tf_coset_eval_xfe_multi
        _check(fn(_ptr(coeffs), n_coeffs, C.c_uint64(offset_raw), _ptr(out), order, batch, ids, k), "fast_coset_evaluate")
        return out
    fn = lib().tf_coset_eval_bfe if width == 1 else lib().tf_coset_eval_xfe
    _check(fn(_ptr(coeffs), n_coeffs, C.c_uint64(offset_raw), _ptr(out), order, batch), "fast_coset_evaluate")
    return out


def fast_coset_interpolate(values: np.ndarray, offset_raw, width: int = 1, batch: int = 1) -> np.ndarray:
    """`batch` x n evaluations on {offset * w^i} -> `batch` x n coefficients (math/polynomial.rs:1907-1918)."""
    values = _words(values, "values")
    if batch and values.size % (batch * width):
        raise ValueError("values size is not batch * n * width")
    n = values.size // (batch * width) if batch else 0
    out = np.empty_like(values)
    xoff = _xfe_offset(offset_raw, width)
    if xoff is not None:  # S = XFieldElement (:1907-1911)
        _check(lib().tf_coset_interpolate_xfe_xoffset(_ptr(values), n, _ptr(xoff), _ptr(out), batch), "fast_coset_interpolate")
        return out
    offset_raw = int(np.asarray(offset_raw).reshape(-1)[0])
    fn = lib().tf_coset_interpolate_bfe if width == 1 else lib().tf_coset_interpolate_xfe
    _check(fn(_ptr(values), n, C.c_uint64(offset_raw), _ptr(out), batch), "fast_coset_interpolate")
    return out


def fast_multiply(a: np.ndarray, b: np.ndarray, width: int = 1, batch: int = 1) -> np.ndarray:
    """Coefficient arrays of `batch` polynomial pairs -> `batch` x (na + nb - 1) product coefficients
    (math/polynomial.rs:900-932, untrimmed)."""
    a, b = _words(a, "a"), _words(b, "b")
    if batch and (a.size % (batch * width) or b.size % (batch * width)):
        raise ValueError("operand size is not batch * n_coeffs * width")
    na = a.size // (batch * width) if batch else 0
    nb = b.size // (batch * width) if batch else 0
    if na == 0 or nb == 0:
        return np.zeros(0, dtype=np.uint64)
    out = np.empty(batch * (na + nb - 1) * width, dtype=np.uint64)
    fn = lib().tf_poly_mul_bfe if width == 1 else lib().tf_poly_mul_xfe
    _check(fn(_ptr(a), na, _ptr(b), nb, _ptr(out), batch), "fast_multiply")
    return out


def fast_square(a: np.ndarray, width: int = 1, batch: int = 1) -> np.ndarray:
    """`batch` polynomials of na coefficients -> `batch` x (2 na - 1) coefficients of their squares
    (math/polynomial.rs:780-798, untrimmed)."""
    a = _words(a, "a")
    if batch and a.size % (batch * width):
        raise ValueError("operand size is not batch * n_coeffs * width")
    na = a.size // (batch * width) if batch else 0
    if na == 0:
        return np.zeros(0, dtype=np.uint64)
    out = np.empty(batch * (2 * na - 1) * width, dtype=np.uint64)
    fn = lib().tf_poly_square_bfe if width == 1 else lib().tf_poly_square_xfe
    _check(fn(_ptr(a), na, _ptr(out), batch), "fast_square")
    return out


def poly_divide(dividends: np.ndarray, divisor: np.ndarray, width: int = 1, batch: int = 1, quotient: bool = True, remainder: bool = True):
    """Polynomial::divide (math/polynomial.rs:539-600) of `batch` dividends (packed, na coefficients each) by ONE divisor: returns
    (q, r) as batch x max(na - nb + 1, 0) and batch x (nb - 1) coefficients, zero padded at the top (None for an output not
    asked for).  The divisor's leading zero coefficients are dropped first; a zero divisor panics (NttPanic code 15)."""
    a = _words(np.ascontiguousarray(dividends, dtype=np.uint64).reshape(-1), "dividends")
    b = _words(np.ascontiguousarray(divisor, dtype=np.uint64).reshape(-1), "divisor")
    if width not in (1, 3) or a.size % (width * max(batch, 1)) or b.size % width:
        raise ValueError("dividends / divisor must hold whole elements of `width` words, batch dividends of equal length")
    nb = b.size // width
    while nb and not b[(nb - 1) * width:nb * width].any():
        nb -= 1
    na = a.size // (width * batch) if batch else 0
    q = np.zeros(batch * max(na - nb + 1, 0) * width, dtype=np.uint64) if quotient else None
    r = np.zeros(batch * max(nb - 1, 0) * width, dtype=np.uint64) if remainder else None
    fn = lib().tf_poly_divide_bfe if width == 1 else lib().tf_poly_divide_xfe
    pad = np.zeros(width, dtype=np.uint64)  # stands for an empty operand (never read) or an empty output (never written)
    out = lambda x: None if x is None else _ptr(x if x.size else pad)  # noqa: E731
    _check(fn(_ptr(a if a.size else pad), na, batch, _ptr(b if b.size else pad), nb, out(q), out(r)), "divide")
    return q, r


def _elements(x, width: int, name: str) -> np.ndarray:
    x = _words(np.ascontiguousarray(x, dtype=np.uint64).reshape(-1), name)
    if width not in (1, 3) or x.size % width:
        raise ValueError(f"{name} must hold whole elements of `width` (1 or 3) words")
    return x


def batch_inversion(x: np.ndarray, width: int = 1) -> np.ndarray:
    """FiniteField::batch_inversion (math/traits.rs:93-121): the inverses of a vector of BFieldElements (width 1) or
    XFieldElements (width 3, three raw words each), as a new array.  A zero element panics (NttPanic code 12, the reference's
    assert! at :106)."""
    x = _elements(x, width, "x")
    out = np.empty_like(x)
    fn = lib().tf_batch_inversion_bfe if width == 1 else lib().tf_batch_inversion_xfe
    _check(fn(_ptr(x), x.size // width, _ptr(out)), "batch_inversion")
    return out


def inverse_or_zero(x: np.ndarray, width: int = 1) -> np.ndarray:
    """Inverse::inverse_or_zero (math/traits.rs:39-45) of every element of a vector: zero stays zero."""
    x = _elements(x, width, "x")
    out = np.empty_like(x)
    fn = lib().tf_inverse_or_zero_bfe if width == 1 else lib().tf_inverse_or_zero_xfe
    _check(fn(_ptr(x), x.size // width, _ptr(out)), "inverse_or_zero")
    return out


def _scalar(x, width: int, name: str) -> np.ndarray:
    """One field element of `width` raw words, from an int (width 1) or a sequence."""
    if width not in (1, 3):
        raise ValueError(f"the width of {name} must be 1 (BFieldElement) or 3 (XFieldElement)")
    s = np.ascontiguousarray(np.atleast_1d(np.asarray(x, dtype=np.uint64)).reshape(-1))
    if s.size != width:
        raise ValueError(f"{name} must hold {width} raw word(s)")
    return s


def linear_combination(columns: np.ndarray, weights: np.ndarray, n: int, width: int = 1, width_w: int = 1, stride=None) -> np.ndarray:
    """out[i] = sum_j columns[j][i] * weights[j] for i < n: "scalar_mul each, then Add them all" (math/polynomial.rs:498-532,
    :2526-2563) in one pass over the columns.  Column j starts `stride` words after column j - 1 (default n * width, packed), the
    layout Tip5.hash_table_rows and MerkleTree.from_columns take; weights holds one element of width_w words per column.  The result
    has n elements of max(width, width_w) words; no column gives n zeros (the reference's empty Sum)."""
    c = _words(np.ascontiguousarray(columns, dtype=np.uint64).reshape(-1), "columns")
    w = _words(np.ascontiguousarray(weights, dtype=np.uint64).reshape(-1), "weights")
    if width not in (1, 3) or width_w not in (1, 3):
        raise ValueError("width and width_w must be 1 (BFieldElement) or 3 (XFieldElement)")
    n = int(n)
    stride = n * width if stride is None else int(stride)
    if n < 0 or stride < n * width:
        raise ValueError("stride must be at least n * width words")
    if w.size % width_w:
        raise ValueError("weights must hold whole elements of width_w words")
    k = w.size // width_w
    if k and c.size < (k - 1) * stride + n * width:
        raise ValueError("columns must hold (k - 1) * stride + n * width words for the k weights")
    out = np.empty(n * max(width, width_w), dtype=np.uint64)
    if n:
        _check(lib().tf_poly_linear_combination(_ptr(c), n, width, stride, k, _ptr(w), width_w, _ptr(out)), "linear_combination")
    return out


def _width_pair(width_x: int, width_y: int) -> None:
    if (width_x, width_y) not in ((1, 1), (3, 3), (1, 3)):
        raise ValueError("(width_x, width_y) must be (1, 1), (3, 3) or (1, 3)")


def get_colinear_y(x0, y0, x1, y1, p2x, width_x: int = 1, width_y: int = 1) -> np.ndarray:
    """Polynomial::get_colinear_y (math/polynomial.rs:386-394) over n triples at once: out[i] is the y-coordinate at p2x of the line
    through (x0[i], y0[i]) and (x1[i], y1[i]).  p2x holds one element (the same point for every triple) or n.  The x-coordinates have
    width_x words, the y-coordinates, p2x and the result width_y; (1, 3) takes BFieldElement x-coordinates as their lifts.  A triple
    with x0 == x1 panics (NttPanic code 12, the reference's assert_ne! at :387)."""
    _width_pair(width_x, width_y)
    x0, x1 = _elements(x0, width_x, "x0"), _elements(x1, width_x, "x1")
    y0, y1, p2x = _elements(y0, width_y, "y0"), _elements(y1, width_y, "y1"), _elements(p2x, width_y, "p2x")
    n = x0.size // width_x
    if x1.size != x0.size or y0.size != n * width_y or y1.size != y0.size:
        raise ValueError("x0, y0, x1 and y1 must hold the same number of elements")
    n_p2x = p2x.size // width_y
    if n and n_p2x not in (1, n):
        raise ValueError("p2x must hold one element or one per triple")
    out = np.empty(n * width_y, dtype=np.uint64)
    if n:
        _check(lib().tf_get_colinear_y(_ptr(x0), _ptr(y0), _ptr(x1), _ptr(y1), n, _ptr(p2x), n_p2x, width_x, width_y, _ptr(out)), "get_colinear_y")
    return out


def are_colinear(xs, ys, k: int, width_x: int = 1, width_y: int = 1) -> np.ndarray:
    """Polynomial::are_colinear (math/polynomial.rs:348-364) over groups of exactly k points: xs and ys hold the groups one after the
    other; the result is one bool per group (False for k < 3 and for a group with a repeated x-coordinate).  k <= 1024."""
    _width_pair(width_x, width_y)
    xs, ys = _elements(xs, width_x, "xs"), _elements(ys, width_y, "ys")
    k = int(k)
    if k <= 0:
        raise ValueError("k must be positive (a group without points has no array layout)")
    if (xs.size // width_x) % k or ys.size // width_y != xs.size // width_x:
        raise ValueError("xs and ys must hold the same whole number of groups of k points")
    n_groups = xs.size // width_x // k
    flags = np.zeros(n_groups, dtype=np.int32)
    if n_groups:
        _check(lib().tf_are_colinear(_ptr(xs), _ptr(ys), n_groups, k, width_x, width_y, C.c_void_p(flags.ctypes.data)), "are_colinear")
    return flags.astype(bool)


def mod_pow(bases, exps, width: int = 1) -> np.ndarray:
    """mod_pow (b_field_element.rs:340-353, ModPowU64 for both fields) element by element: out[i] = bases[i] ^ exps[i].  Either side
    may be a single element (or an int exponent), which is then used for every element of the other.  x^0 = 1, also for x = 0."""
    bases = _elements(bases, width, "bases")
    exps = np.ascontiguousarray(np.atleast_1d(np.asarray(exps, dtype=np.uint64)).reshape(-1))
    n_bases = bases.size // width
    n = max(n_bases, exps.size) if n_bases and exps.size else 0
    if n and (n_bases not in (1, n) or exps.size not in (1, n)):
        raise ValueError("bases and exps must hold one element or the same number of elements")
    out = np.empty(n * width, dtype=np.uint64)
    if n:
        _check(lib().tf_mod_pow(_ptr(bases), n_bases, _ptr(exps), exps.size, width, _ptr(out), n), "mod_pow")
    return out


def powers(first, ratio, n: int, width: int = 1) -> np.ndarray:
    """The geometric sequence out[i] = first * ratio^i for i < n: the elements of a cyclic group (first = 1, n = the order of ratio;
    b_field_element.rs:656-668, x_field_element.rs:423-435), the powers inside Polynomial::scale, the points of an evaluation
    domain (first = the offset, ratio = the generator)."""
    f, r = _scalar(first, width, "first"), _scalar(ratio, width, "ratio")
    n = int(n)
    if n < 0:
        raise ValueError("n must not be negative")
    out = np.empty(n * width, dtype=np.uint64)
    if n:
        _check(lib().tf_powers(_ptr(f), _ptr(r), width, _ptr(out), n), "powers")
    return out


class Polynomial:
    """Coefficients low -> high degree (math/polynomial.rs:78-84); only the hot-path members."""

    def __init__(self, coefficients: np.ndarray, width: int = 1):
        c = _words(np.ascontiguousarray(coefficients, dtype=np.uint64), "coefficients").reshape(-1)
        self.width = width
        n = c.size // width
        c = c.reshape(n, width)
        while n and not c[n - 1].any():  # Polynomial::new normalises: leading zeros do not count (:degree)
            n -= 1
        self.coefficients = np.ascontiguousarray(c[:n]).reshape(-1)

    def degree(self) -> int:
        return self.coefficients.size // self.width - 1

    def fast_coset_evaluate(self, offset_raw: int, order: int) -> np.ndarray:
        if order <= self.degree():  # :1388-1392
            raise NttPanic(6, "fast_coset_evaluate")
        return fast_coset_evaluate(self.coefficients, offset_raw, order, width=self.width, batch=1)

    @classmethod
    def fast_coset_interpolate(cls, offset_raw: int, values: np.ndarray, width: int = 1) -> "Polynomial":
        """math/polynomial.rs:1907-1918; panics (NttPanic) unless len(values) is a power of two."""
        v = np.ascontiguousarray(values, dtype=np.uint64).reshape(-1)
        return cls(fast_coset_interpolate(v, offset_raw, width=width), width=width)

    def batch_evaluate(self, domain: np.ndarray) -> np.ndarray:
        """math/polynomial.rs:1840-1852: f at every point of `domain` (points of the same field as the coefficients)."""
        pts = _words(np.ascontiguousarray(domain, dtype=np.uint64).reshape(-1), "domain")
        n_points = pts.size // self.width
        out = np.empty(n_points * self.width, dtype=np.uint64)
        fn = lib().tf_poly_batch_evaluate_bfe if self.width == 1 else lib().tf_poly_batch_evaluate_xfe
        _check(fn(_ptr(self.coefficients), self.coefficients.size // self.width, _ptr(pts), n_points, _ptr(out)), "batch_evaluate")
        return out

    def evaluate_at_xfe_points(self, points: np.ndarray) -> np.ndarray:
        """Polynomial<BFieldElement>::evaluate::<XFieldElement, XFieldElement> (math/polynomial.rs:309-320) at every point of
        `points` (3 raw words each): n_points x 3 raw words."""
        if self.width != 1:
            return self.batch_evaluate(points)
        pts = _words(np.ascontiguousarray(points, dtype=np.uint64).reshape(-1), "points")
        if pts.size % 3:
            raise ValueError("points must hold whole XFieldElements")
        out = np.zeros(pts.size, dtype=np.uint64)
        _check(lib().tf_poly_evaluate_bfe_at_xfe(_ptr(self.coefficients), self.coefficients.size, 1, _ptr(pts), pts.size // 3, _ptr(out)), "evaluate")
        return out

    def clean_divide(self, divisor: "Polynomial") -> "Polynomial":
        """math/polynomial.rs:2358-2411 (BFieldElement only): self / divisor for a division known to be clean.  Panics (NttPanic)
        on a zero divisor and on an unclean division."""
        if self.width != 1 or divisor.width != 1:
            raise TypeError("clean_divide is defined for Polynomial<BFieldElement> (polynomial.rs:2333)")
        na, nb = self.coefficients.size, divisor.coefficients.size
        out = np.zeros(max(na - nb + 1, 0), dtype=np.uint64)
        _check(lib().tf_poly_clean_divide_bfe(_ptr(self.coefficients), na, _ptr(divisor.coefficients), nb, _ptr(out)), "clean_divide")
        return Polynomial(out)

    def divide(self, divisor: "Polynomial"):
        """Polynomial::divide / naive_divide (math/polynomial.rs:539-600): (quotient, remainder).  A zero divisor panics (NttPanic
        code 15, "divisor should be non-zero")."""
        if self.width != divisor.width:
            raise TypeError("dividend and divisor must be over the same field")
        q, r = poly_divide(self.coefficients, divisor.coefficients, width=self.width)
        return Polynomial(q, width=self.width), Polynomial(r, width=self.width)

    def reduce(self, modulus: "Polynomial") -> "Polynomial":
        """Polynomial::reduce / fast_reduce (math/polynomial.rs:989-1048): the remainder only (the quotient is not written)."""
        if self.width != modulus.width:
            raise TypeError("dividend and modulus must be over the same field")
        _, r = poly_divide(self.coefficients, modulus.coefficients, width=self.width, quotient=False)
        return Polynomial(r, width=self.width)

    def __truediv__(self, other: "Polynomial") -> "Polynomial":  # Div (:2502-2512): the quotient
        return self.divide(other)[0]

    def __mod__(self, other: "Polynomial") -> "Polynomial":  # Rem (:2514-2524): the remainder
        return self.reduce(other)

    def formal_power_series_inverse_newton(self, precision: int) -> "Polynomial":
        """math/polynomial.rs:1281-1366: the reference's return value, the untruncated Newton iterate ((2^R - 1) deg + 1
        coefficients, R = ilog2(next_power_of_two(precision))).  A zero constant term panics (NttPanic code 12)."""
        nf = self.coefficients.size // self.width
        n = int(lib().tf_poly_fps_inverse_newton_len(nf, precision)) if nf else 0
        out = np.zeros(max(n, 1) * self.width, dtype=np.uint64)
        fn = lib().tf_poly_fps_inverse_newton_bfe if self.width == 1 else lib().tf_poly_fps_inverse_newton_xfe
        c = self.coefficients if nf else np.zeros(self.width, dtype=np.uint64)
        _check(fn(_ptr(c), nf, precision, _ptr(out)), "formal_power_series_inverse_newton")
        return Polynomial(out[: n * self.width], width=self.width)

    @classmethod
    def zerofier(cls, roots: np.ndarray, width: int = 1) -> "Polynomial":
        """math/polynomial.rs:1435-1441 (and par_zerofier :1444-1459): the monic polynomial with exactly these roots."""
        r = _words(np.ascontiguousarray(roots, dtype=np.uint64).reshape(-1), "roots")
        if r.size % width:
            raise ValueError("roots size is not n * width")
        n = r.size // width
        out = np.empty((n + 1) * width, dtype=np.uint64)
        fn = lib().tf_poly_zerofier_bfe if width == 1 else lib().tf_poly_zerofier_xfe
        _check(fn(_ptr(r), n, _ptr(out)), "zerofier")
        return cls(out, width=width)

    @classmethod
    def interpolate(cls, domain: np.ndarray, values: np.ndarray, width: int = 1) -> "Polynomial":
        """math/polynomial.rs:1502-1520 (and par_interpolate :1525-1545, fast_interpolate :1611-1654): the lowest-degree
        polynomial through (domain[i], values[i]).  Panics (NttPanic) on an empty domain, on unequal lengths and on repeated
        domain points."""
        return cls.batch_fast_interpolate(domain, [values], width=width)[0]

    @classmethod
    def batch_fast_interpolate(cls, domain: np.ndarray, values_matrix, width: int = 1) -> list:
        """math/polynomial.rs:1703-1731: one interpolant per row of `values_matrix` over the same domain."""
        d = _words(np.ascontiguousarray(domain, dtype=np.uint64).reshape(-1), "domain")
        if d.size % width:
            raise ValueError("domain size is not n * width")
        n = d.size // width
        if n == 0:
            raise NttPanic(14, "interpolate")  # "interpolation must happen through more than zero points" (:1503-1506)
        rows = [np.ascontiguousarray(v, dtype=np.uint64).reshape(-1) for v in values_matrix]
        for v in rows:
            if v.size != n * width:
                raise NttPanic(14, "interpolate: the domain and values lists have to be of equal length")  # :1507-1511
        if not rows:
            return []
        vals = np.ascontiguousarray(np.concatenate(rows))
        out = np.empty(len(rows) * n * width, dtype=np.uint64)
        fn = lib().tf_poly_interpolate_bfe if width == 1 else lib().tf_poly_interpolate_xfe
        _check(fn(_ptr(d), _ptr(vals), n, len(rows), _ptr(out)), "interpolate")
        return [cls(out[i * n * width:(i + 1) * n * width], width=width) for i in range(len(rows))]

    @staticmethod
    def batch_coset_extrapolate(domain_offset_raw: int, codeword_length: int, codewords: np.ndarray, points: np.ndarray,
                                width: int = 1) -> np.ndarray:
        """math/polynomial.rs:2196-2208 (and par_ :2262): every codeword's interpolant at every point, codeword-major.
        Panics (NttPanic) unless codeword_length is a power of two."""
        cw = _words(np.ascontiguousarray(codewords, dtype=np.uint64).reshape(-1), "codewords")
        pts = _words(np.ascontiguousarray(points, dtype=np.uint64).reshape(-1), "points")
        n = int(codeword_length)
        batch = cw.size // (n * width) if n else 0
        n_points = pts.size // width
        out = np.empty(batch * n_points * width, dtype=np.uint64)
        fn = lib().tf_coset_extrapolate_bfe if width == 1 else lib().tf_coset_extrapolate_xfe
        _check(fn(C.c_uint64(domain_offset_raw), _ptr(cw), n, batch, _ptr(pts), n_points, _ptr(out)), "batch_coset_extrapolate")
        return out

    @staticmethod
    def coset_extrapolate(domain_offset_raw: int, codeword: np.ndarray, points: np.ndarray, width: int = 1) -> np.ndarray:
        """math/polynomial.rs:2117-2128"""
        cw = np.ascontiguousarray(codeword, dtype=np.uint64).reshape(-1)
        return Polynomial.batch_coset_extrapolate(domain_offset_raw, cw.size // width, cw, points, width=width)

    def fast_square(self) -> "Polynomial":
        """math/polynomial.rs:780-798"""
        if self.degree() < 0:
            return Polynomial(np.zeros(0, dtype=np.uint64), width=self.width)
        return Polynomial(fast_square(self.coefficients, width=self.width), width=self.width)

    def fast_multiply(self, other: "Polynomial") -> "Polynomial":
        """math/polynomial.rs:900-932 (same field on both sides)."""
        if self.width != other.width:
            raise ValueError("mixed-field products stay on the caller's side")
        if self.degree() < 0 or other.degree() < 0:
            return Polynomial(np.zeros(0, dtype=np.uint64), width=self.width)
        return Polynomial(fast_multiply(self.coefficients, other.coefficients, width=self.width), width=self.width)

    def _len(self) -> int:
        return self.coefficients.size // self.width

    def _add_sub(self, other: "Polynomial", fn, where: str) -> "Polynomial":
        if not isinstance(other, Polynomial):
            return NotImplemented
        if self.width != other.width:
            raise TypeError("both polynomials must be over the same field (Polynomial<FF> + Polynomial<FF>)")
        na, nb = self._len(), other._len()
        out = np.empty(max(na, nb) * self.width, dtype=np.uint64)
        if out.size:
            _check(fn(_ptr(self.coefficients), na, _ptr(other.coefficients), nb, self.width, _ptr(out), 1), where)
        return Polynomial(out, width=self.width)

    def __add__(self, other: "Polynomial") -> "Polynomial":  # Add (:2526-2563)
        return self._add_sub(other, lib().tf_poly_add, "add")

    def __sub__(self, other: "Polynomial") -> "Polynomial":  # Sub (:2565-)
        return self._add_sub(other, lib().tf_poly_sub, "sub")

    def __neg__(self) -> "Polynomial":  # Neg (:2700-)
        out = np.empty_like(self.coefficients)
        if out.size:
            _check(lib().tf_poly_neg(_ptr(self.coefficients), self._len(), self.width, _ptr(out), 1), "neg")
        return Polynomial(out, width=self.width)

    def _by_scalar(self, scalar, width_s: int, fn, where: str) -> "Polynomial":
        s = _scalar(scalar, width_s, "the scalar")
        wo = max(self.width, width_s)
        out = np.empty(self._len() * wo, dtype=np.uint64)
        if out.size:
            _check(fn(_ptr(self.coefficients), self._len(), self.width, _ptr(s), width_s, _ptr(out), 1), where)
        return Polynomial(out, width=wo)

    def scalar_mul(self, scalar, width_s: int = 1) -> "Polynomial":
        """math/polynomial.rs:498-532 (and Mul<S> :2650-2686): every coefficient times `scalar`, a raw word (width_s = 1) or three
        (width_s = 3); the result is over the larger of the two fields."""
        return self._by_scalar(scalar, width_s, lib().tf_poly_scalar_mul, "scalar_mul")

    def scale(self, alpha, width_alpha: int = 1) -> "Polynomial":
        """math/polynomial.rs:760-773: P(alpha * x), coefficient j times alpha^j."""
        return self._by_scalar(alpha, width_alpha, lib().tf_poly_scale, "scale")

    def formal_derivative(self) -> "Polynomial":
        """math/polynomial.rs:275-285"""
        n = self._len()
        out = np.empty(max(n - 1, 0) * self.width, dtype=np.uint64)
        if out.size:
            _check(lib().tf_poly_formal_derivative(_ptr(self.coefficients), n, self.width, _ptr(out), 1), "formal_derivative")
        return Polynomial(out, width=self.width)


def barycentric_evaluate(codewords: np.ndarray, indeterminate, width: int = 1, batch: int = 1) -> np.ndarray:
    """math/polynomial.rs:2609-2637 for `batch` codewords of equal length at one indeterminate (an int / one raw word: BFieldElement;
    three raw words: XFieldElement).  Returns batch x 3 raw words (XFieldElements), or batch words when codewords and indeterminate
    are both in the base field (the reference's BFieldElement result).  Panics (NttPanic) unless the length is a power of two, and
    when the indeterminate lies in the evaluation domain."""
    cw = _words(np.ascontiguousarray(codewords, dtype=np.uint64).reshape(-1), "codewords")
    if width not in (1, 3) or batch < 0 or (batch and cw.size % (batch * width)):
        raise ValueError("codewords size is not batch * n * width")
    n = cw.size // (batch * width) if batch else 0
    xi = np.asarray([indeterminate] if isinstance(indeterminate, (int, np.integer)) else indeterminate, dtype=np.uint64).reshape(-1)
    if xi.size not in (1, 3):
        raise ValueError("the indeterminate is one raw word (BFieldElement) or three (XFieldElement)")
    x = np.zeros(3, dtype=np.uint64)
    x[: xi.size] = xi
    out = np.zeros(3 * batch, dtype=np.uint64)
    fn = lib().tf_barycentric_evaluate_bfe if width == 1 else lib().tf_barycentric_evaluate_xfe
    _check(fn(_ptr(cw), n, batch, _ptr(x), _ptr(out)), "barycentric_evaluate")
    if width == 1 and xi.size == 1:
        return np.ascontiguousarray(out.reshape(batch, 3)[:, 0])
    return out


class ZerofierTree:
    """math/zerofier_tree.rs: the tree of vanishing polynomials of a domain, built once on the device and kept there
    (`ZerofierTree::new_from_domain` :66-87), for `Polynomial::divide_and_conquer_batch_evaluate` (polynomial.rs:1882-1894) and for
    interpolation over the same domain.  Holds device memory: use as a context manager or call close()."""

    def __init__(self, domain: np.ndarray, width: int = 1):
        d = _words(np.ascontiguousarray(domain, dtype=np.uint64).reshape(-1), "domain")
        if width not in (1, 3) or d.size % width:
            raise ValueError("domain size is not n * width")
        self.width = width
        self.num_points = d.size // width
        self._h = C.c_void_p(0)
        self._free = lib().tf_zerofier_tree_free
        fn = lib().tf_zerofier_tree_new_bfe if width == 1 else lib().tf_zerofier_tree_new_xfe
        _check(fn(_ptr(d), self.num_points, C.byref(self._h)), "ZerofierTree::new_from_domain")

    @classmethod
    def new_from_domain(cls, domain: np.ndarray, width: int = 1) -> "ZerofierTree":
        return cls(domain, width)

    def close(self) -> None:
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            self._free(h)  # bound at construction: still callable while the interpreter shuts down
            h.value = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def handle(self):
        if not self._h.value:
            raise ValueError("the tree has been closed")
        return self._h

    def zerofier(self) -> "Polynomial":
        """:93-99"""
        out = np.empty((self.num_points + 1) * self.width, dtype=np.uint64)
        _check(lib().tf_zerofier_tree_zerofier(self.handle, _ptr(out)), "ZerofierTree::zerofier")
        return Polynomial(out, width=self.width)

    def batch_evaluate(self, polynomial: "Polynomial") -> np.ndarray:
        """polynomial.divide_and_conquer_batch_evaluate(&tree) (polynomial.rs:1882-1894): the values on the tree's domain."""
        if polynomial.width != self.width:
            raise TypeError("the polynomial and the tree are over different fields")
        out = np.zeros(self.num_points * self.width, dtype=np.uint64)
        c = polynomial.coefficients
        _check(lib().tf_zerofier_tree_batch_evaluate(self.handle, _ptr(c), c.size // self.width, 1, _ptr(out)), "divide_and_conquer_batch_evaluate")
        return out

    def interpolate(self, values_matrix) -> list:
        """One interpolant per value row over the tree's domain (the memoised form of batch_fast_interpolate, polynomial.rs:1703-1838)."""
        n, w = self.num_points, self.width
        if n == 0:
            raise NttPanic(14, "interpolate")
        rows = [np.ascontiguousarray(v, dtype=np.uint64).reshape(-1) for v in values_matrix]
        for v in rows:
            if v.size != n * w:
                raise NttPanic(14, "interpolate: the domain and values lists have to be of equal length")
        if not rows:
            return []
        vals = np.ascontiguousarray(np.concatenate(rows))
        out = np.empty(len(rows) * n * w, dtype=np.uint64)
        _check(lib().tf_zerofier_tree_interpolate(self.handle, _ptr(vals), len(rows), _ptr(out)), "interpolate")
        return [Polynomial(out[i * n * w:(i + 1) * n * w], width=w) for i in range(len(rows))]


# ----------------------------------------------------------------------------- Tip5
class Digest:
    LEN = 5  # tip5/digest.rs:49
    BYTES = 40

    @staticmethod
    def to_hex(d) -> str:
        """Canonical values as little-endian bytes (tip5/digest.rs:85-90, :144-153)."""
        return b"".join(BFieldElement.value(int(v)).to_bytes(8, "little") for v in d).hex()


class Tip5:
    RATE = 10
    STATE_SIZE = 16

    @staticmethod
    def permute_states(states: np.ndarray) -> None:
        """In-place Tip5::permutation on count x 16 raw words (tip5/mod.rs:529-533)."""
        states = _words(states, "states")
        if states.size % 16:
            raise ValueError("states must hold a multiple of 16 words")
        _check(lib().tf_tip5_permute(_ptr(states), states.size // 16), "Tip5::permutation")

    @staticmethod
    def trace_states(states: np.ndarray) -> np.ndarray:
        """Tip5::trace (tip5/mod.rs:538-548) for count x 16 raw words: returns count x 6 x 16 words (the state before the permutation
        and after each round); `states` ends permuted, like `&mut self`."""
        states = _words(states, "states")
        if states.size % 16:
            raise ValueError("states must hold a multiple of 16 words")
        count = states.size // 16
        trace = np.empty(count * 96, dtype=np.uint64)
        _check(lib().tf_tip5_trace(_ptr(states), _ptr(trace), count), "Tip5::trace")
        return trace.reshape(count, 6, 16)

    @staticmethod
    def permutation(state: np.ndarray) -> np.ndarray:
        s = np.ascontiguousarray(state, dtype=np.uint64).copy()
        Tip5.permute_states(s)
        return s

    @staticmethod
    def hash_pairs(inp: np.ndarray) -> np.ndarray:
        """count x 10 words -> count x 5 words; row i is hash_10 of its 10 words (tip5/mod.rs:559-586)."""
        inp = _words(inp, "in")
        if inp.size % 10:
            raise ValueError("input must hold a multiple of 10 words")
        out = np.empty(inp.size // 2, dtype=np.uint64)
        _check(lib().tf_tip5_hash_pairs(_ptr(inp), _ptr(out), inp.size // 10), "Tip5::hash_pair")
        return out

    @staticmethod
    def hash_10(inp) -> np.ndarray:
        a = np.ascontiguousarray(inp, dtype=np.uint64)
        if a.size != 10:
            raise ValueError("hash_10 takes exactly 10 elements")
        return Tip5.hash_pairs(a)

    @staticmethod
    def hash_pair(left, right) -> np.ndarray:
        a = np.concatenate([np.asarray(left, dtype=np.uint64), np.asarray(right, dtype=np.uint64)])
        if a.size != 10:
            raise ValueError("hash_pair takes two digests")
        return Tip5.hash_pairs(a)

    @staticmethod
    def hash_varlen_rows(rows: np.ndarray, row_len: int) -> np.ndarray:
        rows = _words(rows, "rows")
        if row_len < 0 or (row_len and rows.size % row_len):
            raise ValueError("rows size is not n_rows * row_len")
        n_rows = rows.size // row_len if row_len else 0
        out = np.empty(n_rows * 5, dtype=np.uint64)
        _check(lib().tf_tip5_hash_varlen_rows(_ptr(rows), row_len, n_rows, _ptr(out)), "Tip5::hash_varlen")
        return out

    @staticmethod
    def hash_table_rows(columns: np.ndarray, n_rows: int, width: int = 1) -> np.ndarray:
        """hash_varlen of every row of a column-major table (columns back to back, n_rows elements of `width` words each):
        n_rows x 5 words."""
        t = _words(np.ascontiguousarray(columns, dtype=np.uint64).reshape(-1), "columns")
        col_words = n_rows * width
        n_cols = t.size // col_words if col_words else 0
        out = np.empty(n_rows * 5, dtype=np.uint64)
        _check(lib().tf_tip5_hash_table_rows(_ptr(t), n_rows, n_cols, width, col_words, _ptr(out), 1), "Tip5::hash_varlen")
        return out

    @staticmethod
    def hash_varlen(inp) -> np.ndarray:
        """tip5/mod.rs:617-623.  (One row; the empty input is one row of length 0.)"""
        a = np.ascontiguousarray(inp, dtype=np.uint64).reshape(-1)
        out = np.empty(5, dtype=np.uint64)
        _check(lib().tf_tip5_hash_varlen_rows(_ptr(a), a.size, 1, _ptr(out)), "Tip5::hash_varlen")
        return out


class Tip5Sponge:
    """`batch` independent Tip5 sponges stepped together (impl Sponge for Tip5, tip5/mod.rs:677-699; trait
    util_types/sponge.rs:33-55).  The state lives in a (batch, 16) array of raw words; absorb / squeeze are one batched
    Tip5::permutation on the device each, pad_and_absorb_all and the *_many / sample_* methods one library call (one kernel launch)
    for all their permutations (include/tf_hip.h, "Tip5 sponges")."""

    RATE = Tip5.RATE

    def __init__(self, batch: int = 1, fixed_length: bool = False):
        self.state = np.zeros((batch, Tip5.STATE_SIZE), dtype=np.uint64)  # Domain::VariableLength (tip5/mod.rs:511-526)
        if fixed_length:
            self.state[:, Tip5.RATE:] = BFieldElement.ONE_RAW

    @classmethod
    def init(cls, batch: int = 1) -> "Tip5Sponge":
        return cls(batch)

    def _permute(self) -> None:
        flat = self.state.reshape(-1)
        Tip5.permute_states(flat)

    def absorb(self, inp) -> None:
        """Overwrite-mode absorb of RATE elements per sponge (tip5/mod.rs:684-691)."""
        a = np.ascontiguousarray(inp, dtype=np.uint64).reshape(self.state.shape[0], Tip5.RATE)
        self.state[:, :Tip5.RATE] = a
        self._permute()

    def squeeze(self) -> np.ndarray:
        """tip5/mod.rs:693-698: the rate part, then one permutation."""
        out = self.state[:, :Tip5.RATE].copy()
        self._permute()
        return out

    def pad_and_absorb_all(self, inp) -> None:
        """util_types/sponge.rs:41-55: full chunks, then the remainder padded with 1, 0, 0, ...  One library call (one launch) for
        the whole batch.  inp: an array of batch x len words (equal lengths), or a list / tuple of `batch` rows of unequal length."""
        b = self.state.shape[0]
        st = self.state.reshape(-1)
        if isinstance(inp, (list, tuple)) and len(inp) == b and all(np.ndim(r) == 1 for r in inp):
            rows = [np.ascontiguousarray(r, dtype=np.uint64) for r in inp]
            off = np.zeros(b + 1, dtype=np.uint64)
            off[1:] = np.cumsum([r.size for r in rows], dtype=np.uint64)
            a = np.concatenate(rows) if rows else np.zeros(0, dtype=np.uint64)
            _check(lib().tf_tip5_sponge_pad_and_absorb_all(_ptr(st), b, _ptr(a), 0, _ptr(off)), "Sponge::pad_and_absorb_all")
            return
        a = np.ascontiguousarray(inp, dtype=np.uint64).reshape(b, -1)
        _check(lib().tf_tip5_sponge_pad_and_absorb_all(_ptr(st), b, _ptr(a), a.shape[1], None), "Sponge::pad_and_absorb_all")

    def absorb_many(self, chunks) -> None:
        """k successive absorb calls per sponge in one library call: chunks holds batch x k x RATE words."""
        b = self.state.shape[0]
        a = np.ascontiguousarray(chunks, dtype=np.uint64).reshape(b, -1)
        if a.shape[1] % Tip5.RATE:
            raise ValueError("chunks must hold a multiple of RATE words per sponge")
        _check(lib().tf_tip5_sponge_absorb(_ptr(self.state.reshape(-1)), b, _ptr(a), a.shape[1] // Tip5.RATE), "Sponge::absorb")

    def squeeze_many(self, k: int) -> np.ndarray:
        """k successive squeeze calls per sponge in one library call -> (batch, k, RATE) raw words."""
        b = self.state.shape[0]
        out = np.empty((b, k, Tip5.RATE), dtype=np.uint64)
        _check(lib().tf_tip5_sponge_squeeze(_ptr(self.state.reshape(-1)), b, k, _ptr(out)), "Sponge::squeeze")
        return out

    def sample_scalars(self, num_elements: int) -> np.ndarray:
        """Tip5::sample_scalars (tip5/mod.rs:664-674) per sponge -> (batch, num_elements, 3) raw words, [c0, c1, c2] each."""
        b = self.state.shape[0]
        out = np.empty((b, num_elements, 3), dtype=np.uint64)
        _check(lib().tf_tip5_sponge_sample_scalars(_ptr(self.state.reshape(-1)), b, num_elements, _ptr(out)), "Tip5::sample_scalars")
        return out

    def sample_indices(self, upper_bound: int, num_indices: int) -> np.ndarray:
        """Tip5::sample_indices (tip5/mod.rs:636-656) per sponge -> (batch, num_indices) uint32; upper_bound must be a power of
        two (the reference's assert!: TwentyFirstError with status 26 otherwise)."""
        if not 0 <= upper_bound < 2 ** 32:
            raise ValueError("upper_bound is a u32")
        b = self.state.shape[0]
        out = np.empty((b, num_indices), dtype=np.uint32)
        _check(lib().tf_tip5_sponge_sample_indices(_ptr(self.state.reshape(-1)), b, upper_bound, num_indices, _ptr(out)),
               "Tip5::sample_indices")
        return out


# ----------------------------------------------------------------------------- Merkle tree
class MerkleTree:
    """nodes: (2n, 5) raw words in the reference's heap layout (util_types/merkle_tree.rs:85-88):
    nodes[0] dummy, nodes[1] root, leaves at nodes[n:]."""

    ROOT_INDEX = 1

    def __init__(self, nodes: np.ndarray):
        self.nodes = nodes

    @classmethod
    def par_new(cls, leafs: np.ndarray) -> "MerkleTree":  # :165-212
        leafs = _words(np.ascontiguousarray(leafs, dtype=np.uint64).reshape(-1), "leafs")
        if leafs.size % 5:
            raise ValueError("leafs must hold whole digests (5 words each)")
        n = leafs.size // 5
        nodes = np.empty(max(10 * n, 1), dtype=np.uint64)
        _check(lib().tf_merkle_build(_ptr(leafs), n, _ptr(nodes), 1), "MerkleTree::par_new")
        return cls(nodes[: 10 * n].reshape(2 * n, 5))

    sequential_new = par_new  # :149-153 -- same result by construction (tests :1059-1087)

    @staticmethod
    def build_batch(leafs: np.ndarray, n_leafs: int, devices=None) -> np.ndarray:
        """`batch` independent trees of n_leafs leaves each -> (batch, 2n, 5); devices: as ntt()."""
        leafs = _words(leafs, "leafs")
        if n_leafs <= 0 or leafs.size % (5 * n_leafs):
            if n_leafs == 0:
                raise MerkleTreeError(1, "MerkleTree::par_new")
            raise ValueError("leafs size is not batch * n_leafs * 5")
        batch = leafs.size // (5 * n_leafs)
        nodes = np.empty(batch * 10 * n_leafs, dtype=np.uint64)
        if devices is not None:
            ids, k = _devices(devices)
            _check(lib().tf_merkle_build_multi(_ptr(leafs), n_leafs, _ptr(nodes), batch, ids, k), "MerkleTree::par_new")
        else:
            _check(lib().tf_merkle_build(_ptr(leafs), n_leafs, _ptr(nodes), batch), "MerkleTree::par_new")
        return nodes.reshape(batch, 2 * n_leafs, 5)

    @staticmethod
    def sequential_frugal_root(leafs: np.ndarray) -> np.ndarray:  # :299-309
        leafs = _words(np.ascontiguousarray(leafs, dtype=np.uint64).reshape(-1), "leafs")
        n = leafs.size // 5
        root = np.empty(5, dtype=np.uint64)
        _check(lib().tf_merkle_root(_ptr(leafs), n, _ptr(root), 1), "MerkleTree::sequential_frugal_root")
        return root

    @staticmethod
    def par_frugal_root(leafs: np.ndarray) -> np.ndarray:  # :332-364
        a = np.asarray(leafs)
        if a.size == 0:  # is_power_of_two() is false for 0  (:333-335)
            raise MerkleTreeError(2, "MerkleTree::par_frugal_root")
        return MerkleTree.sequential_frugal_root(leafs)

    @staticmethod
    def roots_batch(leafs: np.ndarray, n_leafs: int, devices=None) -> np.ndarray:
        leafs = _words(leafs, "leafs")
        batch = leafs.size // (5 * n_leafs) if n_leafs else 0
        roots = np.empty(max(batch, 1) * 5, dtype=np.uint64)
        if devices is not None:
            ids, k = _devices(devices)
            _check(lib().tf_merkle_root_multi(_ptr(leafs), n_leafs, _ptr(roots), batch, ids, k), "MerkleTree::par_frugal_root")
        else:
            _check(lib().tf_merkle_root(_ptr(leafs), n_leafs, _ptr(roots), batch), "MerkleTree::par_frugal_root")
        return roots[: batch * 5].reshape(batch, 5)

    @classmethod
    def from_rows(cls, rows: np.ndarray, row_len: int) -> "MerkleTree":
        """Leaves = Tip5::hash_varlen of every row (tip5/mod.rs:617-623), then par_new -- one device pipeline."""
        rows = _words(np.ascontiguousarray(rows, dtype=np.uint64).reshape(-1), "rows")
        n = rows.size // row_len if row_len else 0
        nodes = np.empty(max(10 * n, 1), dtype=np.uint64)
        _check(lib().tf_merkle_from_rows(_ptr(rows), row_len, n, _ptr(nodes), 1), "MerkleTree::par_new")
        return cls(nodes[: 10 * n].reshape(2 * n, 5))

    @classmethod
    def from_columns(cls, columns: np.ndarray, n_rows: int, width: int = 1) -> "MerkleTree":
        """Leaves = Tip5::hash_varlen of every ROW of a column-major table (one codeword per column, n_rows elements of
        `width` words each, columns back to back) -- the layout a batch of coset evaluations produces."""
        t = _words(np.ascontiguousarray(columns, dtype=np.uint64).reshape(-1), "columns")
        col_words = n_rows * width
        n_cols = t.size // col_words if col_words else 0
        nodes = np.empty(max(10 * n_rows, 1), dtype=np.uint64)
        _check(lib().tf_merkle_from_columns(_ptr(t), n_rows, n_cols, width, col_words, _ptr(nodes), 1), "MerkleTree::par_new")
        return cls(nodes[: 10 * n_rows].reshape(2 * n_rows, 5))

    @staticmethod
    def authentication_structure_node_indices(num_leafs: int, leaf_indices) -> np.ndarray:
        """util_types/merkle_tree.rs:449-504 (descending node indices); raises MerkleTreeError variants."""
        li = np.ascontiguousarray(leaf_indices, dtype=np.uint64).reshape(-1)
        cap = max(1, li.size * 66)
        out = np.empty(cap, dtype=np.uint64)
        cnt = C.c_size_t(0)
        rc = lib().tf_merkle_auth_structure_indices(num_leafs, _ptr(li), li.size, _ptr(out), cap, C.byref(cnt))
        if rc == 11:
            raise MerkleTreeError(rc, "MerkleTree::authentication_structure")
        _check(rc, "MerkleTree::authentication_structure")
        return out[: cnt.value].copy()

    def authentication_structure(self, leaf_indices) -> np.ndarray:
        """util_types/merkle_tree.rs:614-622: the digests at authentication_structure_node_indices, in that order."""
        idx = self.authentication_structure_node_indices(self.num_leafs(), leaf_indices)
        return self.nodes[idx.astype(np.int64)]

    @staticmethod
    def authentication_structure_from_leafs(leafs, leaf_indices, batch: int = 1, with_root: bool = False):
        """util_types/merkle_tree.rs:506-542: the authentication structure of `leaf_indices` from the leafs alone -- one level sweep on
        the device, no node array.  leafs: `batch` trees of equally many digests; the one index list opens every tree.  Returns
        (count, 5) raw words for batch == 1, else (batch, count, 5), in the order of authentication_structure; with_root: also the
        root(s), (5,) or (batch, 5)."""
        where = "MerkleTree::authentication_structure_from_leafs"
        leafs = _words(np.ascontiguousarray(leafs, dtype=np.uint64).reshape(-1), "leafs")
        if batch < 1 or leafs.size % (5 * batch):
            raise ValueError("leafs must hold batch trees of whole digests (5 words each)")
        n = leafs.size // (5 * batch)
        li = np.ascontiguousarray(leaf_indices, dtype=np.uint64).reshape(-1)
        lp = _ptr(leafs)
        cnt = C.c_size_t(0)
        _check(lib().tf_merkle_auth_structure_from_leafs(lp, n, batch, _ptr(li), li.size, None, 0, C.byref(cnt), None), where)
        count = cnt.value
        out = np.empty((batch, max(count, 1), 5), dtype=np.uint64)  # (one digest of room: a NULL or empty buffer is the sizing call)
        roots = np.empty((batch, 5), dtype=np.uint64)
        if count or with_root:
            _check(lib().tf_merkle_auth_structure_from_leafs(lp, n, batch, _ptr(li), li.size, _ptr(out), max(count, 1), C.byref(cnt),
                                                             _ptr(roots) if with_root else None), where)
        out = out.reshape(-1)[: batch * count * 5].reshape(batch, count, 5)
        if batch == 1:
            out, roots = out[0], roots[0]
        return (out, roots) if with_root else out

    sequential_authentication_structure_from_leafs = authentication_structure_from_leafs  # :514-522
    par_authentication_structure_from_leafs = authentication_structure_from_leafs  # :532-542 -- same result by construction

    def root(self) -> np.ndarray:  # :624-626
        return self.nodes[1]

    def num_leafs(self) -> int:  # :628-631
        return self.nodes.shape[0] // 2

    def height(self) -> int:  # :633-636
        return self.num_leafs().bit_length() - 1

    def node(self, i: int):  # :638-645
        return self.nodes[i] if 0 <= i < self.nodes.shape[0] else None

    def leafs(self) -> np.ndarray:  # :647-652
        return self.nodes[self.num_leafs():]

    def leaf(self, i: int):  # :654-661
        n = self.num_leafs()
        return self.nodes[n + i] if 0 <= i < n else None

    def indexed_leafs(self, indices) -> list:  # :665-674
        """[(leaf index, digest)] for the given indices; an index outside the tree raises LeafIndexInvalid."""
        out = []
        for i in np.asarray(indices, dtype=np.uint64).reshape(-1).tolist():
            leaf = self.leaf(int(i))
            if leaf is None:
                raise MerkleTreeError(11, "MerkleTree::indexed_leafs")
            out.append((int(i), leaf.copy()))
        return out

    def inclusion_proof_for_leaf_indices(self, indices) -> "MerkleTreeInclusionProof":  # :684-709
        indexed = self.indexed_leafs(indices)
        return MerkleTreeInclusionProof(
            self.height(),
            [i for i, _ in indexed],
            np.array([d for _, d in indexed], dtype=np.uint64).reshape(-1, 5),
            self.authentication_structure(indices),
        )


class MerkleTreeInclusionProof:
    """util_types/merkle_tree.rs:90-113, :712-777: (tree_height, indexed_leafs, authentication_structure), verified on the GPU.

    leaf_indices: (k,) uint64; leaf_digests: (k, 5) raw words, the digest of leaf_indices[i] in row i (duplicates allowed);
    authentication_structure: (a, 5) raw words.  Batches of proofs go to the device in one call (verify_batch / try_verify_batch)."""

    def __init__(self, tree_height: int, leaf_indices, leaf_digests, authentication_structure):
        if not 0 <= int(tree_height) < (1 << 32):
            raise ValueError("tree_height is a u32")
        self.tree_height = int(tree_height)
        self.leaf_indices = np.ascontiguousarray(leaf_indices, dtype=np.uint64).reshape(-1)
        self.leaf_digests = np.ascontiguousarray(leaf_digests, dtype=np.uint64).reshape(-1, 5)
        self.authentication_structure = np.ascontiguousarray(authentication_structure, dtype=np.uint64).reshape(-1, 5)
        if self.leaf_digests.shape[0] != self.leaf_indices.size:
            raise ValueError("one digest per leaf index")

    @staticmethod
    def _pack(proofs):
        heights = np.array([p.tree_height for p in proofs], dtype=np.uint32)
        leaf_off = np.zeros(len(proofs) + 1, dtype=np.uint64)
        auth_off = np.zeros(len(proofs) + 1, dtype=np.uint64)
        leaf_off[1:] = np.cumsum([p.leaf_indices.size for p in proofs])
        auth_off[1:] = np.cumsum([p.authentication_structure.shape[0] for p in proofs])
        cat = lambda xs: np.ascontiguousarray(np.concatenate(xs).reshape(-1) if xs else np.empty(0), dtype=np.uint64)  # noqa: E731
        return (heights, leaf_off, cat([p.leaf_indices for p in proofs]), cat([p.leaf_digests for p in proofs]), auth_off,
                cat([p.authentication_structure for p in proofs]))

    @staticmethod
    def try_verify_batch(proofs, roots) -> np.ndarray:
        """Status of try_verify for every proof (int32; 0 = Ok, else a MerkleTreeError code: MerkleTreeError.VARIANTS)."""
        proofs = list(proofs)
        roots = np.ascontiguousarray(roots, dtype=np.uint64).reshape(-1)
        if roots.size != 5 * len(proofs):
            raise ValueError("one root (5 words) per proof")
        h, lo, li, ld, ao, ad = MerkleTreeInclusionProof._pack(proofs)
        st = np.zeros(max(len(proofs), 1), dtype=np.int32)
        _check(lib().tf_merkle_verify_proofs(_ptr(h), len(proofs), _ptr(lo), _ptr(li), _ptr(ld), _ptr(ao), _ptr(ad), _ptr(roots), _ptr(st)),
               "MerkleTreeInclusionProof::verify")
        return st[: len(proofs)]

    @staticmethod
    def verify_batch(proofs, roots) -> np.ndarray:
        return MerkleTreeInclusionProof.try_verify_batch(proofs, roots) == 0

    def try_verify(self, root) -> None:  # :736-748
        st = int(self.try_verify_batch([self], root)[0])
        if st:
            raise MerkleTreeError(st, "MerkleTreeInclusionProof::try_verify")

    def verify(self, root) -> bool:  # :727-729
        return bool(self.verify_batch([self], root)[0])

    @staticmethod
    def authentication_paths_batch(proofs):
        """(paths, statuses): paths[p] = the (k_p, h_p, 5) authentication paths of proof p (None where statuses[p] != 0)."""
        proofs = list(proofs)
        h, lo, li, ld, ao, ad = MerkleTreeInclusionProof._pack(proofs)
        sizes = [p.leaf_indices.size * p.tree_height if p.tree_height < 64 else 0 for p in proofs]
        out = np.empty(max(5 * sum(sizes), 1), dtype=np.uint64)
        st = np.zeros(max(len(proofs), 1), dtype=np.int32)
        _check(lib().tf_merkle_authentication_paths(_ptr(h), len(proofs), _ptr(lo), _ptr(li), _ptr(ld), _ptr(ao), _ptr(ad), _ptr(out), _ptr(st)),
               "MerkleTreeInclusionProof::into_authentication_paths")
        paths, off = [], 0
        for p, n, s in zip(proofs, sizes, st.tolist()):
            paths.append(out[5 * off: 5 * (off + n)].reshape(p.leaf_indices.size, p.tree_height, 5).copy() if s == 0 else None)
            off += n
        return paths, st[: len(proofs)]

    def into_authentication_paths(self) -> np.ndarray:  # :773-777
        paths, st = self.authentication_paths_batch([self])
        if st[0]:
            raise MerkleTreeError(int(st[0]), "MerkleTreeInclusionProof::into_authentication_paths")
        return paths[0]


# ----------------------------------------------------------------------------- Merkle Mountain Range (util_types/mmr/)
class Table:
    """Whole tables between the two layouts of the library (include/tf_hip.h, "Tables"), host arrays in and out.  An element is
    `width` raw words.  Column-major: column j = n_rows elements at j * col_stride words (what Tip5.hash_table_rows and
    MerkleTree.from_columns read); row-major: row i = n_cols elements at i * row_stride words (what Tip5.hash_varlen_rows reads).  A
    stride left as None is the exact one; the padding words of a source are never read, those of a result are zero."""

    COLUMN_MAJOR = 0
    ROW_MAJOR = 1

    @staticmethod
    def _transposed(src, n_outer: int, n_inner: int, width: int, src_stride, dst_stride, batch: int, where: str) -> np.ndarray:
        src = _words(src, "table")
        if width not in (1, 3) or min(n_outer, n_inner, batch) < 0:
            raise ValueError("width must be 1 or 3 and the counts non-negative")
        ss = n_inner * width if src_stride is None else int(src_stride)
        ds = n_outer * width if dst_stride is None else int(dst_stride)
        if ss < n_inner * width or ds < n_outer * width:
            raise ValueError("a stride is shorter than its line")
        lines = batch * n_outer
        if src.size < ((lines - 1) * ss + n_inner * width if lines and n_inner else 0):
            raise ValueError("the table is smaller than batch * lines at this stride")
        out = np.zeros(batch * n_inner * ds, dtype=np.uint64)
        _check(lib().tf_table_transpose(_ptr(src), n_outer, n_inner, width, ss, _ptr(out), ds, batch), where)
        return out

    @staticmethod
    def columns_to_rows(table: np.ndarray, n_rows: int, n_cols: int, width: int = 1, col_stride=None, row_stride=None, batch: int = 1) -> np.ndarray:
        """`batch` column-major tables -> batch * n_rows * row_stride words of row-major rows."""
        return Table._transposed(table, n_cols, n_rows, width, col_stride, row_stride, batch, "Table::columns_to_rows")

    @staticmethod
    def rows_to_columns(rows: np.ndarray, n_rows: int, n_cols: int, width: int = 1, row_stride=None, col_stride=None, batch: int = 1) -> np.ndarray:
        """`batch` row-major tables -> batch * n_cols * col_stride words of column-major columns."""
        return Table._transposed(rows, n_rows, n_cols, width, row_stride, col_stride, batch, "Table::rows_to_columns")

    @staticmethod
    def gather_rows(table: np.ndarray, n_rows: int, n_cols: int, indices, layout: int = 0, width: int = 1, stride=None, batch: int = 1) -> np.ndarray:
        """Rows indices[q] of every one of `batch` tables, from either layout: (batch, k, n_cols * width) words.  An index >= n_rows
        raises TwentyFirstError (code 17)."""
        table = _words(table, "table")
        idx = np.ascontiguousarray(indices, dtype=np.uint32).reshape(-1)
        if width not in (1, 3) or layout not in (0, 1) or min(n_rows, n_cols, batch) < 0:
            raise ValueError("width must be 1 or 3, layout COLUMN_MAJOR or ROW_MAJOR and the counts non-negative")
        lines, line = (n_rows, n_cols * width) if layout == Table.ROW_MAJOR else (n_cols, n_rows * width)
        st = line if stride is None else int(stride)
        if st < line:
            raise ValueError("stride is shorter than its line")
        if table.size < ((batch * lines - 1) * st + line if batch * lines and line else 0):
            raise ValueError("the table is smaller than batch tables at this stride")
        out = np.zeros(batch * idx.size * n_cols * width, dtype=np.uint64)
        _check(lib().tf_table_gather_rows(_ptr(table), layout, n_rows, n_cols, width, st, _ptr(idx), idx.size, _ptr(out), n_cols * width, batch),
               "Table::gather_rows")
        return out.reshape(batch, idx.size, n_cols * width)


from . import mmr_index  # noqa: E402


def _digests(x, name):
    a = np.ascontiguousarray(x, dtype=np.uint64).reshape(-1, 5)
    return a


class MmrMembershipProof:
    """mmr_membership_proof.rs:23-34: the authentication path, (h, 5) raw words from the leaf upwards."""

    def __init__(self, authentication_path):
        self.authentication_path = _digests(authentication_path, "authentication_path")

    def __eq__(self, other):
        return isinstance(other, MmrMembershipProof) and np.array_equal(self.authentication_path, other.authentication_path)

    @staticmethod
    def _pack(proofs):
        off = np.zeros(len(proofs) + 1, dtype=np.uint64)
        off[1:] = np.cumsum([p.authentication_path.shape[0] for p in proofs])
        paths = np.ascontiguousarray(np.concatenate([p.authentication_path for p in proofs]).reshape(-1) if proofs else np.empty(0),
                                     dtype=np.uint64)
        return off, paths

    @staticmethod
    def verify_status_batch(proofs, leaf_indices, leaf_digests, peaks, num_leafs: int) -> np.ndarray:
        """Status of verify (:36-77) for every proof: 0 = true, else the first reason it is false (22..25, include/tf_hip.h)."""
        proofs = list(proofs)
        idx = np.ascontiguousarray(leaf_indices, dtype=np.uint64).reshape(-1)
        dig = np.ascontiguousarray(leaf_digests, dtype=np.uint64).reshape(-1)
        pk = np.ascontiguousarray(peaks, dtype=np.uint64).reshape(-1)
        if idx.size != len(proofs) or dig.size != 5 * len(proofs) or pk.size % 5:
            raise ValueError("one leaf index and one leaf digest per proof, whole peak digests")
        off, paths = MmrMembershipProof._pack(proofs)
        st = np.zeros(max(len(proofs), 1), dtype=np.int32)
        _check(lib().tf_mmr_verify_membership_proofs(C.c_uint64(num_leafs), _ptr(pk), pk.size // 5, len(proofs), _ptr(idx), _ptr(dig), _ptr(off),
                                                     _ptr(paths), _ptr(st)), "MmrMembershipProof::verify")
        return st[: len(proofs)]

    @staticmethod
    def verify_batch(proofs, leaf_indices, leaf_digests, peaks, num_leafs: int) -> np.ndarray:
        return MmrMembershipProof.verify_status_batch(proofs, leaf_indices, leaf_digests, peaks, num_leafs) == 0

    def verify(self, leaf_index: int, leaf_hash, peaks, num_leafs: int) -> bool:
        return bool(self.verify_batch([self], [leaf_index], leaf_hash, peaks, num_leafs)[0])

    @staticmethod
    def batch_update_from_batch_leaf_mutation(membership_proofs, membership_proof_leaf_indices, leaf_mutations, num_leafs: int):
        """:523-626 on the GPU; the proofs are updated in place, the indices of the changed ones are returned.  num_leafs is the MMR's
        leaf count: this call checks every index against it, where the reference checks none (include/tf_hip.h)."""
        return _mmr_mutate(None, num_leafs, membership_proofs, membership_proof_leaf_indices, leaf_mutations)[1]


    @staticmethod
    def batch_update_from_append_many(membership_proofs, membership_proof_leaf_indices, old_leaf_count: int, new_leafs, old_peaks):
        """batch_update_from_append (:224-331) and append, once per digest of new_leafs, in one call on the GPU: the proofs are
        extended in place to the accumulator of old_leaf_count + len(new_leafs) leafs; returns the indices of those that grew (the
        union of what the reference's calls return).  A proof whose length is not the height of its leaf's peak is an error
        (TF_ERR_MMR_AUTH_PATH_LENGTH_MISMATCH; the reference trusts the length, include/tf_hip.h)."""
        proofs = list(membership_proofs)
        idx = np.ascontiguousarray(membership_proof_leaf_indices, dtype=np.uint64).reshape(-1)
        if idx.size != len(proofs):
            raise ValueError(f"Lists must have same length. Got: {len(proofs)} and {idx.size}")
        leafs = np.ascontiguousarray(_digests(new_leafs, "new_leafs").reshape(-1))
        pk = np.ascontiguousarray(old_peaks, dtype=np.uint64).reshape(-1)
        off, paths = MmrMembershipProof._pack(proofs)
        out_off = np.zeros(len(proofs) + 1, dtype=np.uint64)
        mod = np.zeros(max(len(proofs), 1), dtype=np.int32)

        def call(out, capacity):
            _check(lib().tf_mmr_update_proofs_from_append(C.c_uint64(old_leaf_count), _ptr(pk), _ptr(leafs), leafs.size // 5, len(proofs), _ptr(idx),
                                                          _ptr(off), _ptr(paths), _ptr(out_off), out, capacity, _ptr(mod), None),
                   "MmrMembershipProof::batch_update_from_append")

        call(None, 0)
        out = np.empty(max(5 * int(out_off[-1]), 1), dtype=np.uint64)
        if out_off[-1]:
            call(_ptr(out), int(out_off[-1]))
        for p, a, b in zip(proofs, out_off[:-1].tolist(), out_off[1:].tolist()):
            p.authentication_path = out[5 * a: 5 * b].reshape(-1, 5).copy()
        return [i for i in range(len(proofs)) if mod[i]]

    @staticmethod
    def batch_update_from_append(membership_proofs, membership_proof_leaf_indices, old_leaf_count: int, new_leaf, old_peaks):
        """:224-331 for one appended leaf."""
        return MmrMembershipProof.batch_update_from_append_many(membership_proofs, membership_proof_leaf_indices, old_leaf_count,
                                                                np.asarray(new_leaf, dtype=np.uint64).reshape(1, 5), old_peaks)


class LeafMutation:
    """mmr_trait.rs: the leaf at leaf_index becomes new_leaf; membership_proof is its proof before the mutation."""

    def __init__(self, leaf_index: int, new_leaf, membership_proof: MmrMembershipProof):
        self.leaf_index = int(leaf_index)
        self.new_leaf = np.ascontiguousarray(new_leaf, dtype=np.uint64).reshape(5)
        self.membership_proof = membership_proof


def _mmr_mutate(peaks, leaf_count, proofs, proof_indices, mutations):
    proofs, mutations = list(proofs), list(mutations)
    pidx = np.ascontiguousarray(proof_indices, dtype=np.uint64).reshape(-1)
    if pidx.size != len(proofs):
        raise ValueError(f"Lists must have same length. Got: {len(proofs)} and {pidx.size}")
    midx = np.array([m.leaf_index for m in mutations], dtype=np.uint64)
    leafs = np.ascontiguousarray(np.concatenate([m.new_leaf for m in mutations]) if mutations else np.empty(0), dtype=np.uint64)
    moff, mpaths = MmrMembershipProof._pack([m.membership_proof for m in mutations])
    poff, ppaths = MmrMembershipProof._pack(proofs)
    mod = np.zeros(max(len(proofs), 1), dtype=np.int32)
    pk = None if peaks is None else np.ascontiguousarray(peaks, dtype=np.uint64).reshape(-1)
    _check(lib().tf_mmr_batch_mutate_leafs(C.c_uint64(leaf_count), None if pk is None else _ptr(pk), len(mutations), _ptr(midx), _ptr(leafs),
                                           _ptr(moff), _ptr(mpaths), len(proofs), _ptr(pidx), _ptr(poff), _ptr(ppaths), _ptr(mod)),
           "batch_mutate_leaf_and_update_mps")
    for p, a, b in zip(proofs, poff[:-1].tolist(), poff[1:].tolist()):
        p.authentication_path = ppaths[5 * a: 5 * b].reshape(-1, 5).copy()
    return pk, [i for i in range(len(proofs)) if mod[i]]


class MmrAccumulator:
    """mmr_accumulator.rs: leaf count and peaks (highest first, (popcount, 5) raw words), every operation on the GPU."""

    def __init__(self, leaf_count: int = 0, peaks=None):
        self.init(peaks if peaks is not None else np.empty((0, 5), dtype=np.uint64), leaf_count)

    def init(self, peaks, leaf_count: int):  # :118-124
        leaf_count = int(leaf_count)
        if not 0 <= leaf_count <= mmr_index.MAX_LEAFS:
            raise ValueError("at most 2^63 leafs (mmr.rs:12-13)")
        peaks = _digests(peaks, "peaks").copy()
        if peaks.shape[0] != bin(leaf_count).count("1"):
            raise ValueError(f"an accumulator of {leaf_count} leafs has {bin(leaf_count).count('1')} peaks, got {peaks.shape[0]}")
        self._peaks, self.leaf_count = peaks, leaf_count
        return self

    @classmethod
    def new_from_leafs(cls, leafs):  # :29-115
        acc = cls()
        acc.append_many(leafs, proofs=False)
        return acc

    def peaks(self) -> np.ndarray:
        return self._peaks.copy()

    def num_leafs(self) -> int:
        return self.leaf_count

    def bag_peaks(self) -> np.ndarray:  # :379-391
        return bag_peaks_batch([self.leaf_count], self._peaks)[0]

    def append(self, new_leaf) -> MmrMembershipProof:  # :149-159
        return self.append_many(np.asarray(new_leaf, dtype=np.uint64).reshape(1, 5))[0]

    def append_many(self, leafs, proofs: bool = True):
        """k successive appends in one call; returns their membership proofs (or None with proofs=False)."""
        leafs = _digests(leafs, "leafs")
        k, n = leafs.shape[0], self.leaf_count
        if n + k > mmr_index.MAX_LEAFS:
            raise ValueError("at most 2^63 leafs (mmr.rs:12-13)")
        if k == 0:
            return [] if proofs else None
        lens = [mmr_index.trailing_ones(n + i) for i in range(k)]
        new = np.empty(5 * bin(n + k).count("1"), dtype=np.uint64)
        out = np.empty(max(5 * sum(lens), 1), dtype=np.uint64) if proofs else None
        old = np.ascontiguousarray(self._peaks.reshape(-1))
        _check(lib().tf_mmr_append(C.c_uint64(n), _ptr(old), _ptr(np.ascontiguousarray(leafs.reshape(-1))), k, _ptr(new),
                                   _ptr(out) if proofs else None), "MmrAccumulator::append")
        self._peaks, self.leaf_count = new.reshape(-1, 5), n + k
        if not proofs:
            return None
        res, off = [], 0
        for L in lens:
            res.append(MmrMembershipProof(out[5 * off: 5 * (off + L)].reshape(-1, 5).copy()))
            off += L
        return res

    def mutate_leaf(self, leaf_mutation: LeafMutation) -> None:  # :164-175
        self.batch_mutate_leaf_and_update_mps([], [], [leaf_mutation])

    def batch_mutate_leaf_and_update_mps(self, membership_proofs, membership_proof_leaf_indices, mutation_data):  # :180-302
        """The proofs are updated in place; returns the indices of those that changed."""
        peaks, modified = _mmr_mutate(self._peaks, self.leaf_count, membership_proofs, membership_proof_leaf_indices, mutation_data)
        self._peaks = peaks.reshape(-1, 5)
        return modified


class MmrSuccessorProof:
    """mmr_successor_proof.rs:15-18: `paths`, (len, 5) raw words; states that one accumulator is what appends make of another."""

    def __init__(self, paths):
        self.paths = _digests(paths, "paths")

    def __eq__(self, other):
        return isinstance(other, MmrSuccessorProof) and np.array_equal(self.paths, other.paths)

    @classmethod
    def new_from_batch_append(cls, mmra: "MmrAccumulator", new_leafs) -> "MmrSuccessorProof":  # :34-91
        leafs = np.ascontiguousarray(_digests(new_leafs, "new_leafs").reshape(-1))
        n, k = mmra.num_leafs(), leafs.size // 5
        if n + k > mmr_index.MAX_LEAFS:
            raise ValueError("at most 2^63 leafs (mmr.rs:12-13)")
        out = np.empty(max(5 * int(lib().tf_mmr_successor_proof_len(C.c_uint64(n), C.c_uint64(k))), 1), dtype=np.uint64)
        _check(lib().tf_mmr_successor_proof_new(C.c_uint64(n), None, _ptr(leafs), k, _ptr(out), None), "MmrSuccessorProof::new_from_batch_append")
        return cls(out[: 5 * int(lib().tf_mmr_successor_proof_len(C.c_uint64(n), C.c_uint64(k)))].reshape(-1, 5).copy())

    @staticmethod
    def verify_status_batch(proofs, olds, news) -> np.ndarray:
        """Status of verify_internal (:142-223) for every (proof, old, new): 0 or its first error (27..33, include/tf_hip.h).  An
        accumulator is an MmrAccumulator or a (leaf_count, peaks) pair, which may be inconsistent."""
        proofs = list(proofs)

        def pack(accs):
            pairs = [(a.num_leafs(), a._peaks) if isinstance(a, MmrAccumulator) else (int(a[0]), _digests(a[1], "peaks")) for a in accs]
            off = np.zeros(len(pairs) + 1, dtype=np.uint64)
            off[1:] = np.cumsum([p.shape[0] for _, p in pairs])
            flat = np.ascontiguousarray(np.concatenate([p for _, p in pairs]).reshape(-1) if pairs else np.empty(0), dtype=np.uint64)
            return np.array([c for c, _ in pairs], dtype=np.uint64), off, flat

        oc, oo, od = pack(list(olds))
        nc, no, nd = pack(list(news))
        if oc.size != len(proofs) or nc.size != len(proofs):
            raise ValueError("one old and one new accumulator per proof")
        po = np.zeros(len(proofs) + 1, dtype=np.uint64)
        po[1:] = np.cumsum([p.paths.shape[0] for p in proofs])
        pd = np.ascontiguousarray(np.concatenate([p.paths for p in proofs]).reshape(-1) if proofs else np.empty(0), dtype=np.uint64)
        st = np.zeros(max(len(proofs), 1), dtype=np.int32)
        _check(lib().tf_mmr_verify_successor_proofs(len(proofs), _ptr(oc), _ptr(nc), _ptr(oo), _ptr(od), _ptr(no), _ptr(nd), _ptr(po), _ptr(pd),
                                                    _ptr(st)), "MmrSuccessorProof::verify")
        return st[: len(proofs)]

    def verify(self, old, new) -> bool:  # :94-96
        return bool(self.verify_status_batch([self], [old], [new])[0] == 0)


def bag_peaks_batch(leaf_counts, peaks) -> np.ndarray:
    """bag_peaks of many accumulators at once: peaks = every accumulator's peaks, one after the other; returns (n, 5)."""
    lc = np.ascontiguousarray(leaf_counts, dtype=np.uint64).reshape(-1)
    pk = np.ascontiguousarray(peaks, dtype=np.uint64).reshape(-1)
    out = np.empty(max(5 * lc.size, 1), dtype=np.uint64)
    _check(lib().tf_mmr_bag_peaks(_ptr(lc), lc.size, _ptr(pk), _ptr(out)), "bag_peaks")
    return out[: 5 * lc.size].reshape(-1, 5)


from . import device  # noqa: E402  (torch device-pointer API)
from . import table  # noqa: E402  (tables on the device: transposes, row opening, row-major LDE)
from . import merkle_sampled  # noqa: E402  (Merkle openings at leaf indices that are device data)
from . import fri  # noqa: E402  (the FRI split-and-fold of whole codewords)
from . import scan  # noqa: E402  (prefix scans along columns: running sums, products, the affine recurrence)
from . import deep  # noqa: E402  (DEEP quotients of the extended tables: whole codewords and sampled rows)

fri_fold = fri.fold_host  # the numpy form, next to get_colinear_y and powers
