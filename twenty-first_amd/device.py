"""Device-pointer API: the same operations on data already resident in HBM.

torch is used only as plumbing -- to own device memory and streams.  Tensors are 1-D contiguous
int64 (or uint64) CUDA tensors holding raw Montgomery words; work is enqueued on torch's current
stream (or the given one) through the tf_*_dev entry points and is NOT synchronised here.
"""
from __future__ import annotations

import ctypes as C

from . import _lib


def _chk(rc, where):
    from . import _check

    _check(rc, where)


def _t(t, name="tensor"):
    import torch

    if not isinstance(t, torch.Tensor) or not t.is_cuda or not t.is_contiguous() or t.dtype not in (torch.int64, torch.uint64):
        raise TypeError(f"{name} must be a contiguous CUDA int64/uint64 tensor of raw Montgomery words")
    return t


def _stream(stream):
    import torch

    s = stream if stream is not None else torch.cuda.current_stream()
    return C.c_void_p(s.cuda_stream)


def _p(t):
    return C.c_void_p(t.data_ptr())


def _need(cond: bool, what: str) -> None:
    """Every wrapper checks its tensors against (n, batch, width) BEFORE the C ABI sees a raw pointer: a wrong size is a
    ValueError here, never an out-of-bounds HBM access there."""
    if not cond:
        raise ValueError(what)


def _width(width: int) -> int:
    _need(width in (1, 3), "width must be 1 (BFieldElement) or 3 (XFieldElement)")
    return width


def fill_random(out, seed: int, first_index: int = 0, stream=None) -> None:
    """Synthetic inputs: out[i] = BFieldElement::new(splitmix64(seed ^ (first_index + i)) mod p), generated on
    the device; the oracle's tfo.fill_random(count, seed) is the same sequence."""
    out = _t(out, "out")
    _chk(_lib.lib().tf_debug_fill_random_dev(_p(out), out.numel(), C.c_uint64(seed & (2 ** 64 - 1)), C.c_uint64(first_index),
                                             _stream(stream)), "fill_random")


def debug_mul_pow2_(x, e: int, stream=None) -> None:
    """Test helper, in place on device: x[i] <- x[i] * 2^e mod p (canonical) for ANY 64-bit words, 0 <= e < 192, through the
    power-of-two products of the NTT networks (tf_debug_mul_pow2_dev)."""
    x = _t(x, "x")
    _need(0 <= e < 192, "the exponent must be in [0, 192)")
    _chk(_lib.lib().tf_debug_mul_pow2_dev(_p(x), x.numel(), int(e), _stream(stream)), "debug_mul_pow2")


# op name -> (TF_FIELD_OP_* code of include/tf_hip.h, elements per block W, number of outputs)
FIELD_OPS = {
    "ADD": (0, 1, 1), "SUB": (1, 1, 1), "MONT_MUL": (2, 1, 1), "ADD_SUB": (3, 1, 2), "ADD_SUB2": (4, 2, 2), "ADD_SUB_LAZY2": (5, 2, 2),
    "ADD_LAZY4": (6, 4, 1), "SUB_LAZY4": (7, 4, 1), "MONT_MUL2": (8, 2, 1), "MONT_MUL3": (9, 3, 1), "MONT_MUL4": (10, 4, 1),
    "CANONICAL": (11, 1, 1), "MX_FOLD4_CANON": (12, 4, 1), "MX_FOLD4_LAZY": (13, 4, 1), "MX_FOLD2": (14, 2, 1),
}


def debug_field_op(op: str, a, b, out0, out1=None, stream=None) -> None:
    """Test helper: one hand-scheduled field primitive of the kernels over the operand pairs (a[i], b[i]), W consecutive elements per
    thread (tf_debug_field_op_dev; FIELD_OPS lists the ops).  out1 is needed by the ops with two outputs (sum, difference) only."""
    code, _, n_out = FIELD_OPS[op]
    a, b, out0 = _t(a, "a"), _t(b, "b"), _t(out0, "out0")
    _need(b.numel() == a.numel() and out0.numel() == a.numel(), "a, b and out0 must have one length")
    if n_out == 2:
        _need(out1 is not None and _t(out1, "out1").numel() == a.numel(), f"{op} has two outputs: out1 must be as long as a")
    _chk(_lib.lib().tf_debug_field_op_dev(code, _p(a), _p(b), _p(out0), _p(out1) if n_out == 2 else None, a.numel(), _stream(stream)),
         "debug_field_op")


# form name -> (code of include/tf_hip.h, words per block); INV is the lowest bit of every code
NETWORK_FORMS = {}
for _inv in (0, 1):
    _d = "inv" if _inv else "fwd"
    for _v, _name in enumerate(("lazy", "lazy_wide2", "canonical")):
        NETWORK_FORMS[f"NET32_{_d}_{_name}"] = (0 + 2 * _v + _inv, 32)
    for _p2 in range(1, 6):
        for _lazy in (0, 1):
            NETWORK_FORMS[f"LEVELS{_p2}_{_d}_{'lazy' if _lazy else 'canonical'}"] = (6 + 4 * (_p2 - 1) + 2 * _lazy + _inv, 32)
    NETWORK_FORMS[f"TAIL5_{_d}"] = (26 + _inv, 32)
    for _logr in (1, 2, 3):
        NETWORK_FORMS[f"LAT{_logr}_{_d}"] = (28 + 2 * (_logr - 1) + _inv, 32)
    for _half in (0, 1):
        NETWORK_FORMS[f"PRE2_{_d}_half{_half}"] = (34 + 2 * _half + _inv, 64)
        NETWORK_FORMS[f"C8_{_d}_half{_half}"] = (38 + 2 * _half + _inv, 64)


def debug_ntt_network_(form: str, x, stream=None) -> None:
    """Test helper, in place on device: one composition of the NTT register networks (tf_debug_ntt_network_dev; NETWORK_FORMS lists
    the forms) over blocks of 32 consecutive words, one thread per block.  The PRE2 / C8 forms take blocks of 64 words -- 32 words x,
    then their 32 partner words w -- and write the first 32 only."""
    code, words = NETWORK_FORMS[form]
    x = _t(x, "x")
    _need(x.numel() % words == 0, f"{form} works on whole blocks of {words} words")
    _chk(_lib.lib().tf_debug_ntt_network_dev(code, _p(x), x.numel(), _stream(stream)), "debug_ntt_network")


def debug_ntt_network_config() -> dict:
    """The compile-time switches of the loaded library that decide what the network forms compute."""
    v = [C.c_int(-1) for _ in range(4)]
    _lib.lib().tf_debug_ntt_network_config(*[C.byref(i) for i in v])
    return dict(zip(("lazy", "asm_bfly", "asm_pow2", "pow2_wide"), (i.value for i in v)))


def ntt_(x, n: int, batch: int = 1, width: int = 1, inverse: bool = False, stream=None) -> None:
    """In place on device: `batch` slices of n elements (math/ntt.rs:67-82, :109-125)."""
    x = _t(x, "x")
    _width(width)
    if x.numel() != n * batch * width:
        raise ValueError("tensor size is not batch * n * width")
    fn = _lib.lib().tf_ntt_bfe_dev if width == 1 else _lib.lib().tf_ntt_xfe_dev
    _chk(fn(_p(x), n, batch, int(inverse), _stream(stream)), "intt" if inverse else "ntt")


def coset_evaluate(coeffs, n_coeffs: int, offset_raw: int, out, order: int, batch: int = 1, width: int = 1, stream=None) -> None:
    """math/polynomial.rs:1374-1399 on device buffers (out: batch * order * width words)."""
    coeffs, out = _t(coeffs, "coeffs"), _t(out, "out")
    _width(width)
    if coeffs.numel() != n_coeffs * batch * width or out.numel() != order * batch * width:
        raise ValueError("buffer sizes do not match n_coeffs/order/batch/width")
    fn = _lib.lib().tf_coset_eval_bfe_dev if width == 1 else _lib.lib().tf_coset_eval_xfe_dev
    _chk(fn(_p(coeffs), n_coeffs, C.c_uint64(offset_raw), _p(out), order, batch, _stream(stream)), "fast_coset_evaluate")


def tip5_permute_(states, stream=None) -> None:
    states = _t(states, "states")
    _need(states.numel() % 16 == 0, "states must hold 16 words per Tip5 state")
    _chk(_lib.lib().tf_tip5_permute_dev(_p(states), states.numel() // 16, _stream(stream)), "Tip5::permutation")


def tip5_trace_(states, trace, stream=None) -> None:
    """Tip5::trace (tip5/mod.rs:538-548) on device buffers: trace = count x 6 x 16 words, states permuted in place."""
    states, trace = _t(states, "states"), _t(trace, "trace")
    _need(states.numel() % 16 == 0 and trace.numel() == 6 * states.numel(), "trace must hold 6 x 16 words per Tip5 state")
    _chk(_lib.lib().tf_tip5_trace_dev(_p(states), _p(trace), states.numel() // 16, _stream(stream)), "Tip5::trace")


def tip5_hash_pairs(inp, out, stream=None) -> None:
    inp, out = _t(inp, "in"), _t(out, "out")
    _need(inp.numel() % 10 == 0, "in must hold 10 words per pair of digests")
    count = inp.numel() // 10
    if out.numel() != count * 5:
        raise ValueError("out must hold 5 words per input pair")
    _chk(_lib.lib().tf_tip5_hash_pairs_dev(_p(inp), _p(out), count, _stream(stream)), "Tip5::hash_pair")


def tip5_hash_varlen_rows(rows, row_len: int, out, stream=None) -> None:
    rows, out = _t(rows, "rows"), _t(out, "out")
    _need(out.numel() % 5 == 0, "out must hold 5 words per row")
    n_rows = out.numel() // 5
    _need(row_len >= 0 and rows.numel() == n_rows * row_len, "rows must hold n_rows * row_len words (n_rows = out.numel() / 5)")
    _chk(_lib.lib().tf_tip5_hash_varlen_rows_dev(_p(rows), row_len, n_rows, _p(out), _stream(stream)), "Tip5::hash_varlen")


def merkle_build(leaves, n_leaves: int, nodes_out, batch: int = 1, stream=None) -> None:
    """util_types/merkle_tree.rs:165-212: nodes_out = batch x 2n digests, heap layout."""
    leaves, nodes_out = _t(leaves, "leaves"), _t(nodes_out, "nodes_out")
    if leaves.numel() != batch * n_leaves * 5 or nodes_out.numel() != batch * n_leaves * 10:
        raise ValueError("buffer sizes do not match n_leaves/batch")
    _chk(_lib.lib().tf_merkle_build_dev(_p(leaves), n_leaves, _p(nodes_out), batch, _stream(stream)), "MerkleTree::par_new")


def merkle_root(leaves, n_leaves: int, root_out, batch: int = 1, stream=None) -> None:
    leaves, root_out = _t(leaves, "leaves"), _t(root_out, "root_out")
    _need(leaves.numel() == batch * n_leaves * 5 and root_out.numel() == batch * 5, "buffer sizes do not match n_leaves/batch")
    _chk(_lib.lib().tf_merkle_root_dev(_p(leaves), n_leaves, _p(root_out), batch, _stream(stream)), "MerkleTree::par_frugal_root")


def _proof_layout(tree_heights, leaf_offsets, auth_offsets):
    """Host arrays of a batch of inclusion proofs (include/tf_hip.h, "Inclusion proofs"): heights as u32, CSR offsets as u64."""
    import numpy as np

    h = np.ascontiguousarray(tree_heights, dtype=np.uint32).reshape(-1)
    lo = np.ascontiguousarray(leaf_offsets, dtype=np.uint64).reshape(-1)
    ao = np.ascontiguousarray(auth_offsets, dtype=np.uint64).reshape(-1)
    _need(lo.size == h.size + 1 and ao.size == h.size + 1, "leaf_offsets and auth_offsets need n_proofs + 1 entries")
    return h, lo, ao


def _host(a):
    return C.c_void_p(a.ctypes.data) if a.size else C.c_void_p(0)


def _status_tensor(statuses, n: int):
    import torch

    _need(isinstance(statuses, torch.Tensor) and statuses.is_cuda and statuses.is_contiguous() and statuses.dtype == torch.int32
          and statuses.numel() >= n, "statuses must be a contiguous CUDA int32 tensor of n_proofs entries")
    return statuses


def verify_inclusion_proofs(tree_heights, leaf_offsets, leaf_indices, leaf_digests, auth_offsets, auth_digests, expected_roots, statuses,
                            stream=None) -> None:
    """MerkleTreeInclusionProof::try_verify of a batch (util_types/merkle_tree.rs:736-748): statuses[p] (device int32) receives proof p's
    verdict (0 = Ok, else a MerkleTreeError code).  tree_heights and the offsets are host arrays; leaf_indices (k words),
    leaf_digests (5 k), auth_digests (5 a) and expected_roots (5 n) are device tensors.  Nothing is synchronised."""
    h, lo, ao = _proof_layout(tree_heights, leaf_offsets, auth_offsets)
    n = h.size
    leaf_indices, leaf_digests = _t(leaf_indices, "leaf_indices"), _t(leaf_digests, "leaf_digests")
    auth_digests, expected_roots = _t(auth_digests, "auth_digests"), _t(expected_roots, "expected_roots")
    statuses = _status_tensor(statuses, n)
    k, a = int(lo[-1]) if n else 0, int(ao[-1]) if n else 0
    _need(leaf_indices.numel() >= k and leaf_digests.numel() >= 5 * k and auth_digests.numel() >= 5 * a and expected_roots.numel() >= 5 * n,
          "buffer sizes do not match the offsets")
    _chk(_lib.lib().tf_merkle_verify_proofs_dev(_host(h), n, _host(lo), _p(leaf_indices), _p(leaf_digests), _host(ao), _p(auth_digests),
                                                _p(expected_roots), _p(statuses), _stream(stream)), "MerkleTreeInclusionProof::verify")


def authentication_path_words(tree_heights, leaf_offsets) -> int:
    """Words of paths_out for a batch: 5 k_p h_p per proof of height < 64."""
    import numpy as np

    h = np.asarray(tree_heights, dtype=np.uint64).reshape(-1)
    k = np.diff(np.asarray(leaf_offsets, dtype=np.uint64).reshape(-1))
    return 5 * int(np.sum(np.where(h < 64, k * h, 0)))


def authentication_paths(tree_heights, leaf_offsets, leaf_indices, leaf_digests, auth_offsets, auth_digests, paths_out, statuses,
                         stream=None) -> None:
    """MerkleTreeInclusionProof::into_authentication_paths of a batch (:773-777): paths_out (device, authentication_path_words words)
    receives proof after proof k_p x h_p digests, leaf-major; statuses as verify_inclusion_proofs.  Nothing is synchronised."""
    h, lo, ao = _proof_layout(tree_heights, leaf_offsets, auth_offsets)
    n = h.size
    leaf_indices, leaf_digests = _t(leaf_indices, "leaf_indices"), _t(leaf_digests, "leaf_digests")
    auth_digests, paths_out = _t(auth_digests, "auth_digests"), _t(paths_out, "paths_out")
    statuses = _status_tensor(statuses, n)
    k, a = int(lo[-1]) if n else 0, int(ao[-1]) if n else 0
    _need(leaf_indices.numel() >= k and leaf_digests.numel() >= 5 * k and auth_digests.numel() >= 5 * a
          and paths_out.numel() >= authentication_path_words(h, lo), "buffer sizes do not match the offsets")
    _chk(_lib.lib().tf_merkle_authentication_paths_dev(_host(h), n, _host(lo), _p(leaf_indices), _p(leaf_digests), _host(ao), _p(auth_digests),
                                                       _p(paths_out), _p(statuses), _stream(stream)),
         "MerkleTreeInclusionProof::into_authentication_paths")


# ---- the callers on either side of the path, kept in HBM --------------------------------

def coset_interpolate(values, n: int, offset_raw: int, out, batch: int = 1, width: int = 1, stream=None) -> None:
    """math/polynomial.rs:1907-1918 on device buffers (out: batch * n * width words; may alias values)."""
    values, out = _t(values, "values"), _t(out, "out")
    _width(width)
    _need(values.numel() == n * batch * width and out.numel() == n * batch * width, "buffer sizes do not match n/batch/width")
    fn = _lib.lib().tf_coset_interpolate_bfe_dev if width == 1 else _lib.lib().tf_coset_interpolate_xfe_dev
    _chk(fn(_p(values), n, C.c_uint64(offset_raw), _p(out), batch, _stream(stream)), "fast_coset_interpolate")


def hadamard(a, b, out, width: int = 1, stream=None, width_b=None) -> None:
    """Pointwise field product (math/polynomial.rs:920-925); out may alias a or b.  width = 3 with width_b = 1 is Mul<BFieldElement>
    for XFieldElement (x_field_element.rs:540-548): b holds one word per element of a, and out may alias a."""
    a, b, out = _t(a, "a"), _t(b, "b"), _t(out, "out")
    _width(width)
    if width_b is not None and width_b != width:
        _need(width == 3 and width_b == 1, "the mixed product is XFieldElement (width 3) times BFieldElement (width_b 1)")
        _need(a.numel() % 3 == 0 and b.numel() * 3 == a.numel() and out.numel() == a.numel(), "a and out must hold three words per word of b")
        _chk(_lib.lib().tf_hadamard_xfe_bfe_dev(_p(a), _p(b), _p(out), b.numel(), _stream(stream)), "hadamard")
        return
    _need(a.numel() % width == 0 and b.numel() == a.numel() and out.numel() == a.numel(), "a, b and out must hold the same number of elements")
    fn = _lib.lib().tf_hadamard_bfe_dev if width == 1 else _lib.lib().tf_hadamard_xfe_dev
    _chk(fn(_p(a), _p(b), _p(out), a.numel() // width, _stream(stream)), "hadamard")


def _apart_or_same(x, out, what: str) -> None:
    xb, ob = x.numel() * 8, out.numel() * 8
    _need((out.data_ptr() == x.data_ptr() and ob == xb) or out.data_ptr() >= x.data_ptr() + xb or x.data_ptr() >= out.data_ptr() + ob, what)


def _apart(x, out, what: str) -> None:
    _need(out.data_ptr() >= x.data_ptr() + x.numel() * 8 or x.data_ptr() >= out.data_ptr() + out.numel() * 8, what)


def _poly_add_sub(fn, where, a, na: int, b, nb: int, out, batch: int, width: int, stream) -> None:
    a, b, out = _t(a, "a"), _t(b, "b"), _t(out, "out")
    _width(width)
    _need(na >= 0 and nb >= 0 and batch >= 0, "lengths and batch must not be negative")
    _need(a.numel() == na * batch * width and b.numel() == nb * batch * width, "operand sizes do not match na/nb/batch/width")
    _need(out.numel() == max(na, nb) * batch * width, "out must hold batch * max(na, nb) coefficients")
    _apart_or_same(a, out, "out must be an operand of its own length or not overlap it")
    _apart_or_same(b, out, "out must be an operand of its own length or not overlap it")
    _chk(fn(_p(a), na, _p(b), nb, width, _p(out), batch, _stream(stream)), where)


def poly_add(a, na: int, b, nb: int, out, batch: int = 1, width: int = 1, stream=None) -> None:
    """Polynomial + Polynomial (math/polynomial.rs:2526-2563) on device buffers: out = batch x max(na, nb) coefficients; out may be
    the operand of that length."""
    _poly_add_sub(_lib.lib().tf_poly_add_dev, "add", a, na, b, nb, out, batch, width, stream)


def poly_sub(a, na: int, b, nb: int, out, batch: int = 1, width: int = 1, stream=None) -> None:
    """Polynomial - Polynomial (math/polynomial.rs:2565-) on device buffers, as poly_add."""
    _poly_add_sub(_lib.lib().tf_poly_sub_dev, "sub", a, na, b, nb, out, batch, width, stream)


def poly_neg_(a, na: int, out=None, batch: int = 1, width: int = 1, stream=None) -> None:
    """Neg (math/polynomial.rs:2700-) on device buffers; in place when out is None."""
    a = _t(a, "a")
    out = a if out is None else _t(out, "out")
    _width(width)
    _need(na >= 0 and a.numel() == na * batch * width and out.numel() == a.numel(), "buffer sizes do not match na/batch/width")
    _apart_or_same(a, out, "out must be a itself or not overlap it")
    _chk(_lib.lib().tf_poly_neg_dev(_p(a), na, width, _p(out), batch, _stream(stream)), "neg")


def _scalar_words(x, width: int, name: str):
    import numpy as np

    _width(width)
    s = np.ascontiguousarray(np.atleast_1d(np.asarray(x, dtype=np.uint64)).reshape(-1))
    _need(s.size == width, f"{name} must hold {width} raw word(s)")
    return s


def _poly_by_scalar(fn, where, a, na: int, scalar, out, batch: int, width: int, width_s: int, stream) -> None:
    a, out = _t(a, "a"), _t(out, "out")
    _width(width)
    s = _scalar_words(scalar, width_s, "the scalar")
    wo = max(width, width_s)
    _need(na >= 0 and a.numel() == na * batch * width and out.numel() == na * batch * wo, "buffer sizes do not match na/batch/widths")
    _apart_or_same(a, out, "out must be a itself (same element width) or not overlap it")
    _chk(fn(_p(a), na, width, C.c_void_p(s.ctypes.data), width_s, _p(out), batch, _stream(stream)), where)


def poly_scalar_mul(a, na: int, scalar, out, batch: int = 1, width: int = 1, width_s: int = 1, stream=None) -> None:
    """scalar_mul (math/polynomial.rs:498-532, Mul<S> :2650-2686) on device buffers: every coefficient times the HOST scalar (an int
    or width_s raw words); out holds max(width, width_s) words per coefficient and may be a when the widths agree."""
    _poly_by_scalar(_lib.lib().tf_poly_scalar_mul_dev, "scalar_mul", a, na, scalar, out, batch, width, width_s, stream)


def poly_scale(a, na: int, alpha, out, batch: int = 1, width: int = 1, width_alpha: int = 1, stream=None) -> None:
    """scale (math/polynomial.rs:760-773) on device buffers: out[j] = a[j] * alpha^j, alpha a HOST scalar; sizes as poly_scalar_mul."""
    _poly_by_scalar(_lib.lib().tf_poly_scale_dev, "scale", a, na, alpha, out, batch, width, width_alpha, stream)


def poly_formal_derivative(a, na: int, out, batch: int = 1, width: int = 1, stream=None) -> None:
    """formal_derivative (math/polynomial.rs:275-285) on device buffers: out = batch x (na - 1) coefficients, not overlapping a."""
    a, out = _t(a, "a"), _t(out, "out")
    _width(width)
    _need(na >= 0 and a.numel() == na * batch * width and out.numel() == max(na - 1, 0) * batch * width, "buffer sizes do not match na/batch/width")
    _apart(a, out, "out must not overlap a")
    _chk(_lib.lib().tf_poly_formal_derivative_dev(_p(a), na, width, _p(out), batch, _stream(stream)), "formal_derivative")


def poly_degree(a, na: int, degrees, batch: int = 1, width: int = 1, stream=None) -> None:
    """degree (math/polynomial.rs:181) of `batch` packed polynomials into an int64 tensor of `batch` entries (-1: the zero
    polynomial).  Only enqueues."""
    import torch

    a = _t(a, "a")
    _width(width)
    _need(isinstance(degrees, torch.Tensor) and degrees.is_cuda and degrees.is_contiguous() and degrees.dtype == torch.int64
          and degrees.numel() == batch, "degrees must be a contiguous CUDA int64 tensor of `batch` entries")
    _need(na >= 0 and a.numel() == na * batch * width, "a does not match na/batch/width")
    _chk(_lib.lib().tf_poly_degree_dev(_p(a), na, width, batch, _p(degrees), _stream(stream)), "degree")


def linear_combination(columns, n: int, k: int, weights, out, width: int = 1, width_w: int = 1, stride=None, stream=None) -> None:
    """out[i] = sum_{j<k} columns[j * stride + i] * weights[j], i < n, on device buffers (weights too: k x width_w words, where
    tip5_sponge_sample_scalars leaves them).  stride counts words (default n * width); out = n x max(width, width_w) words and
    overlaps no input."""
    columns, weights, out = _t(columns, "columns"), _t(weights, "weights"), _t(out, "out")
    _width(width)
    _width(width_w)
    stride = n * width if stride is None else int(stride)
    _need(n >= 0 and k >= 0 and stride >= n * width, "stride must be at least n * width words")
    _need(weights.numel() == k * width_w, "weights must hold k elements of width_w words")
    _need(k == 0 or columns.numel() >= (k - 1) * stride + n * width, "columns must hold (k - 1) * stride + n * width words")
    _need(out.numel() == n * max(width, width_w), "out must hold n elements of max(width, width_w) words")
    _apart(columns, out, "out must not overlap the columns")
    _apart(weights, out, "out must not overlap the weights")
    _chk(_lib.lib().tf_poly_linear_combination_dev(_p(columns), n, width, stride, k, _p(weights), width_w, _p(out), _stream(stream)),
         "linear_combination")


def poly_mul(a, na: int, b, nb: int, out, batch: int = 1, width: int = 1, stream=None) -> None:
    """Polynomial::fast_multiply on device (math/polynomial.rs:900-932): out = batch x (na + nb - 1) coefficients."""
    a, b, out = _t(a, "a"), _t(b, "b"), _t(out, "out")
    _width(width)
    _need(a.numel() == na * batch * width and b.numel() == nb * batch * width, "operand sizes do not match na/nb/batch/width")
    _need(not (na and nb) or out.numel() == (na + nb - 1) * batch * width, "out must hold batch * (na + nb - 1) coefficients")
    fn = _lib.lib().tf_poly_mul_bfe_dev if width == 1 else _lib.lib().tf_poly_mul_xfe_dev
    _chk(fn(_p(a), na, _p(b), nb, _p(out), batch, _stream(stream)), "fast_multiply")


def poly_mul_shared(a, na: int, b, out, batch: int, width: int = 1, stream=None) -> None:
    """`batch` polynomials of na coefficients each times ONE polynomial b (tf_poly_mul_shared_*_dev): out = batch x (na + nb - 1)."""
    a, b, out = _t(a, "a"), _t(b, "b"), _t(out, "out")
    w = _width(width)
    _need(b.numel() % w == 0 and a.numel() == batch * na * w, "a must hold batch * na elements, b whole elements")
    nb = b.numel() // w
    _need(nb >= 1 and out.numel() == batch * (na + nb - 1) * w, "out must hold batch * (na + nb - 1) coefficients")
    fn = _lib.lib().tf_poly_mul_shared_bfe_dev if width == 1 else _lib.lib().tf_poly_mul_shared_xfe_dev
    _chk(fn(_p(a), na, batch, _p(b), nb, _p(out), _stream(stream)), "fast_multiply")


def lde(values, n: int, offset_in_raw: int, out, m: int, offset_out_raw: int, batch: int = 1, width: int = 1, stream=None) -> None:
    """Low-degree extension: interpolate on {offset_in w_n^i}, evaluate on {offset_out w_m^i}; coefficients stay in HBM."""
    values, out = _t(values, "values"), _t(out, "out")
    _width(width)
    _need(values.numel() == n * batch * width and out.numel() == m * batch * width, "buffer sizes do not match n/m/batch/width")
    fn = _lib.lib().tf_lde_bfe_dev if width == 1 else _lib.lib().tf_lde_xfe_dev
    _chk(fn(_p(values), n, C.c_uint64(offset_in_raw), _p(out), m, C.c_uint64(offset_out_raw), batch, _stream(stream)), "lde")


def merkle_from_rows(rows, row_len: int, n_rows: int, nodes_out, batch: int = 1, stream=None) -> None:
    """hash_varlen of every row -> leaf level -> tree, without the leaves leaving HBM."""
    rows, nodes_out = _t(rows, "rows"), _t(nodes_out, "nodes_out")
    _need(rows.numel() == batch * n_rows * row_len and nodes_out.numel() == batch * n_rows * 10, "buffer sizes do not match row_len/n_rows/batch")
    _chk(_lib.lib().tf_merkle_from_rows_dev(_p(rows), row_len, n_rows, _p(nodes_out), batch, _stream(stream)), "MerkleTree::par_new")


def authentication_structure(nodes, num_leafs: int, leaf_indices):
    """util_types/merkle_tree.rs:614-622 from a device-resident node array: returns a (k, 5) numpy array."""
    import numpy as np

    nodes = _t(nodes, "nodes")
    _need(nodes.numel() == num_leafs * 10, "nodes must hold 2 * num_leafs digests")
    li = np.ascontiguousarray(leaf_indices, dtype=np.uint64).reshape(-1)
    cap = max(1, li.size * 66)
    out = np.empty(cap * 5, dtype=np.uint64)
    cnt = C.c_size_t(0)
    rc = _lib.lib().tf_merkle_authentication_structure_dev(_p(nodes), num_leafs, C.c_void_p(li.ctypes.data) if li.size else C.c_void_p(0),
                                                           li.size, C.c_void_p(out.ctypes.data), cap, C.byref(cnt), _stream(None))
    _chk(rc, "MerkleTree::authentication_structure")
    return out[: cnt.value * 5].reshape(-1, 5).copy()


def authentication_structure_from_leafs(leafs, num_leafs: int, leaf_indices, out=None, roots=None, batch: int = 1, stream=None):
    """util_types/merkle_tree.rs:506-542 on device buffers: the authentication structure of `leaf_indices` (a HOST list, the same for
    every tree) from `batch` trees of num_leafs leaf digests, without a node array; `roots` (batch * 5 words), when given, receives
    the roots.  Returns the device tensor of batch * count * 5 words (tree-major, the order of authentication_structure): `out` when
    given -- it must hold at least that many words --, otherwise a new tensor.  Nothing is synchronised."""
    import numpy as np
    import torch

    where = "MerkleTree::authentication_structure_from_leafs"
    leafs = _t(leafs, "leafs")
    _need(batch >= 1 and leafs.numel() == batch * num_leafs * 5, "leafs must hold batch * num_leafs digests")
    li = np.ascontiguousarray(leaf_indices, dtype=np.uint64).reshape(-1)
    fn = _lib.lib().tf_merkle_auth_structure_from_leafs_dev
    lp = _p(leafs)
    cnt = C.c_size_t(0)
    _chk(fn(lp, num_leafs, batch, _host(li), li.size, None, 0, C.byref(cnt), None, _stream(stream)), where)
    count = cnt.value
    words = batch * count * 5
    if out is None:
        out = torch.empty(max(words, 5), dtype=torch.int64, device=leafs.device)  # (one digest of room: an empty buffer is the sizing call)
    else:
        out = _t(out, "out")
        _need(out.numel() >= max(words, 1), "out must hold batch * count digests (and at least one word)")
    if roots is not None:
        roots = _t(roots, "roots")
        _need(roots.numel() == batch * 5, "roots must hold one digest per tree")
    if count or roots is not None:
        _chk(fn(lp, num_leafs, batch, _host(li), li.size, _p(out), max(count, 1), C.byref(cnt), _p(roots) if roots is not None else None,
                _stream(stream)), where)
    return out[:words]


def authentication_structure_from_leafs_workspace(num_leafs: int, batch: int, k_nodes: int) -> int:
    """Bytes of device work space authentication_structure_from_leafs requests from the library's pool for k_nodes structure nodes per
    tree (tf_merkle_auth_structure_from_leafs_workspace: host arithmetic, no device needed)."""
    return int(_lib.lib().tf_merkle_auth_structure_from_leafs_workspace(num_leafs, batch, k_nodes))


def batch_evaluate(coeffs, n_coeffs: int, points, out, width: int = 1, stream=None) -> None:
    """Polynomial::batch_evaluate (math/polynomial.rs:1840-1878) on device buffers: out[i] = f(points[i])."""
    coeffs, points, out = _t(coeffs, "coeffs"), _t(points, "points"), _t(out, "out")
    if points.numel() != out.numel() or coeffs.numel() != n_coeffs * width:
        raise ValueError("buffer sizes do not match n_coeffs/points/width")
    fn = _lib.lib().tf_poly_batch_evaluate_bfe_dev if width == 1 else _lib.lib().tf_poly_batch_evaluate_xfe_dev
    _chk(fn(_p(coeffs), n_coeffs, _p(points), points.numel() // width, _p(out), _stream(stream)), "batch_evaluate")


def evaluate_bfe_at_xfe(coeffs, n_coeffs: int, points, out, batch: int = 1, stream=None) -> None:
    """Polynomial<BFieldElement>::evaluate with XFieldElement indeterminates (math/polynomial.rs:309-320) on device buffers: `batch`
    base-field polynomials at the XFieldElement points -> out[(b * n_points + i) * 3]."""
    coeffs, points, out = _t(coeffs, "coeffs"), _t(points, "points"), _t(out, "out")
    _need(points.numel() % 3 == 0 and coeffs.numel() == batch * n_coeffs and out.numel() == batch * points.numel(),
          "coeffs = batch * n_coeffs words, points = n_points XFieldElements, out = batch * n_points XFieldElements")
    _chk(_lib.lib().tf_poly_evaluate_bfe_at_xfe_dev(_p(coeffs), n_coeffs, batch, _p(points), points.numel() // 3, _p(out), _stream(stream)), "evaluate")


def _status(status):
    """`status`: a one-element int32 CUDA tensor the *_dev_async entry points report the reference's panic cases through
    (first non-zero tf_status code wins); with it a wrapper enqueues and returns without ever synchronising the stream."""
    import torch

    if not isinstance(status, torch.Tensor) or not status.is_cuda or status.dtype != torch.int32 or status.numel() != 1:
        raise TypeError("status must be a one-element int32 CUDA tensor")
    return C.c_void_p(status.data_ptr())


def clean_divide(a, b, out, stream=None, status=None) -> None:
    """Polynomial::<BFieldElement>::clean_divide (math/polynomial.rs:2358-2411) on device buffers: a, b normalised coefficient
    arrays, out = the na - nb + 1 quotient coefficients.  status: see _status (no host synchronisation)."""
    a, b, out = _t(a, "a"), _t(b, "b"), _t(out, "out")
    _need(a.numel() >= b.numel() and out.numel() == a.numel() - b.numel() + 1, "out must hold na - nb + 1 coefficients")
    if status is not None:
        _chk(_lib.lib().tf_poly_clean_divide_bfe_dev_async(_p(a), a.numel(), _p(b), b.numel(), _p(out), _stream(stream), _status(status)), "clean_divide")
        return
    _chk(_lib.lib().tf_poly_clean_divide_bfe_dev(_p(a), a.numel(), _p(b), b.numel(), _p(out), _stream(stream)), "clean_divide")


def clean_divide_many(a, na: int, b, out, batch: int, stream=None, status=None) -> None:
    """`batch` dividends of na coefficients each over one divisor (tf_poly_clean_divide_many_bfe_dev): out = batch x (na - nb + 1)."""
    a, b, out = _t(a, "a"), _t(b, "b"), _t(out, "out")
    _need(a.numel() == batch * na and na >= b.numel() and out.numel() == batch * (na - b.numel() + 1), "a = batch * na, out = batch * (na - nb + 1) coefficients")
    if status is not None:
        _chk(_lib.lib().tf_poly_clean_divide_many_bfe_dev_async(_p(a), na, batch, _p(b), b.numel(), _p(out), _stream(stream), _status(status)), "clean_divide")
        return
    _chk(_lib.lib().tf_poly_clean_divide_many_bfe_dev(_p(a), na, batch, _p(b), b.numel(), _p(out), _stream(stream)), "clean_divide")


def divide(a, na: int, b, q, r, batch: int = 1, width: int = 1, stream=None, status=None) -> None:
    """Polynomial::divide (math/polynomial.rs:539-600) of `batch` dividends of na coefficients each over ONE divisor b
    (tf_poly_divide_*_dev): q = batch x max(na - nb + 1, 0), r = batch x (nb - 1) coefficients; either may be None (not written).
    b must be normalised (b[nb-1] != 0, else 17 in status).  status: a one-element int32 CUDA tensor (first non-zero code wins);
    without one a scratch word is used and checked after a synchronisation.  Never synchronises otherwise."""
    import torch

    width = _width(width)
    a, b = _t(a, "a"), _t(b, "b")
    _need(b.numel() % width == 0 and a.numel() == batch * na * width, "a = batch * na elements, b whole elements")
    nb = b.numel() // width
    _need(nb > 0, "the divisor must have a coefficient")  # (the C ABI's nb == 0 is TF_ERR_DIVISION_BY_ZERO)
    k, m = max(na - nb + 1, 0), nb - 1
    if q is not None:
        q = _t(q, "q")
        _need(q.numel() == batch * k * width, "q must hold batch * max(na - nb + 1, 0) elements")
    if r is not None:
        r = _t(r, "r")
        _need(r.numel() == batch * m * width, "r must hold batch * (nb - 1) elements")
    own = status is None
    st = torch.zeros(1, dtype=torch.int32, device=a.device) if own else status
    fn = _lib.lib().tf_poly_divide_bfe_dev if width == 1 else _lib.lib().tf_poly_divide_xfe_dev
    _chk(fn(_p(a), na, batch, _p(b), nb, _p(q) if q is not None else None, _p(r) if r is not None else None, _stream(stream), _status(st)),
         "divide")
    if own:
        (stream or torch.cuda.current_stream()).synchronize()
        _chk(int(st.item()), "divide")


def fps_inverse_newton(f, precision: int, out, width: int = 1, stream=None, status=None) -> None:
    """Polynomial::formal_power_series_inverse_newton (math/polynomial.rs:1281-1366) on device buffers: out receives
    tf_poly_fps_inverse_newton_len(nf, precision) coefficients.  status: as in divide."""
    import torch

    width = _width(width)
    f = _t(f, "f")
    _need(f.numel() % width == 0 and f.numel() > 0, "f must hold at least one whole element")
    nf = f.numel() // width
    n = int(_lib.lib().tf_poly_fps_inverse_newton_len(nf, precision))
    out = _t(out, "out")
    _need(n > 0 and out.numel() == n * width, "out must hold tf_poly_fps_inverse_newton_len(nf, precision) elements")
    own = status is None
    st = torch.zeros(1, dtype=torch.int32, device=f.device) if own else status
    fn = _lib.lib().tf_poly_fps_inverse_newton_bfe_dev if width == 1 else _lib.lib().tf_poly_fps_inverse_newton_xfe_dev
    _chk(fn(_p(f), nf, precision, _p(out), _stream(stream), _status(st)), "formal_power_series_inverse_newton")
    if own:
        (stream or torch.cuda.current_stream()).synchronize()
        _chk(int(st.item()), "formal_power_series_inverse_newton")


def _inversion_args(x, out, width):
    x, out = _t(x, "x"), _t(out, "out")
    w = _width(width)
    _need(x.numel() % w == 0 and out.numel() == x.numel(), "x and out must hold the same number of whole elements")
    nbytes = x.numel() * 8
    _need(out.data_ptr() == x.data_ptr() or out.data_ptr() >= x.data_ptr() + nbytes or x.data_ptr() >= out.data_ptr() + nbytes,
          "out must be x itself or not overlap it")
    return x, out, x.numel() // w


def batch_inversion(x, out, width: int = 1, stream=None, status=None) -> None:
    """FiniteField::batch_inversion (math/traits.rs:93-121) on device buffers: out[i] = x[i]^-1; out may be x.  Without status a zero
    element raises NttPanic (code 12) after the call has synchronised once to read its flag; with status (see _status) nothing is
    synchronised and a zero element writes 12 there."""
    x, out, n = _inversion_args(x, out, width)
    if status is not None:
        fn = _lib.lib().tf_batch_inversion_bfe_dev_async if width == 1 else _lib.lib().tf_batch_inversion_xfe_dev_async
        _chk(fn(_p(x), n, _p(out), _stream(stream), _status(status)), "batch_inversion")
        return
    fn = _lib.lib().tf_batch_inversion_bfe_dev if width == 1 else _lib.lib().tf_batch_inversion_xfe_dev
    _chk(fn(_p(x), n, _p(out), _stream(stream)), "batch_inversion")


def inverse_or_zero(x, out, width: int = 1, stream=None) -> None:
    """Inverse::inverse_or_zero (math/traits.rs:39-45) of every element on device buffers (zero stays zero); out may be x.  Only
    enqueues."""
    x, out, n = _inversion_args(x, out, width)
    fn = _lib.lib().tf_inverse_or_zero_bfe_dev if width == 1 else _lib.lib().tf_inverse_or_zero_xfe_dev
    _chk(fn(_p(x), n, _p(out), _stream(stream)), "inverse_or_zero")


def _width_pair(width_x: int, width_y: int) -> None:
    _need((width_x, width_y) in ((1, 1), (3, 3), (1, 3)), "(width_x, width_y) must be (1, 1), (3, 3) or (1, 3)")


def _own_status(status, like):
    """the status word of a call: the caller's (see _status; nothing is synchronised) or one of the wrapper's own, which
    _raise_own_status reads back after waiting for the stream"""
    import torch

    return torch.zeros(1, dtype=torch.int32, device=like.device) if status is None else status


def _raise_own_status(st, stream, where: str) -> None:
    import torch

    (stream or torch.cuda.current_stream()).synchronize()
    _chk(int(st.item()), where)


def get_colinear_y(x0, y0, x1, y1, p2x, out, width_x: int = 1, width_y: int = 1, stream=None, status=None) -> None:
    """Polynomial::get_colinear_y (math/polynomial.rs:386-394) over n triples on device buffers: out[i] = the y-coordinate at p2x of
    the line through (x0[i], y0[i]) and (x1[i], y1[i]); p2x holds one element (one point for all triples) or n; out may not overlap
    an input.  (width_x, width_y) is (1, 1), (3, 3) or (1, 3).  Without status a triple with x0 == x1 raises NttPanic (code 12)
    after the call has synchronised once to read its flag; with status (see _status) nothing is synchronised and such a triple
    writes 12 there.  Either way the outputs of the other triples are correct."""
    x0, y0, x1, y1, p2x, out = _t(x0, "x0"), _t(y0, "y0"), _t(x1, "x1"), _t(y1, "y1"), _t(p2x, "p2x"), _t(out, "out")
    _width_pair(width_x, width_y)
    _need(x0.numel() % width_x == 0, "x0 must hold whole elements")
    n = x0.numel() // width_x
    _need(x1.numel() == x0.numel() and y0.numel() == n * width_y and y1.numel() == y0.numel() and out.numel() == y0.numel(),
          "x0, y0, x1, y1 and out must hold the same number of elements")
    _need(p2x.numel() in (width_y, n * width_y), "p2x must hold one element or one per triple")
    for a in (x0, y0, x1, y1, p2x):
        _apart(a, out, "out must not overlap an input")
    st = _own_status(status, out)
    _chk(_lib.lib().tf_get_colinear_y_dev(_p(x0), _p(y0), _p(x1), _p(y1), n, _p(p2x), p2x.numel() // width_y, width_x, width_y, _p(out),
                                          _stream(stream), _status(st)), "get_colinear_y")
    if status is None and n:
        _raise_own_status(st, stream, "get_colinear_y")


def are_colinear(xs, ys, k: int, flags, width_x: int = 1, width_y: int = 1, stream=None) -> None:
    """Polynomial::are_colinear (math/polynomial.rs:348-364) over groups of exactly k points on device buffers: flags (int32, one
    entry per group) receives 1 or 0.  Only enqueues."""
    import torch

    xs, ys = _t(xs, "xs"), _t(ys, "ys")
    _width_pair(width_x, width_y)
    _need(isinstance(flags, torch.Tensor) and flags.is_cuda and flags.is_contiguous() and flags.dtype == torch.int32,
          "flags must be a contiguous CUDA int32 tensor")
    n_groups = flags.numel()
    _need(0 <= k <= 1024, "k must be in [0, 1024]")
    _need(xs.numel() == n_groups * k * width_x and ys.numel() == n_groups * k * width_y, "xs and ys must hold flags.numel() groups of k points")
    _chk(_lib.lib().tf_are_colinear_dev(_p(xs), _p(ys), n_groups, k, width_x, width_y, _p(flags), _stream(stream)), "are_colinear")


def mod_pow(bases, exps, out, width: int = 1, stream=None) -> None:
    """mod_pow (b_field_element.rs:340-353, ModPowU64 of both fields) element by element on device buffers: out[i] = bases[i] ^
    exps[i]; exps holds uint64 words; bases and exps hold one element (used for every output) or as many as out.  One base for all
    elements is served from a table of its repeated squares.  Only enqueues."""
    bases, exps, out = _t(bases, "bases"), _t(exps, "exps"), _t(out, "out")
    _width(width)
    _need(bases.numel() % width == 0 and out.numel() % width == 0, "bases and out must hold whole elements")
    n, n_bases = out.numel() // width, bases.numel() // width
    _need(n == 0 or (n_bases in (1, n) and exps.numel() in (1, n)), "bases and exps must hold one element or one per element of out")
    _apart(bases, out, "out must not overlap an input")
    _apart(exps, out, "out must not overlap an input")
    _chk(_lib.lib().tf_mod_pow_dev(_p(bases), n_bases, _p(exps), exps.numel(), width, _p(out), n, _stream(stream)), "mod_pow")


def powers(first, ratio, out, width: int = 1, stream=None) -> None:
    """out[i] = first * ratio^i on a device buffer; first and ratio are HOST scalars (an int or `width` raw words).  The elements of
    a cyclic group, the powers of Polynomial::scale, the points of an evaluation domain.  Only enqueues."""
    out = _t(out, "out")
    f, r = _scalar_words(first, width, "first"), _scalar_words(ratio, width, "ratio")
    _need(out.numel() % width == 0, "out must hold whole elements")
    _chk(_lib.lib().tf_powers_dev(C.c_void_p(f.ctypes.data), C.c_void_p(r.ctypes.data), width, _p(out), out.numel() // width, _stream(stream)),
         "powers")


def gather_elements(src, indices, out, width: int = 1, stream=None, status=None) -> None:
    """out[i] = src[indices[i]] for elements of `width` words (1..16: field elements, digests); indices is a CUDA tensor of 32-bit
    words, as Tip5 sponges sample them.  Without status an index beyond src raises TwentyFirstError (code 17) after the call has
    synchronised once; with status (see _status) nothing is synchronised and such an index writes 17 there.  Such an index is never
    read and leaves its slot of out as it was."""
    import torch

    src, out = _t(src, "src"), _t(out, "out")
    _need(1 <= width <= 16, "width must be in [1, 16]")
    _need(isinstance(indices, torch.Tensor) and indices.is_cuda and indices.is_contiguous() and indices.dtype in (torch.int32, torch.uint32),
          "indices must be a contiguous CUDA tensor of 32-bit words")
    _need(src.numel() % width == 0 and out.numel() == indices.numel() * width, "src must hold whole elements and out one element per index")
    _apart(src, out, "out must not overlap src")
    st = _own_status(status, out)
    _chk(_lib.lib().tf_gather_elements_dev(_p(src), src.numel() // width, width, _p(indices), indices.numel(), _p(out), _stream(stream), _status(st)),
         "gather_elements")
    if status is None and indices.numel():
        _raise_own_status(st, stream, "gather_elements")


def zerofier(roots, out, width: int = 1, stream=None) -> None:
    """Polynomial::zerofier (math/polynomial.rs:1435-1441) on device buffers: out = the n + 1 coefficients of prod (x - roots[i])."""
    roots, out = _t(roots, "roots"), _t(out, "out")
    _need(roots.numel() % width == 0, "roots must hold whole elements")
    n = roots.numel() // width
    _need(out.numel() == (n + 1) * width, "out must hold n_roots + 1 coefficients")
    fn = _lib.lib().tf_poly_zerofier_bfe_dev if width == 1 else _lib.lib().tf_poly_zerofier_xfe_dev
    _chk(fn(_p(roots), n, _p(out), _stream(stream)), "zerofier")


def interpolate(domain, values, out, rows: int = 1, width: int = 1, stream=None, status=None) -> None:
    """Polynomial::interpolate / batch_fast_interpolate (math/polynomial.rs:1502-1838) on device buffers: `rows` value rows over
    one domain -> rows x n coefficients (untrimmed).  status: see _status (no host synchronisation)."""
    domain, values, out = _t(domain, "domain"), _t(values, "values"), _t(out, "out")
    _need(domain.numel() % width == 0, "domain must hold whole elements")
    n = domain.numel() // width
    _need(values.numel() == rows * n * width and out.numel() == rows * n * width, "values / out must hold rows * n elements")
    if status is not None:
        fn = _lib.lib().tf_poly_interpolate_bfe_dev_async if width == 1 else _lib.lib().tf_poly_interpolate_xfe_dev_async
        _chk(fn(_p(domain), _p(values), n, rows, _p(out), _stream(stream), _status(status)), "interpolate")
        return
    fn = _lib.lib().tf_poly_interpolate_bfe_dev if width == 1 else _lib.lib().tf_poly_interpolate_xfe_dev
    _chk(fn(_p(domain), _p(values), n, rows, _p(out), _stream(stream)), "interpolate")


def barycentric_evaluate(codewords, n: int, indeterminate, out, batch: int = 1, width: int = 1, stream=None) -> None:
    """barycentric_evaluate (math/polynomial.rs:2609-2637) on device buffers: `batch` codewords of n elements at one indeterminate
    (3 raw words, host side) -> out = batch x 3 words."""
    import numpy as np

    codewords, out = _t(codewords, "codewords"), _t(out, "out")
    _need(codewords.numel() == batch * n * _width(width) and out.numel() == 3 * batch, "codewords = batch * n elements, out = batch XFieldElements")
    x = np.zeros(3, dtype=np.uint64)
    xi = np.asarray(indeterminate, dtype=np.uint64).reshape(-1)
    _need(xi.size in (1, 3), "the indeterminate is one raw word or three")
    x[: xi.size] = xi
    fn = _lib.lib().tf_barycentric_evaluate_bfe_dev if width == 1 else _lib.lib().tf_barycentric_evaluate_xfe_dev
    _chk(fn(_p(codewords), n, batch, C.c_void_p(x.ctypes.data), _p(out), _stream(stream)), "barycentric_evaluate")


class ZerofierTree:
    """math/zerofier_tree.rs on device buffers: the tree of a device-resident domain, kept in HBM across calls
    (tf_zerofier_tree_* of include/tf_hip.h).  close() (or the context manager) releases the device memory."""

    def __init__(self, domain, width: int = 1, stream=None, asynchronous: bool = False):
        """asynchronous: return without waiting for the build (tf_zerofier_tree_new_*_dev_async): until the caller synchronises,
        the tree may only be used on the stream it was built on."""
        domain = _t(domain, "domain")
        _need(domain.numel() % _width(width) == 0, "domain must hold whole elements")
        self.width = width
        self.num_points = domain.numel() // width
        self._h = C.c_void_p(0)
        self._free = _lib.lib().tf_zerofier_tree_free
        if asynchronous:
            fn = _lib.lib().tf_zerofier_tree_new_bfe_dev_async if width == 1 else _lib.lib().tf_zerofier_tree_new_xfe_dev_async
        else:
            fn = _lib.lib().tf_zerofier_tree_new_bfe_dev if width == 1 else _lib.lib().tf_zerofier_tree_new_xfe_dev
        _chk(fn(_p(domain), self.num_points, _stream(stream), C.byref(self._h)), "ZerofierTree::new_from_domain")

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

    def zerofier(self, out, stream=None) -> None:
        out = _t(out, "out")
        _need(out.numel() == (self.num_points + 1) * self.width, "out must hold n + 1 coefficients")
        _chk(_lib.lib().tf_zerofier_tree_zerofier_dev(self._h, _p(out), _stream(stream)), "ZerofierTree::zerofier")

    def batch_evaluate(self, coeffs, n_coeffs: int, out, batch: int = 1, stream=None) -> None:
        coeffs, out = _t(coeffs, "coeffs"), _t(out, "out")
        _need(coeffs.numel() == batch * n_coeffs * self.width, "coeffs must hold batch * n_coeffs elements")
        _need(out.numel() == batch * self.num_points * self.width, "out must hold batch * n_points elements")
        _chk(_lib.lib().tf_zerofier_tree_batch_evaluate_dev(self._h, _p(coeffs), n_coeffs, batch, _p(out), _stream(stream)),
             "divide_and_conquer_batch_evaluate")

    def interpolate(self, values, out, rows: int = 1, stream=None, status=None) -> None:
        values, out = _t(values, "values"), _t(out, "out")
        _need(values.numel() == rows * self.num_points * self.width and out.numel() == values.numel(), "values / out must hold rows * n elements")
        if status is not None:
            _chk(_lib.lib().tf_zerofier_tree_interpolate_dev_async(self._h, _p(values), rows, _p(out), _stream(stream), _status(status)), "interpolate")
            return
        _chk(_lib.lib().tf_zerofier_tree_interpolate_dev(self._h, _p(values), rows, _p(out), _stream(stream)), "interpolate")


def coset_extrapolate(offset_raw: int, codewords, n: int, points, out, batch: int = 1, width: int = 1, stream=None) -> None:
    """Polynomial::batch_coset_extrapolate (math/polynomial.rs:2196-2208) on device buffers:
    out[(b * n_points + i) * width] = interpolant_b(points[i])."""
    codewords, points, out = _t(codewords, "codewords"), _t(points, "points"), _t(out, "out")
    n_points = points.numel() // width
    if codewords.numel() != batch * n * width or out.numel() != batch * n_points * width:
        raise ValueError("buffer sizes do not match n/batch/points/width")
    fn = _lib.lib().tf_coset_extrapolate_bfe_dev if width == 1 else _lib.lib().tf_coset_extrapolate_xfe_dev
    _chk(fn(C.c_uint64(offset_raw), _p(codewords), n, batch, _p(points), n_points, _p(out), _stream(stream)), "batch_coset_extrapolate")


def hash_table_rows(table, n_rows: int, n_cols: int, out, width: int = 1, col_stride=None, batch: int = 1, stream=None) -> None:
    """hash_varlen of every row of `batch` column-major tables resident in HBM (column j at table + j * col_stride words)."""
    table, out = _t(table, "table"), _t(out, "out")
    _width(width)
    cs = n_rows * width if col_stride is None else col_stride
    _need(cs >= n_rows * width, "col_stride must be at least n_rows * width words")
    _need(table.numel() >= ((batch * n_cols - 1) * cs + n_rows * width if batch * n_cols else 0), "table is smaller than batch * n_cols columns")
    _need(out.numel() == batch * n_rows * 5, "out must hold 5 words per row and table")
    _chk(_lib.lib().tf_tip5_hash_table_rows_dev(_p(table), n_rows, n_cols, width, cs, _p(out), batch, _stream(stream)), "Tip5::hash_varlen")


def merkle_from_columns(table, n_rows: int, n_cols: int, nodes_out, width: int = 1, col_stride=None, batch: int = 1, stream=None) -> None:
    """Rows of column-major tables -> leaves -> trees (nodes_out: batch x 2 n_rows digests), all in HBM."""
    table, nodes_out = _t(table, "table"), _t(nodes_out, "nodes_out")
    _width(width)
    cs = n_rows * width if col_stride is None else col_stride
    _need(cs >= n_rows * width, "col_stride must be at least n_rows * width words")
    _need(table.numel() >= ((batch * n_cols - 1) * cs + n_rows * width if batch * n_cols else 0), "table is smaller than batch * n_cols columns")
    _need(nodes_out.numel() == batch * n_rows * 10, "nodes_out must hold batch x 2 n_rows digests")
    _chk(_lib.lib().tf_merkle_from_columns_dev(_p(table), n_rows, n_cols, width, cs, _p(nodes_out), batch, _stream(stream)), "MerkleTree::par_new")


# ----------------------------------------------------------------------------- Tip5 sponges (include/tf_hip.h, "Tip5 sponges")
# A batch of sponges is a tensor of count x 16 raw words; every call below advances all of them in ONE kernel launch on the stream
# and synchronises nothing.
def _sponge_states(states) -> int:
    states = _t(states, "states")
    _need(states.numel() % 16 == 0, "states must hold 16 words per Tip5 sponge")
    return states.numel() // 16


def _per_sponge(t, count: int, unit: int, what: str) -> int:
    """t holds n x unit words for each of count sponges: n."""
    _need(t.numel() % (unit * count) == 0 if count else t.numel() == 0, what)
    return t.numel() // (unit * count) if count else 0


def tip5_sponge_init_(states, fixed_length: bool = False, stream=None) -> None:
    """Tip5::new(Domain) (tip5/mod.rs:511-526) into every sponge: all zero, or the capacity words ONE (fixed_length)."""
    count = _sponge_states(states)
    _chk(_lib.lib().tf_tip5_sponge_init_dev(_p(states), count, 1 if fixed_length else 0, _stream(stream)), "Tip5::new")


def tip5_sponge_absorb_(states, inp, stream=None) -> None:
    """n_chunks successive Sponge::absorb calls (tip5/mod.rs:684-691) per sponge: inp holds count x n_chunks x 10 words."""
    count, inp = _sponge_states(states), _t(inp, "input")
    n_chunks = _per_sponge(inp, count, 10, "input must hold n_chunks x 10 words per sponge")
    _chk(_lib.lib().tf_tip5_sponge_absorb_dev(_p(states), count, _p(inp), n_chunks, _stream(stream)), "Sponge::absorb")


def tip5_sponge_pad_and_absorb_all_(states, inp, offsets=None, stream=None) -> None:
    """Sponge::pad_and_absorb_all (util_types/sponge.rs:41-55).  offsets None: inp holds the same number of words for every sponge.
    Otherwise offsets is a HOST array of count + 1 non-decreasing word offsets into inp and sponge i absorbs
    inp[offsets[i] : offsets[i + 1]] (a length of 0 is one padding block)."""
    count, inp = _sponge_states(states), _t(inp, "input")
    if offsets is None:
        length = _per_sponge(inp, count, 1, "input must hold the same number of words for every sponge")
        _chk(_lib.lib().tf_tip5_sponge_pad_and_absorb_all_dev(_p(states), count, _p(inp), length, None, _stream(stream)),
             "Sponge::pad_and_absorb_all")
        return
    off = _u64_host(offsets)
    _need(off.size == count + 1, "offsets must hold count + 1 entries")
    # (the library refuses decreasing offsets before it touches the device, so the last one bounds them all)
    _need(count == 0 or int(off[-1]) <= inp.numel(), "offsets reach beyond the input")
    _chk(_lib.lib().tf_tip5_sponge_pad_and_absorb_all_dev(_p(states), count, _p(inp), 0, _host(off), _stream(stream)),
         "Sponge::pad_and_absorb_all")


def tip5_sponge_squeeze(states, out, stream=None) -> None:
    """n_squeezes successive Sponge::squeeze calls (tip5/mod.rs:693-698) per sponge: out receives count x n_squeezes x 10 words."""
    count, out = _sponge_states(states), _t(out, "out")
    n = _per_sponge(out, count, 10, "out must hold n_squeezes x 10 words per sponge")
    _chk(_lib.lib().tf_tip5_sponge_squeeze_dev(_p(states), count, n, _p(out), _stream(stream)), "Sponge::squeeze")


def tip5_sponge_sample_scalars(states, out, stream=None) -> None:
    """Tip5::sample_scalars (tip5/mod.rs:664-674): out receives count x num_elements x 3 words ([c0, c1, c2] per XFieldElement)."""
    count, out = _sponge_states(states), _t(out, "out")
    n = _per_sponge(out, count, 3, "out must hold num_elements x 3 words per sponge")
    _chk(_lib.lib().tf_tip5_sponge_sample_scalars_dev(_p(states), count, n, _p(out), _stream(stream)), "Tip5::sample_scalars")


def tip5_sponge_sample_indices(states, upper_bound: int, out, stream=None) -> None:
    """Tip5::sample_indices (tip5/mod.rs:636-656): out receives count x num_indices indices below upper_bound (a power of two).
    out is a contiguous CUDA int32 tensor whose BITS are the reference's u32 values (torch has no arithmetic on uint32, and this
    module already carries u64 words in int64 tensors): an index of 2^31 or above cannot occur, upper_bound being at most 2^31."""
    import torch

    count = _sponge_states(states)
    _need(isinstance(out, torch.Tensor) and out.is_cuda and out.is_contiguous() and out.dtype in (torch.int32, torch.uint32),
          "out must be a contiguous CUDA int32 tensor of count x num_indices entries")
    n = _per_sponge(out, count, 1, "out must hold num_indices entries per sponge")
    _need(0 <= upper_bound < 2 ** 32, "upper_bound is a u32")
    _chk(_lib.lib().tf_tip5_sponge_sample_indices_dev(_p(states), count, upper_bound, n, _p(out), _stream(stream)), "Tip5::sample_indices")


# ----------------------------------------------------------------------------- Merkle Mountain Range (include/tf_hip.h, "Merkle Mountain Range")
def _u64_host(a):
    import numpy as np

    return np.ascontiguousarray(a, dtype=np.uint64).reshape(-1)


def _opt(t, name):
    return None if t is None else _p(_t(t, name))


def mmr_append(leaf_count: int, old_peaks, new_leafs, new_peaks, proofs=None, stream=None) -> None:
    """k successive MmrAccumulator::append (mmr_accumulator.rs:149-159): new_peaks receives popcount(leaf_count + k) digests, proofs
    (if given) the concatenated proofs, trailing_ones(leaf_count + i) digests for append i.  Nothing is synchronised."""
    new_leafs, new_peaks = _t(new_leafs, "new_leafs"), _t(new_peaks, "new_peaks")
    _need(new_leafs.numel() % 5 == 0, "new_leafs must hold whole digests")
    k = new_leafs.numel() // 5
    _need(new_peaks.numel() >= 5 * bin(leaf_count + k).count("1"), "new_peaks must hold popcount(leaf_count + k) digests")
    _need(old_peaks is None or old_peaks.numel() >= 5 * bin(leaf_count).count("1"), "old_peaks must hold popcount(leaf_count) digests")
    if proofs is not None:
        _need(_t(proofs, "proofs").numel() >= 5 * sum(((leaf_count + i) ^ (leaf_count + i + 1)).bit_length() - 1 for i in range(k)),
              "proofs must hold sum(trailing_ones(leaf_count + i)) digests")
    _chk(_lib.lib().tf_mmr_append_dev(C.c_uint64(leaf_count), _opt(old_peaks, "old_peaks"), _p(new_leafs), k, _p(new_peaks),
                                      _opt(proofs, "proofs"), _stream(stream)), "MmrAccumulator::append")


def mmr_bag_peaks(leaf_counts, peaks, out, stream=None) -> None:
    """bag_peaks (mmr_accumulator.rs:379-391) of len(leaf_counts) accumulators (host counts; device peaks, one accumulator's after the
    other's): out receives one digest each.  Nothing is synchronised."""
    lc = _u64_host(leaf_counts)
    peaks, out = _t(peaks, "peaks"), _t(out, "out")
    import numpy as np

    n_peaks = int(np.unpackbits(lc.view(np.uint8)).sum())  # the peaks of all accumulators
    _need(peaks.numel() >= 5 * n_peaks and out.numel() >= 5 * lc.size, "buffer sizes do not match the counts")
    _chk(_lib.lib().tf_mmr_bag_peaks_dev(_host(lc), lc.size, _p(peaks), _p(out), _stream(stream)), "bag_peaks")


def mmr_verify_membership_proofs(leaf_count: int, peaks, leaf_indices, leaf_digests, path_offsets, paths, statuses, stream=None) -> None:
    """MmrMembershipProof::verify (mmr_membership_proof.rs:36-77) of a batch: statuses[p] (device int32) = 0 or the first reason it is
    false (22..25).  path_offsets is a host array of n_proofs + 1 entries; everything else is on the device.  Nothing is synchronised."""
    off = _u64_host(path_offsets)
    n = off.size - 1
    peaks, leaf_indices, leaf_digests, paths = _t(peaks, "peaks"), _t(leaf_indices, "leaf_indices"), _t(leaf_digests, "leaf_digests"), _t(paths, "paths")
    statuses = _status_tensor(statuses, n)
    _need(n >= 0 and peaks.numel() % 5 == 0 and leaf_indices.numel() >= n and leaf_digests.numel() >= 5 * n
          and (n == 0 or paths.numel() >= 5 * int(off[-1])), "buffer sizes do not match the offsets")
    _chk(_lib.lib().tf_mmr_verify_membership_proofs_dev(C.c_uint64(leaf_count), _p(peaks), peaks.numel() // 5, n, _p(leaf_indices),
                                                        _p(leaf_digests), _host(off), _p(paths), _p(statuses), _stream(stream)),
         "MmrMembershipProof::verify")


def mmr_batch_mutate_leafs(leaf_count: int, peaks, mut_indices, new_leafs, mut_offsets, mut_paths, own_indices, own_offsets, own_paths,
                           modified, stream=None) -> None:
    """batch_mutate_leaf_and_update_mps (mmr_accumulator.rs:180-302), or with peaks=None batch_update_from_batch_leaf_mutation
    (mmr_membership_proof.rs:523-626): peaks and own_paths are updated in place, modified[p] (device int32) = 1 where proof p
    changed.  Indices and offsets are host arrays.  Nothing is synchronised."""
    mi, mo, oi, oo = _u64_host(mut_indices), _u64_host(mut_offsets), _u64_host(own_indices), _u64_host(own_offsets)
    M, P = mi.size, oi.size
    _need(mo.size == M + 1 and oo.size == P + 1, "offsets need one entry more than indices")
    new_leafs, mut_paths, own_paths = _t(new_leafs, "new_leafs"), _t(mut_paths, "mut_paths"), _t(own_paths, "own_paths")
    mod_p = _p(_status_tensor(modified, P)) if P else None
    _need(new_leafs.numel() >= 5 * M and mut_paths.numel() >= 5 * int(mo[-1]) and own_paths.numel() >= 5 * int(oo[-1]), "buffer sizes do not match")
    if peaks is not None:
        _need(_t(peaks, "peaks").numel() >= 5 * bin(leaf_count).count("1"), "peaks must hold popcount(leaf_count) digests")
    _chk(_lib.lib().tf_mmr_batch_mutate_leafs_dev(C.c_uint64(leaf_count), _opt(peaks, "peaks"), M, _host(mi), _p(new_leafs), _host(mo),
                                                  _p(mut_paths), P, _host(oi), _host(oo), _p(own_paths), mod_p, _stream(stream)),
         "batch_mutate_leaf_and_update_mps")


def mmr_successor_proof_len(leaf_count: int, k: int) -> int:
    """Digests of MmrSuccessorProof::new_from_batch_append for an accumulator of leaf_count leafs and k new ones (host arithmetic)."""
    return int(_lib.lib().tf_mmr_successor_proof_len(C.c_uint64(leaf_count), C.c_uint64(k)))


def mmr_successor_proof_new(leaf_count: int, old_peaks, new_leafs, paths_out, new_peaks=None, stream=None) -> int:
    """MmrSuccessorProof::new_from_batch_append (mmr_successor_proof.rs:34-91): paths_out receives the proof's digests (their number is
    returned), new_peaks (if given) the peaks of the accumulator after the appends, from the same level sweep.  old_peaks may be None
    without new_peaks.  Nothing is synchronised."""
    new_leafs = _t(new_leafs, "new_leafs")
    _need(new_leafs.numel() % 5 == 0, "new_leafs must hold whole digests")
    k = new_leafs.numel() // 5
    n = mmr_successor_proof_len(leaf_count, k)
    _need(n == 0 or (paths_out is not None and _t(paths_out, "paths_out").numel() >= 5 * n), "paths_out must hold mmr_successor_proof_len digests")
    if new_peaks is not None:
        _need(_t(new_peaks, "new_peaks").numel() >= 5 * bin(leaf_count + k).count("1"), "new_peaks must hold popcount(leaf_count + k) digests")
        _need(leaf_count == 0 or (old_peaks is not None and _t(old_peaks, "old_peaks").numel() >= 5 * bin(leaf_count).count("1")),
              "old_peaks must hold popcount(leaf_count) digests")
    _chk(_lib.lib().tf_mmr_successor_proof_new_dev(C.c_uint64(leaf_count), _opt(old_peaks, "old_peaks"), _p(new_leafs), k,
                                                   _opt(paths_out, "paths_out"), _opt(new_peaks, "new_peaks"), _stream(stream)),
         "MmrSuccessorProof::new_from_batch_append")
    return n


def mmr_verify_successor_proofs(old_leaf_counts, new_leaf_counts, old_peak_offsets, old_peaks, new_peak_offsets, new_peaks, path_offsets, paths,
                                statuses, stream=None) -> None:
    """MmrSuccessorProof::verify (mmr_successor_proof.rs:94-223) of a batch of (old, new, proof) triples in CSR layout: statuses[p]
    (device int32) = 0 or the first error of verify_internal (27..33).  Counts and the three offset arrays (n_proofs + 1 entries, in
    digests) are host arrays; peaks and paths are on the device.  Nothing is synchronised."""
    oc, nc = _u64_host(old_leaf_counts), _u64_host(new_leaf_counts)
    oo, no, po = _u64_host(old_peak_offsets), _u64_host(new_peak_offsets), _u64_host(path_offsets)
    n = oc.size
    _need(nc.size == n and oo.size == n + 1 and no.size == n + 1 and po.size == n + 1, "one count per proof, offsets one entry more")
    old_peaks, new_peaks, paths = _t(old_peaks, "old_peaks"), _t(new_peaks, "new_peaks"), _t(paths, "paths")
    statuses = _status_tensor(statuses, n)
    _need(old_peaks.numel() >= 5 * int(oo[-1]) and new_peaks.numel() >= 5 * int(no[-1]) and paths.numel() >= 5 * int(po[-1]),
          "buffer sizes do not match the offsets")
    _chk(_lib.lib().tf_mmr_verify_successor_proofs_dev(n, _host(oc), _host(nc), _host(oo), _p(old_peaks), _host(no), _p(new_peaks), _host(po),
                                                       _p(paths), _p(statuses), _stream(stream)), "MmrSuccessorProof::verify")


def mmr_update_proofs_from_append(leaf_count: int, old_peaks, new_leafs, own_indices, own_offsets, own_paths, out_paths=None, new_peaks=None,
                                  stream=None):
    """k rounds of MmrMembershipProof::batch_update_from_append (mmr_membership_proof.rs:224-331) and append for the proofs
    (own_indices, own_offsets: host arrays; own_paths: device): out_paths receives every proof in the accumulator of leaf_count + k
    leafs, at the returned offsets.  Returns (out_offsets, modified) as host arrays; with out_paths=None the call only sizes
    (out_offsets[-1] digests).  new_peaks as in mmr_successor_proof_new.  Nothing is synchronised."""
    import numpy as np

    oi, oo = _u64_host(own_indices), _u64_host(own_offsets)
    P = oi.size
    _need(oo.size == P + 1, "offsets need one entry more than indices")
    new_leafs, own_paths = _t(new_leafs, "new_leafs"), _t(own_paths, "own_paths")
    _need(new_leafs.numel() % 5 == 0, "new_leafs must hold whole digests")
    k = new_leafs.numel() // 5
    _need(own_paths.numel() >= 5 * int(oo[-1]), "own_paths does not match own_offsets")
    if new_peaks is not None:
        _need(_t(new_peaks, "new_peaks").numel() >= 5 * bin(leaf_count + k).count("1"), "new_peaks must hold popcount(leaf_count + k) digests")
    _need(old_peaks is None or _t(old_peaks, "old_peaks").numel() >= 5 * bin(leaf_count).count("1"), "old_peaks must hold popcount(leaf_count) digests")
    out_off = np.zeros(P + 1, dtype=np.uint64)
    modified = np.zeros(max(P, 1), dtype=np.int32)
    capacity = 0 if out_paths is None else _t(out_paths, "out_paths").numel() // 5
    _chk(_lib.lib().tf_mmr_update_proofs_from_append_dev(C.c_uint64(leaf_count), _opt(old_peaks, "old_peaks"), _p(new_leafs), k, P, _host(oi),
                                                         _host(oo), _p(own_paths), _host(out_off), _opt(out_paths, "out_paths"), capacity,
                                                         _host(modified), _opt(new_peaks, "new_peaks"), _stream(stream)),
         "MmrMembershipProof::batch_update_from_append")
    return out_off, modified[:P]
