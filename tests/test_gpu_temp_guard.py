"""The library's own device memory, fenced: every stream-ordered temporary and every buffer of the host-pointer forms under the
guard mode of tf_debug_temp_guard (include/tf_hip.h) -- 20 480 poisoned words on each side of every block the library takes, the
block itself poisoned, both guards checked when it is given back.  tests/fence.py's temp_guarded() switches the mode on around a
call, off in any case, and asserts a clean ledger.

  1. the self-test: each planted defect is reported with its label, side, offset and count; the clean case reports nothing;
  2. every fenced _dev call of tests/test_gpu_fences.py, test_gpu_fri_fold.py, test_gpu_table.py and test_gpu_merkle_sampled.py
     again (shift 0, operand poison "random"), once per temporary poison: the guards of the library's blocks are untouched, and the
     existing output check under three temporary poisons is the "reads a work word it never wrote" test.  Every case of every
     row is kept;
  3. the host-pointer forms, one case per function that owns device buffers: the generator of the matching _dev row supplies shape,
     operands and reference, a shim with device.py's signatures passes the (CPU) payloads to the host entry point, and the arena
     of tests/fence.py checks the host arrays as it checks tensors;
  4. the routes that depend on the state of the caches (temporary inter-pass tables, uncached scaled tables, temporary power
     tables) against the oracle, forced and unforced, before and after tf_release_caches;
  5. the four *_workspace functions against the bytes requested under the call's own labels.

WITNESS and the host cases declare, per case, the labels that must show in the per-label counters after the call;
tests/test_temp_guard_cpu.py asserts on the CPU that their union is exactly the set of labels in csrc/."""
import ctypes as C

import numpy as np
import pytest

from tests import fence
from tests import test_gpu_fences as F
from tests import test_gpu_fri_fold as FRI
from tests import test_gpu_merkle_sampled as MS
from tests import test_gpu_table as TAB

pytestmark = pytest.mark.gpu

G = fence.G
INVALID_ARGUMENT = 17   # TF_ERR_INVALID_ARGUMENT
SOURCES = {"fences": F, "fri": FRI, "table": TAB, "sampled": MS}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(tf):
    assert tf.lib().tf_device_count() > 0, "no HIP device visible: the product has no CPU fallback"


def triples(tf, oracle, src, name, case, d=None):
    """the (shape, operands, call) triples of one case of one row of one of the four tables; `d` replaces the module under test"""
    gen = SOURCES[src].ROWS[name][1]
    if src == "fences":
        return gen(tf, oracle, d or tf.device, *(case if isinstance(case, tuple) else (case,)))
    if src == "fri":
        return gen(tf, d or tf.fri, max(tf.fri.plan(1 << 12, 12)), *case)
    return gen(tf, oracle, d or (tf.table if src == "table" else tf.merkle_sampled), *case)


# ------------------------------------------------------------------ 1. the mechanism sees what it claims
SELFTEST_WORDS = 1000
# defect -> (side, offset of the first offending 32-bit entry relative to the payload, offending entries) or None for a clean ledger
DEFECTS = {0: None, 1: ("front", -2, 2), 2: ("back", 2 * SELFTEST_WORDS, 2), 3: ("back", 2 * (SELFTEST_WORDS + G - 1), 2),
           4: ("back", 2 * SELFTEST_WORDS + 1, 1), 5: None}


@pytest.mark.parametrize("mode", fence.TEMP_POISONS)
@pytest.mark.parametrize("defect", sorted(DEFECTS))
def test_selftest_reports_each_planted_defect(tf, defect, mode):
    lib, word = tf.lib(), C.c_uint64(0)
    assert lib.tf_debug_temp_guard_words() == G
    with fence.temp_guarded(lib, mode, must_see=["selftest"], clean=False) as box:
        assert lib.tf_debug_temp_guard_selftest(defect, SELFTEST_WORDS, C.byref(word)) == 0
    rep = box[0]
    payload_bytes = 8 * SELFTEST_WORDS + (4 if defect == 4 else 0)
    assert rep.labels == {"selftest": (2, payload_bytes + 8)} and rep.blocks_checked == 2, rep
    if DEFECTS[defect] is None:
        assert (rep.blocks_offending, rep.entries_offending, rep.records) == (0, 0, []), rep
    else:
        side, offset, count = DEFECTS[defect]
        assert (rep.blocks_offending, rep.entries_offending) == (1, count) and rep.records == [("selftest", side, offset, count)], rep
    # word 0 of the payload, which nobody wrote, is word G of the block's poison
    assert word.value == (int(fence.poison_words(fence.POISONS[mode - 1], G + 1)[G]) if defect == 5 else 0)


def test_selftest_read_before_write_gives_three_different_words(tf):
    lib, words = tf.lib(), []
    for mode in fence.TEMP_POISONS:
        word = C.c_uint64(0)
        with fence.temp_guarded(lib, mode, must_see=["selftest"]):
            assert lib.tf_debug_temp_guard_selftest(5, SELFTEST_WORDS, C.byref(word)) == 0
        words.append(word.value)
    assert len(set(words)) == 3, words


def test_selftest_needs_the_mode_and_the_mode_is_off_by_default(tf):
    lib, word = tf.lib(), C.c_uint64(7)
    assert lib.tf_debug_temp_guard_selftest(1, SELFTEST_WORDS, C.byref(word)) == INVALID_ARGUMENT   # the mode is off
    assert lib.tf_debug_temp_guard(4) == INVALID_ARGUMENT and lib.tf_debug_temp_guard(-1) == INVALID_ARGUMENT
    assert lib.tf_debug_temp_guard_reset() == 0
    x = np.arange(16, dtype=np.uint64)
    tf.ntt(x)                                                                          # a host round trip with the mode off: not counted
    rep = fence.TempGuardReport(lib)
    assert rep.labels == {} and rep.blocks_checked == 0, rep


# ------------------------------------------------------------------ 2. every fenced _dev call, the library's memory fenced too
# (source, row, case number) -> labels that case must show; generated once from the labels each case reports, then held fixed:
# every label of csrc/ that a _dev call can reach has one witness here (tests/test_temp_guard_cpu.py checks the union)
WITNESS = {
    ("fences", "authentication_structure", 1): ["authentication structure gather"],
    ("fences", "authentication_structure_from_leafs", 0): ["merkle open"],
    ("fences", "barycentric_evaluate", 0): ["barycentric"],
    ("fences", "batch_evaluate", 1): ["batch_evaluate zerofier tree", "zerofier tree walk"],
    ("fences", "batch_inversion", 0): ["batch_inversion flag"],
    ("fences", "clean_divide", 0): ["clean_divide"],
    ("fences", "coset_extrapolate", 0): ["coset_extrapolate"],
    ("fences", "divide", 1): ["divide quotient work", "divide remainder work", "divide unwanted quotient"],
    ("fences", "divide", 4): ["divide newton work"],
    ("fences", "fps_inverse_newton", 1): ["fps_inverse work"],
    ("fences", "interpolate", 0): ["interpolation rows", "interpolation weights"],
    ("fences", "lde", 0): ["lde"],
    ("fences", "merkle_root", 5): ["merkle levels"],
    ("fences", "mmr_append", 0): ["mmr move list", "mmr sweep levels"],
    ("fences", "mmr_bag_peaks", 0): ["mmr bag chains"],
    ("fences", "mmr_batch_mutate_leafs", 0): ["mmr mutation chains", "mmr mutation plan"],
    ("fences", "mmr_update_proofs_from_append", 0): ["mmr gather descriptors", "mmr update wanted digests"],
    ("fences", "mmr_verify_membership_proofs", 0): ["mmr verify chains"],
    ("fences", "mmr_verify_successor_proofs", 0): ["mmr successor chains"],
    ("fences", "poly_mul", 0): ["poly_mul"],
    ("fences", "poly_mul_shared", 0): ["poly_mul_shared"],
    ("fences", "verify_inclusion_proofs", 0): ["proof descriptors"],
    ("fences", "zerofier", 0): ["zerofier tree arena"],
    ("fences", "zerofier", 2): ["zerofier tree build"],
    ("fri", "fold", 2): ["fri_fold second-pass intermediate"],
    ("fri", "fold", 4): ["fri_fold third-pass intermediate"],
    ("sampled", "structure_from_leafs", 0): ["merkle open (sampled)"],
    ("sampled", "structure_from_nodes", 0): ["merkle plan"],
    ("table", "lde_rows", 0): ["table_lde_rows"],
}


def _ids():
    return [pytest.param(src, name, k, id=f"{src}-{name}-{k}") for src, mod in SOURCES.items() for name in mod.ROWS for k in range(len(mod.ROWS[name][0]))]


def run_guarded(tf, oracle, src, name, k, d=None, device="cuda"):
    """every triple of the case once per temporary poison; returns the labels seen"""
    seen = set()
    for shape, operands, call in triples(tf, oracle, src, name, SOURCES[src].ROWS[name][0][k], d):
        for mode in fence.TEMP_POISONS:
            with fence.temp_guarded(tf.lib(), mode) as box:
                fence.run_once(name, f"{shape} [temporary poison {fence.POISONS[mode - 1]}]", operands, call, 0, "random", device=device)
            seen |= set(box[0].labels)
    return seen


@pytest.mark.parametrize("src,name,k", _ids())
def test_fenced_with_the_library_s_memory_fenced(tf, oracle, src, name, k):
    seen = run_guarded(tf, oracle, src, name, k)
    missing = sorted(set(WITNESS.get((src, name, k), ())) - seen)
    assert not missing, f"no block was requested under {missing}; seen {sorted(seen)}"


# ------------------------------------------------------------------ 3. the host-pointer forms
def _a(t):
    """a host pointer: of a CPU tensor (the fence's payload view), of a numpy array, or null"""
    if t is None:
        return None
    if isinstance(t, np.ndarray):
        return C.c_void_p(t.ctypes.data) if t.size else None
    return C.c_void_p(t.data_ptr()) if t.numel() else None


def _u64(a):
    return np.ascontiguousarray(a, dtype=np.uint64).reshape(-1)


class HostForms:
    """device.py's signatures (and those of table.py, fri.py) on host memory: each method hands the payloads to the host-pointer
    entry point of the same operation, so the generators of the _dev rows drive the host forms unchanged.  A status is the return
    value here; a row that passes a status tensor is not used for a host case."""

    def __init__(self, tf):
        self.tf, self.lib = tf, tf.lib()

    def ok(self, rc, where):
        assert rc == 0, f"{where}: status {rc} ({self.lib.tf_last_error().decode()})"

    # tf_abi.hip
    def ntt_(self, x, n, batch=1, width=1, inverse=False):
        self.ok((self.lib.tf_ntt_bfe if width == 1 else self.lib.tf_ntt_xfe)(_a(x), n, batch, int(inverse)), "ntt")

    def coset_evaluate(self, coeffs, n_coeffs, offset_raw, out, order, batch=1, width=1):
        self.ok((self.lib.tf_coset_eval_bfe if width == 1 else self.lib.tf_coset_eval_xfe)(_a(coeffs), n_coeffs, offset_raw, _a(out), order, batch), "coset_evaluate")

    def coset_interpolate(self, values, n, offset_raw, out, batch=1, width=1):
        self.ok((self.lib.tf_coset_interpolate_bfe if width == 1 else self.lib.tf_coset_interpolate_xfe)(_a(values), n, offset_raw, _a(out), batch), "coset_interpolate")

    def poly_mul(self, a, na, b, nb, out, batch=1, width=1):
        self.ok((self.lib.tf_poly_mul_bfe if width == 1 else self.lib.tf_poly_mul_xfe)(_a(a), na, _a(b), nb, _a(out), batch), "poly_mul")

    def zerofier(self, roots, out, width=1):
        self.ok((self.lib.tf_poly_zerofier_bfe if width == 1 else self.lib.tf_poly_zerofier_xfe)(_a(roots), roots.numel() // width, _a(out)), "zerofier")

    def interpolate(self, domain, values, out, rows=1, width=1, status=None):
        assert status is None
        self.ok((self.lib.tf_poly_interpolate_bfe if width == 1 else self.lib.tf_poly_interpolate_xfe)(_a(domain), _a(values), domain.numel() // width, rows, _a(out)),
                "interpolate")

    def batch_evaluate(self, coeffs, n_coeffs, points, out, width=1):
        self.ok((self.lib.tf_poly_batch_evaluate_bfe if width == 1 else self.lib.tf_poly_batch_evaluate_xfe)(_a(coeffs), n_coeffs, _a(points), points.numel() // width,
                                                                                                          _a(out)), "batch_evaluate")

    def coset_extrapolate(self, offset_raw, codewords, n, points, out, batch=1, width=1):
        self.ok((self.lib.tf_coset_extrapolate_bfe if width == 1 else self.lib.tf_coset_extrapolate_xfe)(offset_raw, _a(codewords), n, batch, _a(points),
                                                                                                      points.numel() // width, _a(out)), "coset_extrapolate")

    def barycentric_evaluate(self, codewords, n, indeterminate, out, batch=1, width=1):
        self.ok((self.lib.tf_barycentric_evaluate_bfe if width == 1 else self.lib.tf_barycentric_evaluate_xfe)(_a(codewords), n, batch, _a(_u64(indeterminate)), _a(out)),
                "barycentric_evaluate")

    def evaluate_bfe_at_xfe(self, coeffs, n_coeffs, points, out, batch=1):
        self.ok(self.lib.tf_poly_evaluate_bfe_at_xfe(_a(coeffs), n_coeffs, batch, _a(points), points.numel() // 3, _a(out)), "evaluate_bfe_at_xfe")

    def clean_divide(self, a, b, out, status=None):
        assert status is None
        self.ok(self.lib.tf_poly_clean_divide_bfe(_a(a), a.numel(), _a(b), b.numel(), _a(out)), "clean_divide")

    def clean_divide_many(self, a, na, b, out, batch, status=None):
        assert status is None
        self.ok(self.lib.tf_poly_clean_divide_many_bfe(_a(a), na, batch, _a(b), b.numel(), _a(out)), "clean_divide_many")

    def hash_table_rows(self, table, n_rows, n_cols, out, width=1, col_stride=None, batch=1):
        self.ok(self.lib.tf_tip5_hash_table_rows(_a(table), n_rows, n_cols, width, n_rows * width if col_stride is None else col_stride, _a(out), batch), "hash_table_rows")

    def merkle_from_columns(self, table, n_rows, n_cols, nodes_out, width=1, col_stride=None, batch=1):
        self.ok(self.lib.tf_merkle_from_columns(_a(table), n_rows, n_cols, width, n_rows * width if col_stride is None else col_stride, _a(nodes_out), batch),
                "merkle_from_columns")

    def tip5_permute_(self, states):
        self.ok(self.lib.tf_tip5_permute(_a(states), states.numel() // 16), "tip5_permute")

    def tip5_hash_pairs(self, inp, out):
        self.ok(self.lib.tf_tip5_hash_pairs(_a(inp), _a(out), inp.numel() // 10), "tip5_hash_pairs")

    def merkle_from_rows(self, rows, row_len, n_rows, nodes_out, batch=1):
        self.ok(self.lib.tf_merkle_from_rows(_a(rows), row_len, n_rows, _a(nodes_out), batch), "merkle_from_rows")

    def tip5_trace_(self, states, trace):
        self.ok(self.lib.tf_tip5_trace(_a(states), _a(trace), states.numel() // 16), "tip5_trace")

    def tip5_hash_varlen_rows(self, rows, row_len, out):
        self.ok(self.lib.tf_tip5_hash_varlen_rows(_a(rows), row_len, out.numel() // 5, _a(out)), "hash_varlen_rows")

    def merkle_build(self, leaves, n_leaves, nodes_out, batch=1, devices=None):
        if devices is None:
            self.ok(self.lib.tf_merkle_build(_a(leaves), n_leaves, _a(nodes_out), batch), "merkle_build")
        else:
            ids = (C.c_int * len(devices))(*devices)
            self.ok(self.lib.tf_merkle_build_multi(_a(leaves), n_leaves, _a(nodes_out), batch, ids, len(devices)), "merkle_build_multi")

    def merkle_root(self, leaves, n_leaves, root_out, batch=1, devices=None):
        if devices is None:
            self.ok(self.lib.tf_merkle_root(_a(leaves), n_leaves, _a(root_out), batch), "merkle_root")
        else:
            ids = (C.c_int * len(devices))(*devices)
            self.ok(self.lib.tf_merkle_root_multi(_a(leaves), n_leaves, _a(root_out), batch, ids, len(devices)), "merkle_root_multi")

    def verify_inclusion_proofs(self, tree_heights, leaf_offsets, leaf_indices, leaf_digests, auth_offsets, auth_digests, expected_roots, statuses):
        h, lo, ao = np.asarray(tree_heights, dtype=np.uint32), _u64(leaf_offsets), _u64(auth_offsets)
        self.ok(self.lib.tf_merkle_verify_proofs(_a(h), h.size, _a(lo), _a(leaf_indices), _a(leaf_digests), _a(ao), _a(auth_digests), _a(expected_roots),
                                                 _a(statuses)), "verify_inclusion_proofs")

    def authentication_path_words(self, tree_heights, leaf_offsets):
        return self.tf.device.authentication_path_words(tree_heights, leaf_offsets)

    def authentication_paths(self, tree_heights, leaf_offsets, leaf_indices, leaf_digests, auth_offsets, auth_digests, paths_out, statuses):
        h, lo, ao = np.asarray(tree_heights, dtype=np.uint32), _u64(leaf_offsets), _u64(auth_offsets)
        self.ok(self.lib.tf_merkle_authentication_paths(_a(h), h.size, _a(lo), _a(leaf_indices), _a(leaf_digests), _a(ao), _a(auth_digests), _a(paths_out),
                                                        _a(statuses)), "authentication_paths")

    # tf_merkle_open.hip
    def authentication_structure_from_leafs(self, leafs, num_leafs, leaf_indices, out=None, roots=None, batch=1):
        idx, count = _u64(leaf_indices), C.c_size_t(0)
        self.ok(self.lib.tf_merkle_auth_structure_from_leafs(_a(leafs), num_leafs, batch, _a(idx), idx.size, _a(out), out.numel() // 5, C.byref(count), _a(roots)),
                "authentication_structure_from_leafs")
        return out[:batch * count.value * 5]

    # tf_algebra.hip
    def linear_combination(self, columns, n, k, weights, out, width=1, width_w=1, stride=None):
        self.ok(self.lib.tf_poly_linear_combination(_a(columns), n, width, n * width if stride is None else stride, k, _a(weights), width_w, _a(out)),
                "linear_combination")

    def poly_sub(self, a, na, b, nb, out, batch=1, width=1):
        self.ok(self.lib.tf_poly_sub(_a(a), na, _a(b), nb, width, _a(out), batch), "poly_sub")

    def poly_neg_(self, a, na, out=None, batch=1, width=1):
        self.ok(self.lib.tf_poly_neg(_a(a), na, width, _a(a if out is None else out), batch), "poly_neg")

    def poly_scalar_mul(self, a, na, scalar, out, batch=1, width=1, width_s=1):
        self.ok(self.lib.tf_poly_scalar_mul(_a(a), na, width, _a(_u64(scalar)), width_s, _a(out), batch), "poly_scalar_mul")

    def poly_scale(self, a, na, alpha, out, batch=1, width=1, width_alpha=1):
        self.ok(self.lib.tf_poly_scale(_a(a), na, width, _a(_u64(alpha)), width_alpha, _a(out), batch), "poly_scale")

    def poly_formal_derivative(self, a, na, out, batch=1, width=1):
        self.ok(self.lib.tf_poly_formal_derivative(_a(a), na, width, _a(out), batch), "poly_formal_derivative")

    def poly_degree(self, a, na, degrees, batch=1, width=1):
        self.ok(self.lib.tf_poly_degree(_a(a), na, width, batch, _a(degrees)), "poly_degree")

    def poly_add(self, a, na, b, nb, out, batch=1, width=1):
        self.ok(self.lib.tf_poly_add(_a(a), na, _a(b), nb, width, _a(out), batch), "poly_add")

    # tf_divide.hip
    def divide(self, a, na, b, q, r, batch=1, width=1, status=None):
        assert status is None
        nb = b.numel() // width
        self.ok((self.lib.tf_poly_divide_bfe if width == 1 else self.lib.tf_poly_divide_xfe)(_a(a), na, batch, _a(b), nb, _a(q), _a(r)), "divide")

    def fps_inverse_newton(self, f, precision, out, width=1, status=None):
        assert status is None
        self.ok((self.lib.tf_poly_fps_inverse_newton_bfe if width == 1 else self.lib.tf_poly_fps_inverse_newton_xfe)(_a(f), f.numel() // width, precision, _a(out)),
                "fps_inverse_newton")

    # tf_inverse.hip
    def batch_inversion(self, x, out, width=1, status=None):
        assert status is None
        self.ok((self.lib.tf_batch_inversion_bfe if width == 1 else self.lib.tf_batch_inversion_xfe)(_a(x), x.numel() // width, _a(out)), "batch_inversion")

    def inverse_or_zero(self, x, out, width=1):
        self.ok((self.lib.tf_inverse_or_zero_bfe if width == 1 else self.lib.tf_inverse_or_zero_xfe)(_a(x), x.numel() // width, _a(out)), "inverse_or_zero")

    # tf_points.hip
    def get_colinear_y(self, x0, y0, x1, y1, p2x, out, width_x=1, width_y=1, status=None):
        assert status is None
        self.ok(self.lib.tf_get_colinear_y(_a(x0), _a(y0), _a(x1), _a(y1), x0.numel() // width_x, _a(p2x), p2x.numel() // width_y, width_x, width_y, _a(out)),
                "get_colinear_y")

    def are_colinear(self, xs, ys, k, flags, width_x=1, width_y=1):
        self.ok(self.lib.tf_are_colinear(_a(xs), _a(ys), flags.numel(), k, width_x, width_y, _a(flags)), "are_colinear")

    def mod_pow(self, bases, exps, out, width=1):
        self.ok(self.lib.tf_mod_pow(_a(bases), bases.numel() // width, _a(exps), exps.numel(), width, _a(out), out.numel() // width), "mod_pow")

    def powers(self, first, ratio, out, width=1):
        self.ok(self.lib.tf_powers(_a(_u64(first)), _a(_u64(ratio)), width, _a(out), out.numel() // width), "powers")

    # tf_sponge.hip
    def tip5_sponge_init_(self, states, fixed_length=False):
        self.ok(self.lib.tf_tip5_sponge_init(_a(states), states.numel() // 16, int(fixed_length)), "sponge_init")

    def tip5_sponge_absorb_(self, states, inp):
        count = states.numel() // 16
        self.ok(self.lib.tf_tip5_sponge_absorb(_a(states), count, _a(inp), inp.numel() // (10 * count)), "sponge_absorb")

    def tip5_sponge_pad_and_absorb_all_(self, states, inp, offsets=None):
        count = states.numel() // 16
        off = None if offsets is None else _u64(offsets)
        self.ok(self.lib.tf_tip5_sponge_pad_and_absorb_all(_a(states), count, _a(inp), inp.numel() // count if off is None else 0, _a(off)), "sponge_pad_and_absorb_all")

    def tip5_sponge_sample_scalars(self, states, out):
        count = states.numel() // 16
        self.ok(self.lib.tf_tip5_sponge_sample_scalars(_a(states), count, out.numel() // (3 * count), _a(out)), "sponge_sample_scalars")

    def tip5_sponge_squeeze(self, states, out):
        count = states.numel() // 16
        self.ok(self.lib.tf_tip5_sponge_squeeze(_a(states), count, out.numel() // (10 * count), _a(out)), "sponge_squeeze")

    def tip5_sponge_sample_indices(self, states, upper_bound, out):
        count = states.numel() // 16
        self.ok(self.lib.tf_tip5_sponge_sample_indices(_a(states), count, upper_bound, out.numel() // count, _a(out)), "sponge_sample_indices")

    # tf_mmr.hip
    def mmr_append(self, leaf_count, old_peaks, new_leafs, new_peaks, proofs=None):
        self.ok(self.lib.tf_mmr_append(leaf_count, _a(old_peaks), _a(new_leafs), new_leafs.numel() // 5, _a(new_peaks), _a(proofs)), "mmr_append")

    def mmr_bag_peaks(self, leaf_counts, peaks, out):
        lc = _u64(leaf_counts)
        self.ok(self.lib.tf_mmr_bag_peaks(_a(lc), lc.size, _a(peaks), _a(out)), "mmr_bag_peaks")

    def mmr_verify_membership_proofs(self, leaf_count, peaks, leaf_indices, leaf_digests, path_offsets, paths, statuses):
        off = _u64(path_offsets)
        self.ok(self.lib.tf_mmr_verify_membership_proofs(leaf_count, _a(peaks), peaks.numel() // 5, off.size - 1, _a(leaf_indices), _a(leaf_digests), _a(off),
                                                         _a(paths), _a(statuses)), "mmr_verify_membership_proofs")

    def mmr_batch_mutate_leafs(self, leaf_count, peaks, mut_indices, new_leafs, mut_offsets, mut_paths, own_indices, own_offsets, own_paths, modified):
        mi, mo, oi, oo = _u64(mut_indices), _u64(mut_offsets), _u64(own_indices), _u64(own_offsets)
        self.ok(self.lib.tf_mmr_batch_mutate_leafs(leaf_count, _a(peaks), mi.size, _a(mi), _a(new_leafs), _a(mo), _a(mut_paths), oi.size, _a(oi), _a(oo),
                                                   _a(own_paths), _a(modified)), "mmr_batch_mutate_leafs")

    def mmr_successor_proof_len(self, leaf_count, k):
        return self.tf.device.mmr_successor_proof_len(leaf_count, k)

    def mmr_successor_proof_new(self, leaf_count, old_peaks, new_leafs, paths_out, new_peaks=None):
        k = new_leafs.numel() // 5
        self.ok(self.lib.tf_mmr_successor_proof_new(leaf_count, _a(old_peaks), _a(new_leafs), k, _a(paths_out), _a(new_peaks)), "mmr_successor_proof_new")
        return self.mmr_successor_proof_len(leaf_count, k)

    def mmr_verify_successor_proofs(self, old_leaf_counts, new_leaf_counts, old_peak_offsets, old_peaks, new_peak_offsets, new_peaks, path_offsets, paths, statuses):
        oc, nc, oo, no, po = (_u64(x) for x in (old_leaf_counts, new_leaf_counts, old_peak_offsets, new_peak_offsets, path_offsets))
        self.ok(self.lib.tf_mmr_verify_successor_proofs(oc.size, _a(oc), _a(nc), _a(oo), _a(old_peaks), _a(no), _a(new_peaks), _a(po), _a(paths), _a(statuses)),
                "mmr_verify_successor_proofs")

    def mmr_update_proofs_from_append(self, leaf_count, old_peaks, new_leafs, own_indices, own_offsets, own_paths, out_paths=None, new_peaks=None):
        oi, oo = _u64(own_indices), _u64(own_offsets)
        out_off, modified = np.zeros(oi.size + 1, dtype=np.uint64), np.zeros(max(oi.size, 1), dtype=np.int32)
        self.ok(self.lib.tf_mmr_update_proofs_from_append(leaf_count, _a(old_peaks), _a(new_leafs), new_leafs.numel() // 5, oi.size, _a(oi), _a(oo), _a(own_paths),
                                                          _a(out_off), _a(out_paths), 0 if out_paths is None else out_paths.numel() // 5, _a(modified),
                                                          _a(new_peaks)), "mmr_update_proofs_from_append")
        return out_off, modified[:oi.size]

    # tf_table.hip
    def gather_rows(self, table, n_rows, n_cols, indices, out, layout=0, width=1, stride=None, out_stride=None, batch=1, status=None):
        self.ok(self.lib.tf_table_gather_rows(_a(table), layout, n_rows, n_cols, width, stride, _a(indices), indices.numel(), _a(out), out_stride, batch),
                "table_gather_rows")

    def transpose(self, src, n_outer, n_inner, dst, width=1, src_stride=None, dst_stride=None, batch=1):
        self.ok(self.lib.tf_table_transpose(_a(src), n_outer, n_inner, width, src_stride, _a(dst), dst_stride, batch), "table_transpose")

    # tf_fri.hip
    def workspace(self, *a, **k):
        return self.tf.fri.workspace(*a, **k)

    def fold(self, codewords, n, offset_raw, challenges, out, batch=1, levels=1, n_sets=1, width_c=3, width_a=3):
        self.ok(self.lib.tf_fri_fold(_a(codewords), n, batch, width_c, offset_raw, _a(challenges), levels, n_sets, width_a, _a(out)), "fri_fold")


def _case(src, name, value):
    return SOURCES[src].ROWS[name][0].index(value)


ROUND_TRIP = "host round trip"
# (id, source, row, case of the row (None: its first), the triple of that case (None: all), labels the host form must show)
HOST_CASES = [
    ("ntt", "fences", "ntt_", (1, False, 2, 1, None), 0, [ROUND_TRIP]),
    ("coset_evaluate", "fences", "coset_evaluate", (1, 1), 0, [ROUND_TRIP]),
    ("coset_interpolate", "fences", "coset_interpolate", (1, 1), 0, [ROUND_TRIP]),
    ("poly_mul", "fences", "poly_mul", 1, 0, [ROUND_TRIP]),
    ("zerofier", "fences", "zerofier", ("call", 1, 1), 0, [ROUND_TRIP]),
    ("interpolate", "fences", "interpolate", ("call", 1, 1), 0, [ROUND_TRIP]),
    ("batch_evaluate", "fences", "batch_evaluate", 1, 1, [ROUND_TRIP]),
    ("tip5_permute", "fences", "tip5_permute_", ("permute", 1), 0, [ROUND_TRIP]),
    ("tip5_hash_pairs", "fences", "tip5_hash_pairs", ("pairs", 1), 0, [ROUND_TRIP]),
    ("merkle_from_rows", "fences", "merkle_from_rows", 0, 0, [ROUND_TRIP]),
    ("tip5_sponge_pad_and_absorb_all", "fences", "tip5_sponge_pad_and_absorb_all_", 1, 1, [ROUND_TRIP]),
    ("tip5_sponge_sample_scalars", "fences", "tip5_sponge_sample_scalars", ("scalars", 1), 1, ["sponge_squeeze host buffers"]),   # (the squeeze with 3 words per element)
    ("poly_sub", "fences", "poly_sub", None, 0, [ROUND_TRIP]),
    ("poly_neg", "fences", "poly_neg_", None, 0, [ROUND_TRIP]),
    ("poly_scalar_mul", "fences", "poly_scalar_mul", None, 0, [ROUND_TRIP]),
    ("poly_scale", "fences", "poly_scale", None, 0, [ROUND_TRIP]),
    ("poly_formal_derivative", "fences", "poly_formal_derivative", None, 1, [ROUND_TRIP]),   # (n = 2: the derivative of a constant needs no device)
    ("poly_degree", "fences", "poly_degree", None, 0, [ROUND_TRIP]),
    ("coset_extrapolate", "fences", "coset_extrapolate", None, 0, [ROUND_TRIP]),
    ("barycentric_evaluate", "fences", "barycentric_evaluate", None, 0, [ROUND_TRIP]),
    ("evaluate_bfe_at_xfe", "fences", "evaluate_bfe_at_xfe", None, 1, [ROUND_TRIP]),
    ("clean_divide", "fences", "clean_divide", None, 0, [ROUND_TRIP]),
    ("clean_divide_many", "fences", "clean_divide_many", None, 0, [ROUND_TRIP]),
    ("hash_table_rows", "fences", "hash_table_rows", None, 0, [ROUND_TRIP]),
    ("merkle_from_columns", "fences", "merkle_from_columns", None, 0, [ROUND_TRIP]),
    ("table_transpose", "table", "transpose", None, 0, [ROUND_TRIP]),
    ("tip5_trace", "fences", "tip5_trace_", ("trace", 1), 0, ["tip5_trace host buffers"]),
    ("tip5_hash_varlen_rows", "fences", "tip5_hash_varlen_rows", 1, 0, ["hash_varlen_rows host buffers"]),
    ("merkle_build", "fences", "merkle_build", ("build", 0), 0, [ROUND_TRIP]),
    ("merkle_root", "fences", "merkle_root", ("root", 0), 0, [ROUND_TRIP]),
    ("verify_inclusion_proofs", "fences", "verify_inclusion_proofs", ("verify", 0), 0, ["merkle proofs host buffers", "merkle proofs host roots"]),
    ("authentication_paths", "fences", "authentication_paths", ("paths", 1), 0, ["merkle proofs host buffers", "merkle proofs host paths"]),
    ("authentication_structure_from_leafs", "fences", "authentication_structure_from_leafs", 1, 0, ["merkle open leafs", "merkle open output", "merkle open roots"]),
    ("linear_combination", "fences", "linear_combination", (1, 1), 1, ["poly algebra"]),
    ("poly_add", "fences", "poly_add", ("add", 1, 1), 0, [ROUND_TRIP]),
    ("divide", "fences", "divide", (1, (3, 5)), 0, ["divide host inputs", "divide host remainder"]),
    ("divide with a quotient", "fences", "divide", (1, (7, 2)), 0, ["divide host inputs", "divide host quotient", "divide host remainder"]),
    ("fps_inverse_newton", "fences", "fps_inverse_newton", (1, 1), 0, [ROUND_TRIP]),
    ("batch_inversion", "fences", "batch_inversion", ("batch", 1, 1), 0, ["batch_inversion host buffer"]),
    ("inverse_or_zero", "fences", "inverse_or_zero", ("or_zero", 1, 1), 0, ["batch_inversion host buffer"]),
    ("get_colinear_y", "fences", "get_colinear_y", (1, 1, False), 0, ["get_colinear_y host buffers"]),
    ("are_colinear", "fences", "are_colinear", (1, 1), 3, ["are_colinear host buffers"]),
    ("mod_pow", "fences", "mod_pow", (1, True), 0, ["mod_pow host buffers"]),
    ("powers", "fences", "powers", 1, 0, ["powers host buffer"]),
    ("tip5_sponge_init", "fences", "tip5_sponge_init_", ("init", 1), 0, [ROUND_TRIP]),
    ("tip5_sponge_absorb", "fences", "tip5_sponge_absorb_", ("absorb", 1), 0, [ROUND_TRIP]),
    ("tip5_sponge_squeeze", "fences", "tip5_sponge_squeeze", ("squeeze", 1), 0, ["sponge_squeeze host buffers"]),
    ("tip5_sponge_sample_indices", "fences", "tip5_sponge_sample_indices", ("indices", 1), 0, ["sponge_indices host buffers"]),
    ("mmr_append", "fences", "mmr_append", (3, 13), 1, ["mmr_append host buffers", "mmr_append host proofs"]),
    ("mmr_bag_peaks", "fences", "mmr_bag_peaks", [5], 0, [ROUND_TRIP]),
    ("mmr_verify_membership_proofs", "fences", "mmr_verify_membership_proofs", 1, 0, ["mmr_verify host buffers"]),
    ("mmr_batch_mutate_leafs", "fences", "mmr_batch_mutate_leafs", True, 0, ["mmr_mutate host buffers", "mmr_mutate host peaks"]),
    ("mmr_successor_proof_new", "fences", "mmr_successor_proof_new", (3, 13), 0, ["mmr_successor_new host buffers", "mmr_successor_new host peaks"]),
    ("mmr_verify_successor_proofs", "fences", "mmr_verify_successor_proofs", 1, 0, ["mmr_successor_verify host buffers"]),
    ("mmr_update_proofs_from_append", "fences", "mmr_update_proofs_from_append", (7, 9), 1, ["mmr_update_proofs host buffers", "mmr_update_proofs host sweep inputs", "mmr_update_proofs host new peaks"]),
    ("table_gather_rows", "table", "gather_rows", (0, 1, 1), 0, ["table_gather_rows"]),
    ("fri_fold", "fri", "fold", (1, 1, 1, 5, None, 1), 0, [ROUND_TRIP]),
]


def run_host_case(tf, oracle, src, name, case, triple, labels):
    seen, ran = set(), 0
    for j, (shape, operands, call) in enumerate(triples(tf, oracle, src, name, case, HostForms(tf))):
        if triple is not None and j != triple:
            continue
        if any(op.name == "status" for op in operands):   # the host form's status is its return value
            operands = [op for op in operands if op.name != "status"]
            call = (lambda inner: lambda **t: inner(status=None, **t))(call)
        for mode in fence.TEMP_POISONS:
            with fence.temp_guarded(tf.lib(), mode, must_see=labels) as box:
                fence.run_once(name + " (host form)", f"{shape} [temporary poison {fence.POISONS[mode - 1]}]", operands, call, 0, "random", device="cpu")
            seen |= set(box[0].labels)
        ran += 1
    assert ran, f"triple {triple} of {name} {case} does not exist: the host case ran nothing"
    return seen


@pytest.mark.parametrize("case_id,src,name,case,triple,labels", [pytest.param(*c, id=c[0]) for c in HOST_CASES])
def test_host_form_with_guarded_device_buffers(tf, oracle, case_id, src, name, case, triple, labels):
    cases = SOURCES[src].ROWS[name][0]
    assert case is None or case in cases, "a case of the matching _dev row"
    run_host_case(tf, oracle, src, name, cases[0] if case is None else case, triple, labels)


SUBTREE = {"build": ["merkle subtree host leafs", "merkle subtree host nodes", ROUND_TRIP], "root": ["merkle subtree host leafs", "merkle subtree host root", ROUND_TRIP]}


@pytest.mark.parametrize("op", sorted(SUBTREE))
def test_host_merkle_tree_cut_into_subtrees(tf, oracle, op):
    """one tree of 8 leafs over two workers on device 0: two subtrees through merkle_subtree_host, the top layer through tf_merkle_build
    (which also writes the zero digest of node 0, as the oracle's tree has it)"""
    n, leafs, nodes = F._leafs_and_nodes(oracle, 3, 1)
    assert tf.lib().tf_merkle_multi_subtrees(n, 1, 2) == 2
    h = HostForms(tf)
    for mode in fence.TEMP_POISONS:
        with fence.temp_guarded(tf.lib(), mode, must_see=SUBTREE[op]):
            if op == "build":
                fence.run_once("merkle_build_multi", f"n={n}", [fence.inp("leaves", leafs), fence.out("nodes_out", nodes[0])],
                               lambda leaves, nodes_out: h.merkle_build(leaves, n, nodes_out, devices=[0, 0]), 0, "random", device="cpu")
            else:
                fence.run_once("merkle_root_multi", f"n={n}", [fence.inp("leaves", leafs), fence.out("root_out", nodes[0][1])],
                               lambda leaves, root_out: h.merkle_root(leaves, n, root_out, devices=[0, 0]), 0, "random", device="cpu")


def test_prepare_calls_take_their_buffers_from_the_pool(tf):
    lib = tf.lib()
    for mode in fence.TEMP_POISONS:
        with fence.temp_guarded(lib, mode, must_see=["prepare buffers"]):
            assert lib.tf_prepare_ntt(1 << 6, 2, 1, 0) == 0 and lib.tf_prepare_coset_eval(5, 7, 8, 1, 1) == 0 and lib.tf_prepare_merkle(4, 1) == 0


# ------------------------------------------------------------------ 3b. the sites no row reaches at its shapes
def _extra_divide(tf, oracle, shape, only):
    for t in F.ROWS["divide"][1](tf, oracle, tf.device, 1, shape):
        if only in t[0]:
            yield ("divide",) + t + ("cuda",)


def _extra_large_proof(tf, oracle):
    from tests import test_gpu_merkle_proofs as mp

    height, k = 10, 300   # more leafs than a proof's work space in LDS holds (256): the proof works in device memory
    idx, dig, auth, root = mp.honest(oracle, np.random.default_rng(0x1A26E), height, k)
    status = mp.check(oracle, height, idx, dig, auth, root)[0]
    lo, ao = np.array([0, k], np.uint64), np.array([0, len(auth)], np.uint64)
    ops = [fence.inp("leaf_indices", idx), fence.inp("leaf_digests", dig), fence.inp("auth_digests", auth), fence.inp("expected_roots", root),
           fence.out("statuses", F.i32([status]), dtype="int32")]
    yield ("verify_inclusion_proofs", f"height={height} leafs={k}", ops,
           lambda leaf_indices, leaf_digests, auth_digests, expected_roots, statuses:
           tf.device.verify_inclusion_proofs([height], lo, leaf_indices, leaf_digests, ao, auth_digests, expected_roots, statuses), "cuda")


def _extra_square(tf, oracle):
    na, batch = 17, 3
    a = oracle.fill_random(na * batch, 0x5C0A)
    want = F.cat([oracle.poly_mul(r, r) for r in a.reshape(batch, -1)])
    yield ("fast_square (host form)", f"na={na} batch={batch}", [fence.inp("a", a), fence.out("out", want)],
           lambda a, out: HostForms(tf).ok(tf.lib().tf_poly_square_bfe(_a(a), na, _a(out), batch), "fast_square"), "cpu")


EXTRA_CASES = {
    "divide by a constant": (lambda tf, oracle: _extra_divide(tf, oracle, (7, 1), "q only"), ["divide constant divisor"]),
    "divide a long dividend by a short divisor": (lambda tf, oracle: _extra_divide(tf, oracle, (5000, 3), "batch=3 status"), ["divide fold step"]),
    "a proof of 300 leafs": (_extra_large_proof, ["proof descriptors", "proof work space"]),
    "fast_square": (_extra_square, ["poly_square", ROUND_TRIP]),
}


@pytest.mark.parametrize("case_id", sorted(EXTRA_CASES))
def test_sites_that_no_row_reaches(tf, oracle, case_id):
    gen, labels = EXTRA_CASES[case_id]
    ran = 0
    for name, shape, operands, call, device in gen(tf, oracle):
        for mode in fence.TEMP_POISONS:
            with fence.temp_guarded(tf.lib(), mode, must_see=labels):
                fence.run_once(name, f"{shape} [temporary poison {fence.POISONS[mode - 1]}]", operands, call, 0, "random", device=device)
        ran += 1
    assert ran


def host_labels():
    """every label a host case declares (for tests/test_temp_guard_cpu.py)"""
    out = {"prepare buffers", "selftest"}
    for c in HOST_CASES:
        out |= set(c[5])
    for v in list(SUBTREE.values()) + [c[1] for c in EXTRA_CASES.values()]:
        out |= set(v)
    return out


# ------------------------------------------------------------------ 4. results do not depend on the state of the caches
CACHE_LABELS = {"temporary twiddle table", "temporary scaled twiddle table", "temporary power table", "ntt inter-pass scratch", "lat2 inter-pass scratch"}


def _dev(x):
    import torch

    return torch.from_numpy(np.ascontiguousarray(x).view(np.int64).copy()).cuda()


def _host(t):
    return t.cpu().numpy().view(np.uint64)


def _plan(lib, n, width=1):
    radices = (C.c_int * 4)()
    return lib.tf_ntt_plan(n, width, radices)


NTT_SCRATCH, LAT2_SCRATCH = "ntt inter-pass scratch", "lat2 inter-pass scratch"


def _ntt_routes(lib):
    """(n, min_passes, latency mode, passes, scratch label) of the multi-pass routes, read off the planner: the smallest n whose plan
    has an inter-pass table, as the pass kernels run it (latency kernels off: the plan tf_ntt_plan reports) and as a small call runs
    it by default (the two latency-shaped launches of launch_lat2, which take a scratch of their own), and one size in three passes"""
    two = next(1 << k for k in range(1, 21) if _plan(lib, 1 << k) >= 2)
    assert _plan(lib, two) == 2 and two <= 1 << 16, two
    three = 1 << 15
    lib.tf_set_ntt_min_passes(3)
    try:
        assert _plan(lib, three) == 3 and _plan(lib, three, 3) == 3
        assert all(lib.tf_ntt_launch_count(three, batch, width) == 3 for batch in (1, 3) for width in (1, 3))
    finally:
        lib.tf_set_ntt_min_passes(0)
    # by default a call of at most 2^21 words between 2^13 and 2^20 points takes the latency-shaped pair (lat2_wanted, tf_plan.hip)
    assert 13 <= two.bit_length() - 1 <= 20 and 9 * two <= 1 << 21 and all(lib.tf_ntt_launch_count(two, batch, width) == 2 for batch in (1, 3) for width in (1, 3))
    return [(two, 0, 0, 2, NTT_SCRATCH), (two, 0, -1, 2, LAT2_SCRATCH), (three, 3, -1, 3, NTT_SCRATCH)]


@pytest.mark.parametrize("width", [1, 3])
def test_ntt_with_temporary_inter_pass_tables(tf, oracle, width):
    lib, d = tf.lib(), tf.device
    runs = []   # (n, batch, inverse, min_passes, latency mode, scratch label, input, expected)
    for n, passes, lat, _, scratch in _ntt_routes(lib):
        for batch in (1, 3):
            x = oracle.fill_random(n * batch * width, 0x7E00 + n + batch + width)
            for inverse in (False, True):
                runs.append((n, batch, inverse, passes, lat, scratch, x, oracle.ntt(x, width=width, inverse=inverse, batch=batch)))

    def go(guard_mode=0, forced=False):
        got = []
        for n, batch, inverse, passes, lat, scratch, x, want in runs:
            t = _dev(x)
            what = f"ntt n={n} batch={batch} width={width} inverse={inverse} min_passes={passes} latency={lat} guard={guard_mode} forced={forced}"
            lib.tf_set_ntt_min_passes(passes)
            lib.tf_set_ntt_latency_kernel(lat)
            try:
                if guard_mode:
                    # every run declares what it must see: its own scratch, and under forcing the temporary table -- and never the other route's scratch
                    with fence.temp_guarded(lib, guard_mode, must_see=[scratch] + (["temporary twiddle table"] if forced else [])) as box:
                        d.ntt_(t, n, batch=batch, width=width, inverse=inverse)
                    other = LAT2_SCRATCH if scratch == NTT_SCRATCH else NTT_SCRATCH
                    assert other not in box[0].labels, (what, box[0])
                    assert forced or "temporary twiddle table" not in box[0].labels, (what, box[0])
                else:
                    d.ntt_(t, n, batch=batch, width=width, inverse=inverse)
            finally:
                lib.tf_set_ntt_min_passes(0)
                lib.tf_set_ntt_latency_kernel(-1)
            got.append(_host(t))
            assert np.array_equal(got[-1], want), what
        return got

    try:
        assert lib.tf_debug_force_temp_tables(1) == 0
        forced = go(forced=True)
        for mode in fence.TEMP_POISONS:
            go(mode, forced=True)
    finally:
        lib.tf_debug_force_temp_tables(0)
    assert lib.tf_release_caches() == 0
    plain = go()
    go(3)   # the cached tables, the scratch guarded
    assert all(np.array_equal(a, b) for a, b in zip(forced, plain))


def _scaled_order(tf, oracle):
    """the smallest order at which a BFE coset evaluation of `order` coefficients takes the scaled inter-pass table (the two-pass plans
    of tf_ntt_plan, 2^21 and 2^22 points): read off the labels of a forced, guarded call"""
    lib, d = tf.lib(), tf.device
    for k in (21, 22):
        order = 1 << k
        assert _plan(lib, order) == 2
        c, out = _dev(oracle.fill_random(order, 0x5CA1ED)), _dev(np.zeros(order, np.uint64))
        with fence.temp_guarded(lib, 3) as box:
            d.coset_evaluate(c, order, oracle.bfe_new(3), out, order)
        if "temporary scaled twiddle table" in box[0].labels:
            return order
    return None


def test_coset_evaluation_with_uncached_scaled_tables_and_temporary_power_tables(tf, oracle):
    lib, d = tf.lib(), tf.device
    assert lib.tf_release_caches() == 0
    try:
        assert lib.tf_debug_force_temp_tables(1) == 0
        order = _scaled_order(tf, oracle)
    finally:
        lib.tf_debug_force_temp_tables(0)
    assert order is not None, "neither two-pass plan takes the scaled inter-pass table"
    assert lib.tf_release_caches() == 0
    coeffs = oracle.fill_random(order, 0xC05E7)
    offsets = [oracle.bfe_new(v) for v in (7, 11, 13, 17, 19)]
    wants = [oracle.coset_evaluate(coeffs, off, order) for off in offsets]
    c = _dev(coeffs)

    SCALED, PLAIN = "temporary scaled twiddle table", "temporary twiddle table"

    def go(guard_mode=0, must_see=lambda j: (), must_not_see=lambda j: ()):
        got = []
        for j, (off, want) in enumerate(zip(offsets, wants)):
            out = _dev(np.zeros(order, np.uint64))
            if guard_mode:
                with fence.temp_guarded(lib, guard_mode, must_see=[NTT_SCRATCH] + list(must_see(j))) as box:
                    d.coset_evaluate(c, order, off, out, order)
                assert not set(must_not_see(j)) & set(box[0].labels), (j, box[0])
            else:
                d.coset_evaluate(c, order, off, out, order)
            got.append(_host(out))
            assert np.array_equal(got[-1], want), f"coset evaluation order={order} offset {j} guard={guard_mode}"
        return got

    # five offsets, unforced: four scaled tables are cached, the fifth falls off the four-entry cache on its own (its plain table is cached)
    natural = go(3, must_see=lambda j: [SCALED] if j == 4 else [], must_not_see=lambda j: [PLAIN] if j == 4 else [SCALED, PLAIN])
    try:
        assert lib.tf_debug_force_temp_tables(1) == 0
        forced = go()
        go(2, must_see=lambda j: [SCALED, PLAIN])   # every offset on both temporary routes
    finally:
        lib.tf_debug_force_temp_tables(0)
    assert lib.tf_release_caches() == 0
    plain = go()
    assert all(np.array_equal(a, b) for a, b in zip(natural, plain)) and all(np.array_equal(a, b) for a, b in zip(forced, plain))
    assert lib.tf_release_caches() == 0


def test_seventeenth_power_table_is_a_temporary(tf, oracle):
    """sixteen power tables stay cached; the seventeenth offset builds its table into a scratch block, in guard mode a guarded one"""
    lib, d = tf.lib(), tf.device
    assert lib.tf_release_caches() == 0
    nc, order = 700, 1024
    coeffs = oracle.fill_random(nc, 0x9077)
    c = _dev(coeffs)
    try:
        for j in range(17):
            off = oracle.bfe_new(101 + j)
            out = _dev(np.zeros(order, np.uint64))
            with fence.temp_guarded(lib, 1 + j % 3) as box:
                d.coset_evaluate(c, nc, off, out, order)
            assert np.array_equal(_host(out), oracle.coset_evaluate(coeffs, off, order)), j
            assert ("temporary power table" in box[0].labels) == (j == 16), (j, box[0])
    finally:
        assert lib.tf_release_caches() == 0


# ------------------------------------------------------------------ 5. the workspace functions: the bytes the call requests
def _requested(report, labels):
    assert set(report.labels) >= set(labels), report
    return sum(report.labels[l][1] for l in labels)


@pytest.mark.parametrize("case", FRI.ROWS["fold"][0][:5])   # one pass (nothing), two passes (one intermediate), four (both)
def test_fri_fold_workspace_is_what_the_call_requests(tf, oracle, case):
    wc, wa, k, batch, extra, n_sets = case
    rmax = max(tf.fri.plan(1 << 12, 12))
    n, levels = 1 << k, (k if extra is None else rmax + extra)
    for shape, operands, call in triples(tf, oracle, "fri", "fold", case):
        with fence.temp_guarded(tf.lib(), 3) as box:
            fence.run_once("fold", shape, operands, call, 0, "random")
        own = [l for l in box[0].labels if l.startswith("fri_fold")]
        assert tf.lib().tf_fri_fold_workspace(n, batch, wc, wa, levels) == sum(box[0].labels[l][1] for l in own), box[0]


@pytest.mark.parametrize("case", TAB.ROWS["lde_rows"][0])
def test_table_lde_rows_workspace_is_what_the_call_requests(tf, oracle, case):
    w, c = case
    n, m, n_cols = 8, 32, 5   # the row's shape
    for shape, operands, call in triples(tf, oracle, "table", "lde_rows", case):
        with fence.temp_guarded(tf.lib(), 3) as box:
            fence.run_once("lde_rows", shape, operands, call, 0, "random")
        own = [l for l in box[0].labels if l == "table_lde_rows"]
        assert tf.lib().tf_table_lde_rows_workspace(n, m, n_cols, w, c) == sum(box[0].labels[l][1] for l in own), box[0]


@pytest.mark.parametrize("height,batch", [(2, 1), (10, 3)])
def test_merkle_open_workspace_is_what_the_call_requests(tf, oracle, height, batch):
    d = tf.device
    n, leafs, nodes = F._leafs_and_nodes(oracle, height, batch)
    idx = F._index_sets(n)[2 if height < 5 else -1]
    ids = oracle.auth_structure_indices(n, idx).astype(np.int64)
    assert ids.size
    out = _dev(np.zeros(batch * ids.size * 5 + 5, np.uint64))
    with fence.temp_guarded(tf.lib(), 3, must_see=["merkle open"]) as box:
        d.authentication_structure_from_leafs(_dev(leafs), n, idx, out=out, batch=batch)
    assert np.array_equal(_host(out)[:batch * ids.size * 5], F.cat([t[ids] for t in nodes]))
    assert tf.lib().tf_merkle_auth_structure_from_leafs_workspace(n, batch, ids.size) == _requested(box[0], ["merkle open"]), box[0]


@pytest.mark.parametrize("case", MS.ROWS["structure_from_leafs"][0][:2])
def test_merkle_open_sampled_workspace_is_what_the_call_requests(tf, oracle, case):
    height, n_lists, tpl, k = case
    for shape, operands, call in triples(tf, oracle, "sampled", "structure_from_leafs", case):
        with fence.temp_guarded(tf.lib(), 3, must_see=["merkle open (sampled)"]) as box:
            fence.run_once("structure_from_leafs", shape, operands, call, 0, "random")
        want = tf.lib().tf_merkle_auth_structure_from_leafs_sampled_workspace(1 << height, n_lists * tpl, k, n_lists)
        assert want == _requested(box[0], ["merkle open (sampled)"]), box[0]
