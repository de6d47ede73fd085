/*
 * tf_hip.h -- C ABI of libtf_hip.so: the MI355X (gfx950) backend for the data-parallel hot path of
 * Neptune-Crypto/twenty-first (Goldilocks NTT/iNTT, fast_coset_evaluate, Tip5, Merkle builder).
 *
 * The reference has no FFI of its own (it is a pure-Rust crate); each entry point below replaces the
 * body of one Rust function, cited as file:line relative to twenty-first/src/.  INTEGRATION.md shows
 * the Rust `extern "C"` shim a maintainer would add.
 *
 * Data contract (identical to the reference's in-memory layout, so `&mut [BFieldElement]` can be
 * passed as `*mut u64` without conversion):
 *   BFieldElement  = 1 little-endian u64: x * 2^64 mod p, canonical (< p)   math/b_field_element.rs:84-86 (#[repr(transparent)])
 *   XFieldElement  = 3 consecutive BFieldElements [c0, c1, c2]              math/x_field_element.rs:56-59 (#[repr(transparent)])
 *   Digest         = 5 consecutive BFieldElements                           tip5/digest.rs:29
 *   Tip5 state     = 16 consecutive BFieldElements                          tip5/mod.rs:159-165
 * Inputs must be canonical (true for anything built through BFieldElement::new); outputs always are.
 * All pointers 8-byte aligned.  Results are bit-identical to the reference's CPU path.
 *
 * Two flavours of every entry point:
 *   tf_xxx(...)            host pointers; copies in, runs on the current HIP device, copies out, returns when done.
 *   tf_xxx_dev(..., stream) device pointers (memory of the current HIP device); work is enqueued on `stream`
 *                          (a hipStream_t, NULL = default stream) and the call returns without synchronising.
 * Every function is re-entrant and may be called concurrently from many host threads
 * (the reference's ntt is called from rayon workers, math/ntt.rs:250-274).
 *
 * There is NO CPU fallback: without a usable HIP device every call returns TF_ERR_NO_DEVICE.
 *
 * Return value: 0 on success, otherwise one of the codes below.  Codes 1-3, 11 and 19-21 are the reference's
 * MerkleTreeError variants (util_types/merkle_tree.rs:933-965); codes 4-6 replace panics.
 * No C++ exception leaves the library: every status-returning entry point catches what its host-side C++ (tables, caches,
 * worker threads) may throw and returns TF_ERR_OUT_OF_MEMORY (a failed host allocation) or TF_ERR_INTERNAL, with the
 * message in tf_last_error() (csrc/tf_guard.h) -- a Rust `extern "C"` caller never sees an unwind.
 */
#ifndef TF_HIP_H
#define TF_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum tf_status {
    TF_OK = 0,
    TF_ERR_TOO_FEW_LEAFS = 1,              /* MerkleTreeError::TooFewLeafs            merkle_tree.rs:394-396 */
    TF_ERR_INCORRECT_NUMBER_OF_LEAFS = 2,  /* MerkleTreeError::IncorrectNumberOfLeafs merkle_tree.rs:398-401 */
    TF_ERR_TREE_TOO_HIGH = 3,              /* MerkleTreeError::TreeTooHigh (allocation failure) :405-410 */
    TF_ERR_LEN_NOT_POWER_OF_TWO = 4,       /* ntt/intt panic: assert!(len == 0 || len.is_power_of_two()) math/ntt.rs:137 */
    TF_ERR_LEN_TOO_LARGE = 5,              /* ntt/intt panic: len > u32::MAX (math/ntt.rs:134-139), i.e. a power of two above 2^31 */
    TF_ERR_ORDER_NOT_ABOVE_DEGREE = 6,     /* fast_coset_evaluate panic: order <= degree  math/polynomial.rs:1388-1392 */
    TF_ERR_NULL_POINTER = 7,
    TF_ERR_NO_DEVICE = 8,                  /* no HIP device / HIP runtime unusable */
    TF_ERR_HIP = 9,                        /* a HIP call failed; see tf_last_error() */
    TF_ERR_OUT_OF_MEMORY = 10,
    TF_ERR_LEAF_INDEX_INVALID = 11,        /* MerkleTreeError::LeafIndexInvalid  merkle_tree.rs:486-488 */
    TF_ERR_INVERSE_OF_ZERO = 12,           /* offset.inverse() of zero panics    b_field_element.rs:264-268 */
    TF_ERR_BUFFER_TOO_SMALL = 13,
    TF_ERR_EMPTY_DOMAIN = 14,              /* interpolate panic: "interpolation must happen through more than zero points"  math/polynomial.rs:1503-1506 */
    TF_ERR_DIVISION_BY_ZERO = 15,          /* naive_divide panic: "divisor should be non-zero"  math/polynomial.rs:556-559 */
    TF_ERR_DIVISION_NOT_CLEAN = 16,        /* clean_divide panic: the quotient does not come back to the base field  math/polynomial.rs:2374, :2410 */
    TF_ERR_INVALID_ARGUMENT = 17,          /* an index / count argument of a host-logic helper (tf_shard_range, tf_merkle_subtree_layer_range) is out of range;
                                            * a divisor / power series whose last coefficient is zero (tf_poly_divide_*, tf_poly_fps_inverse_newton_*) */
    TF_ERR_INTERNAL = 18,                  /* a C++ exception other than an allocation failure was caught at the ABI (csrc/tf_guard.h); see tf_last_error() */
    TF_ERR_AUTH_STRUCTURE_LENGTH_MISMATCH = 19,  /* MerkleTreeError::AuthenticationStructureLengthMismatch  merkle_tree.rs:933-965 (raised :910-912) */
    TF_ERR_REPEATED_LEAF_DIGEST_MISMATCH = 20,   /* MerkleTreeError::RepeatedLeafDigestMismatch  merkle_tree.rs:933-965 (raised :921-923) */
    TF_ERR_ROOT_MISMATCH = 21,                   /* MerkleTreeError::RootMismatch  merkle_tree.rs:933-965 (raised :740-742) */
    /* the reasons MmrMembershipProof::verify returns false, in its order (mmr/mmr_membership_proof.rs:36-77) */
    TF_ERR_MMR_LEAF_INDEX_OUT_OF_RANGE = 22,     /* leaf_index >= num_leafs  :43-46 */
    TF_ERR_MMR_PEAK_COUNT_MISMATCH = 23,         /* peaks.len() != num_leafs.count_ones()  :50-54 */
    TF_ERR_MMR_AUTH_PATH_LENGTH_MISMATCH = 24,   /* authentication path length != height of the leaf's peak  :56-60 */
    TF_ERR_MMR_PEAK_MISMATCH = 25,               /* the path does not hash to the leaf's peak  :76 */
    TF_ERR_UPPER_BOUND_NOT_POWER_OF_TWO = 26,    /* Tip5::sample_indices panic: assert!(upper_bound.is_power_of_two())  tip5/mod.rs:637 */
    /* the errors of MmrSuccessorProof::verify_internal, in the order it can raise them (mmr/mmr_successor_proof.rs:142-223) */
    TF_ERR_MMR_INCONSISTENT_OLD = 27,            /* the old accumulator has not popcount(num_leafs) peaks  :143-145 */
    TF_ERR_MMR_INCONSISTENT_NEW = 28,            /* the new accumulator has not popcount(num_leafs) peaks  :147-149 */
    TF_ERR_MMR_OLD_HAS_MORE_LEAFS = 29,          /* OldHasMoreLeafsThanNew  :170 */
    TF_ERR_MMR_SUCCESSOR_PATH_TOO_SHORT = 30,    /* AuthenticationPathTooShort  :196, :203 */
    TF_ERR_MMR_SUCCESSOR_PATH_TOO_LONG = 31,     /* AuthenticationPathTooLong  :151-157, :213-215 */
    TF_ERR_MMR_DIFFERENT_SHARED_PEAK = 32,       /* DifferentSharedPeak  :164-168, :182-184 */
    TF_ERR_MMR_DIFFERENT_UNSHARED_PEAK = 33      /* DifferentUnsharedPeak  :217-220 */
};

/* Human-readable name of a status code. */
const char *tf_status_string(int status);
/* Text of the last HIP failure on the calling thread ("" if none). */
const char *tf_last_error(void);
/* Library/ABI version (major * 1000 + minor). */
int tf_version(void);
/* First 16 hex digits of the SHA-256 of the sources this library was built from (csrc/Makefile).  Stored rocprof records carry
 * it so that a figure is never quoted for another build. */
const char *tf_source_hash(void);
/* Number of visible HIP devices (0 if the runtime is unusable). */
int tf_device_count(void);
/* What the library keeps in HBM for speed, per device and for the life of the process: work space between the passes of the
 * multi-pass transforms (at most 12 GiB), inter-pass twiddle tables (at most 4 GiB), coset power tables (at most 1 GiB), and
 * the freed blocks of the memory pool its stream-ordered temporaries come from (a pool of the library's own per device: the
 * application's default pool and its attributes are left alone.  Only if the runtime refuses to create a pool does the library
 * fall back to the device's default pool, and then it changes ONE attribute of it -- hipMemPoolReuseFollowEventDependencies
 * off, which correctness needs when several streams share the library's scratch cache -- and nothing else).
 * tf_release_caches() waits for the current device and frees all of it (the next call rebuilds what it needs); meant for hosts
 * that share the GPU with other users of its memory.  Call it when no other thread is inside the library on that device: a
 * call in flight on another host thread may hold a pointer to a table this frees. */
int tf_release_caches(void);

/* ---------------------------------------------------------------------------------------------
 * Devices.  Every entry point of this header runs on the calling thread's CURRENT HIP device (hipSetDevice semantics: per host
 * thread, default 0); the library keeps its tables, pools and streams per device, and any number of host threads may be inside it
 * on the same or on different devices.  tf_set_device / tf_get_device are that selector for callers that do not link the HIP
 * runtime themselves (a Rust crate binds only this library).
 * Errors: device < 0 or >= tf_device_count() -> TF_ERR_NO_DEVICE.
 */
int tf_set_device(int device);
int tf_get_device(int *device);

/* ---------------------------------------------------------------------------------------------
 * Warm-up.  The FIRST call of a shape on a device builds that shape's tables, opens kernel attributes, uploads the Tip5 constants and
 * creates the library's pool / side streams / scratch on that device -- steps that wait for the device and may synchronise it as a whole.
 * tf_prepare_* runs the shape once on zeroed scratch of the same size on the CURRENT device and returns when it is done; afterwards every
 * tf_*_dev call of that shape (same n, batch, width, direction / offset) on that device only enqueues work on the caller's stream.  A host
 * thread that drives several GPUs round-robin ("eight GPUs from one thread") calls these once per device at start-up.
 * Errors: as the call they prepare; width not 1 / 3 -> TF_ERR_INVALID_ARGUMENT; scratch allocation -> TF_ERR_OUT_OF_MEMORY. */
int tf_prepare_ntt(size_t n, size_t batch, int width, int inverse);
int tf_prepare_coset_eval(size_t n_coeffs, uint64_t offset_raw, size_t order, size_t batch, int width);
int tf_prepare_merkle(size_t n_leaves, size_t batch);

/* ---------------------------------------------------------------------------------------------
 * One host-resident batch over several GPUs.      replaces  the rayon fan-out over independent units in the reference's callers:
 *                                                            par_iter over polynomials around ntt / fast_coset_evaluate
 *                                                            (math/ntt.rs:250-274 is the unit), MerkleTree::par_new's
 *                                                            thread split util_types/merkle_tree.rs:165-212
 * Same arguments and results as tf_ntt_{bfe,xfe}, tf_coset_eval_{bfe,xfe}, tf_merkle_{build,root} on HOST pointers, plus a device
 * list: `devices` = n_devices device indices, or NULL for every visible device (n_devices is then ignored).  The `batch` units
 * (transforms, polynomials, trees) are independent; they are cut into n_devices contiguous slices by tf_shard_range's rule
 * (slice g takes units [g*base + min(g, extra), ...) with base = batch / G, extra = batch % G: the first `extra` slices hold one
 * more unit) and one worker thread per slice runs the single-device entry point on devices[g]: its own stream, its own H2D /
 * compute / D2H, all slices concurrently -- a host-resident batch crosses every listed GPU's PCIe link at once.  Nothing is
 * exchanged between devices and no collective library is involved; every result lands in the caller's buffer at its unit's
 * offset, so the output is word for word that of the single-device call.  A device may be listed more than once (several
 * workers, i.e. several copy/compute streams, on one GPU).  The calling thread's current device is not changed.
 * Errors: argument errors exactly as the single-device call (checked before any worker starts); a device index out of range ->
 * TF_ERR_NO_DEVICE; if workers fail, the status of the first failing slice in batch order is returned and tf_last_error() names
 * the device and slice.  tf_shard_range: n_shards <= 0 or shard outside [0, n_shards) -> TF_ERR_INVALID_ARGUMENT.
 *
 * FEWER TREES THAN DEVICES (in particular ONE tree): tf_merkle_{build,root}_multi cut every tree into S subtrees, S the largest power of
 * two with batch * S <= n_devices and at least two leaves per subtree -- exactly the cut MerkleTree::par_new makes over its threads
 * (util_types/merkle_tree.rs:165-212; layer l of subtree s of S is the run [(S + s) 2^l, (S + s + 1) 2^l) of the heap-ordered node
 * array, subtrees_mut :247-275).  Unit u = (tree u / S, subtree u % S); the batch * S units are dealt to the listed devices by
 * tf_shard_range's rule; every worker copies its subtrees' layers straight to their place in the caller's node array; the S subtree
 * roots of a tree (40 bytes each) are gathered on the host and the top log2 S layers are built on devices[0].  Same words as the
 * single-device call.  tf_merkle_multi_subtrees returns S for a shape (host logic, no device touched); tf_merkle_subtree_layer_range
 * the node-index run of one layer of one subtree (errors: TF_ERR_INVALID_ARGUMENT for a subtree / layer that does not exist, the
 * leaf-count errors of tf_merkle_build).
 */
int tf_shard_range(size_t total_units, int n_shards, int shard, size_t *begin, size_t *end);
int tf_merkle_multi_subtrees(size_t n_leaves, size_t batch, int n_devices);
int tf_merkle_subtree_layer_range(size_t n_leaves, size_t n_subtrees, size_t subtree, unsigned layer, size_t *begin, size_t *end);
int tf_ntt_bfe_multi(uint64_t *x, size_t n, size_t batch, int inverse, const int *devices, int n_devices);
int tf_ntt_xfe_multi(uint64_t *x, size_t n, size_t batch, int inverse, const int *devices, int n_devices);
int tf_coset_eval_bfe_multi(const uint64_t *coeffs, size_t n_coeffs, uint64_t offset_raw, uint64_t *out, size_t order, size_t batch,
                            const int *devices, int n_devices);
int tf_coset_eval_xfe_multi(const uint64_t *coeffs, size_t n_coeffs, uint64_t offset_raw, uint64_t *out, size_t order, size_t batch,
                            const int *devices, int n_devices);
int tf_merkle_build_multi(const uint64_t *leaves, size_t n_leaves, uint64_t *nodes_out, size_t batch, const int *devices, int n_devices);
int tf_merkle_root_multi(const uint64_t *leaves, size_t n_leaves, uint64_t *root_out, size_t batch, const int *devices, int n_devices);

/* ---------------------------------------------------------------------------------------------
 * NTT / iNTT            replaces  pub fn ntt<FF>(x: &mut [FF])   math/ntt.rs:67-82
 *                                 pub fn intt<FF>(x: &mut [FF])  math/ntt.rs:109-125
 * x: `batch` contiguous slices of n elements each, transformed in place, natural order in and out.
 * batch = 1 reproduces one Rust call; n = 0 and n = 1 are no-ops exactly as in the reference.
 * inverse != 0 selects intt (w^-1 twiddles and the n^-1 unscale of ntt.rs:220-228).
 * Errors: n not 0/power of two -> TF_ERR_LEN_NOT_POWER_OF_TWO; n > 2^31 -> TF_ERR_LEN_TOO_LARGE.
 */
int tf_ntt_bfe(uint64_t *x, size_t n, size_t batch, int inverse);
int tf_ntt_xfe(uint64_t *x /* 3n words per slice */, size_t n, size_t batch, int inverse);
int tf_ntt_bfe_dev(uint64_t *d_x, size_t n, size_t batch, int inverse, void *stream);
int tf_ntt_xfe_dev(uint64_t *d_x, size_t n, size_t batch, int inverse, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Coset evaluation      replaces  Polynomial::fast_coset_evaluate(&self, offset, order) -> Vec<FF>
 *                                 math/polynomial.rs:1374-1399  (= scale :760-773, zero-pad, ntt)
 * coeffs: `batch` polynomials of n_coeffs coefficients each (low to high degree), read only;
 * out:    `batch` x `order` evaluations: out[i] = f(offset * w_order^i).
 * offset_raw is a BFieldElement (raw Montgomery word); an XFieldElement offset stays on the caller's side.
 * Errors: n_coeffs > order -> TF_ERR_ORDER_NOT_ABOVE_DEGREE (trim leading zero coefficients first, as
 * Polynomial::degree() does); order not a power of two / too large as for tf_ntt_*.
 */
int tf_coset_eval_bfe(const uint64_t *coeffs, size_t n_coeffs, uint64_t offset_raw, uint64_t *out, size_t order, size_t batch);
int tf_coset_eval_xfe(const uint64_t *coeffs, size_t n_coeffs, uint64_t offset_raw, uint64_t *out, size_t order, size_t batch);
int tf_coset_eval_bfe_dev(const uint64_t *d_coeffs, size_t n_coeffs, uint64_t offset_raw, uint64_t *d_out, size_t order, size_t batch, void *stream);
int tf_coset_eval_xfe_dev(const uint64_t *d_coeffs, size_t n_coeffs, uint64_t offset_raw, uint64_t *d_out, size_t order, size_t batch, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Tip5                  replaces  Tip5::permutation  tip5/mod.rs:529-533   (states: count x 16 words, in place)
 *                                 Tip5::hash_10 / hash_pair  :559-586       (in: count x 10 words, out: count x 5)
 *                                 Tip5::hash_varlen  :617-623 (+ sponge.rs:41-55)   one digest per row
 *                                 Tip5::trace  :538-548   trace: count x 6 x 16 words (the state before the permutation and
 *                                                          after each of the 5 rounds); states end permuted, as `&mut self` does
 * Batching is the only reason to cross the boundary; a single hash_pair belongs on the CPU.
 */
int tf_tip5_permute(uint64_t *states, size_t count);
int tf_tip5_trace(uint64_t *states, uint64_t *trace, size_t count);
int tf_tip5_trace_dev(uint64_t *d_states, uint64_t *d_trace, size_t count, void *stream);
int tf_tip5_hash_pairs(const uint64_t *in, uint64_t *out, size_t count);
int tf_tip5_hash_varlen_rows(const uint64_t *rows, size_t row_len, size_t n_rows, uint64_t *out);
int tf_tip5_permute_dev(uint64_t *d_states, size_t count, void *stream);
int tf_tip5_hash_pairs_dev(const uint64_t *d_in, uint64_t *d_out, size_t count, void *stream);
int tf_tip5_hash_varlen_rows_dev(const uint64_t *d_rows, size_t row_len, size_t n_rows, uint64_t *d_out, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Merkle tree           replaces  MerkleTree::par_new / sequential_new   util_types/merkle_tree.rs:149-212
 *                                 MerkleTree::par_frugal_root / sequential_frugal_root   :299-364
 * leaves:    `batch` x n_leaves digests.
 * nodes_out: `batch` x 2*n_leaves digests in the reference's heap layout: nodes[0] = all-zero dummy,
 *            nodes[1] = root, nodes[i] = hash_pair(nodes[2i], nodes[2i+1]), leaves at nodes[n..2n).
 * root_out:  `batch` digests.
 * Errors: n_leaves == 0 -> TF_ERR_TOO_FEW_LEAFS (as par_new/sequential_new :394-396 and sequential_frugal_root
 * :300-302; par_frugal_root reports IncorrectNumberOfLeafs for 0 leaves, :333-335 -- its shim checks that first);
 * not a power of two -> TF_ERR_INCORRECT_NUMBER_OF_LEAFS; device allocation failure -> TF_ERR_TREE_TOO_HIGH.
 */
int tf_merkle_build(const uint64_t *leaves, size_t n_leaves, uint64_t *nodes_out, size_t batch);
int tf_merkle_root(const uint64_t *leaves, size_t n_leaves, uint64_t *root_out, size_t batch);
int tf_merkle_build_dev(const uint64_t *d_leaves, size_t n_leaves, uint64_t *d_nodes_out, size_t batch, void *stream);
int tf_merkle_root_dev(const uint64_t *d_leaves, size_t n_leaves, uint64_t *d_root_out, size_t batch, void *stream);

/* ---------------------------------------------------------------------------------------------
 * "Next" rows of the scope table: the callers on either side of the path, kept in HBM.
 *
 * Coset interpolation   replaces  Polynomial::fast_coset_interpolate(offset, values)  math/polynomial.rs:1907-1918
 *   values: batch x n evaluations on {offset * w_n^i}; out: batch x n coefficients (intt, then coefficient j
 *   times offset^-j, fused into the last pass).  offset_raw == 0 -> TF_ERR_INVERSE_OF_ZERO.
 * Hadamard product      the pointwise product inside fast_multiply  math/polynomial.rs:920-925
 *   (BFieldElement b_field_element.rs:755-762; XFieldElement x_field_element.rs:512-536); out may alias a or b.
 * Polynomial product    replaces  Polynomial::fast_multiply  math/polynomial.rs:900-932
 *   a: batch x na coefficients, b: batch x nb, out: batch x (na + nb - 1); zero-pad to the next power of two,
 *   ntt both, pointwise product, intt, truncate -- all on the device.  na == 0 or nb == 0: nothing is written.
 * Low-degree extension  fast_coset_interpolate followed by fast_coset_evaluate with the coefficients staying in HBM:
 *   values on {offset_in * w_n^i} -> values on {offset_out * w_m^i}, m >= n, both powers of two.
 * Rows -> Merkle tree   Tip5::hash_varlen of every row (tip5/mod.rs:617-623) written straight into the leaf level
 *   of the tree (util_types/merkle_tree.rs:165-212); rows: batch x n_rows x row_len words; nodes_out as tf_merkle_build.
 * Authentication structure  replaces MerkleTree::authentication_structure_node_indices / authentication_structure
 *   util_types/merkle_tree.rs:449-504, :614-622: node indices (needed minus computable, descending) and the gather of
 *   those digests from a device-resident node array.  *out_count receives the number of nodes; leaf index >=
 *   num_leafs -> TF_ERR_LEAF_INDEX_INVALID; num_leafs not a power of two -> TF_ERR_INCORRECT_NUMBER_OF_LEAFS.
 *   tf_merkle_authentication_structure_dev synchronises `stream` (its result is host data).
 */
int tf_coset_interpolate_bfe(const uint64_t *values, size_t n, uint64_t offset_raw, uint64_t *out, size_t batch);
int tf_coset_interpolate_xfe(const uint64_t *values, size_t n, uint64_t offset_raw, uint64_t *out, size_t batch);
int tf_coset_interpolate_bfe_dev(const uint64_t *d_values, size_t n, uint64_t offset_raw, uint64_t *d_out, size_t batch, void *stream);
int tf_coset_interpolate_xfe_dev(const uint64_t *d_values, size_t n, uint64_t offset_raw, uint64_t *d_out, size_t batch, void *stream);
int tf_hadamard_bfe_dev(const uint64_t *d_a, const uint64_t *d_b, uint64_t *d_out, size_t count, void *stream);
int tf_hadamard_xfe_dev(const uint64_t *d_a, const uint64_t *d_b, uint64_t *d_out, size_t count, void *stream);
int tf_poly_mul_bfe(const uint64_t *a, size_t na, const uint64_t *b, size_t nb, uint64_t *out, size_t batch);
int tf_poly_mul_xfe(const uint64_t *a, size_t na, const uint64_t *b, size_t nb, uint64_t *out, size_t batch);
int tf_poly_mul_bfe_dev(const uint64_t *d_a, size_t na, const uint64_t *d_b, size_t nb, uint64_t *d_out, size_t batch, void *stream);
int tf_poly_mul_xfe_dev(const uint64_t *d_a, size_t na, const uint64_t *d_b, size_t nb, uint64_t *d_out, size_t batch, void *stream);
/* Polynomial::fast_square  math/polynomial.rs:780-798: out = batch x (2 na - 1) coefficients (one forward transform). */
int tf_poly_square_bfe(const uint64_t *a, size_t na, uint64_t *out, size_t batch);
int tf_poly_square_xfe(const uint64_t *a, size_t na, uint64_t *out, size_t batch);
int tf_poly_square_bfe_dev(const uint64_t *d_a, size_t na, uint64_t *d_out, size_t batch, void *stream);
int tf_poly_square_xfe_dev(const uint64_t *d_a, size_t na, uint64_t *d_out, size_t batch, void *stream);
/* fast_multiply (math/polynomial.rs:900-932) of `batch` polynomials of na coefficients each (packed) by ONE polynomial b -- a table of
 * numerators times the same zerofier: b is transformed once.  out: batch x (na + nb - 1) coefficients.  Device-resident only. */
int tf_poly_mul_shared_bfe_dev(const uint64_t *d_a, size_t na, size_t batch, const uint64_t *d_b, size_t nb, uint64_t *d_out, void *stream);
int tf_poly_mul_shared_xfe_dev(const uint64_t *d_a, size_t na, size_t batch, const uint64_t *d_b, size_t nb, uint64_t *d_out, void *stream);
int tf_lde_bfe_dev(const uint64_t *d_values, size_t n, uint64_t offset_in_raw, uint64_t *d_out, size_t m, uint64_t offset_out_raw, size_t batch, void *stream);
int tf_lde_xfe_dev(const uint64_t *d_values, size_t n, uint64_t offset_in_raw, uint64_t *d_out, size_t m, uint64_t offset_out_raw, size_t batch, void *stream);
/* Polynomial::batch_evaluate / iterative_batch_evaluate  math/polynomial.rs:1840-1894: out[i] = f(points[i]),
 * points in the same field as the coefficients (bfe: 1 word per point, xfe: 3).  Few points / short polynomials: Horner per
 * point; many points on a long polynomial: remaindering down a zerofier tree built from batched fast_multiply calls
 * (O((n + m) log^2 m), the reference's divide_and_conquer_batch_evaluate :1882-1894 / math/zerofier_tree.rs). */
int tf_poly_batch_evaluate_bfe(const uint64_t *coeffs, size_t n_coeffs, const uint64_t *points, size_t n_points, uint64_t *out);
int tf_poly_batch_evaluate_xfe(const uint64_t *coeffs, size_t n_coeffs, const uint64_t *points, size_t n_points, uint64_t *out);
int tf_poly_batch_evaluate_bfe_dev(const uint64_t *d_coeffs, size_t n_coeffs, const uint64_t *d_points, size_t n_points, uint64_t *d_out, void *stream);
int tf_poly_batch_evaluate_xfe_dev(const uint64_t *d_coeffs, size_t n_coeffs, const uint64_t *d_points, size_t n_points, uint64_t *d_out, void *stream);
/* Polynomial::zerofier / par_zerofier  math/polynomial.rs:1435-1485 (smart_zerofier :1462, fast_zerofier :1478): the monic
 * prod_i (x - roots[i]); out receives n_roots + 1 coefficients, low to high (out[n_roots] = 1; n_roots = 0 gives the constant 1).
 * Repeated roots are allowed.  On the device: the root of the zerofier tree of the batch evaluation above. */
int tf_poly_zerofier_bfe(const uint64_t *roots, size_t n_roots, uint64_t *out);
int tf_poly_zerofier_xfe(const uint64_t *roots, size_t n_roots, uint64_t *out);
int tf_poly_zerofier_bfe_dev(const uint64_t *d_roots, size_t n_roots, uint64_t *d_out, void *stream);
int tf_poly_zerofier_xfe_dev(const uint64_t *d_roots, size_t n_roots, uint64_t *d_out, void *stream);
/* Polynomial::interpolate / par_interpolate / lagrange_interpolate / fast_interpolate  math/polynomial.rs:1502-1701, and
 * batch_fast_interpolate :1703-1838 (`rows` value rows over one domain, the tree and the inverse weights shared as the reference
 * memoises them): out[row * n_points + j] = coefficient j of the unique polynomial of degree < n_points through
 * (domain[i], values[row * n_points + i]).  Always n_points coefficients per row: the reference trims leading zero coefficients
 * in Polynomial::new, the caller does that -- the length here is data independent.
 * Errors: n_points == 0 -> TF_ERR_EMPTY_DOMAIN (:1503-1506); a repeated domain point -> TF_ERR_INVERSE_OF_ZERO (the reference
 * panics dividing by zero: traits.rs:106 / b_field_element.rs:264-268).  The _dev calls synchronise the stream once (the
 * repeated-point check); tf_poly_interpolate_*_dev_async (below) report it through a device status word instead. */
int tf_poly_interpolate_bfe(const uint64_t *domain, const uint64_t *values, size_t n_points, size_t rows, uint64_t *out);
int tf_poly_interpolate_xfe(const uint64_t *domain, const uint64_t *values, size_t n_points, size_t rows, uint64_t *out);
int tf_poly_interpolate_bfe_dev(const uint64_t *d_domain, const uint64_t *d_values, size_t n_points, size_t rows, uint64_t *d_out, void *stream);
int tf_poly_interpolate_xfe_dev(const uint64_t *d_domain, const uint64_t *d_values, size_t n_points, size_t rows, uint64_t *d_out, void *stream);
/* fast_coset_evaluate / fast_coset_interpolate of XFieldElement polynomials with an XFieldElement OFFSET (S = XFieldElement in
 * math/polynomial.rs:1374-1378 and :1907-1911; offset = 3 raw words).  Same arguments, errors and layout as tf_coset_eval_xfe /
 * tf_coset_interpolate_xfe; a zero offset -> TF_ERR_INVERSE_OF_ZERO in the interpolation (x_field_element.rs:371-375).  The
 * scaling by offset^i is a separate device pass here (the reference's docs recommend a base-field offset, :1366-1368, which is
 * the fused fast path). */
int tf_coset_eval_xfe_xoffset(const uint64_t *coeffs, size_t n_coeffs, const uint64_t offset[3], uint64_t *out, size_t order, size_t batch);
int tf_coset_interpolate_xfe_xoffset(const uint64_t *values, size_t n, const uint64_t offset[3], uint64_t *out, size_t batch);
int tf_coset_eval_xfe_xoffset_dev(const uint64_t *d_coeffs, size_t n_coeffs, const uint64_t offset[3], uint64_t *d_out, size_t order, size_t batch, void *stream);
int tf_coset_interpolate_xfe_xoffset_dev(const uint64_t *d_values, size_t n, const uint64_t offset[3], uint64_t *d_out, size_t batch, void *stream);
/* Polynomial<BFieldElement>::evaluate::<XFieldElement, XFieldElement>  math/polynomial.rs:309-320 (the generic evaluate with the
 * indeterminate in the extension field), batched: `batch` base-field polynomials of n_coeffs packed coefficients at n_points
 * XFieldElement points (3 words each) -> out[(b * n_points + i) * 3].  Horner; the coefficients are read as 8-byte words, not
 * lifted. */
int tf_poly_evaluate_bfe_at_xfe(const uint64_t *coeffs, size_t n_coeffs, size_t batch, const uint64_t *points, size_t n_points, uint64_t *out);
int tf_poly_evaluate_bfe_at_xfe_dev(const uint64_t *d_coeffs, size_t n_coeffs, size_t batch, const uint64_t *d_points, size_t n_points, uint64_t *d_out, void *stream);
/* barycentric_evaluate  math/polynomial.rs:2609-2637: out[b] = the value at `indeterminate` of the interpolant of codeword b given
 * on the subgroup of order n (natural order, no offset), for `batch` codewords of n elements at ONE indeterminate -- the
 * out-of-domain evaluation of every column of a table.  indeterminate: 3 raw words (an XFieldElement; a BFieldElement x as
 * [x, 0, 0]); _bfe / _xfe is the codewords' field; out: batch x 3 words (an XFieldElement each; limbs 1 and 2 are zero when
 * codewords and indeterminate are in the base field, the reference's BFieldElement result being limb 0).  One pass over the
 * codewords (8 / 24 bytes per element) against the shared weights d_i / (x - d_i).
 * Errors where the reference panics: n not a power of two -> TF_ERR_LEN_NOT_POWER_OF_TWO (primitive_root_of_unity(..).unwrap(),
 * :2620); the indeterminate inside the subgroup, or n == 0 -> TF_ERR_INVERSE_OF_ZERO (batch_inversion / inverse of zero). */
int tf_barycentric_evaluate_bfe(const uint64_t *codewords, size_t n, size_t batch, const uint64_t indeterminate[3], uint64_t *out);
int tf_barycentric_evaluate_xfe(const uint64_t *codewords, size_t n, size_t batch, const uint64_t indeterminate[3], uint64_t *out);
/* (at most 131 069 codewords per call -- two rows per workgroup, the shared denominator being one more row, in 65 535 row groups:
 *  more -> TF_ERR_LEN_TOO_LARGE; split the batch) */
int tf_barycentric_evaluate_bfe_dev(const uint64_t *d_codewords, size_t n, size_t batch, const uint64_t indeterminate[3], uint64_t *d_out, void *stream);
int tf_barycentric_evaluate_xfe_dev(const uint64_t *d_codewords, size_t n, size_t batch, const uint64_t indeterminate[3], uint64_t *d_out, void *stream);
/* Polynomial::<BFieldElement>::clean_divide  math/polynomial.rs:2358-2411: the quotient a / b of a division KNOWN to be clean
 * (b | a), by pointwise division on a coset of the extension field: two forward XFE transforms of order
 * next_power_of_two(na), one inverse.  a, b: normalised coefficient arrays (na, nb count up to the non-zero leading coefficient,
 * as Polynomial::degree does); out receives na - nb + 1 coefficients.
 * Errors (where the reference panics): nb == 0 -> TF_ERR_DIVISION_BY_ZERO; the division is not clean (including
 * 0 < na < nb) -> TF_ERR_DIVISION_NOT_CLEAN (the reference: "might panic or produce a wrong result"; here it is always
 * detected).  na == 0 (zero dividend): TF_OK, nothing written.  The _dev call synchronises its stream once.
 * Where this differs from the reference: (1) the reference takes the coset route only for divisors of degree >= 512 and long
 * division below (:2360-2364); here every divisor takes the coset route.  A divisor with a root ON the coset x * <w_order>
 * (x^3 - x + 1 and its relatives y^3 - w^2i y + w^3i) cannot be inverted there: the blocking calls repeat the division once on
 * the coset (x + 1) * <w_order> (a clean quotient is the same on any coset) and only then report TF_ERR_INVERSE_OF_ZERO, the
 * code of the reference's batch_inversion panic; the _dev_async variant reports it after the first coset.  (2) 0 < na < nb is
 * TF_ERR_DIVISION_NOT_CLEAN, where a release build of the reference returns the zero quotient.  (3) An unclean division is
 * always detected. */
int tf_poly_clean_divide_bfe(const uint64_t *a, size_t na, const uint64_t *b, size_t nb, uint64_t *out);
int tf_poly_clean_divide_bfe_dev(const uint64_t *d_a, size_t na, const uint64_t *d_b, size_t nb, uint64_t *d_out, void *stream);
/* The same for `batch` dividends of na coefficients each (packed; na counts up to the longest dividend, shorter ones zero padded)
 * over ONE divisor -- a prover's quotients: many numerators over the same zerofier.  The divisor's transform is inverted once.
 * out: batch x (na - nb + 1) coefficients.  Any unclean row fails the call.  At most 65 535 dividends per call. */
int tf_poly_clean_divide_many_bfe(const uint64_t *a, size_t na, size_t batch, const uint64_t *b, size_t nb, uint64_t *out);
int tf_poly_clean_divide_many_bfe_dev(const uint64_t *d_a, size_t na, size_t batch, const uint64_t *d_b, size_t nb, uint64_t *d_out, void *stream);
/* Polynomial::divide / naive_divide (math/polynomial.rs:539-600), Div / Rem (:2502-2524), reduce / fast_reduce (:989-1048).
 * batch dividends of na coefficients each (packed; shorter ones zero padded) over ONE divisor of nb coefficients.
 * Words: raw Montgomery words as everywhere; an XFieldElement is 3 words per coefficient.
 * Divisor: normalised, b[nb-1] != 0 (clean_divide's contract).  nb == 0 -> TF_ERR_DIVISION_BY_ZERO (the reference's panic,
 *   :556-559); b[nb-1] == 0 -> TF_ERR_INVALID_ARGUMENT (the host form returns it, the _dev form writes it to *d_status).
 * Dividends need not be normalised: quotient and remainder are unique, trailing zeros only give zero coefficients at the top.
 * Outputs, fixed length and zero padded at the top (the reference's Polynomial trims those zeros; its equality ignores them):
 *   q: batch x max(na - nb + 1, 0) coefficients;  r: batch x (nb - 1) coefficients.
 *   na < nb: the quotient is empty and r is the dividend, zero padded (the reference's (zero, self), :560-563).
 *   nb == 1: q = a * lc^-1 and r is empty.
 *   q or r may be NULL and is then not written (r alone is `reduce`); both NULL -> TF_ERR_NULL_POINTER.
 * Limits: batch <= 65 535, na <= 2^30, nb <= 2^30; above them TF_ERR_LEN_TOO_LARGE.  Device work space: at most
 *   (batch + 6) x next_power_of_two(2k - 1) elements, k = na - nb + 1 (na = 2^24 over BFieldElement or 2^23 over XFieldElement:
 *   about 2 GiB / 5 GiB in one call); a failed allocation is TF_ERR_OUT_OF_MEMORY.
 * Construction (csrc/divide_kernels.h): h = rev(b)^-1 mod x^k by Newton doublings, every doubling with
 *   transforms of order <= 2^12 (BFieldElement) / 2^9 (XFieldElement: the order whose three limb lines run without register
 *   spills) in ONE launch, the larger ones on the library's transforms; rev(q) = (rev(a) mod x^k) h mod x^k with h's transform
 *   shared by the batch; the remainder as (a - q b) mod (x^N - 1), N = next_power_of_two(nb - 1), one cyclic product of order N.
 * _dev forms: device pointers; they never synchronise `stream`.  The data-dependent panic case (b[nb-1] == 0) goes to d_status
 *   (one int of device memory, first non-zero code wins, as the _dev_async calls below); d_status == NULL -> TF_ERR_NULL_POINTER.
 *   Everything checkable on the host (null pointers, nb == 0, sizes) is the return value, returned before any HIP call. */
int tf_poly_divide_bfe(const uint64_t *a, size_t na, size_t batch, const uint64_t *b, size_t nb, uint64_t *q, uint64_t *r);
int tf_poly_divide_xfe(const uint64_t *a, size_t na, size_t batch, const uint64_t *b, size_t nb, uint64_t *q, uint64_t *r);
int tf_poly_divide_bfe_dev(const uint64_t *d_a, size_t na, size_t batch, const uint64_t *d_b, size_t nb,
                           uint64_t *d_q, uint64_t *d_r, void *stream, int *d_status);
int tf_poly_divide_xfe_dev(const uint64_t *d_a, size_t na, size_t batch, const uint64_t *d_b, size_t nb,
                           uint64_t *d_q, uint64_t *d_r, void *stream, int *d_status);
/* Polynomial::formal_power_series_inverse_newton (math/polynomial.rs:1281-1366): exactly the reference's return value, the R-th
 * Newton iterate f_(i+1) = 2 f_i - f_i^2 g from f_0 = g(0)^-1, R = ilog2(next_power_of_two(precision)) (precision 0 counts as 1).
 * The iterate is NOT truncated to x^precision (neither is the reference's): out receives (2^R - 1) d + 1 coefficients, d = nf - 1,
 * or exactly one when d == 0 -- tf_poly_fps_inverse_newton_len(nf, precision) returns that count, or 0 when it exceeds 2^30 (or
 * nf == 0).  Errors: nf == 0 or f[0] == 0 -> TF_ERR_INVERSE_OF_ZERO (the reference panics by index or in inverse());
 * f[nf-1] == 0 -> TF_ERR_INVALID_ARGUMENT; a count above 2^30 -> TF_ERR_LEN_TOO_LARGE.  The _dev forms report the two
 * data-dependent cases through d_status as tf_poly_divide_*_dev does and never synchronise. */
int tf_poly_fps_inverse_newton_bfe(const uint64_t *f, size_t nf, size_t precision, uint64_t *out);
int tf_poly_fps_inverse_newton_xfe(const uint64_t *f, size_t nf, size_t precision, uint64_t *out);
int tf_poly_fps_inverse_newton_bfe_dev(const uint64_t *d_f, size_t nf, size_t precision, uint64_t *d_out, void *stream, int *d_status);
int tf_poly_fps_inverse_newton_xfe_dev(const uint64_t *d_f, size_t nf, size_t precision, uint64_t *d_out, void *stream, int *d_status);
size_t tf_poly_fps_inverse_newton_len(size_t nf, size_t precision);
/* ZerofierTree  math/zerofier_tree.rs (new_from_domain :66-87, zerofier :93-99) with Polynomial::divide_and_conquer_batch_evaluate
 * math/polynomial.rs:1882-1894: the tree of a domain built ONCE and kept in HBM (levels, the cached level transforms, the root,
 * the domain, and after the first interpolation the inverse weights), for callers that evaluate or interpolate on the same
 * points many times -- the build is 1.4 walks, and an interpolation over a prepared tree is one walk up.  A handle belongs to the
 * device that was current when it was made; every call brings its own stream-ordered work space, so one handle serves concurrent
 * calls on different streams.  An empty domain gives the empty tree (zerofier 1, no values; :136-138).
 * tf_zerofier_tree_new_*: domain of n points (host pointer; _dev: device pointer, the call synchronises `stream` before returning).
 * tf_zerofier_tree_zerofier*: n + 1 coefficients.   tf_zerofier_tree_batch_evaluate*: `batch` polynomials of n_coeffs packed
 * coefficients -> out[(b * n + i) * width] = f_b(domain[i]).   tf_zerofier_tree_interpolate*: `rows` value rows -> rows * n
 * coefficients (errors as tf_poly_interpolate_*; the first call computes the weights and synchronises its stream once). */
typedef struct tf_zerofier_tree tf_zerofier_tree;
int tf_zerofier_tree_new_bfe(const uint64_t *domain, size_t n_points, tf_zerofier_tree **tree);
int tf_zerofier_tree_new_xfe(const uint64_t *domain, size_t n_points, tf_zerofier_tree **tree);
int tf_zerofier_tree_new_bfe_dev(const uint64_t *d_domain, size_t n_points, void *stream, tf_zerofier_tree **tree);
int tf_zerofier_tree_new_xfe_dev(const uint64_t *d_domain, size_t n_points, void *stream, tf_zerofier_tree **tree);
void tf_zerofier_tree_free(tf_zerofier_tree *tree);
size_t tf_zerofier_tree_num_points(const tf_zerofier_tree *tree);
int tf_zerofier_tree_width(const tf_zerofier_tree *tree);   /* 1 = BFieldElement, 3 = XFieldElement */
int tf_zerofier_tree_zerofier(const tf_zerofier_tree *tree, uint64_t *out);
int tf_zerofier_tree_batch_evaluate(const tf_zerofier_tree *tree, const uint64_t *coeffs, size_t n_coeffs, size_t batch, uint64_t *out);
int tf_zerofier_tree_interpolate(tf_zerofier_tree *tree, const uint64_t *values, size_t rows, uint64_t *out);
int tf_zerofier_tree_zerofier_dev(const tf_zerofier_tree *tree, uint64_t *d_out, void *stream);
int tf_zerofier_tree_batch_evaluate_dev(const tf_zerofier_tree *tree, const uint64_t *d_coeffs, size_t n_coeffs, size_t batch, uint64_t *d_out, void *stream);
int tf_zerofier_tree_interpolate_dev(tf_zerofier_tree *tree, const uint64_t *d_values, size_t rows, uint64_t *d_out, void *stream);
/* ---- enqueue-and-return variants of the three _dev entry points above that otherwise synchronise their stream ------------------
 * The reference PANICS on a repeated interpolation point (traits.rs:106), on a divisor with a root on the division coset and on
 * an unclean division (polynomial.rs:2374, :2410).  The plain _dev calls detect these by copying a flag back, i.e. they block the
 * host once; the _async variants never synchronise: they take `d_status`, ONE int in device memory owned by the caller (zero it
 * before the first call of a chain), and a panic case writes its tf_status code there -- the first non-zero code written wins, so
 * one word can serve a whole chain of calls; the output of a call that reported an error is unspecified.  Everything that can be
 * checked on the host (null pointers, lengths, an empty domain, a zero divisor length) is still the return value.
 * tf_zerofier_tree_new_*_dev_async returns the handle without waiting for the build: until the caller has synchronised (or
 * ordered its other streams behind `stream` with an event) the handle may only be used on `stream`; the same holds for the
 * inverse weights the first tf_zerofier_tree_interpolate_dev_async computes.  A handle whose weights met a repeated point keeps
 * reporting TF_ERR_INVERSE_OF_ZERO through d_status on every later asynchronous interpolation. */
int tf_poly_interpolate_bfe_dev_async(const uint64_t *d_domain, const uint64_t *d_values, size_t n_points, size_t rows, uint64_t *d_out, void *stream, int *d_status);
int tf_poly_interpolate_xfe_dev_async(const uint64_t *d_domain, const uint64_t *d_values, size_t n_points, size_t rows, uint64_t *d_out, void *stream, int *d_status);
int tf_poly_clean_divide_bfe_dev_async(const uint64_t *d_a, size_t na, const uint64_t *d_b, size_t nb, uint64_t *d_out, void *stream, int *d_status);
int tf_poly_clean_divide_many_bfe_dev_async(const uint64_t *d_a, size_t na, size_t batch, const uint64_t *d_b, size_t nb, uint64_t *d_out, void *stream, int *d_status);
int tf_zerofier_tree_new_bfe_dev_async(const uint64_t *d_domain, size_t n_points, void *stream, tf_zerofier_tree **tree);
int tf_zerofier_tree_new_xfe_dev_async(const uint64_t *d_domain, size_t n_points, void *stream, tf_zerofier_tree **tree);
int tf_zerofier_tree_interpolate_dev_async(tf_zerofier_tree *tree, const uint64_t *d_values, size_t rows, uint64_t *d_out, void *stream, int *d_status);
/* The route tf_poly_batch_evaluate_* takes for a shape: 1 = Horner, 2 = zerofier tree (0: width not 1 / 3).  Pure host logic (the
 * fitted cost model of the router), checked by the CPU tests; honours tf_set_batch_eval_route / TF_BATCH_EVAL. */
int tf_batch_eval_plan(size_t n_coeffs, size_t n_points, size_t batch, int width);
/* Route of the batch evaluation (test / A-B hook): 0 = automatic (zerofier tree for many points on a long polynomial, Horner
 * otherwise), 1 = always Horner, 2 = the zerofier tree whenever it applies (at least two leaves: 512 points over BFE, 256 over XFE).  Same values either way. */
void tf_set_batch_eval_route(int route);
/* Polynomial::coset_extrapolate :2117-2128 / batch_coset_extrapolate :2196-2208 (and the par_ variant :2262): for each of
 * `batch` codewords of length n (a power of two, else TF_ERR_LEN_NOT_POWER_OF_TWO) given on {offset * w_n^i}, the values of
 * its interpolant at `points` (same field as the codeword): out[(b * n_points + i) * width]. */
int tf_coset_extrapolate_bfe(uint64_t offset_raw, const uint64_t *codewords, size_t n, size_t batch, const uint64_t *points, size_t n_points, uint64_t *out);
int tf_coset_extrapolate_xfe(uint64_t offset_raw, const uint64_t *codewords, size_t n, size_t batch, const uint64_t *points, size_t n_points, uint64_t *out);
int tf_coset_extrapolate_bfe_dev(uint64_t offset_raw, const uint64_t *d_codewords, size_t n, size_t batch, const uint64_t *d_points, size_t n_points, uint64_t *d_out, void *stream);
int tf_coset_extrapolate_xfe_dev(uint64_t offset_raw, const uint64_t *d_codewords, size_t n, size_t batch, const uint64_t *d_points, size_t n_points, uint64_t *d_out, void *stream);
/* Rows of a COLUMN-major table (the layout a batch of coset evaluations leaves behind: one codeword per column).
 * table: `batch` tables of n_cols columns; column j = n_rows elements of `width` words (1 = BFieldElement, 3 = XFieldElement
 * flattened as math/x_field_element.rs:217-231) at table + j * col_stride (col_stride >= n_rows * width, in words; tables are
 * n_cols * col_stride words apart).  Row i = the concatenation over the columns of element i.
 *   tf_tip5_hash_table_rows : digests[(t * n_rows + i) * 5 ..] = Tip5::hash_varlen(row i of table t)   tip5/mod.rs:617-623
 *   tf_merkle_from_columns  : those digests as the leaves of one tree per table (nodes: batch x 2 n_rows digests), errors as
 *                             tf_merkle_build. */
int tf_tip5_hash_table_rows(const uint64_t *table, size_t n_rows, size_t n_cols, int width, size_t col_stride, uint64_t *digests, size_t batch);
int tf_tip5_hash_table_rows_dev(const uint64_t *d_table, size_t n_rows, size_t n_cols, int width, size_t col_stride, uint64_t *d_digests, size_t batch, void *stream);
int tf_merkle_from_columns(const uint64_t *table, size_t n_rows, size_t n_cols, int width, size_t col_stride, uint64_t *nodes_out, size_t batch);
int tf_merkle_from_columns_dev(const uint64_t *d_table, size_t n_rows, size_t n_cols, int width, size_t col_stride, uint64_t *d_nodes_out, size_t batch, void *stream);
int tf_merkle_from_rows(const uint64_t *rows, size_t row_len, size_t n_rows, uint64_t *nodes_out, size_t batch);
int tf_merkle_from_rows_dev(const uint64_t *d_rows, size_t row_len, size_t n_rows, uint64_t *d_nodes_out, size_t batch, void *stream);
/* *out_count always receives the full count.  out_indices == NULL or capacity == 0 is the sizing call (returns TF_OK);
 * otherwise capacity < count -> TF_ERR_BUFFER_TOO_SMALL and nothing is written (same rule as the _dev sibling below). */
int tf_merkle_auth_structure_indices(size_t num_leafs, const uint64_t *leaf_indices, size_t k, uint64_t *out_indices, size_t capacity, size_t *out_count);
int tf_merkle_authentication_structure_dev(const uint64_t *d_nodes, size_t num_leafs, const uint64_t *leaf_indices, size_t k,
                                           uint64_t *out_digests, size_t capacity_digests, size_t *out_count, void *stream);
/* MerkleTree::sequential_authentication_structure_from_leafs / par_authentication_structure_from_leafs   util_types/merkle_tree.rs:506-542
 * The authentication structure AND the root of `batch` trees from their leafs alone: commit and open in one call, without the node
 * array of 2 n digests per tree that tf_merkle_authentication_structure_dev reads (the companion of tf_merkle_root).
 * leafs: batch x num_leafs digests, as for tf_merkle_build.  ONE list of leaf indices opens every tree of the batch (a prover's query
 * indices on its main, auxiliary and quotient trees).  *out_count: structure nodes per tree, what tf_merkle_auth_structure_indices
 * reports for the same indices.  out_digests: tree-major, batch x count digests; within a tree in the reference's order (descending
 * node index, :502-503), each the digest nodes[i] of the full tree.  roots: NULL, or batch x 5 words (the values of tf_merkle_root).
 * k == 0, every leaf opened, and num_leafs == 1 all give count 0: roots only.
 * Sizing as the pair above: *out_count is always written; out_digests == NULL or capacity_digests == 0 is the sizing call (TF_OK,
 * nothing else written, roots included); capacity_digests (digests PER TREE) < count -> TF_ERR_BUFFER_TOO_SMALL, nothing written.
 * Errors, before any device is touched and in this order: TF_ERR_TOO_FEW_LEAFS (num_leafs == 0), TF_ERR_INCORRECT_NUMBER_OF_LEAFS
 * (not a power of two), TF_ERR_TREE_TOO_HIGH (more than 2^31 leafs), TF_ERR_LEAF_INDEX_INVALID (an index >= num_leafs),
 * TF_ERR_NULL_POINTER (leafs; leaf_indices with k > 0; out_count).  batch == 0: TF_OK with *out_count set.
 * _dev: leaf_indices is a HOST array (*out_count is host arithmetic, valid on return); leafs, digests and roots are device memory.
 * Nothing is copied back and `stream` is not synchronised.  Work space comes from the library's stream-ordered pool and goes back
 * on `stream`: tf_merkle_auth_structure_from_leafs_workspace is the number of bytes the call requests for k_nodes structure nodes per
 * tree (pure host arithmetic; 0 for arguments the call rejects).  It never shrinks as batch grows and is at most
 *   batch * (3 num_leafs / 4) + 2^15 + 128 batch   digests of 40 bytes, plus 8 bytes per structure node,
 * and never more than 2 num_leafs batch digests plus those 8 bytes per node (trees of up to 2^14 / batch leafs are built whole). */
int tf_merkle_auth_structure_from_leafs(const uint64_t *leafs, size_t num_leafs, size_t batch, const uint64_t *leaf_indices, size_t k,
                                        uint64_t *out_digests, size_t capacity_digests, size_t *out_count, uint64_t *roots);
int tf_merkle_auth_structure_from_leafs_dev(const uint64_t *d_leafs, size_t num_leafs, size_t batch, const uint64_t *leaf_indices, size_t k,
                                            uint64_t *d_out_digests, size_t capacity_digests, size_t *out_count, uint64_t *d_roots, void *stream);
size_t tf_merkle_auth_structure_from_leafs_workspace(size_t num_leafs, size_t batch, size_t k_nodes);
/* The same openings with the leaf indices in DEVICE memory: n_lists independent lists of k u32 each, list l at d_leaf_indices + l * k,
 * the layout tf_tip5_sponge_sample_indices_dev writes; all lists open trees of num_leafs leafs.  MerkleTree::
 * authentication_structure_node_indices (util_types/merkle_tree.rs:449-504) is computed by a kernel where the indices lie: the calls
 * only enqueue on `stream`, read nothing back and never synchronise.  k <= 8192 per list (index lists as long as the tree is wide
 * keep the host-index calls above).
 *   tf_merkle_auth_structure_max_nodes   sum over the levels l below the root of min(k, (num_leafs >> l) / 2): no list of k indices
 *       has more structure nodes, so it is what `capacity` is sized with -- the true count is device data.  An upper bound only:
 *       k = 1 attains it, two or more paths share nodes near the root and stay below it.  Pure host arithmetic; 0 for arguments the calls reject.
 *   tf_merkle_auth_structure_indices_dev   the plan alone: list l writes its node indices (the reference's order, descending) to
 *       d_node_indices + l * capacity, their number to d_counts[l] and, when d_level_ends is given, 32 run ends to
 *       d_level_ends + 32 * l: entry j = the structure nodes on the levels of n, n / 2, ..., n >> j nodes (descending order puts the
 *       leaf level first, so every level is one run); entries for levels at or above the root repeat the count.
 *   tf_merkle_authentication_structure_sampled_dev   the gather from node arrays: n_lists * trees_per_list trees of 2 num_leafs digests
 *       each, as tf_merkle_build leaves them; tree t is opened at list t / trees_per_list (a prover's main, auxiliary and quotient trees
 *       under one transcript, many transcripts at once).  d_out_digests is tree-major, `capacity` digests per tree: the first
 *       d_counts[list] are the structure, the words behind them stay as they were.
 *   tf_merkle_auth_structure_from_leafs_sampled_dev   commit and open: the sweep of tf_merkle_auth_structure_from_leafs_dev over the
 *       n_lists * trees_per_list trees of d_leafs, same output layout; d_roots is NULL or receives one root per tree, whatever the
 *       status.  tf_merkle_auth_structure_from_leafs_sampled_workspace is what the call requests from the pool for `trees` trees in
 *       all: the request of the host-index form plus the plan (4 bytes per node of the bound and 128 bytes per list); never shrinks
 *       as `trees` grows; 0 for arguments the call rejects.
 * The return value is what the host can decide, before any device is touched and in this order: TF_ERR_TOO_FEW_LEAFS,
 * TF_ERR_INCORRECT_NUMBER_OF_LEAFS, TF_ERR_TREE_TOO_HIGH (more than 2^31 leafs), TF_ERR_LEN_TOO_LARGE (k > 8192; 2^31 lists or more;
 * more than 2^31 trees), TF_ERR_NULL_POINTER (d_status, always; with n_lists > 0: d_leaf_indices with k > 0, d_counts; the trees and,
 * with capacity > 0, the output).  n_lists == 0 or trees_per_list == 0: TF_OK, nothing is enqueued.
 * What depends on the indices goes to *d_status, one caller-owned int in device memory that keeps the first non-zero code (as
 * tf_table_gather_rows_dev):
 *   a list with an index >= num_leafs stores TF_ERR_LEAF_INDEX_INVALID and gets d_counts[l] = 0;
 *   a list with more than `capacity` nodes stores TF_ERR_BUFFER_TOO_SMALL and gets its full count in d_counts[l] (the plan alone has
 *   then written the first `capacity` node indices);
 * neither writes a digest for its trees, and the other lists of the call are unaffected.  k == 0, every leaf opened, and
 * num_leafs == 1 all give count 0. */
size_t tf_merkle_auth_structure_max_nodes(size_t num_leafs, size_t k);
int tf_merkle_auth_structure_indices_dev(size_t num_leafs, const uint32_t *d_leaf_indices, size_t k, size_t n_lists, uint32_t *d_node_indices,
                                         size_t capacity, uint32_t *d_counts, uint32_t *d_level_ends, void *stream, int *d_status);
int tf_merkle_authentication_structure_sampled_dev(const uint64_t *d_nodes, size_t num_leafs, const uint32_t *d_leaf_indices, size_t k,
                                                   size_t n_lists, size_t trees_per_list, uint64_t *d_out_digests, size_t capacity,
                                                   uint32_t *d_counts, void *stream, int *d_status);
int tf_merkle_auth_structure_from_leafs_sampled_dev(const uint64_t *d_leafs, size_t num_leafs, const uint32_t *d_leaf_indices, size_t k,
                                                    size_t n_lists, size_t trees_per_list, uint64_t *d_out_digests, size_t capacity,
                                                    uint32_t *d_counts, uint64_t *d_roots, void *stream, int *d_status);
size_t tf_merkle_auth_structure_from_leafs_sampled_workspace(size_t num_leafs, size_t trees, size_t k, size_t n_lists);

/* ---------------------------------------------------------------------------------------------
 * Inclusion proofs, batched.   replaces  MerkleTreeInclusionProof::try_verify / verify   util_types/merkle_tree.rs:727-748
 *                                        MerkleTreeInclusionProof::into_authentication_paths :773-777 (PartialMerkleTree :779-931)
 * A proof is (tree_height, indexed_leafs, authentication_structure), in CSR layout over n_proofs proofs:
 *   proof p owns the leafs leaf_offsets[p] .. leaf_offsets[p + 1] - 1 (leaf_indices: one word each; leaf_digests: 5 words each, at
 *   5 * index) and the structure digests auth_offsets[p] .. auth_offsets[p + 1] - 1 (auth_digests: 5 words each); both offset arrays
 *   have n_proofs + 1 entries and never decrease.  expected_roots: 5 words per proof.
 * statuses[p] receives the reference's verdict for proof p: TF_OK, TF_ERR_TREE_TOO_HIGH (height >= 64), TF_ERR_LEAF_INDEX_INVALID,
 * TF_ERR_AUTH_STRUCTURE_LENGTH_MISMATCH, TF_ERR_REPEATED_LEAF_DIGEST_MISMATCH or (verify only) TF_ERR_ROOT_MISMATCH, decided in the
 * reference's order.  A proof with neither leafs nor structure verifies whatever its height and root (:737-739); the paths call has
 * no such shortcut (:773-777).
 * paths_out: proof after proof, each k_p x h_p digests, leaf-major in the order of indexed_leafs, duplicates included (entry e, level
 * l = the sibling of leaf e's ancestor at height l, bottom first); proof p starts at digest sum_(q < p, h_q < 64) k_q * h_q.  The
 * slot of a proof whose status is not TF_OK holds unspecified words.
 * The return value concerns the call alone: TF_ERR_NULL_POINTER, TF_ERR_INVALID_ARGUMENT (decreasing offsets), TF_ERR_NO_DEVICE,
 * TF_ERR_OUT_OF_MEMORY (device work space: proofs of more than 256 leafs keep their levels in device memory, about 200 bytes per leaf).
 * _dev: tree_heights and the offsets are HOST arrays (the host reads them, O(n_proofs) work); leaf indices, digests, roots, paths and
 * statuses are device memory.  Nothing is copied back and `stream` is not synchronised: d_statuses is valid once the stream has
 * reached the call. */
int tf_merkle_verify_proofs(const uint32_t *tree_heights, size_t n_proofs, const uint64_t *leaf_offsets, const uint64_t *leaf_indices,
                            const uint64_t *leaf_digests, const uint64_t *auth_offsets, const uint64_t *auth_digests,
                            const uint64_t *expected_roots, int *statuses);
int tf_merkle_verify_proofs_dev(const uint32_t *tree_heights, size_t n_proofs, const uint64_t *leaf_offsets, const uint64_t *d_leaf_indices,
                                const uint64_t *d_leaf_digests, const uint64_t *auth_offsets, const uint64_t *d_auth_digests,
                                const uint64_t *d_expected_roots, int *d_statuses, void *stream);
int tf_merkle_authentication_paths(const uint32_t *tree_heights, size_t n_proofs, const uint64_t *leaf_offsets, const uint64_t *leaf_indices,
                                   const uint64_t *leaf_digests, const uint64_t *auth_offsets, const uint64_t *auth_digests,
                                   uint64_t *paths_out, int *statuses);
int tf_merkle_authentication_paths_dev(const uint32_t *tree_heights, size_t n_proofs, const uint64_t *leaf_offsets,
                                       const uint64_t *d_leaf_indices, const uint64_t *d_leaf_digests, const uint64_t *auth_offsets,
                                       const uint64_t *d_auth_digests, uint64_t *d_paths_out, int *d_statuses, void *stream);

/* ---- Merkle Mountain Range accumulators (util_types/mmr/; mmr.rs, mmr_accumulator.rs, mmr_membership_proof.rs, shared_basic.rs)
 * (and mmr_successor_proof.rs)
 * A digest is 5 raw Montgomery words; a list of peaks runs from the highest to the lowest, popcount(leaf_count) digests.  Every
 * call returns TF_ERR_INVALID_ARGUMENT for a leaf count above 2^63 (the limit of mmr.rs:12-13), before the device is touched; so
 * do the other argument errors named below.  The host forms take host pointers and return when the results are in place; the
 * _dev forms take device pointers for the digests (and statuses / flags), enqueue on `stream`, never synchronise and copy nothing
 * back.  Counts, leaf indices of a mutation and every offset array stay on the host: the planner reads them.
 *
 * tf_mmr_append: k successive MmrAccumulator::append calls (mmr_accumulator.rs:149-159, calculate_new_peaks_from_append
 *   shared_basic.rs:75-105) on the accumulator (leaf_count, old_peaks): new_peaks receives the popcount(leaf_count + k) peaks (it
 *   must not overlap old_peaks); proofs, if not NULL, the membership proof each append returns, concatenated: proof i has
 *   trailing_ones(leaf_count + i) digests.  leaf_count = 0 is MmrAccumulator::new_from_leafs (:29-115).
 *   Errors: leaf_count + k > 2^63 -> TF_ERR_INVALID_ARGUMENT; NULL new_peaks / new_leafs (k > 0) / old_peaks (leaf_count > 0)
 *   -> TF_ERR_NULL_POINTER. */
int tf_mmr_append(uint64_t leaf_count, const uint64_t *old_peaks, const uint64_t *new_leafs, size_t k, uint64_t *new_peaks, uint64_t *proofs);
int tf_mmr_append_dev(uint64_t leaf_count, const uint64_t *d_old_peaks, const uint64_t *d_new_leafs, size_t k, uint64_t *d_new_peaks,
                      uint64_t *d_proofs, void *stream);
/* tf_mmr_bag_peaks: bag_peaks (mmr_accumulator.rs:379-391) of n_acc accumulators: accumulator a has leaf_counts[a] leafs and its
 *   popcount(leaf_counts[a]) peaks follow those of accumulator a - 1 in peaks; out receives one digest per accumulator. */
int tf_mmr_bag_peaks(const uint64_t *leaf_counts, size_t n_acc, const uint64_t *peaks, uint64_t *out);
int tf_mmr_bag_peaks_dev(const uint64_t *leaf_counts, size_t n_acc, const uint64_t *d_peaks, uint64_t *d_out, void *stream);
/* tf_mmr_verify_membership_proofs: MmrMembershipProof::verify (mmr_membership_proof.rs:36-77) of n_proofs proofs against one
 *   accumulator (leaf_count, the n_peaks digests of peaks).  Proof p: leaf index leaf_indices[p], leaf digest leaf_digests + 5 p,
 *   path digests [path_offsets[p], path_offsets[p + 1]) of paths.  statuses[p] = 0 where verify returns true, else the first reason
 *   it returns false: TF_ERR_MMR_LEAF_INDEX_OUT_OF_RANGE / _PEAK_COUNT_MISMATCH / _AUTH_PATH_LENGTH_MISMATCH / _PEAK_MISMATCH.
 *   Errors: decreasing path_offsets -> TF_ERR_INVALID_ARGUMENT. */
int tf_mmr_verify_membership_proofs(uint64_t leaf_count, const uint64_t *peaks, size_t n_peaks, size_t n_proofs, const uint64_t *leaf_indices,
                                    const uint64_t *leaf_digests, const uint64_t *path_offsets, const uint64_t *paths, int *statuses);
int tf_mmr_verify_membership_proofs_dev(uint64_t leaf_count, const uint64_t *d_peaks, size_t n_peaks, size_t n_proofs,
                                        const uint64_t *d_leaf_indices, const uint64_t *d_leaf_digests, const uint64_t *path_offsets,
                                        const uint64_t *d_paths, int *d_statuses, void *stream);
/* tf_mmr_batch_mutate_leafs: MmrAccumulator::batch_mutate_leaf_and_update_mps (mmr_accumulator.rs:180-302).  Mutation m sets leaf
 *   mut_indices[m] to new_leafs + 5 m, with the path [mut_offsets[m], mut_offsets[m + 1]) of mut_paths.  Own proof p (leaf
 *   own_indices[p], path [own_offsets[p], own_offsets[p + 1]) of own_paths) is updated in place and modified[p] = 1 where a digest
 *   was replaced, else 0.  peaks (popcount(leaf_count) digests) is updated in place; with peaks = NULL the call is
 *   MmrMembershipProof::batch_update_from_batch_leaf_mutation (mmr_membership_proof.rs:523-626).  The result is the reference's for
 *   every input it does not panic on, consistent or not.
 *   Errors: a repeated mutation index -> TF_ERR_INVALID_ARGUMENT (the reference panics); decreasing offsets ->
 *   TF_ERR_INVALID_ARGUMENT.  Two divergences from the reference: (1) a mutation or own index >= leaf_count ->
 *   TF_ERR_LEAF_INDEX_INVALID also with peaks = NULL, where the reference checks no index, so pass the MMR's leaf count in both
 *   modes; (2) a mutation path of more than 63 digests -> TF_ERR_INVALID_ARGUMENT in both modes (no node of an MMR of at most 2^63
 *   leafs is that high; the reference's u64 node index arithmetic overflows there, and batch_update_from_batch_leaf_mutation, which
 *   skips the last step, would otherwise accept a path of 64). */
int tf_mmr_batch_mutate_leafs(uint64_t leaf_count, uint64_t *peaks, size_t n_mut, const uint64_t *mut_indices, const uint64_t *new_leafs,
                              const uint64_t *mut_offsets, const uint64_t *mut_paths, size_t n_own, const uint64_t *own_indices,
                              const uint64_t *own_offsets, uint64_t *own_paths, int *modified);
int tf_mmr_batch_mutate_leafs_dev(uint64_t leaf_count, uint64_t *d_peaks, size_t n_mut, const uint64_t *mut_indices, const uint64_t *d_new_leafs,
                                  const uint64_t *mut_offsets, const uint64_t *d_mut_paths, size_t n_own, const uint64_t *own_indices,
                                  const uint64_t *own_offsets, uint64_t *d_own_paths, int *d_modified, void *stream);
/* tf_mmr_successor_proof_new: MmrSuccessorProof::new_from_batch_append (mmr_successor_proof.rs:34-91) for the accumulator
 *   (leaf_count, old_peaks) and k new leafs.  paths_out receives tf_mmr_successor_proof_len(leaf_count, k) digests (host arithmetic:
 *   0 where leaf_count = 0 or k < 2^trailing_zeros(leaf_count), and for arguments the calls reject); it may be NULL when that is 0.
 *   new_peaks is NULL or receives the popcount(leaf_count + k) peaks tf_mmr_append writes: proof and peaks come from ONE level
 *   sweep over the new leafs, not from one tree per proof digest.  The proof's digests are roots of new leafs alone, so old_peaks
 *   is read only when new_peaks is given and leaf_count > 0.
 *   Errors: leaf_count + k > 2^63 -> TF_ERR_INVALID_ARGUMENT; a NULL pointer where one is needed -> TF_ERR_NULL_POINTER. */
size_t tf_mmr_successor_proof_len(uint64_t leaf_count, uint64_t k);
int tf_mmr_successor_proof_new(uint64_t leaf_count, const uint64_t *old_peaks, const uint64_t *new_leafs, size_t k, uint64_t *paths_out,
                               uint64_t *new_peaks);
int tf_mmr_successor_proof_new_dev(uint64_t leaf_count, const uint64_t *d_old_peaks, const uint64_t *d_new_leafs, size_t k, uint64_t *d_paths_out,
                                   uint64_t *d_new_peaks, void *stream);
/* tf_mmr_verify_successor_proofs: MmrSuccessorProof::verify (:94-223) of n_proofs independent (old accumulator, new accumulator,
 *   proof) triples in CSR layout: triple p has old_leaf_counts[p] / new_leaf_counts[p] leafs, the old peaks [old_peak_offsets[p],
 *   old_peak_offsets[p + 1]) of old_peaks, the new peaks [new_peak_offsets[p], ..) of new_peaks and the proof digests
 *   [path_offsets[p], ..) of paths; the three offset arrays have n_proofs + 1 entries, count digests and never decrease.  The peak
 *   counts are those of the offsets, so an inconsistent accumulator can be stated.  statuses[p] = 0 where verify returns true, else
 *   the first error of verify_internal: TF_ERR_MMR_INCONSISTENT_OLD, _INCONSISTENT_NEW; for an empty old accumulator a proof that is
 *   not empty -> _SUCCESSOR_PATH_TOO_LONG; for equal counts unequal peaks -> _DIFFERENT_SHARED_PEAK, then the same length check;
 *   _OLD_HAS_MORE_LEAFS; else the shared peaks (_DIFFERENT_SHARED_PEAK), then the proof's length (_SUCCESSOR_PATH_TOO_SHORT /
 *   _TOO_LONG, also where the new leafs do not reach the lowest old peak and the proof is not empty), then the hash chain against
 *   the first unshared new peak (_DIFFERENT_UNSHARED_PEAK).  MissingOldPeak / MissingNewPeak cannot occur past the first two.
 *   Errors of the call: a count above 2^63 or decreasing offsets -> TF_ERR_INVALID_ARGUMENT.  n_proofs = 0 returns TF_OK. */
int tf_mmr_verify_successor_proofs(size_t n_proofs, const uint64_t *old_leaf_counts, const uint64_t *new_leaf_counts, const uint64_t *old_peak_offsets,
                                   const uint64_t *old_peaks, const uint64_t *new_peak_offsets, const uint64_t *new_peaks, const uint64_t *path_offsets,
                                   const uint64_t *paths, int *statuses);
int tf_mmr_verify_successor_proofs_dev(size_t n_proofs, const uint64_t *old_leaf_counts, const uint64_t *new_leaf_counts,
                                       const uint64_t *old_peak_offsets, const uint64_t *d_old_peaks, const uint64_t *new_peak_offsets,
                                       const uint64_t *d_new_peaks, const uint64_t *path_offsets, const uint64_t *d_paths, int *d_statuses,
                                       void *stream);
/* tf_mmr_update_proofs_from_append: k rounds of MmrMembershipProof::batch_update_from_append (mmr_membership_proof.rs:224-331) and
 *   append, for n_own membership proofs of the accumulator (leaf_count, old_peaks): own proof p belongs to leaf own_indices[p]
 *   (repeats allowed) and has the digests [own_offsets[p], own_offsets[p + 1]) of own_paths.  The updated proof p, valid in the
 *   accumulator of leaf_count + k leafs, is written to the digests [out_offsets[p], out_offsets[p + 1]) of out_paths: the old path,
 *   then the digests the appends add.  out_offsets (n_own + 1 entries, out_offsets[0] = 0) and modified (NULL, or n_own flags: 1
 *   where the path grew, the union of the indices the k reference calls return) are HOST arrays in both forms, pure arithmetic and
 *   written by every call that passes the argument checks.  With out_paths = NULL or capacity_digests = 0 and a result that is not
 *   empty the call only sizes; capacity_digests < out_offsets[n_own] -> TF_ERR_BUFFER_TOO_SMALL and out_paths is untouched.
 *   out_paths must not overlap own_paths.  new_peaks is NULL or as in tf_mmr_successor_proof_new.  old_peaks and new_leafs are read
 *   where a proof grows or new_peaks is given.
 *   Errors, before a device is touched: leaf_count + k > 2^63 -> TF_ERR_INVALID_ARGUMENT; an own index >= leaf_count ->
 *   TF_ERR_LEAF_INDEX_INVALID; an own path whose length is not bit_length(index ^ leaf_count) - 1, the height of the leaf's peak ->
 *   TF_ERR_MMR_AUTH_PATH_LENGTH_MISMATCH; decreasing own_offsets -> TF_ERR_INVALID_ARGUMENT.  The length error is a divergence: the
 *   reference takes the path's length for the peak's height, and on such input panics or writes a proof that cannot verify. */
int tf_mmr_update_proofs_from_append(uint64_t leaf_count, const uint64_t *old_peaks, const uint64_t *new_leafs, size_t k, size_t n_own,
                                     const uint64_t *own_indices, const uint64_t *own_offsets, const uint64_t *own_paths, uint64_t *out_offsets,
                                     uint64_t *out_paths, size_t capacity_digests, int *modified, uint64_t *new_peaks);
int tf_mmr_update_proofs_from_append_dev(uint64_t leaf_count, const uint64_t *d_old_peaks, const uint64_t *d_new_leafs, size_t k, size_t n_own,
                                         const uint64_t *own_indices, const uint64_t *own_offsets, const uint64_t *d_own_paths,
                                         uint64_t *out_offsets, uint64_t *d_out_paths, size_t capacity_digests, int *modified,
                                         uint64_t *d_new_peaks, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Tip5 sponges.     replaces  Tip5::new(Domain)              tip5/mod.rs:511-526
 *                             Sponge::absorb / squeeze       :684-698   (overwrite-mode absorb; squeeze = the rate words, THEN the permutation)
 *                             Sponge::pad_and_absorb_all     util_types/sponge.rs:41-55
 *                             Tip5::sample_indices / sample_scalars   tip5/mod.rs:636-674
 * A batch of `count` independent sponges is count x 16 raw Montgomery words (the layout of tf_tip5_permute).  Every call advances all
 * of them and is ONE kernel launch (plus, for a ragged absorb, the upload of its offsets); every result is word for word that of the
 * reference function applied to each sponge on its own.  The `_dev` forms take device pointers and enqueue on `stream` without
 * waiting for it: states, rows and roots that are already in device memory are absorbed where they lie.
 *   init               all words 0 (fixed_length == 0, Domain::VariableLength) or words 10..15 = ONE (Domain::FixedLength).
 *   absorb             n_chunks successive absorb calls per sponge; input: count x n_chunks x 10 words.
 *   pad_and_absorb_all offsets == NULL: sponge i absorbs the `len` words at input + i len.  Otherwise offsets is a HOST array (in the
 *                      _dev form too) of count + 1 non-decreasing word offsets, sponge i absorbs input[offsets[i] .. offsets[i + 1]) and
 *                      len is ignored; the offsets reach the device through pinned staging, the stream is not waited for.  A length
 *                      of 0 is legal (one padding block).
 *   squeeze            n_squeezes successive squeeze calls per sponge; out: count x n_squeezes x 10 words.
 *   sample_scalars     ceil(3 num_elements / 10) squeezes; element e is words 3 e .. 3 e + 2 of their concatenation ([c0, c1, c2],
 *                      XFieldElement::new), the unused tail of the last squeeze is dropped; out: count x num_elements x 3 words.
 *   sample_indices     squeeze whenever the ten-element buffer is used up; an element equal to BFieldElement::MAX (p - 1) is
 *                      skipped, any other yields (value() as u32) % upper_bound; stops after num_indices, the rest of the buffer
 *                      is discarded.  out_u32: count x num_indices uint32_t.  The number of squeezes depends on the data (an
 *                      element is MAX with probability 2^-64), so sponges of one call may end after different numbers of steps.
 * count == 0 -> TF_OK.  n_chunks / n_squeezes / num_elements / num_indices == 0 -> TF_OK, states untouched.  A NULL pointer with a
 * non-zero size -> TF_ERR_NULL_POINTER; decreasing offsets -> TF_ERR_INVALID_ARGUMENT; an upper_bound that is not a power of two (0
 * included) -> TF_ERR_UPPER_BOUND_NOT_POWER_OF_TWO.  All of these are returned before a device is touched.
 * What is absorbed are words: BFieldCodec encoding is the caller's. */
int tf_tip5_sponge_init(uint64_t *states, size_t count, int fixed_length);
int tf_tip5_sponge_init_dev(uint64_t *d_states, size_t count, int fixed_length, void *stream);
int tf_tip5_sponge_absorb(uint64_t *states, size_t count, const uint64_t *input, size_t n_chunks);
int tf_tip5_sponge_absorb_dev(uint64_t *d_states, size_t count, const uint64_t *d_input, size_t n_chunks, void *stream);
int tf_tip5_sponge_pad_and_absorb_all(uint64_t *states, size_t count, const uint64_t *input, size_t len, const uint64_t *offsets);
int tf_tip5_sponge_pad_and_absorb_all_dev(uint64_t *d_states, size_t count, const uint64_t *d_input, size_t len, const uint64_t *offsets,
                                          void *stream);
int tf_tip5_sponge_squeeze(uint64_t *states, size_t count, size_t n_squeezes, uint64_t *out);
int tf_tip5_sponge_squeeze_dev(uint64_t *d_states, size_t count, size_t n_squeezes, uint64_t *d_out, void *stream);
int tf_tip5_sponge_sample_scalars(uint64_t *states, size_t count, size_t num_elements, uint64_t *out);
int tf_tip5_sponge_sample_scalars_dev(uint64_t *d_states, size_t count, size_t num_elements, uint64_t *d_out, void *stream);
int tf_tip5_sponge_sample_indices(uint64_t *states, size_t count, uint32_t upper_bound, size_t num_indices, uint32_t *out_u32);
int tf_tip5_sponge_sample_indices_dev(uint64_t *d_states, size_t count, uint32_t upper_bound, size_t num_indices, uint32_t *d_out_u32,
                                      void *stream);

/* ---------------------------------------------------------------------------------------------
 * Batch inversion.   replaces  FiniteField::batch_inversion   math/traits.rs:93-121  (Montgomery's trick over a Vec<Self>)
 *                               Inverse::inverse_or_zero       math/traits.rs:39-45   (element by element)
 * `n` counts ELEMENTS: a BFieldElement is 1 word, an XFieldElement 3 words [c0, c1, c2] (x_field_element.rs:217-231); inputs are
 * raw Montgomery words below p, as everywhere in this ABI.
 *   out[i] = in[i]^-1, canonical raw words.  The inverse is unique, so the words are BFieldElement::inverse /
 *            XFieldElement::inverse of each element, and the reference's batch_inversion output (traits.rs:111-118).
 *   n == 0   TF_OK, nothing touched (the reference returns an empty Vec, :95-97).  A NULL pointer with n > 0: TF_ERR_NULL_POINTER.
 *   zero     batch_inversion: any zero element -> TF_ERR_INVERSE_OF_ZERO (the reference's assert!, traits.rs:106).  The host form
 *            and the plain _dev form copy a flag back, so they block once (as tf_poly_interpolate_*_dev); _dev_async follows the
 *            contract of the asynchronous variants above: it writes 12 to d_status (first non-zero code wins) and never
 *            synchronises.  The output of a failed call is unspecified.  An XFieldElement is zero only when all three words are:
 *            (a, 0, 0) and (0, a, 0) with a != 0 are inverted.
 *            inverse_or_zero: zero -> zero, anything else -> its inverse (traits.rs:39-45); it never fails on values, and its _dev
 *            form only enqueues.
 *   in == out is allowed (the reference consumes its Vec and returns it, :113); a partial overlap is not.
 * Each wave inverts 64 K consecutive elements with one exponentiation (csrc/inverse_kernels.h). */
int tf_batch_inversion_bfe(const uint64_t *in, size_t n, uint64_t *out);
int tf_batch_inversion_xfe(const uint64_t *in, size_t n, uint64_t *out);
int tf_batch_inversion_bfe_dev(const uint64_t *d_in, size_t n, uint64_t *d_out, void *stream);
int tf_batch_inversion_xfe_dev(const uint64_t *d_in, size_t n, uint64_t *d_out, void *stream);
int tf_batch_inversion_bfe_dev_async(const uint64_t *d_in, size_t n, uint64_t *d_out, void *stream, int *d_status);
int tf_batch_inversion_xfe_dev_async(const uint64_t *d_in, size_t n, uint64_t *d_out, void *stream, int *d_status);
int tf_inverse_or_zero_bfe(const uint64_t *in, size_t n, uint64_t *out);
int tf_inverse_or_zero_xfe(const uint64_t *in, size_t n, uint64_t *out);
int tf_inverse_or_zero_bfe_dev(const uint64_t *d_in, size_t n, uint64_t *d_out, void *stream);
int tf_inverse_or_zero_xfe_dev(const uint64_t *d_in, size_t n, uint64_t *d_out, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Polynomial arithmetic on packed coefficients and codewords (math/polynomial.rs unless noted).  replaces
 *   Add :2526-2563, Sub :2565-, Neg :2700-              tf_poly_add / _sub / _neg
 *   scalar_mul / scalar_mul_mut :498-532, Mul<S> :2650-2686   tf_poly_scalar_mul
 *   scale :760-773                                      tf_poly_scale           out[j] = a[j] * alpha^j
 *   formal_derivative :275-285                          tf_poly_formal_derivative   out[j] = FF::from(j + 1) * a[j + 1]
 *   degree :181                                         tf_poly_degree
 *   Mul<BFieldElement> for XFieldElement, x_field_element.rs:540-548   tf_hadamard_xfe_bfe_dev   d_out[i] = d_a[i] * d_b[i]
 *   "scalar_mul each, then Add them all"                tf_poly_linear_combination   out[i] = sum_{j<k} polys[j * stride + i] * weights[j]
 * `width` is 1 for BFieldElement and 3 for XFieldElement, as in tf_tip5_hash_table_rows.  Lengths count coefficients.  Words are
 * canonical raw Montgomery words in and out: every result is the unique representative of its field element, so it equals the
 * reference's word for word however a power or a sum is formed.  The `batch` polynomials of a call are packed, n* coefficients each.
 * Each entry point has a host form (host pointers, blocking) and a _dev form (device pointers, enqueued on `stream`); the _dev
 * forms never synchronise, copy nothing back and use no work space.  There is no data-dependent error, so none takes a status word.
 *   add, sub         out: batch x max(na, nb) coefficients; the shorter operand reads as zero above its length.  One width: the
 *                    reference's Add is Polynomial<FF> + Polynomial<FF>.
 *   neg, formal_derivative, degree   one width.  The derivative writes batch x (na - 1) coefficients; na <= 1 writes nothing.
 *   scalar_mul, scale    `scalar` / `alpha` is a HOST array of width_s / width_alpha words in both forms (the _dev form passes it to
 *                    the kernel by value); out has max(width_a, width_s) words per coefficient.  All four combinations 1.1, 3.3,
 *                    3.1, 1.3 are valid: they are the reference's Mul impls, with x_field_element.rs:491-556 between the fields.
 *   degree           degrees[row] = index of the highest non-zero coefficient, -1 for the zero polynomial and for na == 0; an
 *                    XFieldElement is zero only if all three limbs are.  The _dev form writes int64_t words in device memory (set
 *                    to -1 on the stream, then raised by the scan, which starts at the top and stops at the first non-zero block).
 *   linear_combination   column j starts `stride` WORDS after column j - 1, stride >= n * width_p; the words between n * width_p
 *                    and stride are never read.  This is the column-major layout tf_tip5_hash_table_rows and
 *                    tf_merkle_from_columns take, so a table can be combined and committed without a copy.  `weights` holds
 *                    k x width_w words and is a DEVICE pointer in the _dev form (tf_tip5_sponge_sample_scalars_dev leaves its
 *                    output there).  out has max(width_p, width_w) words per element; the four width combinations are valid.
 *                    k == 0 writes n zeros, the reference's empty Sum (b_field_element.rs:214, x_field_element.rs:294).
 *   aliasing         out may be an input of the same element width and length in add, sub, neg, scalar_mul and scale.  It may not
 *                    overlap an input in linear_combination or formal_derivative.
 *   lengths          outputs have a fixed length and are zero padded at the top, as the division calls above document (the
 *                    reference trims, and its equality ignores the padding).  tf_poly_degree gives the normalised length the
 *                    division calls require.
 *   empty calls      na == 0 (add / sub: na == nb == 0), n == 0 or batch == 0: TF_OK, nothing written, NULL pointers allowed --
 *                    except that degree with na == 0 writes -1 per row.
 *   errors           returned before any HIP call, in this order: TF_ERR_NULL_POINTER (a pointer the call would use);
 *                    TF_ERR_INVALID_ARGUMENT (a width other than 1 or 3, stride < n * width_p); TF_ERR_LEN_TOO_LARGE (a length
 *                    above 2^30, k > 65 535); then TF_ERR_NO_DEVICE on a machine without a GPU.
 * Not provided because they are no kernel: shift_coefficients, mod_x_to_the_n and truncate are a pointer offset or a
 * hipMemcpyAsync on packed coefficients.
 * The weighted sum keeps the unreduced 128-bit products in a three-word accumulator per output word and reduces once
 * (csrc/algebra_kernels.h). */
int tf_poly_add(const uint64_t *a, size_t na, const uint64_t *b, size_t nb, int width, uint64_t *out, size_t batch);
int tf_poly_add_dev(const uint64_t *d_a, size_t na, const uint64_t *d_b, size_t nb, int width, uint64_t *d_out, size_t batch, void *stream);
int tf_poly_sub(const uint64_t *a, size_t na, const uint64_t *b, size_t nb, int width, uint64_t *out, size_t batch);
int tf_poly_sub_dev(const uint64_t *d_a, size_t na, const uint64_t *d_b, size_t nb, int width, uint64_t *d_out, size_t batch, void *stream);
int tf_poly_neg(const uint64_t *a, size_t na, int width, uint64_t *out, size_t batch);
int tf_poly_neg_dev(const uint64_t *d_a, size_t na, int width, uint64_t *d_out, size_t batch, void *stream);
int tf_poly_scalar_mul(const uint64_t *a, size_t na, int width_a, const uint64_t *scalar, int width_s, uint64_t *out, size_t batch);
int tf_poly_scalar_mul_dev(const uint64_t *d_a, size_t na, int width_a, const uint64_t *scalar, int width_s, uint64_t *d_out, size_t batch,
                           void *stream);
int tf_poly_scale(const uint64_t *a, size_t na, int width_a, const uint64_t *alpha, int width_alpha, uint64_t *out, size_t batch);
int tf_poly_scale_dev(const uint64_t *d_a, size_t na, int width_a, const uint64_t *alpha, int width_alpha, uint64_t *d_out, size_t batch,
                      void *stream);
int tf_poly_formal_derivative(const uint64_t *a, size_t na, int width, uint64_t *out, size_t batch);
int tf_poly_formal_derivative_dev(const uint64_t *d_a, size_t na, int width, uint64_t *d_out, size_t batch, void *stream);
int tf_poly_degree(const uint64_t *a, size_t na, int width, size_t batch, int64_t *degrees);
int tf_poly_degree_dev(const uint64_t *d_a, size_t na, int width, size_t batch, int64_t *d_degrees, void *stream);
int tf_hadamard_xfe_bfe_dev(const uint64_t *d_a, const uint64_t *d_b, uint64_t *d_out, size_t count, void *stream);
int tf_poly_linear_combination(const uint64_t *polys, size_t n, int width_p, size_t stride, size_t k, const uint64_t *weights, int width_w,
                               uint64_t *out);
int tf_poly_linear_combination_dev(const uint64_t *d_polys, size_t n, int width_p, size_t stride, size_t k, const uint64_t *d_weights,
                                   int width_w, uint64_t *d_out, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Points, powers and gathers: what a FRI query round does between sampling its indices and checking a fold.  replaces
 *   Polynomial::get_colinear_y   math/polynomial.rs:386-394        get_colinear_y   out[i] = (dy (p2x - x0) + dx y0) / dx,
 *                                                                                   dx = x0[i] - x1[i], dy = y0[i] - y1[i]
 *   Polynomial::are_colinear     math/polynomial.rs:348-364        are_colinear     flags[g] = 1 or 0 per group of k points
 *   BFieldElement::mod_pow b_field_element.rs:340-353, ModPowU32 / ModPowU64 :650, :809, x_field_element.rs:654-680
 *                                                                  mod_pow          out[i] = bases[i]^exps[i], element by element
 *   CyclicGroupGenerator::get_cyclic_group_elements b_field_element.rs:656-668, x_field_element.rs:423-435, the powers inside
 *   Polynomial::scale, the points of an evaluation domain          powers           out[i] = first * ratio^i
 *   (indexing a Vec)                                               gather_elements  out[i] = src[indices[i]]
 * `width` is 1 for BFieldElement and 3 for XFieldElement [c0, c1, c2]; lengths count ELEMENTS.  Words are canonical raw Montgomery
 * words in and out.  Each call has a host form (host pointers, blocking) and a _dev form (device pointers, enqueued on `stream`;
 * it never synchronises and copies nothing back); the gather has the _dev form only.  out may not overlap an input.
 *   widths           get_colinear_y and are_colinear take width_x for the x-coordinates and width_y for the y-coordinates (p2x and out
 *                    included).  The valid pairs are (1, 1), (3, 3) and (1, 3); in the mixed form a BFieldElement x stands for its
 *                    lift (x_field_element.rs:491-556) and the result is word for word that of (3, 3) on the lifted x-coordinates.
 *   get_colinear_y   structure of arrays: x0, y0, x1, y1 hold n elements each; p2x holds n_p2x = 1 (one point for all triples, the
 *                    folding challenge) or n_p2x = n elements.  A triple with x0 == x1 is where the reference panics (assert_ne!, :387):
 *                    it raises TF_ERR_INVERSE_OF_ZERO -- the host form returns it, the _dev form writes it to *d_status, one int of
 *                    device memory in which the first non-zero code wins and which is never cleared (the contract of the division
 *                    calls above).  The outputs of the other triples of such a call are still correct, in both forms; only the
 *                    offending triple's slot is unspecified.
 *   are_colinear     xs and ys hold n_groups groups of exactly k points each, group after group; flags holds one int per group.  In the
 *                    reference's order: k < 3 gives 0; two equal x-coordinates anywhere in the group give 0 (an XFieldElement is
 *                    compared on all three limbs); otherwise 1 exactly when every point from the third on lies on the line through
 *                    the first two.  No data-dependent error, so no status word.  k <= 1024 (the uniqueness test is pairwise).  The
 *                    host form answers k < 3 without a device.
 *   mod_pow          bases holds n_bases = 1 or n elements, exps n_exps = 1 or n uint64_t words; a count of 1 is broadcast.  x^0 = 1
 *                    for every x, zero included, as the reference's loop gives.  One base for all elements (g^index, offset^j) is
 *                    served from a table of its repeated squares.
 *   powers           first and ratio are HOST arrays of `width` words in both forms (the _dev form passes them to the kernel by
 *                    value).  With first = 1 this is get_cyclic_group_elements for n = the order of ratio (or its `max`); the
 *                    reference's data-dependent stop -- back at 1 -- is the caller's: it knows the order it asked a root of unity
 *                    for, and n is a fixed length here.
 *   gather_elements  an element is `width` words, 1 <= width <= 16: field elements and 5-word digests alike.  indices is the
 *                    uint32_t array a sponge's index sampler writes.  An index >= src_len is not read: it writes
 *                    TF_ERR_INVALID_ARGUMENT to *d_status and leaves its slot of d_out as it was; the other outputs are correct.
 *                    The second half of a fold (index + n / 2) is a pointer offset on d_src.
 *   empty calls      n == 0 (are_colinear: n_groups == 0): TF_OK, nothing touched, NULL pointers allowed.
 *   errors           returned before any HIP call, in this order: TF_ERR_NULL_POINTER (a pointer the call would use, d_status
 *                    included; xs / ys may be NULL when k == 0, d_src when src_len == 0); TF_ERR_INVALID_ARGUMENT (a width or width
 *                    pair not listed above, n_p2x / n_bases / n_exps neither 1 nor n); TF_ERR_LEN_TOO_LARGE (n, n_groups, n_groups * k
 *                    or src_len above 2^30, k above 1024); then TF_ERR_NO_DEVICE on a machine without a GPU.
 * get_colinear_y divides by Montgomery's trick per wave, in the field of the x-coordinates (csrc/points_kernels.h). */
int tf_get_colinear_y(const uint64_t *x0, const uint64_t *y0, const uint64_t *x1, const uint64_t *y1, size_t n, const uint64_t *p2x,
                      size_t n_p2x, int width_x, int width_y, uint64_t *out);
int tf_get_colinear_y_dev(const uint64_t *d_x0, const uint64_t *d_y0, const uint64_t *d_x1, const uint64_t *d_y1, size_t n,
                          const uint64_t *d_p2x, size_t n_p2x, int width_x, int width_y, uint64_t *d_out, void *stream, int *d_status);
int tf_are_colinear(const uint64_t *xs, const uint64_t *ys, size_t n_groups, size_t k, int width_x, int width_y, int *flags);
int tf_are_colinear_dev(const uint64_t *d_xs, const uint64_t *d_ys, size_t n_groups, size_t k, int width_x, int width_y, int *d_flags,
                        void *stream);
int tf_mod_pow(const uint64_t *bases, size_t n_bases, const uint64_t *exps, size_t n_exps, int width, uint64_t *out, size_t n);
int tf_mod_pow_dev(const uint64_t *d_bases, size_t n_bases, const uint64_t *d_exps, size_t n_exps, int width, uint64_t *d_out, size_t n,
                   void *stream);
int tf_powers(const uint64_t *first, const uint64_t *ratio, int width, uint64_t *out, size_t n);
int tf_powers_dev(const uint64_t *first, const uint64_t *ratio, int width, uint64_t *d_out, size_t n, void *stream);
int tf_gather_elements_dev(const uint64_t *d_src, size_t src_len, int width, const uint32_t *d_indices, size_t n, uint64_t *d_out,
                           void *stream, int *d_status);

/* ---------------------------------------------------------------------------------------------
 * FRI folding: the commit side of FRI, split-and-fold of whole codewords, one to many levels per call.  replaces
 *   Polynomial::get_colinear_y   math/polynomial.rs:386-394   through (x_i, c[i]) and (-x_i, c[i + n/2]) at the challenge, for every
 *                                                             i < n/2 of a codeword on an evaluation domain
 * A codeword c of n = 2^k elements (n >= 2) lies on {g w_n^i} in natural order, g = offset_raw a non-zero BFieldElement and w_n the
 * reference's primitive_root_of_unity(n).  One level folds it by the challenge alpha into n/2 elements on {g^2 w_{n/2}^i}:
 *     out[i] = get_colinear_y((x_i, c[i]), (-x_i, c[i + n/2]), alpha) = 1/2 [(1 + alpha / x_i) c[i] + (1 - alpha / x_i) c[i + n/2]],
 *     x_i = g w_n^i, 0 <= i < n/2
 * and `levels` = r with the challenges alpha_1 .. alpha_r is r such folds in a row: level j runs on the offset g^(2^(j-1)) and the
 * length n / 2^(j-1), the result has n / 2^r elements on the offset g^(2^r).  Words are canonical raw Montgomery words in and out,
 * so the result is word for word that of the composition it replaces (tf_powers twice, tf_get_colinear_y with n_p2x = 1).
 *   layout           codewords holds `batch` codewords of n elements of width_c words each, packed; out holds batch x n / 2^levels
 *                    elements of width_a words.  out may not overlap an input.
 *   widths           (width_c, width_a) is (1, 1), (3, 3) or (1, 3).  In the mixed form a BFieldElement codeword is folded by an
 *                    XFieldElement challenge: the result is word for word that of (3, 3) on the lifted codeword, and the levels after
 *                    the first run as (3, 3).
 *   challenges       n_sets x levels elements of width_a words; n_sets is 1 (one set for every codeword) or `batch` (set b for
 *                    codeword b: many transcripts).  In the _dev form this is device memory, exactly as
 *                    tf_tip5_sponge_sample_scalars_dev leaves it.
 *   forms            tf_fri_fold takes host pointers and returns when the result is in place.  tf_fri_fold_dev takes device pointers
 *                    and only enqueues on `stream`: it never synchronises and copies nothing back.  Nothing in a fold depends on the
 *                    data, so there is no status word.
 *   passes           one launch folds up to R_max = 4 levels in registers; more levels run as several passes, R_max each and the
 *                    remainder last, with the intermediates in stream-ordered temporaries from the library's pool (a failed
 *                    allocation is TF_ERR_OUT_OF_MEMORY).  tf_fri_fold_plan writes the levels of each pass (at most `capacity`
 *                    entries; levels_per_pass may be NULL) and returns the number of passes, or minus the status the fold would
 *                    return for these arguments.  tf_fri_fold_workspace returns the bytes of those temporaries: nothing for one
 *                    pass, the first intermediate (batch x n / 2^R_max elements of width_a words) for two, the first and the second
 *                    for three and more (the later, smaller ones reuse the two blocks in turn); 0 for a call that is rejected or
 *                    empty.  Both are host arithmetic and need no device.
 *   empty calls      batch == 0: TF_OK, nothing touched, NULL pointers allowed.
 *   errors           returned before any HIP call, in this order: TF_ERR_NULL_POINTER; TF_ERR_INVALID_ARGUMENT (a width pair not
 *                    listed above, levels == 0, n_sets neither 1 nor batch); TF_ERR_LEN_NOT_POWER_OF_TWO (n, 0 included);
 *                    TF_ERR_INVALID_ARGUMENT (2^levels > n); TF_ERR_LEN_TOO_LARGE (n above 2^30, or more than 2^35 words read);
 *                    TF_ERR_INVERSE_OF_ZERO (offset_raw == 0: x_i == -x_i, the reference's assert_ne!(x0, x1), the code
 *                    tf_get_colinear_y uses); then TF_ERR_NO_DEVICE on a machine without a GPU.
 * No division: the inverse points g^-1 w_n^-i are a geometric sequence, and the twiddles inside a pass and the halvings are
 * power-of-two products (csrc/fri_kernels.h). */
int tf_fri_fold(const uint64_t *codewords, size_t n, size_t batch, int width_c, uint64_t offset_raw, const uint64_t *challenges,
                size_t levels, size_t n_sets, int width_a, uint64_t *out);
int tf_fri_fold_dev(const uint64_t *d_codewords, size_t n, size_t batch, int width_c, uint64_t offset_raw, const uint64_t *d_challenges,
                    size_t levels, size_t n_sets, int width_a, uint64_t *d_out, void *stream);
size_t tf_fri_fold_workspace(size_t n, size_t batch, int width_c, int width_a, size_t levels);
int tf_fri_fold_plan(size_t n, size_t levels, int width_c, int width_a, int *levels_per_pass, int capacity);

/* ---------------------------------------------------------------------------------------------
 * Prefix scans: the one operation of a prover whose value at row i depends on row i - 1 -- the auxiliary columns of an AIR.  replaces
 * the sequential loop a caller runs on the host between two device calls:
 *   running sum        y_i = y_(i-1) + b_i             tf_scan_sum_dev       a log-derivative column, b_i = m_i / d_i
 *   running product    y_i = y_(i-1) a_i               tf_scan_product_dev   a permutation argument, a_i = alpha - v_i
 *   running evaluation y_i = a_i y_(i-1) + b_i         tf_scan_affine_dev    a_i = alpha: Horner; also the recurrence behind tf_powers
 * The recurrence is inclusive and runs along each of `batch` columns of n elements:
 *     y_(-1) = init,   y_i = a_i y_(i-1) + b_i   (0 <= i < n),   out[i] = y_i
 * with the field's own product (BFieldElement, or XFieldElement per x_field_element.rs:512-536).  Words are canonical raw Montgomery
 * words in and out, so every result is the unique representative of its element and equals the sequential loop word for word,
 * however the kernels regroup the products.
 *   layout           column c of an operand starts stride_* WORDS after column c - 1, stride >= n * width: the column-major layout of
 *                    tf_poly_linear_combination and tf_merkle_from_columns.  a, b and out each have a stride of their own; words
 *                    between n * width and the stride are never read and never written.
 *   widths           (width_a, width_b) is (1, 1), (3, 3) or (3, 1): the last is an XFieldElement multiplier over a BFieldElement
 *                    column, word for word (3, 3) on the lifted column.  out and init have width_out = max(width_a, width_b) words per
 *                    element.  sum and product take one width.
 *   multipliers      of tf_scan_affine_dev: a_len == n: one element per row, column c at a + c * stride_a.  a_len == 1: one element for
 *                    the whole column; `a` then holds a_sets elements packed, a_sets = 1 (one challenge for every column) or batch
 *                    (element c for column c) -- device memory exactly as tf_tip5_sponge_sample_scalars_dev leaves it; stride_a and
 *                    a_sets are looked at in their own form only.  With n == 1 both forms have a_len == 1 and stride_a decides:
 *                    stride_a == 0, which no table has, is the packed form (a_sets elements); stride_a >= width_a is a table of one
 *                    row and `batch` elements are READ at a + c * stride_a -- a caller that holds one broadcast challenge passes
 *                    stride_a = 0, as it may for every n, or the call reads past its one element.
 *   init             device pointer to n_init elements, n_init = 0 (NULL allowed: the neutral start, 0 for sum and affine, 1 for
 *                    product), 1 (one start for every column) or batch.
 *   forms            only _dev forms: device pointers, enqueued on `stream`, never synchronised, nothing copied back.  Nothing
 *                    depends on the data, so there is no status word.
 *   work space       the caller's: d_work, work_bytes.  tf_scan_workspace(mode, n, batch, width_out) returns the bytes a call needs
 *                    (mode is TF_SCAN_SUM / _PRODUCT / _AFFINE): 0 for a column of at most one tile (one launch), for an empty and
 *                    for a rejected call; else tiles * batch * (M + width_out) * 8, M = width_out words per tile map (2 width_out for
 *                    affine).  d_work may be NULL when that is 0; it is 8-byte aligned; a smaller work_bytes is
 *                    TF_ERR_INVALID_ARGUMENT; nothing behind the returned size is touched.  The library allocates nothing.
 *   plan             tf_scan_plan writes (at most `capacity` entries; info may be NULL) info[0] elements per tile T, [1] tiles per
 *                    column, [2] tile maps the spine takes per turn S, [3] launches (0 empty, 1 one tile, 3 otherwise), [4] elements up
 *                    to which a column is scanned by one wave, [5] M; it returns the launches, or minus the status the call would
 *                    return for (mode, n, batch, width_out).  Host arithmetic like tf_scan_workspace: no device needed.
 *   aliasing         out may be exactly b (sum, and affine with width_a == width_b) or exactly a (product): the same pointer, the same
 *                    stride, the same width.  Any other overlap of out or d_work with an operand, or of out with d_work, is the
 *                    caller's error.
 *   empty calls      n == 0 or batch == 0: TF_OK, nothing touched, NULL pointers allowed.
 *   errors           returned before any HIP call, in this order: TF_ERR_NULL_POINTER (an operand, out, init with n_init != 0, d_work
 *                    where an otherwise valid call needs work space); TF_ERR_INVALID_ARGUMENT (a width or pair not listed, a_len not
 *                    in {1, n}, a_sets not in {1, batch} in the packed form, a stride below n * width, n_init not in {0, 1, batch}, a short
 *                    work space); TF_ERR_LEN_TOO_LARGE (n above 2^30; n * batch * width_out above 2^35 words -- 2^34 for affine,
 *                    which reads two operands; or, for columns above info[4] elements, batch * tiles above 2^24 - 1, the
 *                    workgroups of one launch: first met at 2^24 columns of 1025 BFieldElements); then TF_ERR_NO_DEVICE on a
 *                    machine without a GPU.
 * Not built: the exclusive scan (it is the inclusive scan of n - 1 elements written one slot further, with init in slot 0), and
 * row-major tables (tf_table_transpose exists).  Three launches in stream order (tile maps, one spine per column, tiles from their
 * start values) and no workgroup ever waits for another (csrc/scan_kernels.h). */
#define TF_SCAN_SUM 0
#define TF_SCAN_PRODUCT 1
#define TF_SCAN_AFFINE 2
int tf_scan_sum_dev(const uint64_t *d_in, size_t n, size_t batch, int width, size_t stride_in, const uint64_t *d_init, size_t n_init,
                    uint64_t *d_out, size_t stride_out, void *d_work, size_t work_bytes, void *stream);
int tf_scan_product_dev(const uint64_t *d_in, size_t n, size_t batch, int width, size_t stride_in, const uint64_t *d_init, size_t n_init,
                        uint64_t *d_out, size_t stride_out, void *d_work, size_t work_bytes, void *stream);
int tf_scan_affine_dev(const uint64_t *d_a, size_t a_len, size_t a_sets, int width_a, size_t stride_a, const uint64_t *d_b, int width_b,
                       size_t stride_b, size_t n, size_t batch, const uint64_t *d_init, size_t n_init, uint64_t *d_out, size_t stride_out,
                       void *d_work, size_t work_bytes, void *stream);
size_t tf_scan_workspace(int mode, size_t n, size_t batch, int width_out);
int tf_scan_plan(int mode, size_t n, size_t batch, int width_out, int *info, int capacity);

/* ---------------------------------------------------------------------------------------------
 * DEEP quotients: the codeword FRI is run on, from the extended tables and the out-of-domain values, and the same value at sampled
 * rows for the verifier.  replaces the composition, per point, of tf_poly_linear_combination_dev, tf_powers_dev, a broadcast
 * subtraction, tf_batch_inversion_xfe_dev and two Hadamard passes:
 *     out[i] = sum_{p < n_points} ( sum_c w[p][c] * (T_c[i] - v[p][c]) ) / (x_i - z_p),    x_i = offset * w_n^i
 * T_c are the columns of two column-major tables: k1 BFieldElement columns (`main`, column c = n words at d_main + c * stride_main)
 * followed by k3 XFieldElement columns (`aux`, column c = 3 n words at d_aux + c * stride_aux); a BFieldElement stands for its lift.
 * z_p are the out-of-domain points (in practice z and w z), v the claimed values there, w the sampled weights.  Every result is the
 * canonical raw Montgomery word of the field element the formula defines, whatever the grouping of the operations: there is no
 * tolerance anywhere.
 *   domain           w_n is the reference's primitive_root_of_unity(n), natural order: the domain of tf_fri_fold_dev and
 *                    tf_coset_eval_*.  offset_raw is a non-zero BFieldElement.
 *   operands         all in device memory.  d_points: n_points XFieldElements.  d_weights, d_values: n_points * (k1 + k3)
 *                    XFieldElements each, point-major, the main columns first: element (p, c) at ((p * (k1 + k3)) + c) * 3 -- where
 *                    tf_tip5_sponge_sample_scalars_dev and tf_barycentric_evaluate_*_dev leave them.  d_out: n XFieldElements.
 *                    Words between the end of a column and its stride are never read.
 *   limits           1 <= n_points <= 4; k1 + k3 <= 65 535, the counter bound of the carry-deferred accumulators
 *                    (csrc/algebra_kernels.h); n a power of two, at most 2^32.
 *   empty tables     either table may be empty: k1 == 0 allows d_main == NULL, k3 == 0 allows d_aux == NULL, and the stride of an
 *                    empty table is not looked at.  k1 + k3 == 0 writes zeros (the empty sum), needs no d_weights, d_values or work
 *                    space and leaves the status alone.
 *   empty calls      n == 0 (rows form: n_rows == 0): TF_OK, nothing touched, NULL pointers allowed.
 *   zero denominator x_i == z_p (z_p the lift of a point of the domain) writes TF_ERR_INVERSE_OF_ZERO to *d_status, one int of device
 *                    memory in which the first non-zero code stays and which is never cleared (the contract of the _async calls).
 *                    That element of d_out is unspecified; every other element, those of the same wave included, is correct.
 *   rows form        tf_deep_quotient_rows_dev computes out[r] = the value above at i = d_indices[r], r < n_rows, from row-major rows:
 *                    row r of d_main_rows = k1 words at r * row_stride_main, row r of d_aux_rows = 3 k3 words at r * row_stride_aux
 *                    -- what tf_table_gather_rows_dev wrote for the same index list.  Repeated indices are allowed.  An index >= n
 *                    writes TF_ERR_INVALID_ARGUMENT to *d_status, the code tf_table_gather_rows_dev stores for it; that row of
 *                    d_out is unspecified, every other row is correct.  No work space.
 *   work space       the caller's: d_work, work_bytes.  tf_deep_quotient_workspace returns the bytes a codeword call needs: one
 *                    XFieldElement per point (C_p = sum_c w[p][c] v[p][c], formed once per call by a small launch ahead of the
 *                    passes); 0 for k1 + k3 == 0, for an empty and for a rejected call.  d_work may be NULL when that is 0; it is
 *                    8-byte aligned; a smaller work_bytes is TF_ERR_INVALID_ARGUMENT.  The library allocates nothing and has no
 *                    host-pointer form of these calls.
 *   passes           one pass of the codeword kernel serves up to two points and reads every word of both tables once; n_points = 3
 *                    and 4 run a second pass over the tables, which adds its points' terms into d_out (a one-pass form of four
 *                    points does not fit the register file without scratch).  No codeword-sized intermediate is written.
 *   plan             tf_deep_quotient_plan writes (at most `capacity` entries; fields may be NULL) fields[0] elements per wave and step
 *                    (the chunk C), [1] elements per lane, [2] points per pass, [3] passes, [4] launches (the constants and the
 *                    passes; 1 for k1 + k3 == 0, 0 for n == 0), [5] the grid cap in chunks: above that many chunks a wave takes
 *                    further chunks in a grid-stride loop.  It returns the launches, or minus the status the call would return for
 *                    (n, k1, k3, n_points).  Host arithmetic, as tf_deep_quotient_workspace: no device needed.
 *   aliasing         d_out, d_work and d_status must not overlap an input or each other.
 *   forms            only _dev forms: device pointers, enqueued on `stream`; nothing is synchronised or copied back.
 *   errors           returned before any HIP call, in this order: TF_ERR_NULL_POINTER (a pointer the call would use: d_points, d_out
 *                    and d_status always, a table with columns, d_weights and d_values with k1 + k3 > 0, d_indices, d_work where an
 *                    otherwise valid call needs it); TF_ERR_INVALID_ARGUMENT (n_points outside 1..4, the stride of a table with
 *                    columns below its line: n or 3 n words, k1 or 3 k3 words in the rows form; a short work space);
 *                    TF_ERR_LEN_NOT_POWER_OF_TWO (n; in the rows form n == 0 too); TF_ERR_LEN_TOO_LARGE (n above 2^32, k1 + k3 above
 *                    65 535, n_rows above 2^30, a table whose lines at its stride span more than 2^40 words);
 *                    TF_ERR_INVERSE_OF_ZERO (offset_raw == 0); then TF_ERR_NO_DEVICE on a machine without a GPU.
 * Lanes run along i: a wave owns C consecutive elements, inverts all their denominators with one inversion (Montgomery's trick over
 * the wave, as tf_batch_inversion_*) and accumulates the weighted sums unreduced (csrc/deep_kernels.h). */
int tf_deep_quotient_dev(const uint64_t *d_main, size_t k1, size_t stride_main, const uint64_t *d_aux, size_t k3, size_t stride_aux, size_t n,
                         uint64_t offset_raw, const uint64_t *d_points, size_t n_points, const uint64_t *d_weights, const uint64_t *d_values,
                         uint64_t *d_out, void *d_work, size_t work_bytes, void *stream, int *d_status);
size_t tf_deep_quotient_workspace(size_t n, size_t k1, size_t k3, size_t n_points);
int tf_deep_quotient_plan(size_t n, size_t k1, size_t k3, size_t n_points, int *fields, int capacity);
int tf_deep_quotient_rows_dev(const uint64_t *d_main_rows, size_t k1, size_t row_stride_main, const uint64_t *d_aux_rows, size_t k3,
                              size_t row_stride_aux, size_t n, uint64_t offset_raw, const uint32_t *d_indices, size_t n_rows,
                              const uint64_t *d_points, size_t n_points, const uint64_t *d_weights, const uint64_t *d_values,
                              uint64_t *d_out, void *stream, int *d_status);

/* ---------------------------------------------------------------------------------------------
 * Tables: moving a table between the two layouts the library itself uses, and opening its rows.  replaces
 *   Array2 .t() / reversed_axes, a prover's own transposes           table_transpose     dst line i, element o = src line o, element i
 *   table.row(i) / select(Axis(0), indices)                          table_gather_rows   out row q = row indices[q]
 *   the per-column low-degree extension of a trace kept row by row   table_lde_rows      tf_lde_*_dev of every column of a row-major table
 * An element is `width` consecutive words: 1 for BFieldElement, 3 for XFieldElement [c0, c1, c2].  Strides count WORDS, every other
 * length counts elements.  Words are moved as they are.
 *   column-major     exactly the layout of tf_tip5_hash_table_rows: column j = n_rows elements at table + j * col_stride, col_stride >=
 *                    n_rows * width; tables n_cols * col_stride words apart.  What a batch of coset evaluations leaves, and what
 *                    tf_merkle_from_columns and tf_poly_linear_combination read.
 *   row-major        row i = n_cols elements at rows + i * row_stride, row_stride >= n_cols * width; tables n_rows * row_stride words
 *                    apart.  What tf_tip5_hash_varlen_rows and tf_merkle_from_rows read (row_stride = row_len), and how a prover keeps
 *                    its trace and reveals rows.
 *   padding          words between the end of a line and its stride are never read in a source and never written in a destination.
 *   table_transpose  src: `batch` matrices of n_outer lines of n_inner elements, line o at src + o * src_stride, matrices
 *                    n_outer * src_stride apart; dst: n_inner lines of n_outer elements at dst_stride, matrices n_inner * dst_stride apart.
 *                      column-major -> row-major:  (table, n_cols, n_rows, width, col_stride, rows, row_stride, batch)
 *                      row-major -> column-major:  (rows, n_rows, n_cols, width, row_stride, table, col_stride, batch)
 *   table_gather_rows  out row q of table t (at out + (t * k + q) * out_stride, n_cols elements, out_stride >= n_cols * width) = row
 *                    indices[q] of table t: one index list for all `batch` tables, repeats allowed; indices is the uint32_t array a
 *                    sponge's index sampler writes.  `layout` is TF_TABLE_COLUMN_MAJOR or TF_TABLE_ROW_MAJOR and `stride` the
 *                    col_stride or row_stride that goes with it.  An index >= n_rows is not read: the host form returns
 *                    TF_ERR_INVALID_ARGUMENT; the _dev form writes it to *d_status, one int of device memory in which the first
 *                    non-zero code stays and which is never cleared (the contract of tf_gather_elements_dev).  Either way that row's
 *                    slot of out stays as it was, in every table, and every other row is correct.
 *   table_lde_rows   ONE row-major table, device-resident only (as tf_lde_*_dev): rows in = n x n_cols values on {offset_in * w_n^i},
 *                    rows out = m x n_cols values on {offset_out * w_m^i}.  Works through blocks of c = cols_per_block columns, the last
 *                    one ragged: transpose the block in, tf_lde_*_dev with batch = c, transpose it out.  cols_per_block == 0 picks the
 *                    largest c <= n_cols with c * (n + m) * width * 8 <= 256 MiB (at least 1; a chosen bound on the work space, not a
 *                    measured optimum); a value above n_cols means n_cols.  Blocking bounds memory and costs time (2^18 -> 2^20 x 64
 *                    BFieldElements: three blocks of 25 columns take about one and a half times as long as one block of 64,
 *                    DESIGN 7.5): a caller
 *                    with c = n_cols worth of work space to spare should pass cols_per_block = n_cols.  The two column-major
 *                    temporaries are taken once per call
 *                    on the caller's stream; tf_table_lde_rows_workspace returns their size in bytes (what tf_lde_*_dev takes itself
 *                    comes on top), 0 for arguments the call rejects.  One stream, no side streams.
 *   forms            a _dev form takes device pointers and only enqueues on `stream`: it never synchronises and copies nothing back.
 *                    A host form takes host pointers and returns when the result is in place.  Source and destination may not overlap.
 *   empty calls      any of n_outer, n_inner, n_cols, k, batch zero (the LDE: n_cols == 0 or m == 0): TF_OK, nothing touched, NULL
 *                    pointers allowed.
 *   errors           returned before any HIP call, in this order: TF_ERR_NULL_POINTER (d_status included); TF_ERR_INVALID_ARGUMENT (a
 *                    width other than 1 or 3, a stride shorter than its line, a layout other than the two); TF_ERR_LEN_TOO_LARGE (any
 *                    of n_outer, n_inner, n_rows, n_cols, k above 2^30, more than 2^35 words moved by the call, or an operand
 *                    whose lines at its stride span more than 2^40 words -- a stride no device memory holds, which may
 *                    not wrap the 64-bit offsets); then TF_ERR_NO_DEVICE.  table_lde_rows answers with the argument errors of tf_lde_*_dev first, in their order and
 *                    before anything is enqueued (n > m, a length that is no power of two or too large, a NULL pointer, a zero
 *                    offset_in), then with TF_ERR_LEN_TOO_LARGE for n_cols above 2^30 or more than 2^35 words of output, TF_ERR_INVALID_ARGUMENT for
 *                    a short stride and TF_ERR_LEN_TOO_LARGE for a span above 2^40 words.  tf_table_lde_rows_workspace is 0 for
 *                    every call that is rejected or empty (m == 0 included).
 * The transpose stages tiles of 64 x 64 BFieldElements or 32 x 32 XFieldElements in LDS (csrc/table_kernels.h). */
#define TF_TABLE_COLUMN_MAJOR 0
#define TF_TABLE_ROW_MAJOR 1
int tf_table_transpose(const uint64_t *src, size_t n_outer, size_t n_inner, int width, size_t src_stride, uint64_t *dst, size_t dst_stride,
                       size_t batch);
int tf_table_transpose_dev(const uint64_t *d_src, size_t n_outer, size_t n_inner, int width, size_t src_stride, uint64_t *d_dst,
                           size_t dst_stride, size_t batch, void *stream);
int tf_table_gather_rows(const uint64_t *table, int layout, size_t n_rows, size_t n_cols, int width, size_t stride, const uint32_t *indices,
                         size_t k, uint64_t *out, size_t out_stride, size_t batch);
int tf_table_gather_rows_dev(const uint64_t *d_table, int layout, size_t n_rows, size_t n_cols, int width, size_t stride,
                             const uint32_t *d_indices, size_t k, uint64_t *d_out, size_t out_stride, size_t batch, void *stream,
                             int *d_status);
int tf_table_lde_rows_bfe_dev(const uint64_t *d_rows, size_t n, size_t n_cols, size_t row_stride_in, uint64_t offset_in_raw, uint64_t *d_out,
                              size_t m, size_t row_stride_out, uint64_t offset_out_raw, size_t cols_per_block, void *stream);
int tf_table_lde_rows_xfe_dev(const uint64_t *d_rows, size_t n, size_t n_cols, size_t row_stride_in, uint64_t offset_in_raw, uint64_t *d_out,
                              size_t m, size_t row_stride_out, uint64_t offset_out_raw, size_t cols_per_block, void *stream);
size_t tf_table_lde_rows_workspace(size_t n, size_t m, size_t n_cols, int width, size_t cols_per_block);

/* ---------------------------------------------------------------------------------------------
 * Deployment settings (process-wide).  These two are the ONLY environment variables the library reads (once, at the first
 * call); the TF_* switches that DESIGN_HISTORY.md names belonged to variants that lost their measurements and are gone.
 *   TF_NTT_TILE_BYTES : bytes of batch processed between the passes of a multi-pass NTT (scratch size),
 *                       (default 2 GiB: measured on MI355X the pass kernels are VALU-bound and larger
 *                       launches overlap better than Infinity-Cache-sized ones).
 */
void tf_set_ntt_tile_bytes(size_t bytes);
size_t tf_get_ntt_tile_bytes(void);
/*   TF_NTT_PIPE       : K = 1..4 side streams the batch tiles of a multi-pass NTT are dealt to round-robin (each with its own
 *                       scratch tile), so the column pass of tile t + 1 overlaps the transposing pass of tile t and a tile
 *                       sized for the Infinity Cache is re-read out of it; the caller's stream forks/joins with events. */
void tf_set_ntt_pipe(int streams);  /* 0 = automatic (the default: two streams for the two-pass plans of 2^21 / 2^22 points when a call has
                                     * several batch tiles, one otherwise; profiles/r06_pipe_tiles.txt).  All callers of a device share
                                     * its K side streams: concurrent callers stay correct (event forks / joins) but wait for each other */
int tf_get_ntt_pipe(void);

/* ---------------------------------------------------------------------------------------------
 * Test hooks.  The planner picks between code paths by shape (number of passes, tile geometry, latency-shaped kernels, the
 * batch-evaluation route); each hook forces one side so that the parity tests can run BOTH against the oracle at any size.  Every
 * setting produces the same words.  Process-wide, not meant for production callers.
 *
 * Plan at least `passes` (2..4) global passes whenever n >= 32^passes, so the three- and four-pass paths (normally
 * n > 2^22 and n = 2^31) can be checked at small sizes.  0 restores the automatic plan. */
void tf_set_ntt_min_passes(int passes);
/* Calls with little work (<= 2^21 words) are planned with narrower tiles (256-thread workgroups); -1 = automatic
 * (default), 0 = never, 1 = always. */
void tf_set_ntt_small_launch(int mode);
/* Transforms of 2^21 and 2^22 points run in TWO global passes (a 2048-point pass = pairs of 1024-point workgroups sharing their
 * input) instead of three; -1 = automatic (default), 0 = never (the three-pass plan, which also serves the shapes the
 * two-pass plan does not: small launches, truncated products), 1 = the 2048-point pairs whenever the shape supports them.
 * (2 is taken as 1: it once selected a 1024 x 4096 plan, a measured loss, profiles/r04_c4_plan_ab.txt.)
 * 3 = the two-pass plan with its FIRST pass as one workgroup per 2048-row x 8-column tile (every element loaded and scaled once,
 * DESIGN 4.1b, round 6) wherever the two-pass plan applies; the automatic plan takes that kernel for coset evaluations of 2^22 points,
 * where it measured faster (profiles/r06_c4_cols8_ab.txt). */
void tf_set_ntt_two_pass(int mode);
/* The latency-shaped kernels (8 elements per thread, radix-8 stages through LDS) instead of the 32-elements-per-thread
 * pass kernels: ntt_lat_kernel for 64 .. 4096-point transforms in calls of up to 2^22 words (BFieldElement; 3 * 2^19 words
 * XFieldElement), ntt_lat2_kernel for 2^13 .. 2^20-point transforms in calls below a per-length threshold (tf_plan.hip:
 * lat_wanted / lat2_wanted hold the measured crossovers).  -1 = automatic (default), 0 = never, 1 = whenever the shape allows. */
void tf_set_ntt_latency_kernel(int mode);
/* Number of transform-kernel launches one plain tf_ntt_*_dev call enqueues for this shape: read from the very plan such a call
 * executes (plan_ntt, tf_plan.hip -- tiny / rows / latency-shaped kernels, whole-transform-per-workgroup kernels, tiles x passes of
 * ntt_pass_kernel, the narrow-tile three-pass plan of small 2^21 / 2^22 calls).  Diagnostic; bench.py uses it to turn a
 * HIP-event interval into an average launch duration.  Table builders of a first call are not counted. */
int tf_ntt_launch_count(size_t n, size_t batch, int width);
/* Planner introspection (no device needed): number of global passes of one n-point transform (0 for lengths ntt rejects)
 * and log2 of each pass's radix in log2_radix_out[0..3] (unused entries 0).  The radices multiply to n.  This is the plan of a
 * LARGE call (plan_ntt with the latency-shaped kernels and the narrow tiles ruled out: enough work for 512-thread tiles); a call small enough for the narrow tiles -- e.g. ONE 2^21-point BFieldElement
 * slice -- runs 2^21 / 2^22 points on the three-pass plan instead of {10, 11} / {11, 11}: tf_ntt_launch_count(n, batch, width)
 * is exact for a given batch. */
int tf_ntt_plan(size_t n, int width, int* log2_radix_out);
/* Measurement helper: the shader clock (MHz) the current device is running at right now (one-wave ~0.5 ms spin; < 0 on failure). */
double tf_debug_sclk_mhz(void);

/* Synthetic inputs for benches/tests: d_out[i] = BFieldElement::new(splitmix64(seed ^ (first_index + i)) mod p),
 * raw Montgomery words, generated on the device (the oracle's tfo_fill_random is the same counter-based sequence). */
int tf_debug_fill_random_dev(uint64_t *d_out, size_t count, uint64_t seed, uint64_t first_index, void *stream);
/* Test helper: d_x[i] <- d_x[i] * 2^e mod p (canonical word) for ANY 64-bit words d_x[i], 0 <= e < 192, in place, through the
 * power-of-two products (and their sign) of the NTT networks -- hand-scheduled blocks of four and of two per thread.
 * TF_ERR_INVALID_ARGUMENT for an exponent outside [0, 192). */
int tf_debug_mul_pow2_dev(uint64_t *d_x, size_t count, int e, void *stream);
/* Test helper: ONE hand-scheduled field primitive of the kernels (csrc/gl64.h, csrc/tip5_kernels.h) over `count` operand pairs
 * (d_a[i], d_b[i]), called exactly as the kernels call it -- the same function, whatever form the build's switches select.  A thread
 * runs one block of the primitive on W consecutive elements, so element index mod W is the position in the block (which carry chain:
 * vcc or an SGPR pair).  Loads and stores are guarded by count (missing operands are 0); nothing behind count is written.
 *   op                               primitive                        W   operands                                 outputs
 *   ADD, SUB                         gl::add, gl::sub                 1   a, b canonical                           out0
 *   MONT_MUL                         gl::mont_mul                     1   any two words                            out0
 *   ADD_SUB                          gl::add_sub                      1   canonical                                out0 = a + b, out1 = a - b
 *   ADD_SUB2                         gl::add_sub2                     2   canonical                                out0, out1
 *   ADD_SUB_LAZY2                    gl::add_sub_lazy2                2   a any word, b <= p                       out0, out1
 *   ADD_LAZY4, SUB_LAZY4             gl::add_lazy4, gl::sub_lazy4     4   a any word, b <= p                       out0
 *   MONT_MUL2 / 3 / 4                gl::mont_mul2 / 3 / 4            2 / 3 / 4   any two words                    out0
 *   CANONICAL                        gl::canonical_asm                1   a any word (d_b is not read)             out0
 *   MX_FOLD4_CANON, MX_FOLD4_LAZY    tfk::mx_fold4_tail<true / false> 4   a = (th : tl) < 2^63 + 2^59, h0 = low    out0
 *   MX_FOLD2                         tfk::mx_fold2_tail               2   half of b                                out0
 * d_out1 is written by the ops with two outputs only and may be null otherwise.  TF_ERR_INVALID_ARGUMENT for an unknown op or a count
 * above 2^32, checked before anything else; a count of 0 is TF_OK. */
enum {
    TF_FIELD_OP_ADD = 0,
    TF_FIELD_OP_SUB = 1,
    TF_FIELD_OP_MONT_MUL = 2,
    TF_FIELD_OP_ADD_SUB = 3,
    TF_FIELD_OP_ADD_SUB2 = 4,
    TF_FIELD_OP_ADD_SUB_LAZY2 = 5,
    TF_FIELD_OP_ADD_LAZY4 = 6,
    TF_FIELD_OP_SUB_LAZY4 = 7,
    TF_FIELD_OP_MONT_MUL2 = 8,
    TF_FIELD_OP_MONT_MUL3 = 9,
    TF_FIELD_OP_MONT_MUL4 = 10,
    TF_FIELD_OP_CANONICAL = 11,
    TF_FIELD_OP_MX_FOLD4_CANON = 12,
    TF_FIELD_OP_MX_FOLD4_LAZY = 13,
    TF_FIELD_OP_MX_FOLD2 = 14,
    TF_FIELD_OP_COUNT = 15
};
int tf_debug_field_op_dev(int op, const uint64_t *d_a, const uint64_t *d_b, uint64_t *d_out0, uint64_t *d_out1, size_t count, void *stream);

/* Test helper: ONE composition of the shift-only register networks of the NTT kernels (csrc/ntt_network.h: dit_half, dit_level,
 * DitRange, class_fused, leftover_fused, tw_operand) and of the glue that hands words to their first level (csrc/ntt_kernels.h:
 * pre2_combine8, pre2_shift, c8_combine8), instantiated with the template arguments of its call sites.  Thread t loads the block
 * x[q] = d_x[B t + q], q < 32, runs the form and stores x[0 .. 31] back in place; nothing else is written.  B = 32, except for the
 * PRE2 and C8 forms: B = 64 there, the second 32 words of a block being the partner words w (read only; w[q] pairs with x[q]).
 *   form (INV = form & 1 everywhere)       what runs                                                        input contract
 *   NET32   0 + 2 v + INV                  dit_half<0>, dit_half<16>, dit_level<5>; v = 0 lazy, 1 lazy with  lazy: even slots any word,
 *                                          two products per block (WIDE = 2), 2 canonical                   odd slots < p; canonical:
 *   LEVELS  6 + 4 (p2 - 1) + 2 LAZY + INV  dit_level<1> .. dit_level<p2>, p2 = 1 .. 5                       every word < p
 *   TAIL5   26 + INV                       canonical dit_half<0>, dit_half<16>, then the partial ranges     every word < p
 *                                          DitRange<5, Q0, Q0 + 4>, Q0 = 0, 4, 8, 12
 *   LAT     28 + 2 (LOGR - 1) + INV        canonical DitRange<l, 0, 4>, l = 1 .. LOGR <= 3 (slots 0 .. 7)    every word < p
 *   PRE2    34 + 2 half + INV              pre2_combine8 x 4, pre2_shift where half = 1, lazy NET32         x and w < p
 *   C8      38 + 2 half + INV              c8_combine8 x 4, pre2_shift where half = 1, lazy levels 1 .. 5   x and w < p
 * A lazy form leaves words that are only congruent to the elements (the kernels follow it with a Montgomery product); with TF_LAZY = 0
 * every form is canonical.  TF_ERR_INVALID_ARGUMENT -- before any launch -- for an unknown form, a count that is not a multiple of B
 * or above 2^32; a count of 0 is TF_OK. */
enum { TF_NTT_NETWORK_FORM_COUNT = 42 };
int tf_debug_ntt_network_dev(int form, uint64_t *d_x, size_t count, void *stream);
/* The compile-time switches of the loaded library that decide what the forms above compute: TF_LAZY, TF_ASM_BFLY, TF_ASM_POW2 and
 * TF_POW2_WIDE (null pointers are skipped). */
void tf_debug_ntt_network_config(int *lazy, int *asm_bfly, int *asm_pow2, int *pow2_wide);

/* Guard mode for the library's own device memory (debugging aid; process-wide, 0 = off is the default).  Every stream-ordered
 * temporary of the library -- the work areas of every call, the staged descriptors, every input and output buffer of the host-pointer
 * forms -- is taken at ONE place and given back at one place.  With tf_debug_temp_guard(mode), mode 1, 2 or 3, each such block is
 *     [ TF_TEMP_GUARD_WORDS guard words | the request | TF_TEMP_GUARD_WORDS guard words ]
 * and guards AND request are filled on the caller's stream with the mode's poison: 1 zeros, 2 all ones, 3 canonical pseudo-random
 * words (word i of the block, counted from its base, is splitmix64 of i + 0xFE4CE reduced to [1, p - 1]: the sequence of tests/fence.py).
 * When the block is given back, a kernel on the same stream compares both guards with the poison, 32-bit entry by entry (a request that
 * is no multiple of 8 bytes is guarded from the next 4-byte boundary), and records what it finds in a per-device ledger; then the block
 * is freed.  In this mode the scratch between the passes of a multi-pass transform is not taken from its block cache but guarded,
 * checked and freed in the same way.  A kernel that stores past its work area shows in the ledger; a kernel that reads a work word
 * it never wrote computes with the poison, so its result differs between the modes.  With the mode off, taking and giving back a block
 * costs one relaxed atomic load and a branch more than without the feature.  Not covered: memory the library keeps for the life of the
 * process (cached twiddle and power tables, Tip5 constants, a persistent zerofier-tree arena) and its page-locked staging blocks.
 *
 * Every allocation site has a label (a short text; the error message of a failed allocation names it too).  The library counts blocks
 * and bytes REQUESTED per label while the mode is on.
 *   tf_debug_temp_guard_report  waits for the current device, then copies its ledger into ledger[TF_TEMP_GUARD_LEDGER_WORDS]:
 *                               [0] blocks checked, [1] blocks with an offending entry, [2] offending 32-bit entries in total,
 *                               [3] records r that follow (the first 16 offending guards), then per record four words: label id,
 *                               side (0 front, 1 back), offset of the first offending entry relative to the first entry of the request
 *                               (two's complement; negative in the front guard), offending entries of that guard.  *n_labels is the
 *                               number of labels known so far; label_blocks[i] / label_bytes[i], i < min(*n_labels, capacity), are
 *                               the blocks / bytes requested under label i since the last reset.  A block that is still alive -- the
 *                               arena of a zerofier-tree handle -- is counted at once but checked only when it is freed.
 *   tf_debug_temp_guard_reset   waits for the current device, clears its ledger and every label's counters (the label ids stay).
 *   tf_debug_temp_guard_label   the text of label `id` (valid for the life of the process), null for an unknown id.
 *   tf_debug_temp_guard_words   TF_TEMP_GUARD_WORDS as the loaded library was built.
 *   tf_debug_temp_guard_selftest  proves the mechanism: takes one guarded block of n_words words (defect 4: n_words words and four
 *                               bytes) under the label "selftest" (and one word more for the result, same label), runs a one-thread
 *                               kernel with ONE planted defect and frees both.  defect 0: none; 1: a 64-bit store at word -1; 2: at
 *                               word n_words; 3: at word n_words + TF_TEMP_GUARD_WORDS - 1 (the last guard word); 4: a 32-bit store at
 *                               entry 2 n_words + 1, just behind the odd payload; 5: no store, *out_word = word 0 of the block, which
 *                               nobody wrote (else *out_word = 0).  Every store lands in the block's own guards.
 *                               TF_ERR_INVALID_ARGUMENT when the mode is off.
 * tf_debug_force_temp_tables(1) makes every multi-pass transform build its inter-pass twiddle table as a stream-ordered temporary
 * (the route of a table above 2^28 words or over the cache budget) and every scaled inter-pass table of a coset evaluation take the
 * uncached route (that of a fifth coset offset), whatever the caches hold; 0 restores the normal choice.  Results do not depend on it. */
enum { TF_TEMP_GUARD_WORDS = 20480, TF_TEMP_GUARD_LEDGER_WORDS = 68 };
int tf_debug_temp_guard(int mode);
int tf_debug_temp_guard_report(uint64_t *ledger, uint64_t *label_blocks, uint64_t *label_bytes, size_t capacity, size_t *n_labels);
int tf_debug_temp_guard_reset(void);
const char *tf_debug_temp_guard_label(size_t id);
size_t tf_debug_temp_guard_words(void);
int tf_debug_temp_guard_selftest(int defect, size_t n_words, uint64_t *out_word);
int tf_debug_force_temp_tables(int on);

#ifdef __cplusplus
}
#endif
#endif /* TF_HIP_H */
