// tf_internal.h -- what the translation units of libtf_hip.so share on the host side (nothing here is part of the ABI: the
// library is built with -fvisibility=hidden and only the tf_* functions of include/tf_hip.h are exported).
//   tf_plan.hip   the NTT planner (ntt_plan.h): route, passes, radices, tiles and streams of a call -- host logic only, no kernel
//   tf_ntt.hip    device context, table caches, run_ntt(ctx, NttCall, stream) (plan, then execute) and every launcher of ntt_kernels.h
//   tf_lat.hip    the latency-shaped transforms and the one-launch-per-level kernels of the tree walks (lat_kernels.h)
//   tf_tip5.hip   Tip5 / Merkle launchers (tip5_kernels.h), authentication structures
//   tf_poly.hip   the callers on either side of the path, SURVEY 8(f) (poly_kernels.h)
//   tf_abi.hip    host-pointer wrappers and the extern "C" entry points
//   tf_multi.hip  one host-resident batch over several GPUs (tf_*_multi), device selection
//   tf_proof.hip  batched verification of Merkle inclusion proofs (proof_kernels.h)
//   tf_mmr.hip    batched Merkle Mountain Range accumulators and membership proofs (mmr_kernels.h), with their host flavours
//   tf_divide.hip division with remainder and the power-series inverse (divide_kernels.h), with their entry points
//   tf_inverse.hip batch inversion and inverse_or_zero over vectors (inverse_kernels.h), with their host and device flavours
//   tf_algebra.hip add / sub / neg, scalar_mul, scale, formal_derivative, degree and weighted sums of columns (algebra_kernels.h)
//   tf_points.hip get_colinear_y / are_colinear, element-wise mod_pow, geometric sequences and index gathers (points_kernels.h)
//   tf_fri.hip    the FRI split-and-fold of codewords on an evaluation domain, one to many levels per call (fri_kernels.h)
//   tf_scan.hip   prefix scans along the columns of a table: running sums, products and the affine recurrence (scan_kernels.h)
//   tf_deep.hip   the DEEP quotient of the extended tables: whole codewords and sampled rows (deep_kernels.h)
//   tf_table.hip  tables between the column-major and the row-major layout: transpose, row gather, row-major LDE (table_kernels.h)
//   tf_merkle_open.hip authentication structures and roots straight from the leafs: the root-only sweep with the wanted nodes copied out
//   tf_temp_guard.hip the guard mode for all of the above's device temporaries (tf_debug_temp_guard): guards, poison, ledger, self-test
//   tf_temp.h     (header, included by the units above) DevTemp, the one owner of a stream-ordered temporary; the staged upload, the
//                 per-unit Tip5 constants upload and the host round trip that every unit used to spell out for itself
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <set>
#include <string>
#include <vector>

#pragma GCC visibility push(default)
#include "../../include/tf_hip.h"
#pragma GCC visibility pop
#include "gl64.h"
#include "ntt_args.h"
#include "ntt_plan.h"
#include "tf_guard.h"

namespace tfi {

using gl::u32;
using gl::u64;

// ------------------------------------------------------------------------------------ errors
extern thread_local std::string t_last_error;
int hip_fail(hipError_t e, const char* what, const char* file, int line);
#define HIPCHK(call)                                                        \
    do {                                                                    \
        hipError_t e_ = (call);                                             \
        if (e_ != hipSuccess) return hip_fail(e_, #call, __FILE__, __LINE__); \
    } while (0)

#define TRY(x)            \
    do {                  \
        int rc_ = (x);    \
        if (rc_) return rc_; \
    } while (0)

// The library has ONE plan and one set of kernels (the variants that lost their measurements are listed in DESIGN_HISTORY.md, with
// their records under profiles/).  It reads exactly two environment variables, both deployment settings: TF_NTT_TILE_BYTES (scratch
// budget between the passes) and TF_NTT_PIPE (side streams for pipelined batch tiles).

u64 root_of_unity_mont(int log_n);

// ------------------------------------------------------------------------------------ per-device context
struct DeviceCtx {
    std::mutex mu;
    std::map<u64, u64*> tables;           // twiddle tables, never freed while the process lives
    std::map<std::pair<u64, u64>, u64*> pow_tables;  // (offset_raw, n) -> offset^j table
    std::map<std::pair<u64, u64>, u64*> scaled_post;  // (offset_raw, log_m << 8 | a) -> T[k B + b] * offset^b (get_scaled_post_table)
    size_t cached_scaled_post_bytes = 0;
    bool tip5_ready = false;               // guarded by mu
    std::atomic<bool> pool_ready{false};  // double-checked under mu
    hipMemPool_t pool = nullptr;           // the library's stream-ordered temporaries (current_ctx); written once before pool_ready
    hipStream_t side[4] = {nullptr, nullptr, nullptr, nullptr};  // pipelined tiles (run_ntt); created on first use under mu
    struct ScratchBlock {
        u64* p = nullptr;
        size_t bytes = 0;
        hipEvent_t ready = nullptr;  // recorded on the last user's stream when it gave the block back
    };
    std::vector<ScratchBlock> scratch_free;  // work space of the multi-pass transforms (guarded by mu), see scratch_acquire
    size_t scratch_bytes = 0;                // bytes held by blocks in scratch_free
    size_t cached_post_bytes = 0;          // inter-pass twiddle tables kept for the life of the process (guarded by mu)
    size_t cached_pow_bytes = 0;           // coset power tables kept for the life of the process (guarded by mu)
};

constexpr int kMaxDevices = 64;
extern DeviceCtx g_ctx[kMaxDevices];

// ------------------------------------------------------------------------------------ tf_plan.hip
// the planner's functions: ntt_plan.h.  Configuration (tf_set_* hooks of the ABI; the two TF_NTT_* settings read once by read_env):
constexpr int kMaxPipe = 4;
void read_env();
extern size_t g_tile_bytes;
extern std::atomic<int> g_pipe, g_min_passes, g_lat_mode, g_pre2_mode, g_small_launch_mode;

// ------------------------------------------------------------------------------------ tf_ntt.hip
int current_ctx(DeviceCtx** out);
int device_cus();  // compute units of the calling thread's CURRENT device (cached per device; 256 if the runtime will not say)
// every stream-ordered temporary of the library, taken through DevTemp (tf_temp.h) and given back with pool_free_async on the same
// stream; `what` is the site's label: the error text names it, and the guard mode (tf_debug_temp_guard) counts and reports under it
hipError_t pool_malloc_async(void** p, size_t bytes, hipStream_t stream, const char* what);
hipError_t pool_free_async(void* p, hipStream_t stream);
// (in guard mode the block is a guarded pool block under the label `what`, and the cache is bypassed: ready stays null)
int scratch_acquire(DeviceCtx* ctx, size_t bytes, hipStream_t stream, DeviceCtx::ScratchBlock* out, const char* what);
void scratch_release(DeviceCtx* ctx, DeviceCtx::ScratchBlock blk, hipStream_t stream);
int release_caches(DeviceCtx* ctx);
// tf_temp_guard.hip: the guard mode's state (low 8 bits the mode, above them the guarded blocks alive; zero: nothing to do anywhere),
// the two slow paths behind it, and the switch of tf_debug_force_temp_tables
extern std::atomic<unsigned long long> g_temp_guard_state;
extern std::atomic<int> g_force_temp_tables;
hipError_t temp_guard_malloc(void** p, size_t bytes, hipStream_t stream, const char* what, hipMemPool_t pool, int dev, int mode);
hipError_t temp_guard_free(void* p, hipStream_t stream);
int temp_guard_set_mode(int mode);  // the bodies of the tf_debug_temp_guard* entry points (tf_abi.hip)
int force_temp_tables(int on);
int temp_guard_reset();
int temp_guard_report(uint64_t* ledger, uint64_t* label_blocks, uint64_t* label_bytes, size_t capacity, size_t* n_labels);
const char* temp_guard_label(size_t id);
int temp_guard_selftest(int defect, size_t n_words, uint64_t* out_word);
int ensure_dynamic_lds(const void* fn, int bytes, std::atomic<unsigned long long>& done_mask);
// offset^j tables of the coset transforms, owned for the scope of the call that reads them (in the style of DevTemp, tf_temp.h).
// cosets = 1: table[j] = offset^j, j < n.  cosets = C > 1 (the blown-up coset evaluation, NttCall::cosets; C <= kMaxCosetSplit): C
// tables back to back, table[c * n + j] = (offset * w^c)^j with w the root of unity of order 2^log_order.  At most 16 tables /
// kPowCacheBudget bytes (tf_ntt.hip) per device stay cached for the life of the process; a table beyond that is a block of the scratch cache, private to this
// owner, which release() -- or the destructor, on any early return -- hands back on the stream behind the launches enqueued so far.
class PowTable {
   public:
    PowTable(DeviceCtx* ctx, hipStream_t stream) : ctx_(ctx), s_(stream) {}
    PowTable(const PowTable&) = delete;
    PowTable& operator=(const PowTable&) = delete;
    ~PowTable() { release(); }
    int acquire(u64 offset_raw, size_t n, size_t cosets = 1, int log_order = 0);
    const u64* get() const { return table_; }
    void release() {  // (a cached table holds no block: nothing goes back)
        scratch_release(ctx_, blk_, s_);
        blk_ = DeviceCtx::ScratchBlock{}, table_ = nullptr;
    }

   private:
    DeviceCtx* ctx_;
    hipStream_t s_;
    const u64* table_ = nullptr;
    DeviceCtx::ScratchBlock blk_;  // the temporary's block; empty for a cached table
};

// keys of DeviceCtx::tables
enum : u64 { TAG_INNER = 1, TAG_POST = 2, TAG_TINY = 3, TAG_BLOCK1 = 4, TAG_BLOCK2 = 5, TAG_LAT = 6 };
inline u64 make_key(u64 tag, u64 a, u64 b, u64 c, u64 d) { return (tag << 56) | (a << 40) | (b << 24) | (c << 8) | d; }
int upload_table(const std::vector<u64>& host, u64** dev);
class DevTemp;  // tf_temp.h
// (a table too large to cache is a stream-ordered temporary: *own takes it and gives it back after the passes that read it)
int get_post_table(DeviceCtx* ctx, int log_m, int a, bool inverse, hipStream_t stream, const u64** out, DevTemp* own);

int check_len(size_t n);
// One transform call: the operands and the shape, and nothing about where or how it runs.  The constructor takes what every call
// has; the optional operands are set by name.
struct NttCall {
    const u64* in;  // device pointers; in == out for ntt / intt, distinct for a coset evaluation
    u64* out;
    size_t n, batch;  // points per transform, transforms
    int L;            // words per element (1 BFieldElement, 3 XFieldElement)
    bool inverse;
    long long in_bs = 0, out_bs = 0;  // words between the polynomials of the batch; 0: packed, n * L words (with_strides)
    long long n_coeffs = -1;          // >= 0: rows >= n_coeffs of the input read as zero (the zero padding of a forward transform)
    // >= 0 (only with can_truncate(n, L)): the last pass stores output elements j < n_out only and out_bs may be n_out * L -- the
    // truncation of fast_multiply without a copy; `in` is then used as work space and CLOBBERED
    long long n_out = -1;
    const u64* pre_scale = nullptr;   // coefficient j is multiplied by pre_scale[j] on load (coset evaluation: a PowTable)
    const u64* post_scale = nullptr;  // output j is multiplied by post_scale[j] on store (coset interpolation; inverse only)
    const u64* in2 = nullptr;         // the pointwise product in[j] * in2[j] is what is transformed (batch stride in_bs as well)
    const u64* coset_offset = nullptr;  // host pointer to the offset behind pre_scale, for the table with offset^b folded in (c8)
    // C > 1 (forward coset evaluation only, n > 1024): the output has C * n points per polynomial, out[j * C + c] = (transform of
    // the coefficients scaled by pre_scale[c * n_coeffs + .])[j] -- the evaluation on the coset of order C * n done as C transforms
    // of length n whose outputs interleave (w_{Cn}^(jC + c) = w_{Cn}^c * w_n^j).  The first pass reads the coefficients once per c
    // and writes rows (k_1, c); from there on it is the ordinary plan with N_1 * C rows.
    size_t cosets = 1;
    NttCall(const u64* in_, u64* out_, size_t n_, size_t batch_, int L_, bool inverse_) : in(in_), out(out_), n(n_), batch(batch_), L(L_), inverse(inverse_) {}
};
// the forward transform of `n_coeffs` coefficients per polynomial (packed) zero padded to n points
inline NttCall ntt_of_coeffs(const u64* in, size_t n_coeffs, u64* out, size_t n, size_t batch, int L) {
    NttCall c(in, out, n, batch, L, false);
    c.in_bs = (long long)n_coeffs * L, c.n_coeffs = (long long)n_coeffs;
    return c;
}
// the ONE reading of "0 means packed": run_ntt, shape_of and the launchers called directly (tf_lat.hip) take their strides through it
inline NttCall with_strides(NttCall c) {
    if (!c.in_bs) c.in_bs = (long long)c.n * c.L;
    if (!c.out_bs) c.out_bs = (long long)c.n * c.L;
    return c;
}
NttShape shape_of(const NttCall& c);  // what the planner sees of a call
int run_ntt(DeviceCtx* ctx, const NttCall& c, hipStream_t stream);
int ntt_dev(u64* d_x, size_t n, size_t batch, int L, int inverse, void* stream);
int coset_eval_dev(const u64* d_coeffs, size_t n_coeffs, u64 offset_raw, u64* d_out, size_t order, size_t batch, int L, void* stream);
// ------------------------------------------------------------------------------------ tf_lat.hip
// latency-shaped transforms (mods: the tree walks' load / store modifiers) and the one-launch-per-level kernels of the tree walks
int launch_lat2(DeviceCtx* ctx, const NttCall& c, hipStream_t stream);
int launch_lat(DeviceCtx* ctx, const NttCall& c, hipStream_t stream, const tfk::NttLatArgs* mods = nullptr);
int get_lat_table(DeviceCtx* ctx, int log_n, bool inverse, const u64** out, int scale_log);  // (scale_log < 0: log_n)
bool tree_level_wanted(long long order, long long lines, int L = 1, bool up = false);
template <bool UP>
int launch_tree_level(DeviceCtx* ctx, int log_n, tfk::TreeLevelArgs a, hipStream_t s, int L = 1);
bool tree_build_level_wanted(long long order, long long parents);
int launch_tree_build_level(DeviceCtx* ctx, int log_n2, tfk::TreeBuildArgs a, hipStream_t s);

// ------------------------------------------------------------------------------------ tf_tip5.hip
int check_leaves(size_t n);
int tip5_permute_dev(u64* d_states, size_t count, void* stream);
int tip5_trace_dev(u64* d_states, u64* d_trace, size_t count, void* stream);
int tip5_hash_pairs_dev(const u64* d_in, u64* d_out, size_t count, void* stream);
int tip5_hash_varlen_rows_dev(const u64* d_rows, size_t row_len, size_t n_rows, u64* d_out, void* stream);
int hash_table_rows_dev(const u64* d_table, size_t n_rows, size_t n_cols, int width, size_t col_stride, u64* d_digests, size_t batch, void* stream);
int merkle_build_dev(const u64* d_leaves, size_t n, u64* d_nodes, size_t batch, void* stream);
int merkle_subtree_host(const u64* leaves_sub, size_t m, u64* nodes_tree, size_t n_sub, size_t sub, u64* root_out);  // tf_abi.hip
int merkle_root_dev(const u64* d_leaves, size_t n, u64* d_root, size_t batch, void* stream);
int merkle_from_rows_dev(const u64* d_rows, size_t row_len, size_t n_rows, u64* d_nodes, size_t batch, void* stream);
int merkle_from_columns_dev(const u64* d_table, size_t n_rows, size_t n_cols, int width, size_t col_stride, u64* d_nodes, size_t batch, void* stream);
int gather_digests_dev(const u64* d_nodes, const unsigned long long* d_idx, size_t count, u64* d_out, hipStream_t s);
// the pieces of the level sweeps, for the unit that runs one of its own (tf_merkle_open.hip); tf_tip5.hip documents them
int ensure_tip5(DeviceCtx* ctx);
int launch_hash_pairs(const u64* in, u64* out, u64* leaf_copy, long long count, long long per_tree, long long in_ts, long long out_ts, long long copy_ts,
                      hipStream_t s);
int merkle_narrow_levels(const u64* level, long long in_ts, long long w, u64* d_nodes, long long nodes_ts, u64* d_root, u64* scratch, size_t batch,
                         bool copy_input, hipStream_t s);
bool merkle_narrow_from(long long w, size_t batch);  // narrow_from: the level of w nodes per tree and all above it go to merkle_narrow_levels
// tf_debug_field_op_dev: one kernel per op, all instantiated in tf_tip5.hip -- the unit that sees the fold tails of tip5_kernels.h next
// to gl64.h, and a code object of its own: the ABI unit's (which every caller loads with its first fill_random) stays as it was.
// A thread runs one block of the primitive on W = field_op_width(op) consecutive elements.
constexpr int field_op_width(int op) {
    return op == TF_FIELD_OP_ADD_SUB2 || op == TF_FIELD_OP_ADD_SUB_LAZY2 || op == TF_FIELD_OP_MONT_MUL2 || op == TF_FIELD_OP_MX_FOLD2 ? 2
           : op == TF_FIELD_OP_MONT_MUL3                                                                                             ? 3
           : op == TF_FIELD_OP_ADD_LAZY4 || op == TF_FIELD_OP_SUB_LAZY4 || op == TF_FIELD_OP_MONT_MUL4 || op == TF_FIELD_OP_MX_FOLD4_CANON ||
                   op == TF_FIELD_OP_MX_FOLD4_LAZY
               ? 4
               : 1;
}
constexpr bool field_op_two_outputs(int op) { return op == TF_FIELD_OP_ADD_SUB || op == TF_FIELD_OP_ADD_SUB2 || op == TF_FIELD_OP_ADD_SUB_LAZY2; }
void debug_field_op_dev(int op, const u64* d_a, const u64* d_b, u64* d_out0, u64* d_out1, size_t count, hipStream_t s);
// tf_debug_ntt_network_dev / _config: the forms are instantiated in tf_ntt.hip, the unit that sees ntt_kernels.h and its switches
int debug_ntt_network_words(int form);  // words per block of the form: 32, or 64 for the forms with a partner block
void debug_ntt_network_dev(int form, u64* d_x, size_t count, hipStream_t s);
void debug_ntt_network_config(int* lazy, int* asm_bfly, int* asm_pow2, int* pow2_wide);
extern const u64 kRoundConstants[80];  // ROUND_CONSTANTS, tip5/mod.rs:68-149 (canonical values; tf_tip5.hip)
// the planner's rules for a launch of `count` permutation chains (tf_tip5.hip has the measurements behind them)
constexpr long long kCoopMaxCount = 1ll << 13;
static_assert(kCoopMaxCount >= 64 && (kCoopMaxCount & (kCoopMaxCount - 1)) == 0, "a power of two: the level at which a tree narrows is found by halving");

// Round 6: a launch of at most 8 permutation chains per compute unit leaves half the chip's 16-lane rows idle; it runs every chain on a row
// PAIR instead (tip5_permutation_coop2: the circulant's sixteen rotation terms split over the two rows; 2.01 -> 1.68 us per permutation,
// profiles/r06_microbench_coop2.txt).  A workgroup then holds 8 chains, so up to this count every workgroup still has a CU of its own.
inline bool coop_two_rows(long long chains) {
    return chains <= 8ll * device_cus();
}
// grid of a matrix-pipe launch: one workgroup (4 waves x 16 permutations) per 64 items, capped at kMxBlocksPerCu per CU -- beyond
// that the waves walk the items with a grid stride, so the tables are staged once per wave and not once per 16 items (8 workgroups
// are resident per CU at the kernels' VGPR count; 56 keeps the hardware's dynamic balancing: measured 7 / 14 / 28 / 56 / no cap on
// the 2^24-leaf tree: 4.87 / 5.00 / 5.06 / 5.07 / 5.06 G leaves/s, profiles/r05_tip5_grid_cap.txt)
constexpr long long kMxBlocksPerCu = 56;
inline unsigned mx_blocks(long long count) {
    const long long cap = (long long)device_cus() * kMxBlocksPerCu;
    const long long want = (count + 63) / 64;
    return (unsigned)(want < cap ? want : cap);
}

// ------------------------------------------------------------------------------------ tf_proof.hip
// page-locked staging for descriptors built on the host (shared with tf_mmr.hip): stage_acquire hands out a block of at least `bytes`
// whose last copy has completed; stage_release takes it back once the copy that reads it is enqueued on `s`
struct Staging {
    void* p = nullptr;
    size_t bytes = 0;
    hipEvent_t done = nullptr;
};
int stage_acquire(int dev, size_t bytes, Staging* out);
void stage_release(int dev, Staging st, hipStream_t s);
// batched MerkleTreeInclusionProof::try_verify (paths = false) / into_authentication_paths (paths = true); the leaf and structure
// arrays are indexed from leaf_base / auth_base (the host flavours upload only [offsets[0], offsets[n]))
int merkle_proofs_dev(const uint32_t* heights, size_t n, const uint64_t* leaf_offsets, const u64* d_leaf_indices, const u64* d_leaf_digests,
                      const uint64_t* auth_offsets, const u64* d_auth, const u64* d_roots, int* d_statuses, u64* d_paths, bool paths,
                      uint64_t leaf_base, uint64_t auth_base, hipStream_t s);

// ------------------------------------------------------------------------------------ tf_mmr.hip
// the MMR calls of include/tf_hip.h: _dev forms (path arrays indexed from mbase / pbase / path_base, as merkle_proofs_dev) and host forms
int mmr_append_dev(u64 n, const u64* old_peaks, const u64* leafs, size_t k, u64* new_peaks, u64* proofs, hipStream_t s);
int mmr_append_host(u64 n, const u64* old_peaks, const u64* leafs, size_t k, u64* new_peaks, u64* proofs);
int mmr_bag_peaks_dev(const uint64_t* leaf_counts, size_t n_acc, const u64* peaks, u64* out, hipStream_t s);
int mmr_bag_peaks_host(const uint64_t* leaf_counts, size_t n_acc, const u64* peaks, u64* out);
int mmr_verify_dev(u64 leaf_count, const u64* peaks, size_t n_peaks, size_t n, const u64* idx, const u64* digests, const uint64_t* offsets,
                   const u64* paths, int* statuses, uint64_t path_base, hipStream_t s);
int mmr_verify_host(u64 leaf_count, const u64* peaks, size_t n_peaks, size_t n, const u64* idx, const u64* digests, const uint64_t* offsets,
                    const u64* paths, int* statuses);
int mmr_mutate_dev(u64 leaf_count, u64* peaks, size_t M, const uint64_t* midx, const u64* leafs, const uint64_t* moff, const u64* mpaths, size_t P,
                   const uint64_t* pidx, const uint64_t* poff, u64* ppaths, int* modified, uint64_t mbase, uint64_t pbase, hipStream_t s);
int mmr_mutate_host(u64 leaf_count, u64* peaks, size_t M, const uint64_t* midx, const u64* leafs, const uint64_t* moff, const u64* mpaths, size_t P,
                    const uint64_t* pidx, const uint64_t* poff, u64* ppaths, int* modified);
// successor proofs and membership proofs under appends: the same level sweep as mmr_append_dev with other digests taken from it
size_t mmr_successor_proof_len(u64 n, u64 k);
int mmr_successor_new_dev(u64 n, const u64* old_peaks, const u64* leafs, size_t k, u64* paths_out, u64* new_peaks, hipStream_t s);
int mmr_successor_new_host(u64 n, const u64* old_peaks, const u64* leafs, size_t k, u64* paths_out, u64* new_peaks);
int mmr_successor_verify_dev(size_t P, const uint64_t* old_counts, const uint64_t* new_counts, const uint64_t* old_off, const u64* old_peaks,
                             const uint64_t* new_off, const u64* new_peaks, const uint64_t* path_off, const u64* paths, int* statuses, uint64_t old_base,
                             uint64_t new_base, uint64_t path_base, hipStream_t s);
int mmr_successor_verify_host(size_t P, const uint64_t* old_counts, const uint64_t* new_counts, const uint64_t* old_off, const u64* old_peaks,
                              const uint64_t* new_off, const u64* new_peaks, const uint64_t* path_off, const u64* paths, int* statuses);
int mmr_update_proofs_dev(u64 n, const u64* old_peaks, const u64* leafs, size_t k, size_t P, const uint64_t* own_idx, const uint64_t* own_off,
                          const u64* own_paths, uint64_t* out_off, u64* out_paths, size_t capacity, int* modified, u64* new_peaks, uint64_t own_base,
                          hipStream_t s);
int mmr_update_proofs_host(u64 n, const u64* old_peaks, const u64* leafs, size_t k, size_t P, const uint64_t* own_idx, const uint64_t* own_off,
                           const u64* own_paths, uint64_t* out_off, u64* out_paths, size_t capacity, int* modified, u64* new_peaks);

// ------------------------------------------------------------------------------------ tf_merkle_open.hip
// authentication structure and roots of `batch` trees from their leafs (include/tf_hip.h has the contract): _dev takes device
// pointers and HOST leaf indices and never waits for its stream, _host takes host pointers; the work-space rule is pure host arithmetic
int merkle_open_dev(const u64* d_leafs, size_t n, size_t batch, const uint64_t* leaf_indices, size_t k, u64* d_out, size_t capacity, size_t* out_count,
                    u64* d_roots, hipStream_t s);
int merkle_open_host(const u64* leafs, size_t n, size_t batch, const uint64_t* leaf_indices, size_t k, u64* out, size_t capacity, size_t* out_count,
                     u64* roots);
size_t merkle_open_workspace(size_t n, size_t batch, size_t k_nodes);
// the same with the leaf indices in DEVICE memory (n_lists lists of k u32): the plan is made by a kernel, nothing is read back, and
// what depends on the indices goes to *d_status.  merkle_plan_max_nodes bounds a list's structure nodes (host arithmetic).
size_t merkle_plan_max_nodes(size_t n, size_t k);
int merkle_plan_dev(size_t n, const uint32_t* d_leaf_indices, size_t k, size_t n_lists, uint32_t* d_node_indices, size_t capacity, uint32_t* d_counts,
                    uint32_t* d_level_ends, hipStream_t s, int* d_status);
int merkle_nodes_sampled_dev(const u64* d_nodes, size_t n, const uint32_t* d_leaf_indices, size_t k, size_t n_lists, size_t trees_per_list,
                             u64* d_out, size_t capacity, uint32_t* d_counts, hipStream_t s, int* d_status);
int merkle_open_sampled_dev(const u64* d_leafs, size_t n, const uint32_t* d_leaf_indices, size_t k, size_t n_lists, size_t trees_per_list,
                            u64* d_out, size_t capacity, uint32_t* d_counts, u64* d_roots, hipStream_t s, int* d_status);
size_t merkle_open_sampled_workspace(size_t n, size_t trees, size_t k, size_t n_lists);

// ------------------------------------------------------------------------------------ tf_sponge.hip
// the sponge calls of include/tf_hip.h.  absorb: pad = false, len = 10 n_chunks, no offsets; pad_and_absorb_all: pad = true (the _dev
// form indexes `in` from in_base, as merkle_proofs_dev).  squeeze: per_sponge = n_squeezes, words_each = 10; sample_scalars:
// per_sponge = num_elements, words_each = 3.
int sponge_init_dev(u64* states, size_t count, int fixed_length, hipStream_t s);
int sponge_init_host(u64* states, size_t count, int fixed_length);
int sponge_absorb_dev(u64* states, size_t count, const u64* in, size_t len, const uint64_t* offsets, bool pad, uint64_t in_base, hipStream_t s);
int sponge_absorb_host(u64* states, size_t count, const u64* in, size_t len, const uint64_t* offsets, bool pad);
int sponge_squeeze_dev(u64* states, size_t count, size_t per_sponge, size_t words_each, u64* out, hipStream_t s);
int sponge_squeeze_host(u64* states, size_t count, size_t per_sponge, size_t words_each, u64* out);
int sponge_indices_dev(u64* states, size_t count, uint32_t upper_bound, size_t num, uint32_t* out, hipStream_t s);
int sponge_indices_host(u64* states, size_t count, uint32_t upper_bound, size_t num, uint32_t* out);

// ------------------------------------------------------------------------------------ tf_abi.hip
// the host-pointer entry points' plumbing: h2d waits for its upload (pageable host memory), d2h and sync do not / do
hipStream_t host_stream();
int h2d(u64* d, const u64* h, size_t words, hipStream_t s);
int d2h(u64* h, const u64* d, size_t words, hipStream_t s);
int sync(hipStream_t s);

// ------------------------------------------------------------------------------------ tf_divide.hip
// division with remainder of `batch` dividends over one divisor, and the power-series inverse (include/tf_hip.h has the contract);
// the _dev flavours take device pointers and a status word (may be null), the _host flavours host pointers
int divide_dev(const u64* a, size_t na, size_t batch, const u64* b, size_t nb, u64* q, u64* r, void* stream, int* status, int L);
int divide_host(const u64* a, size_t na, size_t batch, const u64* b, size_t nb, u64* q, u64* r, int L);
size_t fps_len(size_t nf, size_t precision);
int fps_dev(const u64* f, size_t nf, size_t precision, u64* out, void* stream, int* status, int L);
int fps_host(const u64* f, size_t nf, size_t precision, u64* out, int L);

// ------------------------------------------------------------------------------------ tf_inverse.hip
// FiniteField::batch_inversion (or_zero = false) / inverse_or_zero (or_zero = true) of n elements of L words (include/tf_hip.h has the
// contract); _dev: device pointers, d_status as the _dev_async entry points (null: a blocking check of a flag word), _host: host pointers
int batch_inverse_dev(const u64* in, size_t n, u64* out, int L, bool or_zero, void* stream, int* d_status);
int batch_inverse_host(const u64* in, size_t n, u64* out, int L, bool or_zero);

// ------------------------------------------------------------------------------------ tf_algebra.hip
// the plain polynomial arithmetic of include/tf_hip.h ("Polynomial arithmetic"): host = false takes device pointers and only
// enqueues on `stream`, host = true takes host pointers and blocks.  Lengths count coefficients of `width` words.
int poly_addsub(const u64* a, size_t na, const u64* b, size_t nb, int width, u64* out, size_t batch, bool sub, bool host, void* stream);
int poly_neg(const u64* a, size_t na, int width, u64* out, size_t batch, bool host, void* stream);
int poly_scalar_mul(const u64* a, size_t na, int width_a, const u64* scalar, int width_s, u64* out, size_t batch, bool scale, bool host, void* stream);
int poly_derivative(const u64* a, size_t na, int width, u64* out, size_t batch, bool host, void* stream);
int poly_degree(const u64* a, size_t na, int width, size_t batch, long long* degrees, bool host, void* stream);
int hadamard_xfe_bfe_dev(const u64* a, const u64* b, u64* out, size_t count, void* stream);
int poly_lincomb(const u64* polys, size_t n, int width_p, size_t stride, size_t k, const u64* weights, int width_w, u64* out, bool host, void* stream);

// ------------------------------------------------------------------------------------ tf_points.hip
// the point, power and gather calls of include/tf_hip.h ("Points, powers and gathers"): host = false takes device pointers and only
// enqueues on `stream`, host = true takes host pointers and blocks.  Lengths count elements of `width` words.
int get_colinear_y(const u64* x0, const u64* y0, const u64* x1, const u64* y1, size_t n, const u64* p2x, size_t n_p2x, int wx, int wy, u64* out,
                   bool host, void* stream, int* d_status);
int are_colinear(const u64* xs, const u64* ys, size_t n_groups, size_t k, int wx, int wy, int* flags, bool host, void* stream);
int mod_pow(const u64* bases, size_t n_bases, const uint64_t* exps, size_t n_exps, int width, u64* out, size_t n, bool host, void* stream);
int powers(const u64* first, const u64* ratio, int width, u64* out, size_t n, bool host, void* stream);
int gather_elements_dev(const u64* src, size_t src_len, int width, const uint32_t* indices, size_t n, u64* out, void* stream, int* d_status);

// ------------------------------------------------------------------------------------ tf_fri.hip
// the fold of include/tf_hip.h ("FRI folding"): host = false takes device pointers and only enqueues on `stream`, host = true takes
// host pointers and blocks; the work-space rule and the plan of passes are pure host arithmetic (the plan: passes, or minus a status)
int fri_fold(const u64* codewords, size_t n, size_t batch, int wc, u64 offset_raw, const u64* challenges, size_t levels, size_t n_sets, int wa, u64* out,
             bool host, void* stream);
size_t fri_fold_workspace(size_t n, size_t batch, int wc, int wa, size_t levels);
int fri_fold_plan(size_t n, size_t levels, int wc, int wa, int* levels_per_pass, int capacity);

// ------------------------------------------------------------------------------------ tf_scan.hip
// the scans of include/tf_hip.h ("Prefix scans"): device pointers, only enqueues on `stream`, the work space is the caller's.  mode is
// TF_SCAN_*: a sum reads `b` alone, a product `a` alone (one multiplier per row); an affine call with a_len == 1 takes a_sets packed
// multipliers.  The work-space rule and the plan are pure host arithmetic (the plan: launches, or minus a status)
int scan_dev(int mode, const u64* a, size_t a_len, size_t a_sets, int wa, size_t stride_a, const u64* b, int wb, size_t stride_b, size_t n, size_t batch,
             const u64* init, size_t n_init, u64* out, size_t stride_out, void* d_work, size_t work_bytes, void* stream);
size_t scan_workspace(int mode, size_t n, size_t batch, int w);
int scan_plan(int mode, size_t n, size_t batch, int w, int* info, int capacity);

// ------------------------------------------------------------------------------------ tf_deep.hip
// the DEEP quotients of include/tf_hip.h ("DEEP quotients"): device pointers, only enqueues on `stream`, the work space is the caller's;
// the work-space rule and the plan are pure host arithmetic (the plan: launches, or minus a status)
int deep_quotient_dev(const u64* d_main, size_t k1, size_t stride_main, const u64* d_aux, size_t k3, size_t stride_aux, size_t n, u64 offset_raw,
                      const u64* d_points, size_t n_points, const u64* d_weights, const u64* d_values, u64* d_out, void* d_work, size_t work_bytes,
                      void* stream, int* d_status);
size_t deep_quotient_workspace(size_t n, size_t k1, size_t k3, size_t n_points);
int deep_quotient_plan(size_t n, size_t k1, size_t k3, size_t n_points, int* fields, int capacity);
int deep_quotient_rows_dev(const u64* d_main_rows, size_t k1, size_t row_stride_main, const u64* d_aux_rows, size_t k3, size_t row_stride_aux, size_t n,
                           u64 offset_raw, const uint32_t* d_indices, size_t n_rows, const u64* d_points, size_t n_points, const u64* d_weights,
                           const u64* d_values, u64* d_out, void* stream, int* d_status);

// ------------------------------------------------------------------------------------ tf_table.hip
// the table calls of include/tf_hip.h ("Tables"): host = false takes device pointers and only enqueues on `stream`, host = true
// takes host pointers and blocks.  Strides count words, the other lengths elements of `width` words.
int table_transpose(const u64* src, size_t n_outer, size_t n_inner, int width, size_t src_stride, u64* dst, size_t dst_stride, size_t batch, bool host,
                    void* stream);
int table_gather_rows(const u64* table, int layout, size_t n_rows, size_t n_cols, int width, size_t stride, const uint32_t* indices, size_t k, u64* out,
                      size_t out_stride, size_t batch, bool host, void* stream, int* d_status);
int table_lde_rows_dev(const u64* rows, size_t n, size_t n_cols, size_t row_stride_in, u64 offset_in, u64* out, size_t m, size_t row_stride_out,
                       u64 offset_out, size_t cols_per_block, int width, void* stream);
size_t table_lde_rows_workspace(size_t n, size_t m, size_t n_cols, int width, size_t cols_per_block);

// ------------------------------------------------------------------------------------ tf_poly.hip
extern std::atomic<int> g_batch_eval_route;
int coset_interp_dev(const u64* d_values, size_t n, u64 offset_raw, u64* d_out, size_t batch, int L, void* stream);
int hadamard_dev(const u64* a, const u64* b, u64* out, size_t count, int L, void* stream);
int poly_mul_dev(const u64* a, size_t na, const u64* b, size_t nb, u64* out, size_t batch, int L, void* stream, long long a_bs = 0, long long b_bs = 0);
int poly_mul_shared_dev(const u64* a, size_t na, size_t batch, const u64* b, size_t nb, u64* out, int L, void* stream);
int poly_square_dev(const u64* a, size_t na, u64* out, size_t batch, int L, void* stream);
int lde_dev(const u64* values, size_t n, u64 offset_in, u64* out, size_t m, u64 offset_out, size_t batch, int L, void* stream);
bool tree_route(size_t n_coeffs, size_t n_points, size_t batch, int L);
int batch_evaluate_horner(const u64* coeffs, size_t n_coeffs, size_t poly_stride, size_t batch, const u64* points, size_t n_points, u64* out, int L,
                          void* stream, int CL);
int batch_evaluate_dev(const u64* coeffs, size_t n_coeffs, size_t poly_stride, size_t batch, const u64* points, size_t n_points, u64* out, int L,
                       void* stream);
int coset_extrapolate_dev(u64 offset_raw, const u64* codewords, size_t n, size_t batch, const u64* points, size_t n_points, u64* out, int L, void* stream);
int zerofier_dev(const u64* roots, size_t n_roots, u64* out, int L, void* stream);
int interpolate_dev(const u64* domain, const u64* values, size_t n, size_t rows, u64* out, int L, void* stream, int* d_status = nullptr);
int clean_divide_dev(const u64* a, size_t na, const u64* b, size_t nb, u64* out, void* stream, size_t batch = 1, int* d_status = nullptr);
int coset_eval_xoffset_dev(const u64* d_coeffs, size_t n_coeffs, const u64 offset[3], u64* d_out, size_t order, size_t batch, void* stream);
int coset_interp_xoffset_dev(const u64* d_values, size_t n, const u64 offset[3], u64* d_out, size_t batch, void* stream);
int barycentric_dev(const u64* codewords, size_t n, size_t batch, int cw_width, const u64 x[3], u64* out, void* stream);
int auth_structure_indices(size_t num_leafs, const uint64_t* leaf_indices, size_t k, std::vector<unsigned long long>* out);
struct TreeHandle;  // a zerofier tree that outlives the call (math/zerofier_tree.rs), opaque outside tf_poly.hip
int tree_handle_new(const u64* d_domain, size_t n, int L, void* stream, TreeHandle** out, bool async = false);
void tree_handle_free(TreeHandle* H);
size_t tree_handle_num_points(const TreeHandle* H);
int tree_handle_width(const TreeHandle* H);
int tree_handle_zerofier(const TreeHandle* H, u64* d_out, void* stream);
int tree_handle_batch_evaluate(const TreeHandle* H, const u64* d_coeffs, size_t n_coeffs, size_t batch, u64* d_out, void* stream);
int tree_handle_interpolate(TreeHandle* H, const u64* d_values, size_t rows, u64* d_out, void* stream, int* d_status = nullptr);


}  // namespace tfi
