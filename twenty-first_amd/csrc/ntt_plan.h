// ntt_plan.h -- what one transform call looks like to the planner (NttShape) and what the planner decides for it (NttPlan).
// plan_ntt (tf_plan.hip) is pure host logic: no HIP call, no device context, no lock, no heap.  run_ntt (tf_ntt.hip) plans a call
// once and executes the plan; the introspection calls of the ABI (tf_ntt_plan, tf_ntt_launch_count), can_truncate and the coset-split
// rule of fast_coset_evaluate read the same plan.
#pragma once
#include <cstddef>

namespace tfi {

// Everything the decision depends on, and no pointer.
struct NttShape {
    size_t n = 0, batch = 0;  // points per transform, transforms
    int L = 1;                // words per element (1 BFieldElement, 3 XFieldElement)
    bool inverse = false;
    size_t cosets = 1;        // > 1: the blown-up coset evaluation (run_ntt)
    long long n_coeffs = -1;  // >= 0: rows beyond n_coeffs read as zero
    long long n_out = -1;     // >= 0: the last pass stores output elements j < n_out only
    bool pre_scale = false, post_scale = false, in2 = false, coset_offset = false;  // which optional operands the call carries
    bool packed = true;       // both batch strides are the contiguous n * L words
};

enum class NttRoute {
    Rows32,  // n <= 32 (BFieldElement: 64), contiguous: wave-private tiles (ntt_rows32w_kernel)
    Tiny,    // n <= 16: one thread per transform (ntt_tiny_kernel)
    Lat,     // 64 <= n <= 4096, little work: one launch of 8-element threads (ntt_lat_kernel)
    Lat2,    // 2^13 <= n <= 2^20, little work: two launches of 8-element threads (ntt_lat2_kernel)
    Row,     // n <= 1024: one pass, a tile is whole transforms (ntt_pass_kernel)
    Block,   // 2^11 <= n <= 2^14 (XFieldElement: 2^12): whole transform per workgroup (ntt_block_kernel)
    Passes   // n = N_1 * ... * N_P: P - 1 column passes and a transposing last pass
};

struct NttPlan {
    NttRoute route = NttRoute::Passes;
    int wg = 512;         // threads per workgroup of the pass kernels in this call: 512, or 256 for the narrow tiles
    bool narrow = false;  // the narrow tiles were chosen for this call (too little work for the wide ones)
    // Passes only
    int P = 0;                                    // global passes
    int a[4] = {0, 0, 0, 0};                      // log2 of each pass's radix; sum = log2 n
    bool pre2[4] = {false, false, false, false};  // pass i is a 2048-point pass run as pairs of 1024-point workgroups (PRE2)
    bool c8 = false;                              // the first pass is the one-workgroup 2048-point column pass (ntt_col2048_kernel)
    bool plain1024 = false;                       // the last pass takes the plain R = 1024 kernel (LAST1024) ...
    int words = 0;                                // ... and its tiles are this many adjacent output words (0: whole elements)
    size_t tb = 0, ntiles = 0;                    // polynomials per batch tile (after the equal-tiles rebalance), tiles
    int K = 1;                                    // tile streams wanted (run_ntt lowers it to 1 when it cannot have side streams)
    bool truncates = false;  // the call ends in a kernel that can truncate its output (Block, Passes)
    int launches = 0;        // transform-kernel launches of the whole call (table builders of a first call not counted)
};

NttPlan plan_ntt(const NttShape& s);
// The plan of a plain in-place transform in a call with enough work that neither the latency-shaped kernels nor the narrow tiles
// apply -- what tf_ntt_plan documents.
NttPlan plan_ntt_large(size_t n, int L);

// ---- the rules plan_ntt is made of (tf_plan.hip keeps each next to the measurements behind it)
int ilog2(size_t v);
int pass_count(int log_n);
void choose_split(int log_n, int P, int L, int (&a)[4]);
bool can_truncate(size_t n, int L);
bool lat_wanted(int log_n, size_t batch, int L);
bool lat2_wanted(int log_n, size_t batch, int L);
// fast_coset_evaluate: the number of cosets of the padded coefficient length the evaluation is split into (1: the plain plan)
constexpr size_t kMaxCosetSplit = 64;
size_t coset_split(size_t n_coeffs, size_t order, size_t batch, int L);

}  // namespace tfi
