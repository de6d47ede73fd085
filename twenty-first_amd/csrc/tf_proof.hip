// tf_proof.hip -- launcher of the batched Merkle inclusion-proof verifier (proof_kernels.h): MerkleTreeInclusionProof::try_verify /
// into_authentication_paths, util_types/merkle_tree.rs:683-931.
#include "tf_temp.h"

#include <type_traits>

// The kernels read the Tip5 round constants from __constant__ memory, and every translation unit is its own code object with its own
// copy of tip5_kernels.h's constants: this unit includes the device functions in a namespace of its own (no second host-side symbol
// tfp::tfk::g_tip5) and uploads its copy once per device (Tip5ConstsOnce).
namespace tfp {
#include "proof_kernels.h"
}

namespace tfi {

// ------------------------------------------------------------------------------------ pinned staging for the descriptors
// The descriptors are built on the host (O(n_proofs), from heights and offsets) and must reach the device without waiting for the
// caller's stream: a copy from pageable memory is staged by the runtime and may block until the stream reaches it.  They go through
// page-locked blocks kept per device; a block is reused once the copy that last read it has completed (its event), so a call never
// waits for earlier work on its stream.
namespace {
std::mutex g_stage_mu[kMaxDevices];
std::vector<Staging> g_stage[kMaxDevices];
}  // namespace

int stage_acquire(int dev, size_t bytes, Staging* out) {
    {
        std::lock_guard<std::mutex> lk(g_stage_mu[dev]);
        auto& v = g_stage[dev];
        for (size_t i = 0; i < v.size(); ++i) {
            if (v[i].bytes >= bytes && hipEventQuery(v[i].done) == hipSuccess) {
                *out = v[i];
                v.erase(v.begin() + (long)i);
                return TF_OK;
            }
        }
    }
    Staging st;
    st.bytes = std::max<size_t>(bytes, 64 << 10);
    HIPCHK(hipHostMalloc(&st.p, st.bytes, hipHostMallocDefault));
    const hipError_t e = hipEventCreateWithFlags(&st.done, hipEventDisableTiming);
    if (e != hipSuccess) {
        (void)hipHostFree(st.p);
        return hip_fail(e, "hipEventCreateWithFlags", __FILE__, __LINE__);
    }
    *out = st;
    return TF_OK;
}

// after the copy that reads `st` has been enqueued on `s`
void stage_release(int dev, Staging st, hipStream_t s) {
    (void)hipEventRecord(st.done, s);
    std::lock_guard<std::mutex> lk(g_stage_mu[dev]);
    g_stage[dev].push_back(st);
}

namespace {
Tip5ConstsOnce g_consts;

// threads of an LDS-route workgroup: a row per distinct leaf at the widest level, 256 .. 1024
int lds_threads(long long max_k) {
    long long t = 16 * tfp::tfk::proof_pow2(max_k);
    return (int)std::min<long long>(1024, std::max<long long>(256, t));
}
}  // namespace

int merkle_proofs_dev(const uint32_t* heights, size_t n, const uint64_t* leaf_offsets, const u64* d_leaf_indices, const u64* d_leaf_digests,
                      const uint64_t* auth_offsets, const u64* d_auth, const u64* d_roots, int* d_statuses, u64* d_paths, bool paths,
                      uint64_t leaf_base, uint64_t auth_base, hipStream_t s) {
    if (n == 0) return TF_OK;
    if (!heights || !leaf_offsets || !auth_offsets || !d_statuses) return TF_ERR_NULL_POINTER;
    unsigned long long path_words = 0;  // digests of paths_out
    for (size_t p = 0; p < n; ++p) {
        if (leaf_offsets[p + 1] < leaf_offsets[p] || auth_offsets[p + 1] < auth_offsets[p]) return TF_ERR_INVALID_ARGUMENT;
        if (heights[p] < 64) path_words += (leaf_offsets[p + 1] - leaf_offsets[p]) * heights[p];
    }
    if (leaf_offsets[0] < leaf_base || auth_offsets[0] < auth_base) return TF_ERR_INVALID_ARGUMENT;
    if (leaf_offsets[n] > leaf_offsets[0] && (!d_leaf_indices || !d_leaf_digests)) return TF_ERR_NULL_POINTER;
    if (auth_offsets[n] > auth_offsets[0] && !d_auth) return TF_ERR_NULL_POINTER;
    if (paths ? (path_words && !d_paths) : !d_roots) return TF_ERR_NULL_POINTER;

    int dev = 0;
    TRY(g_consts.ensure(&dev, tfp::tfk::g_tip5));

    // descriptors: LDS-route proofs first, then the scratch route
    std::vector<tfp::tfk::ProofDesc> small, large;
    unsigned long long scratch_words = 0, path_off = 0;
    long long max_small_k = 1;
    for (size_t p = 0; p < n; ++p) {
        tfp::tfk::ProofDesc dsc{};
        const unsigned long long k = leaf_offsets[p + 1] - leaf_offsets[p], a = auth_offsets[p + 1] - auth_offsets[p];
        dsc.leaf_off = leaf_offsets[p] - leaf_base;
        dsc.auth_off = auth_offsets[p] - auth_base;
        dsc.k = k;
        dsc.a = a;
        dsc.proof = p;
        dsc.h = heights[p];
        dsc.path_off = path_off;
        // the verdicts that heights and lengths decide alone (try_verify :737-739, num_leafs :795-798, the expected length of a
        // proof without leafs is 0)
        if (!paths && k == 0 && a == 0) dsc.verdict = TF_OK;
        else if (heights[p] >= 64) dsc.verdict = TF_ERR_TREE_TOO_HIGH;
        else if (k == 0) dsc.verdict = a == 0 ? TF_OK : TF_ERR_AUTH_STRUCTURE_LENGTH_MISMATCH;
        else dsc.verdict = -1;
        if (heights[p] < 64) path_off += k * heights[p];
        if (dsc.verdict < 0 && (long long)k > tfp::tfk::kProofLdsMaxLeafs) {
            if (k >= (1ull << 32)) return TF_ERR_OUT_OF_MEMORY;  // positions are 32-bit; such a proof needs > 700 GiB of work space
            dsc.scratch_off = scratch_words;
            scratch_words += (unsigned long long)tfp::tfk::proof_words((long long)k);
            large.push_back(dsc);
        } else {
            if (dsc.verdict < 0) max_small_k = std::max<long long>(max_small_k, (long long)k);
            small.push_back(dsc);
        }
    }
    const size_t n_small = small.size();
    small.insert(small.end(), large.begin(), large.end());
    StagedUpload up(s);
    TRY(up.put(dev, small.data(), n * sizeof(tfp::tfk::ProofDesc), "proof descriptors"));
    const tfp::tfk::ProofDesc* d_desc = up.as<tfp::tfk::ProofDesc>();
    DevTemp scratch(s);
    TRY(scratch.alloc(scratch_words, "proof work space"));
    u64* const d_scratch = scratch.p;
    if (n_small) {
        const size_t lds = (size_t)tfp::tfk::proof_words(max_small_k) * sizeof(u64);
        const dim3 grid((unsigned)n_small), block((unsigned)lds_threads(max_small_k));
        if (paths)
            hipLaunchKernelGGL((tfp::tfk::merkle_proof_kernel<true, true>), grid, block, lds, s, d_desc, d_leaf_indices, d_leaf_digests, d_auth,
                               d_roots, nullptr, d_statuses, d_paths);
        else
            hipLaunchKernelGGL((tfp::tfk::merkle_proof_kernel<true, false>), grid, block, lds, s, d_desc, d_leaf_indices, d_leaf_digests, d_auth,
                               d_roots, nullptr, d_statuses, d_paths);
    }
    if (!large.empty()) {
        const dim3 grid((unsigned)large.size()), block(1024);
        if (paths)
            hipLaunchKernelGGL((tfp::tfk::merkle_proof_kernel<false, true>), grid, block, 0, s, d_desc + n_small, d_leaf_indices, d_leaf_digests,
                               d_auth, d_roots, d_scratch, d_statuses, d_paths);
        else
            hipLaunchKernelGGL((tfp::tfk::merkle_proof_kernel<false, false>), grid, block, 0, s, d_desc + n_small, d_leaf_indices,
                               d_leaf_digests, d_auth, d_roots, d_scratch, d_statuses, d_paths);
    }
    const hipError_t le = hipGetLastError();
    if (le != hipSuccess) return hip_fail(le, "merkle_proof_kernel launch", __FILE__, __LINE__);
    return TF_OK;
}

}  // namespace tfi
