// proof_kernels.h -- batched verification of Merkle inclusion proofs for gfx950 (device side).
//
// Reference: twenty-first/src/util_types/merkle_tree.rs
//   MerkleTreeInclusionProof::try_verify :736-748, into_authentication_paths :773-777
//   PartialMerkleTree::try_from :890-931, fill :806-858, into_authentication_paths :861-888
//   MerkleTree::authentication_structure_node_indices :449-504
//
// One workgroup per proof, every step of the proof in that workgroup (no launch per level or per proof):
//   1. leaf indices against 2^h (LeafIndexInvalid);
//   2. bitonic sort of the leaf indices (with their positions in the proof);
//   3. one pass over neighbours of the sorted list: the length of the authentication structure the reference derives, and the
//      digests of repeated indices (AuthenticationStructureLengthMismatch, RepeatedLeafDigestMismatch).  The length needs no walk
//      over the levels: level l holds m_l = 1 + #{j : bitlen(x_j ^ x_(j-1)) > l} distinct nodes, and the structure has
//      sum_(l < h) (2 m_(l+1) - m_l) = h + sum_(j : x_j != x_(j-1)) (bitlen(x_j ^ x_(j-1)) - 2) digests;
//   4. the levels, bottom-up: the sorted, de-duplicated node set of the level; a prefix sum over "first child of its parent" gives
//      each parent its rank i and its first child j, so the 2 i - j structure digests that the parents before it consume are known
//      and the missing sibling of parent i is digest (level base + A_l - 1 - (2 i - j)) of the structure (descending within a
//      level, levels bottom first).  The parents' hash_pair inputs are gathered, then hashed one per 16-lane row
//      (tip5_permutation_coop, or a row pair where the level leaves rows to spare -- as merkle_subtree does), a barrier per level;
//   5. the root against the expected one (RootMismatch), or, for authentication paths, each leaf's sibling at every level.
//
// Work space of one proof (proof_words): in LDS for proofs of up to kProofLdsMaxLeafs leafs, in device scratch above that.  Either
// way only this workgroup reads and writes it, and the hand-off between its waves is store -> __syncthreads() -> load on one CU
// (the per-CU L1 is shared by the workgroup; there is no cross-CU hand-off on this path).
#pragma once

#include "tip5_kernels.h"

namespace tfk {

// One proof of a launch (built on the host from heights and offsets alone).
struct ProofDesc {
    unsigned long long leaf_off;     // first leaf of the proof in the leaf arrays
    unsigned long long auth_off;     // first digest of its authentication structure
    unsigned long long k;            // leafs (duplicates included)
    unsigned long long a;            // authentication-structure digests
    unsigned long long scratch_off;  // words into the device scratch (scratch route only)
    unsigned long long path_off;     // digests into paths_out (authentication paths only)
    unsigned long long proof;        // index of the proof in the call: statuses[proof], expected_roots + 5 proof
    unsigned h;                      // tree height (< 64 whenever verdict < 0)
    int verdict;                     // >= 0: the status, decided on the host from heights and lengths alone; < 0: run the proof
};
static_assert(sizeof(ProofDesc) == 64, "one 64-byte descriptor per proof");

constexpr long long kProofLdsMaxLeafs = 256;  // LDS route: at most 6 016 words (47 KiB) of work space

__host__ __device__ inline long long proof_pow2(long long k) {
    long long p = 1;
    while (p < k) p <<= 1;
    return p;
}
// words of work space: sorted keys (K2 words), their positions (K2 u32), two levels of node indices (2 k) and digests (10 k), the
// hash_pair inputs of the next level (10 k)
__host__ __device__ inline long long proof_words(long long k) {
    const long long k2 = proof_pow2(k);
    return k2 + (k2 + 1) / 2 + 22 * k;
}

// exclusive prefix sum of v over the workgroup (blockDim.x a multiple of 64, at most 1024); *total = the sum.  red: 16 words of LDS.
__device__ __forceinline__ long long proof_block_scan(long long v, long long* red, long long& total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    long long x = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const long long y = __shfl_up(x, d, 64);
        if (lane >= d) x += y;
    }
    if (lane == 63) red[w] = x;
    __syncthreads();
    long long before = 0, tot = 0;
    for (int i = 0; i < nw; ++i) {
        const long long s = red[i];
        before += i < w ? s : 0;
        tot += s;
    }
    __syncthreads();  // red may be written again by the next scan
    total = tot;
    return before + x - v;
}

// PATHS = false: statuses[p] = verdict of try_verify(expected_roots[p]);  PATHS = true: statuses[p] = verdict of
// into_authentication_paths, paths_out[path_off + e h + l] = sibling at level l of leaf entry e.
// LDS = true: the work space is dynamic LDS of proof_words(max k) words; false: scratch + desc.scratch_off.
template <bool LDS, bool PATHS>
__global__ void __launch_bounds__(1024) merkle_proof_kernel(const ProofDesc* descs, const u64* leaf_indices, const u64* leaf_digests,
                                                            const u64* auth_digests, const u64* expected_roots, u64* scratch,
                                                            int* statuses, u64* paths_out) {
    extern __shared__ __attribute__((aligned(16))) u64 proof_lds[];
    __shared__ __attribute__((aligned(16))) unsigned char lut[256];
    __shared__ long long red[16];
    __shared__ int flag;
    const ProofDesc d = descs[blockIdx.x];
    const int t = threadIdx.x, T = blockDim.x;
    if (d.verdict >= 0) {  // uniform over the workgroup
        if (t == 0) statuses[d.proof] = d.verdict;
        return;
    }
    const long long k = (long long)d.k, a = (long long)d.a;
    const int h = (int)d.h;
    const u64* li = leaf_indices + d.leaf_off;
    const u64* ld = leaf_digests + 5 * d.leaf_off;
    const u64* au = auth_digests + 5 * d.auth_off;
    const long long K2 = proof_pow2(k);
    u64* ws = LDS ? proof_lds : scratch + d.scratch_off;
    u64* key = ws;
    u32* pos = reinterpret_cast<u32*>(ws + K2);
    u64* S[2] = {ws + K2 + (K2 + 1) / 2, ws + K2 + (K2 + 1) / 2 + k};
    u64* V[2] = {S[1] + k, S[1] + 6 * k};
    u64* P = S[1] + 11 * k;

    // ---- 1. leaf indices (try_from :901-904)
    if (t == 0) flag = 0;
    __syncthreads();
    bool bad = false;
    for (long long e = t; e < K2; e += T) {
        u64 x = ~0ull;  // padding sorts last (a leaf index is < 2^63)
        if (e < k) {
            x = li[e];
            bad |= (x >> h) != 0;
        }
        key[e] = x;
        pos[e] = (u32)e;
    }
    if (bad) flag = 1;
    __syncthreads();
    if (flag) {
        if (t == 0) statuses[d.proof] = TF_ERR_LEAF_INDEX_INVALID;
        return;
    }

    // ---- 2. bitonic sort of (index, position) by index
    for (long long size = 2; size <= K2; size <<= 1) {
        for (long long stride = size >> 1; stride > 0; stride >>= 1) {
            for (long long i = t; i < K2 / 2; i += T) {
                const long long lo = 2 * i - (i & (stride - 1)), hi = lo + stride;
                const bool up = (lo & size) == 0;
                const u64 x = key[lo], y = key[hi];
                if ((x > y) == up && x != y) {
                    key[lo] = y;
                    key[hi] = x;
                    const u32 p = pos[lo];
                    pos[lo] = pos[hi];
                    pos[hi] = p;
                }
            }
            __syncthreads();
        }
    }

    // ---- 3. structure length (try_from :906-912) and repeated leafs (:914-925)
    long long acc = 0;
    bool rep = false;
    for (long long j = 1 + t; j < k; j += T) {
        const u64 dx = key[j] ^ key[j - 1];
        if (dx) {
            acc += (64 - __clzll((long long)dx)) - 2;
        } else {
            const u64* p0 = ld + 5 * (long long)pos[j - 1];
            const u64* p1 = ld + 5 * (long long)pos[j];
#pragma unroll
            for (int w = 0; w < 5; ++w) rep |= p0[w] != p1[w];
        }
    }
    long long sum = 0;
    (void)proof_block_scan(acc, red, sum);
    long long reps = 0;
    (void)proof_block_scan(rep ? 1 : 0, red, reps);
    if (h + sum != a) {
        if (t == 0) statuses[d.proof] = TF_ERR_AUTH_STRUCTURE_LENGTH_MISMATCH;
        return;
    }
    if (reps) {
        if (t == 0) statuses[d.proof] = TF_ERR_REPEATED_LEAF_DIGEST_MISMATCH;
        return;
    }

    // ---- 4. level 0: the distinct leafs and their digests, then the levels above
    long long m = 0;
    {
        const long long c = (k + T - 1) / T, b0 = t * c < k ? t * c : k, b1 = b0 + c < k ? b0 + c : k;
        long long cnt = 0;
        for (long long j = b0; j < b1; ++j) cnt += (j == 0 || key[j] != key[j - 1]);
        long long r = proof_block_scan(cnt, red, m);
        for (long long j = b0; j < b1; ++j) {
            if (j == 0 || key[j] != key[j - 1]) {
                S[0][r] = key[j];
                const u64* src = ld + 5 * (long long)pos[j];
#pragma unroll
                for (int w = 0; w < 5; ++w) V[0][5 * r + w] = src[w];
                ++r;
            }
        }
    }
    if (t == 0) flag = 0;
    const int j16 = t & 15, row = t >> 4, rows = T >> 4, half = row & 1;
    u64 rcs[5];
    coop_round_constants(j16, rcs);
    CoopHalfMatrix hm;
    coop_half_matrix(half, hm);
    stage_lut(lut);  // its barrier also publishes level 0

    int cur = 0;
    long long base = 0;  // structure digests consumed by the levels below
    for (int l = 0; l < h; ++l) {
        const u64* Sc = S[cur];
        const u64* Vc = V[cur];
        u64* Sn = S[cur ^ 1];
        u64* Vn = V[cur ^ 1];
        // parents of the level: rank i of parent q = number of first children before its own first child j
        const long long c = (m + T - 1) / T, b0 = t * c < m ? t * c : m, b1 = b0 + c < m ? b0 + c : m;
        long long cnt = 0;
        for (long long j = b0; j < b1; ++j) cnt += (j == 0 || (Sc[j] >> 1) != (Sc[j - 1] >> 1));
        long long mn = 0;
        long long i = proof_block_scan(cnt, red, mn);
        const long long A = 2 * mn - m;  // structure digests of this level
        bool oob = false;
        for (long long j = b0; j < b1; ++j) {
            const u64 q = Sc[j] >> 1;
            if (j != 0 && (Sc[j - 1] >> 1) == q) continue;
            Sn[i] = q;
            u64* pi = P + 10 * i;
            const u64* own = Vc + 5 * j;
            if (j + 1 < m && (Sc[j + 1] >> 1) == q) {
#pragma unroll
                for (int w = 0; w < 10; ++w) pi[w] = own[w];
            } else {
                long long ap = base + A - 1 - (2 * i - j);
                if (ap < 0 || ap >= a) {  // cannot happen once the length matched; never read outside the structure
                    oob = true;
                    ap = 0;
                }
                const u64* sib = au + 5 * ap;
                const bool right = Sc[j] & 1;
#pragma unroll
                for (int w = 0; w < 5; ++w) {
                    pi[w] = right ? sib[w] : own[w];
                    pi[5 + w] = right ? own[w] : sib[w];
                }
            }
            ++i;
        }
        if (oob) flag = 1;
        __syncthreads();
        // hash_pair of every parent (fill :806-858), one per row or row pair
        if (2 * mn <= rows) {
            const long long ip = row >> 1;
            if (ip < mn) {  // whole row pairs take the branch together
                u64 s = j16 < 10 ? P[10 * ip + j16] : gl::ONE;
                tip5_permutation_coop2(s, j16, half, lut, rcs, hm);
                if (j16 < 5 && !half) Vn[5 * ip + j16] = s;
            }
        } else {
            for (long long b = 0; b < mn; b += rows) {
                const long long ip = b + row;
                if (ip < mn) {  // whole rows take the branch together
                    u64 s = j16 < 10 ? P[10 * ip + j16] : gl::ONE;
                    tip5_permutation_coop(s, j16, lut, rcs);
                    if (j16 < 5) Vn[5 * ip + j16] = s;
                }
            }
        }
        if constexpr (PATHS) {
            // the sibling of leaf entry e at this level is the other half of its parent's hash_pair input
            u64* po = paths_out + 5 * d.path_off;
            for (long long e = t; e < k; e += T) {
                const u64 x = li[e], q = x >> (l + 1);
                long long lo = 0, hi = mn - 1;
                while (lo < hi) {
                    const long long mid = (lo + hi) >> 1;
                    if (Sn[mid] < q) lo = mid + 1;
                    else hi = mid;
                }
                const u64* sib = P + 10 * lo + 5 * (((x >> l) & 1) ^ 1);
                u64* dst = po + 5 * (e * h + l);
#pragma unroll
                for (int w = 0; w < 5; ++w) dst[w] = sib[w];
            }
        }
        __syncthreads();
        base += A;
        m = mn;
        cur ^= 1;
    }

    // ---- 5. the root (try_verify :741-743)
    const bool internal = flag != 0;
    __syncthreads();
    if constexpr (PATHS) {
        if (t == 0) statuses[d.proof] = internal ? TF_ERR_INTERNAL : TF_OK;
    } else {
        if (t == 0) flag = 0;
        __syncthreads();
        if (t < 5 && V[cur][t] != expected_roots[5 * d.proof + t]) flag = 1;
        __syncthreads();
        if (t == 0) statuses[d.proof] = internal ? TF_ERR_INTERNAL : (flag ? TF_ERR_ROOT_MISMATCH : TF_OK);
    }
}

}  // namespace tfk
