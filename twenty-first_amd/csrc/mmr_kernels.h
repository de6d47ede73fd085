// mmr_kernels.h -- batched Merkle Mountain Range operations for gfx950 (device side).
//
// Reference: twenty-first/src/util_types/mmr/
//   mmr_membership_proof.rs  MmrMembershipProof::verify :36-77
//   mmr_accumulator.rs       bag_peaks :379-391, batch_mutate_leaf_and_update_mps :180-302
//   shared_basic.rs          leaf_index_to_mt_index_and_peak_index :24-62
//
// Every MMR operation here is a set of independent hash_pair chains: a membership proof is one chain from its leaf to its peak,
// bagging is one chain over an accumulator's peaks, one level of a batch mutation is one step of every mutation's chain.  They
// run in the matrix-pipe layout of tip5_hash_pairs_mx_kernel (four lanes per permutation, sixteen chains per wave): lane
// (j = lane & 15, q = lane >> 4) holds state words q, 4 + q, 8 + q of chain j.  Between two steps the digest (state words 0..4:
// register 0 of the four quarters, register 1 of quarter 0) becomes one half of the next input; two wave shuffles bring the words
// a lane needs, so a chain never leaves the registers.  The host orders chains by length, so the sixteen chains of a wave end
// together; a wave runs as many steps as its longest chain, and a finished chain keeps its digest while the others go on (the
// matrix instructions want all 64 lanes).  The append sweep uses the library's hash_pairs launches (tf_tip5.hip) and the moves
// below.
#pragma once

#include "tip5_kernels.h"

namespace tfk {

enum : int { kMmrVerify = 0, kMmrBag = 1, kMmrStep = 2 };
constexpr unsigned long long kMmrFromAcc = 1ull << 63;  // kMmrStep: the sibling is a digest of the accumulator level, not of a path

// One chain of a launch (built on the host).
//   kMmrVerify: a = proof, b = first path digest, c = path length
//   kMmrBag:    a = leaf count, b = first peak, c = accumulator
//   kMmrStep:   a = unused, b = sibling (path digest, or kMmrFromAcc | slot of the level), c = 1 if the chain is the right child
struct MmrChain {
    unsigned long long a, b, c, d;
};
static_assert(sizeof(MmrChain) == 32, "one 32-byte descriptor per chain");

// MODE = kMmrVerify: statuses[p] = verify(idx[p], init[p], path of p, peaks, leaf_count) as a status (0, 22, 23, 24, 25);
//   init = leaf digests, sib = paths, sib2 = peaks (n_peaks digests).
// MODE = kMmrBag: out[c] = bag_peaks(peaks + b, leaf count a); sib = peaks.
// MODE = kMmrStep: out[i] = hash_pair of init[i] (the chain's digest at this level) and its sibling, in the chain's order;
//   sib = paths, sib2 = the level (init).
template <int MODE>
__global__ void __launch_bounds__(256) mmr_chain_kernel(const MmrChain* chains, long long n, const u64* init, const u64* sib, const u64* sib2,
                                                        u64* out, const u64* idx, u64 leaf_count, long long n_peaks, int* statuses) {
    __shared__ __attribute__((aligned(32))) Tip5MxLds lds;
    stage_mx(&lds);
    MxA a;
    mx_a_operands(&lds, a);
    const int lane = threadIdx.x & 63, j = lane & 15, q = lane >> 4;
    const long long item = ((long long)blockIdx.x * 4 + (threadIdx.x >> 6)) * 16 + j;
    if (item - j >= n) return;  // whole wave past the end (uniform over the wave)
    const bool live = item < n;
    const MmrChain d = chains[live ? item : n - 1];

    // the chain's first digest (word q in a0, word 4 in a1 of quarter 0), its length, and what decides the order of each step
    u64 a0 = 0, a1 = 0, li = 0;
    long long steps = 0, peak = 0;
    int status = -1;
    if (MODE == kMmrVerify) {
        li = idx[d.a];
        if (li >= leaf_count) status = TF_ERR_MMR_LEAF_INDEX_OUT_OF_RANGE;
        else if (__popcll(leaf_count) != n_peaks) status = TF_ERR_MMR_PEAK_COUNT_MISMATCH;
        else {
            const int h = 63 - __clzll((long long)(li ^ leaf_count));  // leaf_index_to_mt_index_and_peak_index
            if ((unsigned long long)h != d.c) status = TF_ERR_MMR_AUTH_PATH_LENGTH_MISMATCH;
            else {
                peak = __popcll(leaf_count) - __popcll(leaf_count & ((1ull << h) - 1)) - 1;
                steps = h;
            }
        }
        const u64* p = init + 5 * d.a;
        a0 = p[q];
        a1 = p[4];
    } else if (MODE == kMmrBag) {
        // hash_10 of the u64 codec [lo, hi, 0 ...] is hash_pair([lo, hi, 0, 0, 0], 0): step 0 below
        a0 = q == 0 ? gl::to_mont(d.a & 0xffffffffull) : (q == 1 ? gl::to_mont(d.a >> 32) : 0);
        steps = 1 + __popcll(d.a);
    } else {
        const u64* p = init + 5 * (live ? item : n - 1);
        a0 = p[q];
        a1 = p[4];
        steps = 1;
    }
    if (!live) steps = 0;
    long long wave_steps = steps;
#pragma unroll
    for (int m = 1; m < 16; m <<= 1) wave_steps = max(wave_steps, (long long)__shfl_xor(wave_steps, m, 64));

    for (long long l = 0; l < wave_steps; ++l) {
        const bool on = l < steps;
        const u64 acc4 = __shfl(a1, j, 64);                      // digest word 4
        const u64 accm = __shfl(a0, j + 16 * ((q + 3) & 3), 64);  // digest word (q - 1) mod 4
        const u64* sp = nullptr;
        bool right = false;
        if (MODE == kMmrVerify) {
            sp = sib + 5 * (d.b + l);
            right = (li >> l) & 1;
        } else if (MODE == kMmrBag) {
            sp = l == 0 ? nullptr : sib + 5 * (d.b + steps - 1 - l);  // the peaks in reverse
            right = l != 0;
        } else {
            sp = (d.b & kMmrFromAcc) ? sib2 + 5 * (d.b & ~kMmrFromAcc) : sib + 5 * d.b;
            right = d.c & 1;
        }
        u64 w0 = 0, w1 = 0;  // the sibling words this lane needs
        if (on && sp) {
            if (right) {
                w0 = sp[q];
                if (q == 0) w1 = sp[4];
            } else {
                if (q > 0) w0 = sp[q - 1];
                if (q < 2) w1 = sp[3 + q];
            }
        }
        u64 s[4];
        if (right) {  // input = sibling | digest
            s[0] = w0;
            s[1] = q == 0 ? w1 : accm;
            s[2] = q == 0 ? accm : (q == 1 ? acc4 : gl::ONE);
        } else {  // input = digest | sibling
            s[0] = a0;
            s[1] = q == 0 ? acc4 : w0;
            s[2] = q < 2 ? w1 : gl::ONE;
        }
        s[3] = gl::ONE;
        tip5_permutation_mx_fixed<1>(s, &lds, a, q);
        if (on) {
            a0 = s[0];
            a1 = s[1];
        }
    }

    if (MODE == kMmrVerify) {
        bool differs = false;
        if (status < 0) {
            const u64* pk = sib2 + 5 * peak;
            differs = a0 != pk[q] || (q == 0 && a1 != pk[4]);
        }
        const unsigned long long bad = __ballot(differs);
        if (live && q == 0) {
            if (status < 0) status = ((bad >> j) | (bad >> (j + 16)) | (bad >> (j + 32)) | (bad >> (j + 48))) & 1 ? TF_ERR_MMR_PEAK_MISMATCH : TF_OK;
            statuses[d.a] = status;
        }
    } else if (live) {
        u64* o = out + 5 * (MODE == kMmrBag ? (long long)d.c : item);
        o[q] = a0;
        if (q == 0) o[4] = a1;
    }
}

// Digest moves between up to four source and four destination arrays: move k copies digest (moves[2 k] & kMmrIndexMask) of
// src[moves[2 k] >> kMmrSelShift] to digest (moves[2 k + 1] & kMmrIndexMask) of dst[moves[2 k + 1] >> kMmrSelShift].  The leaf level
// of a batch mutation, the peaks it writes back, and per level of an append: the proof siblings, the peak, the old peak the next
// level starts with.
constexpr int kMmrSelShift = 62;
constexpr unsigned long long kMmrIndexMask = (1ull << kMmrSelShift) - 1;
struct MmrMoveArrays {
    const u64* src[4];
    u64* dst[4];
};
__global__ void __launch_bounds__(256) mmr_move_digests_kernel(MmrMoveArrays a, const unsigned long long* moves, long long count) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count * 5) return;
    const long long k = i / 5, w = i - 5 * k;
    const unsigned long long from = moves[2 * k], to = moves[2 * k + 1];
    a.dst[to >> kMmrSelShift][(to & kMmrIndexMask) * 5 + w] = a.src[from >> kMmrSelShift][(from & kMmrIndexMask) * 5 + w];
}

// The own proofs of a batch mutation: fix k = (path digest e, map digest v, proof p): where the map's digest differs from the path's,
// it replaces it and flags the proof (every writer of a flag writes 1).
__global__ void __launch_bounds__(256) mmr_update_paths_kernel(const unsigned long long* fixes, long long count, const u64* map, u64* paths,
                                                               int* modified) {
    const long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= count) return;
    const unsigned long long e = fixes[3 * k], v = fixes[3 * k + 1], p = fixes[3 * k + 2];
    u64 x[5];
    bool differs = false;
#pragma unroll
    for (int w = 0; w < 5; ++w) {
        x[w] = map[5 * v + w];
        differs |= x[w] != paths[5 * e + w];
    }
    if (!differs) return;
#pragma unroll
    for (int w = 0; w < 5; ++w) paths[5 * e + w] = x[w];
    modified[p] = 1;
}

}  // namespace tfk
