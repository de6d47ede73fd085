// mmr_kernels.h -- batched Merkle Mountain Range operations for gfx950 (device side).
//
// Reference: twenty-first/src/util_types/mmr/
//   mmr_membership_proof.rs  MmrMembershipProof::verify :36-77
//   mmr_accumulator.rs       bag_peaks :379-391, batch_mutate_leaf_and_update_mps :180-302
//   shared_basic.rs          leaf_index_to_mt_index_and_peak_index :24-62
//   mmr_successor_proof.rs   MmrSuccessorProof::verify_internal :142-223
//   mmr_membership_proof.rs  batch_update_from_append :224-331 (the copy that writes the extended proofs)
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

// One step of a chain in lane (j, q), as the loop of mmr_chain_kernel spells it out (that kernel keeps its own text: routed through
// this function its three instances come out with another register allocation).  The digest (a0: word q; a1: word 4 in quarter 0;
// acc4, accm: its word 4 and word (q - 1) mod 4, shuffled in by the caller) is hashed with the sibling at sp (nullptr: five zero
// words), which stands on the left where `right` says that the chain's node is the right child.  A chain that is not `on` runs the
// permutation with the others and keeps its digest.
__device__ __forceinline__ void mmr_chain_step(u64& a0, u64& a1, u64 acc4, u64 accm, const u64* sp, bool right, bool on, int q, const Tip5MxLds* lds,
                                               const MxA& a) {
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
    tip5_permutation_mx_fixed<1>(s, lds, a, q);
    if (on) {
        a0 = s[0];
        a1 = s[1];
    }
}

// MmrSuccessorProof::verify_internal (mmr_successor_proof.rs:142-223) of one (old accumulator, new accumulator, proof) triple per
// chain, in the layout of mmr_chain_kernel.  The host has decided everything the counts decide: `cmp` leading peaks of both lists
// must be equal (the shared peaks; all of them where the counts are equal; none where an earlier check has failed), `verdict` is
// the status that holds if they are (0, or the failed count / length check), and only a proof that has passed all of it has `steps`:
// the chain starts at its first path digest and, at step l, takes the next path digest on its right (bit l of `bits` clear) or the
// next old peak from the back on its left (bit set); it must arrive at new peak `cmp`.
struct MmrSuccessorChain {
    unsigned long long p, bits, path, old_first, new_first;  // proof; mt index >> height of the lowest old peak; first digest of each list
    unsigned int old_count, cmp, steps, verdict;
    unsigned long long pad;
};
static_assert(sizeof(MmrSuccessorChain) == 64, "one 64-byte descriptor per chain");

__global__ void __launch_bounds__(256) mmr_successor_kernel(const MmrSuccessorChain* chains, long long n, const u64* old_peaks, const u64* new_peaks,
                                                            const u64* paths, int* statuses) {
    __shared__ __attribute__((aligned(32))) Tip5MxLds lds;
    stage_mx(&lds);
    MxA a;
    mx_a_operands(&lds, a);
    const int lane = threadIdx.x & 63, j = lane & 15, q = lane >> 4;
    const long long item = ((long long)blockIdx.x * 4 + (threadIdx.x >> 6)) * 16 + j;
    if (item - j >= n) return;  // whole wave past the end (uniform over the wave)
    const bool live = item < n;
    const MmrSuccessorChain d = chains[live ? item : n - 1];

    bool shared_differs = false;
    if (live) {
        const u64 *x = old_peaks + 5 * d.old_first, *y = new_peaks + 5 * d.new_first;
        for (unsigned i = 0; i < d.cmp; ++i, x += 5, y += 5) shared_differs |= x[q] != y[q] || (q == 0 && x[4] != y[4]);
    }
    const long long steps = live ? d.steps : 0;
    u64 a0 = 0, a1 = 0;
    if (steps) {
        const u64* p = paths + 5 * d.path;
        a0 = p[q];
        a1 = p[4];
    }
    long long wave_steps = steps;
#pragma unroll
    for (int m = 1; m < 16; m <<= 1) wave_steps = max(wave_steps, (long long)__shfl_xor(wave_steps, m, 64));

    for (long long l = 0; l < wave_steps; ++l) {
        const bool on = l < steps;
        const u64 acc4 = __shfl(a1, j, 64);
        const u64 accm = __shfl(a0, j + 16 * ((q + 3) & 3), 64);
        const bool right = (d.bits >> l) & 1;
        const long long rights = __popcll(d.bits & ((1ull << l) - 1));  // old peaks used so far; the other steps took a path digest
        const u64* sp = nullptr;
        if (on) sp = right ? old_peaks + 5 * (d.old_first + d.old_count - 1 - rights) : paths + 5 * (d.path + 1 + (l - rights));
        mmr_chain_step(a0, a1, acc4, accm, sp, right, on, q, &lds, a);
    }

    bool peak_differs = false;
    if (steps) {
        const u64* pk = new_peaks + 5 * (d.new_first + d.cmp);
        peak_differs = a0 != pk[q] || (q == 0 && a1 != pk[4]);
    }
    const unsigned long long bad_shared = __ballot(shared_differs), bad_peak = __ballot(peak_differs);
    auto any_quarter = [j](unsigned long long b) { return ((b >> j) | (b >> (j + 16)) | (b >> (j + 32)) | (b >> (j + 48))) & 1; };
    if (live && q == 0)
        statuses[d.p] = any_quarter(bad_shared) ? TF_ERR_MMR_DIFFERENT_SHARED_PEAK
                        : d.verdict             ? (int)d.verdict
                        : any_quarter(bad_peak) ? TF_ERR_MMR_DIFFERENT_UNSHARED_PEAK
                                                : TF_OK;
}

// The membership proofs of an append (tf_mmr_update_proofs_from_append): proof p of the output is its old path (old_len digests from
// digest `src` of own) followed by suf_len digests from digest `suffix` of the table of suffixes (one list per old peak), at digest
// `dst` of out.  Sixteen lanes copy one proof.  Every store but the first and last word of a proof is 16 bytes wide (a digest is 40
// bytes, so a proof starts on a 16-byte boundary only at every other digest); a load of the old path is 16 bytes wide where its
// source has the parity of the destination, else two words, as are the loads of the table.
struct MmrGatherDesc {
    unsigned long long src, dst, suffix;
    unsigned int old_len, suf_len;
};
static_assert(sizeof(MmrGatherDesc) == 32, "one 32-byte descriptor per proof");
typedef u64 MmrWordPair __attribute__((ext_vector_type(2)));

__global__ void __launch_bounds__(256) mmr_gather_paths_kernel(const MmrGatherDesc* descs, long long n, const u64* own, const u64* table, u64* out) {
    const int lane = threadIdx.x & 15;
    const long long p = ((long long)blockIdx.x * 256 + threadIdx.x) >> 4;
    if (p >= n) return;
    const MmrGatherDesc d = descs[p];
    const long long w_old = 5ll * d.old_len, total = w_old + 5ll * d.suf_len;
    const u64 *s0 = own + 5 * d.src, *s1 = table + 5 * d.suffix;
    u64* o = out + 5 * d.dst;
    auto word = [&](long long w) { return w < w_old ? s0[w] : s1[w - w_old]; };
    const long long head = min((long long)((reinterpret_cast<unsigned long long>(o) >> 3) & 1), total);  // words before the 16-byte boundary
    const long long pairs = (total - head) >> 1;
    if (lane == 0 && head) o[0] = word(0);
    for (long long i = lane; i < pairs; i += 16) {
        const long long w = head + 2 * i;
        const u64* s = w + 1 < w_old ? s0 + w : nullptr;  // the old path, read once; the table's few digests are read by many proofs
        MmrWordPair v;
        if (s && !(reinterpret_cast<unsigned long long>(s) & 15))  // non-temporal, which also keeps this load apart from the two below
            v = __builtin_nontemporal_load(reinterpret_cast<const MmrWordPair*>(s));
        else v = MmrWordPair{word(w), word(w + 1)};
        *reinterpret_cast<MmrWordPair*>(o + w) = v;
    }
    if (lane == 15 && head + 2 * pairs < total) o[total - 1] = word(total - 1);
}

}  // namespace tfk
