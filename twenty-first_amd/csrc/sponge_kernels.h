// sponge_kernels.h -- batches of device-resident Tip5 sponges for gfx950 (device side).
//
// Reference: twenty-first/src/tip5/mod.rs
//   Tip5::new(Domain) :511-526, Sponge::absorb :684-691 (overwrite mode), Sponge::squeeze :693-698 (the rate words, THEN the
//   permutation), Tip5::sample_indices :636-656, Tip5::sample_scalars :664-674; util_types/sponge.rs:41-55 pad_and_absorb_all.
//
// A batch is count x 16 raw Montgomery words (the layout of tip5_permute_*_kernel).  Every call of the sponge ABI is ONE launch of the
// sponge-program kernel below: a step is "optionally overwrite the rate words from memory, optionally store the rate words (or
// the indices they yield), permute", and the calls differ only in which of the three happen (OP) and in how the number of steps is
// found.  Two lane layouts, as everywhere in tip5_kernels.h: the cooperative form (16 or 32 lanes per sponge, one chain = latency)
// for at most kCoopMaxCount sponges, the matrix-pipe form (4 lanes per sponge) above that.
//
// THE STEP COUNT IS UNIFORM OVER THE WAVE.  Both permutations exchange data across lanes (DPP rows, v_permlane16_swap, MFMA
// operands), which is defined only with every lane executing.  The steps of a sponge can depend on the sponge -- a ragged absorb,
// and sample_indices, where an element equal to BFieldElement::MAX is skipped and may cost another squeeze -- so a wave loops until
// ALL its sponges are done (one ballot per step) and a finished sponge keeps permuting a dead copy `t` of its state while its
// committed state `s` and its outputs are frozen by predicate.  No lane-dependent trip count, no return ahead of a permutation:
// lanes past the end of the batch run a clamped sponge and store nothing.
#pragma once

#include "tip5_kernels.h"

namespace tfk {

enum : int { kSpongeAbsorb = 0, kSpongeSqueeze = 1, kSpongeIndices = 2 };

struct SpongeArgs {
    u64* states;
    long long count;  // >= 1
    // kSpongeAbsorb: sponge i absorbs in[offsets[i] .. offsets[i + 1]) if offsets != null, else in[i len .. (i + 1) len); pad = 1:
    // pad_and_absorb_all (len / 10 + 1 steps, a one after the input, then zeros), pad = 0: len / 10 plain absorbs (len % 10 == 0)
    const u64* in;
    const unsigned long long* offsets;
    long long len;
    int pad;
    // kSpongeSqueeze: ceil(out_words / 10) squeezes per sponge, the first out_words words of their concatenation to out + i out_words
    // (squeeze: out_words = 10 n_squeezes; sample_scalars: out_words = 3 num_elements, the tail of the last squeeze is dropped)
    u64* out;
    long long out_words;
    // kSpongeIndices: num_indices values (canonical value as u32) & mask per sponge to out_idx + i num_indices
    u32* out_idx;
    long long num_indices;
    u32 mask;  // upper_bound - 1, upper_bound a power of two
};

__global__ void __launch_bounds__(256) tip5_sponge_init_kernel(u64* states, long long words, int fixed_length) {
    const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
    if (t < words) states[t] = (fixed_length && (t & 15) >= 10) ? gl::ONE : 0;  // Tip5::new, mod.rs:511-526
}

// what sponge i absorbs, and in how many steps
__device__ __forceinline__ void sponge_input(const SpongeArgs& g, long long i, const u64*& p, long long& len, long long& steps) {
    if (g.offsets) {
        const unsigned long long b = g.offsets[i];
        p = g.in + b;
        len = (long long)(g.offsets[i + 1] - b);
    } else {
        p = g.in + i * g.len;
        len = g.len;
    }
    steps = len / 10 + (g.pad ? 1 : 0);
}
// word w of the (padded) input: never reads at or beyond p + len
__device__ __forceinline__ u64 sponge_rate_word(const u64* p, long long len, int pad, long long w) {
    return w < len ? p[w] : ((pad && w == len) ? gl::ONE : 0);
}
// BFieldElement::value(): the canonical value of a raw word (one Montgomery reduction, b_field_element.rs:357-370)
__device__ __forceinline__ u64 sponge_value(u64 raw) { return gl::montyred(raw, 0); }

// ---- latency form: lane j of a row (ROWS = 1) or of both rows of a row pair (ROWS = 2) holds state word j of one sponge -----------
template <int ROWS, int OP>
__global__ void __launch_bounds__(256) tip5_sponge_coop_kernel(const SpongeArgs g) {
    __shared__ __attribute__((aligned(16))) unsigned char lut[256];
    const int j = threadIdx.x & 15, half = CoopGeom<ROWS>::half();
    const long long item = CoopGeom<ROWS>::item();
    const bool live = item < g.count;  // whole rows (row pairs) are live or not
    const long long i = live ? item : g.count - 1;
    u64 s = g.states[i * 16 + j];
    const u64* p = nullptr;
    long long len = 0, steps = 0;
    u64 nxt = 0;
    if constexpr (OP == kSpongeAbsorb) {
        sponge_input(g, i, p, len, steps);
        if (j < 10 && steps > 0) nxt = sponge_rate_word(p, len, g.pad, j);
    } else if constexpr (OP == kSpongeSqueeze) {
        steps = (g.out_words + 9) / 10;
    }
    u64 rcs[5];
    coop_round_constants(j, rcs);
    CoopHalfMatrix hm;
    coop_half_matrix(half, hm);
    stage_lut(lut);
    long long produced = 0;                                             // kSpongeIndices: indices of this sponge so far
    const int group = (int)(threadIdx.x & 63) & ~(16 * ROWS - 1);       // first lane of this sponge in the wave
    for (long long c = 0;; ++c) {
        const bool active = live && (OP == kSpongeIndices ? produced < g.num_indices : c < steps);
        if (__ballot(active) == 0) break;  // uniform over the wave
        u64 t = s;
        if constexpr (OP == kSpongeAbsorb) {
            // as tip5_hash_varlen_rows_coop_kernel: the next chunk is fetched before the permutation of the current one
            if (active && j < 10) t = nxt;
            if (j < 10 && c + 1 < steps) nxt = sponge_rate_word(p, len, g.pad, (c + 1) * 10 + j);
        } else if constexpr (OP == kSpongeSqueeze) {
            const long long w = c * 10 + j;
            if (active && !half && j < 10 && w < g.out_words) g.out[i * g.out_words + w] = s;
        } else {
            // mod.rs:645-653: an element equal to MAX is dropped; a kept one goes to the place given by the kept elements before it
            const u64 v = sponge_value(s);
            const bool keep = j < 10 && v != gl::P - 1;
            const u32 kept = (u32)(__ballot(keep) >> group) & 0x3ffu;  // the ten rate lanes of this sponge
            const long long pos = produced + __popc(kept & ((1u << j) - 1u));
            if (active && keep && !half && pos < g.num_indices) g.out_idx[i * g.num_indices + pos] = (u32)v & g.mask;
            produced += __popc(kept);
        }
        tip5_permutation_coop_n<ROWS>(t, j, half, lut, rcs, hm);
        if (active) s = t;
    }
    if (live && !half) g.states[i * 16 + j] = s;
}

// ---- throughput form: lane (j = lane & 15, q = lane >> 4) holds state words q, 4 + q, 8 + q, 12 + q of sponge base + j ------------
// (generic permutation: the round-0 specialisations of TF_MX_SPONGE assume a fresh sponge, a caller's state is anything)
template <int OP>
__global__ void __launch_bounds__(256) tip5_sponge_mx_kernel(const SpongeArgs g) {
    constexpr int NS = 1;
    TF_MX_PROLOGUE();
    TF_MX_GROUPS(g.count) {
        const bool live = base + j < g.count;
        const long long i = live ? base + j : g.count - 1;
        u64 s[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) s[r] = g.states[i * 16 + 4 * r + q];
        const u64* p = nullptr;
        long long len = 0, steps = 0, produced = 0;
        if constexpr (OP == kSpongeAbsorb) sponge_input(g, i, p, len, steps);
        else if constexpr (OP == kSpongeSqueeze) steps = (g.out_words + 9) / 10;
        for (long long c = 0;; ++c) {
            const bool active = live && (OP == kSpongeIndices ? produced < g.num_indices : c < steps);
            if (__ballot(active) == 0) break;  // uniform over the wave
            u64 t[4] = {s[0], s[1], s[2], s[3]};
            if constexpr (OP == kSpongeAbsorb) {
#pragma unroll
                for (int r = 0; r < 3; ++r)
                    if (active && 4 * r + q < 10) t[r] = sponge_rate_word(p, len, g.pad, c * 10 + 4 * r + q);
            } else if constexpr (OP == kSpongeSqueeze) {
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    const long long w = c * 10 + 4 * r + q;
                    if (active && 4 * r + q < 10 && w < g.out_words) g.out[i * g.out_words + w] = s[r];
                }
            } else {
                // rate word 4 r + qq of sponge j is register r of lane 16 qq + j: three ballots give every lane its sponge's kept set
                u64 v[3];
                bool keep[3];
                u32 kept = 0;
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    v[r] = sponge_value(s[r]);
                    keep[r] = 4 * r + q < 10 && v[r] != gl::P - 1;
                    const unsigned long long b = __ballot(keep[r]) >> j;
#pragma unroll
                    for (int qq = 0; qq < 4; ++qq)
                        if (4 * r + qq < 10) kept |= ((u32)(b >> (16 * qq)) & 1u) << (4 * r + qq);
                }
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    const long long pos = produced + __popc(kept & ((1u << (4 * r + q)) - 1u));
                    if (active && keep[r] && pos < g.num_indices) g.out_idx[i * g.num_indices + pos] = (u32)v[r] & g.mask;
                }
                produced += __popc(kept);
            }
            tip5_permutation_mx<NS>(t, &lds, a, q);
            if (active) {
#pragma unroll
                for (int r = 0; r < 4; ++r) s[r] = t[r];
            }
        }
        if (live) {
#pragma unroll
            for (int r = 0; r < 4; ++r) g.states[i * 16 + 4 * r + q] = s[r];
        }
    }
}

}  // namespace tfk
