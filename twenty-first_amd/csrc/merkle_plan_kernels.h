// merkle_plan_kernels.h -- MerkleTree::authentication_structure_node_indices (util_types/merkle_tree.rs:449-504) on the device, for
// leaf indices that are device data (what tf_tip5_sponge_sample_indices_dev wrote), and the two kernels that open trees from that plan:
//   merkle_plan_kernel          one workgroup plans one index list in LDS: node indices (descending), their count, the per-level run ends
//   merkle_plan_gather_kernel   out = nodes[plan] for the trees of every list, from heap-ordered node arrays
//   merkle_plan_emit_kernel     merkle_open_emit_kernel driven by the device plan: copies a level's run out while the sweep goes by
// The planner is structure_nodes of tf_merkle_open.hip: sort the nodes n + idx and drop repeats; on every level emit the siblings that
// are not in the set, highest first; halve, drop repeats, go on until the root.  Every output position is a prefix sum (wave ballots
// and a scan over the waves' totals), so the order is the reference's whatever the hardware does; no atomic decides a position.
#pragma once

#include "gl64.h"

namespace tfk {

using gl::u64;
typedef unsigned int u32;

constexpr int kPlanMaxIndices = 8192;  // per list: the sorted set (32 KiB of LDS) and the scan scratch stay within the 64 KiB of static LDS
constexpr int kPlanLevels = 32;        // run ends per list (a tree of 2^31 leafs has 31 levels below the root)
constexpr u32 kPlanPad = 0xFFFFFFFFu;  // sorts behind every node index (and equals the last node of a tree of 2^31 leafs: see the load)

// A workgroup of T threads; T == 64 is one wave, where the compiler knows from __launch_bounds__ that the workgroup fits a wave and
// drops the barrier instruction: what is left of __syncthreads() orders the wave's own LDS accesses.
template <int T>
__device__ __forceinline__ void plan_sync() {
    __syncthreads();
}

// Exclusive prefix sum of `flag` over the workgroup in thread order, *total = the sum.  The caller ends the round with plan_sync<T>()
// before the next call (wave_tot is read by every thread until then).
template <int T>
__device__ __forceinline__ u32 plan_scan(bool flag, u32* wave_tot, u32* total) {
    const unsigned long long b = __ballot(flag);
    const u32 lane = threadIdx.x & 63;
    const u32 pre = (u32)__popcll(b & ((1ull << lane) - 1ull));
    if (T == 64) {
        *total = (u32)__popcll(b);
        return pre;
    }
    const u32 wave = threadIdx.x >> 6;
    if (lane == 0) wave_tot[wave] = (u32)__popcll(b);
    __syncthreads();
    u32 base = 0, sum = 0;
#pragma unroll
    for (u32 w = 0; w < (u32)(T / 64); ++w) {
        const u32 v = wave_tot[w];
        base += w < wave ? v : 0u;
        sum += v;
    }
    *total = sum;
    return base + pre;
}

// cur[0 .. m) sorted ascending -> its distinct values, in place; returns their number.  A kept value moves to a position at or below
// its own, and the only position a later round still reads (the last one of this round, as its left neighbour) is rewritten, if at
// all, with the value it holds.
template <int T>
__device__ __forceinline__ u32 plan_unique(u32* cur, u32 m, u32* wave_tot) {
    u32 kept = 0;
    for (u32 base = 0; base < m; base += T) {
        const u32 i = base + threadIdx.x;
        const bool valid = i < m;
        const u32 v = valid ? cur[i] : 0u;
        const bool keep = valid && (i == 0 || cur[i - 1] != v);
        u32 total;
        const u32 pos = plan_scan<T>(keep, wave_tot, &total);  // (its barrier: every read of this round precedes every write)
        if (keep) cur[kept + pos] = v;
        kept += total;
        plan_sync<T>();
    }
    return kept;
}

// List l = blockIdx.x: k leaf indices at leaf_indices + l * k, of a tree of n = 2^height leafs.  padded = the power of two >= max(k, 1)
// the bitonic network runs on, at most CAP.
//   node_indices + l * stride   the structure's node indices, descending; slots at or beyond `stride` are not written
//   counts[l]                   their number; 0 for a list with an index >= n, which stores TF_ERR_LEAF_INDEX_INVALID (code_index)
//   level_ends + l * 32         (unless null) entry j = structure nodes on the levels of n, n / 2, ..., n >> j nodes; entries at or
//                               above the root repeat the count
// A count above `capacity` stores code_small; *status keeps the first non-zero code.
template <int T, int CAP>
__global__ void __launch_bounds__(T) merkle_plan_kernel(const u32* __restrict__ leaf_indices, u32 k, u32 padded, u32 n, int height,
                                                         u32* __restrict__ node_indices, unsigned long long stride, u32 capacity, u32* __restrict__ counts,
                                                         u32* __restrict__ level_ends, int* status, int code_index, int code_small) {
    static_assert(T % 64 == 0 && CAP % T == 0 && CAP <= kPlanMaxIndices, "whole waves; whole rounds; the LDS budget");
    __shared__ u32 cur[CAP];
    __shared__ u32 wave_tot[T / 64];
    const u32 tid = threadIdx.x;
    const size_t list = blockIdx.x;
    const u32* idx = leaf_indices + list * k;
    u32* out = node_indices + list * stride;
    u32* ends = level_ends ? level_ends + list * kPlanLevels : nullptr;

    // n + idx <= 2^32 - 1 (n <= 2^31).  The pad value may equal that last node: the sort leaves k real values in cur[0 .. k) either way.
    int bad = 0;
    for (u32 i = tid; i < padded; i += T) {
        u32 v = kPlanPad;
        if (i < k) {
            const u32 leaf = idx[i];
            bad |= leaf >= n ? 1 : 0;
            v = n + leaf;
        }
        cur[i] = v;
    }
    if (__syncthreads_or(bad)) {  // (also the barrier behind the load)
        if (tid == 0) {
            counts[list] = 0;
            atomicCAS(status, 0, code_index);
        }
        if (ends && tid < kPlanLevels) ends[tid] = 0;
        return;
    }

    // bitonic network, ascending
    for (u32 size = 2; size <= padded; size <<= 1) {
        for (u32 step = size >> 1; step > 0; step >>= 1) {
            for (u32 t = tid; t < (padded >> 1); t += T) {
                const u32 lo = ((t & ~(step - 1)) << 1) | (t & (step - 1)), hi = lo | step;
                const u32 a = cur[lo], b = cur[hi];
                if ((a > b) == ((lo & size) == 0)) {
                    cur[lo] = b;
                    cur[hi] = a;
                }
            }
            plan_sync<T>();
        }
    }
    u32 m = plan_unique<T>(cur, k, wave_tot);

    u32 count = 0;
    for (int level = 0; level < height; ++level) {
        // the siblings missing from the set, highest first: item j of the scan is cur[m - 1 - j]
        for (u32 base = 0; base < m; base += T) {
            const u32 j = base + tid;
            bool emit = false;
            u32 sib = 0;
            if (j < m) {
                const u32 i = m - 1 - j, v = cur[i];
                sib = v ^ 1u;
                emit = !(sib > v ? (i + 1 < m && cur[i + 1] == sib) : (i > 0 && cur[i - 1] == sib));
            }
            u32 total;
            const u32 pos = plan_scan<T>(emit, wave_tot, &total);
            if (emit && (unsigned long long)(count + pos) < stride) out[count + pos] = sib;
            count += total;
            plan_sync<T>();
        }
        if (ends && tid == 0) ends[level] = count;
        // the parents: halve in place, then drop the repeats
        for (u32 i = tid; i < m; i += T) cur[i] >>= 1;
        plan_sync<T>();
        m = plan_unique<T>(cur, m, wave_tot);
    }
    if (ends && (int)tid >= height && tid < kPlanLevels) ends[tid] = count;
    if (tid == 0) {
        counts[list] = count;
        if (count > capacity) atomicCAS(status, 0, code_small);
    }
}

// out[tree * out_ts + slot * 5 + word] = nodes[tree * nodes_ts + plan[list][slot] * 5 + word], list = tree / trees_per_list, for
// slot < counts[list]; a list whose count is above `capacity` writes nothing.  The grid runs over `bound` slots per tree (the host
// does not know the counts); the digests' five words on consecutive lanes, a grid stride beyond the launch's blocks.
__global__ void __launch_bounds__(256) merkle_plan_gather_kernel(const u64* __restrict__ nodes, long long nodes_ts, const u32* __restrict__ plan,
                                                                long long stride, const u32* __restrict__ counts, u32 capacity,
                                                                long long trees_per_list, long long trees, long long bound,
                                                                u64* __restrict__ out, long long out_ts) {
    const long long per_tree = bound * 5, total = per_tree * trees, step = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += step) {
        const long long tree = i / per_tree, r = i - tree * per_tree, slot = r / 5, w = r - 5 * slot;
        const long long list = tree / trees_per_list;
        const u32 cnt = counts[list];
        if (cnt > capacity || slot >= (long long)cnt) continue;
        const long long node = (long long)plan[list * stride + slot];
        out[tree * out_ts + slot * 5 + w] = nodes[tree * nodes_ts + node * 5 + w];
    }
}

// One level of the sweep (merkle_open_emit_kernel with the plan read from device memory): the run of level `run` of list
// tree / trees_per_list is [level_ends[run - 1] (0 for run 0), last), last = level_ends[run], or the count when to_count is set (the
// top block takes every level from its own up).  A node's digest is at level + tree * level_ts + (node - first_node) * 5 (first_node:
// the first node of a wide level; 0 in the top block, which is heap ordered).  `bound` slots per tree are looked at; threads beyond
// the run leave, and so does every thread of a list whose count is above `capacity`.
__global__ void __launch_bounds__(256) merkle_plan_emit_kernel(const u64* __restrict__ level, long long level_ts, u32 first_node,
                                                              const u32* __restrict__ plan, long long stride, const u32* __restrict__ counts,
                                                              const u32* __restrict__ level_ends, int run, int to_count, u32 capacity,
                                                              long long trees_per_list, long long trees, long long bound,
                                                              u64* __restrict__ out, long long out_ts) {
    const long long per_tree = bound * 5, total = per_tree * trees, step = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += step) {
        const long long tree = i / per_tree, r = i - tree * per_tree, e = r / 5, w = r - 5 * e;
        const long long list = tree / trees_per_list;
        const u32 cnt = counts[list];
        if (cnt > capacity) continue;
        const u32* ends = level_ends + list * kPlanLevels;
        const long long first = run ? (long long)ends[run - 1] : 0, last = to_count ? (long long)cnt : (long long)ends[run];
        const long long slot = first + e;
        if (slot >= last) continue;
        const long long rel = (long long)(plan[list * stride + slot] - first_node);
        out[tree * out_ts + slot * 5 + w] = level[tree * level_ts + rel * 5 + w];
    }
}

}  // namespace tfk
