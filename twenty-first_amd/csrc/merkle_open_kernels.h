// merkle_open_kernels.h -- the one kernel of MerkleTree::{sequential,par}_authentication_structure_from_leafs
// (util_types/merkle_tree.rs:506-542) that tf_tip5.hip does not already have: while the root-only sweep of a batch of trees goes by,
// the digests of the authentication structure are copied out of the level that holds them.  The hashing itself is the sweep's
// (tip5_kernels.h, launched through tf_tip5.hip); nothing here computes a digest.
#pragma once

#include "gl64.h"

namespace tfk {

using gl::u64;

// one wanted node: `rel` = its index within the level being emitted (node - first node of the level; within the top block the
// node index itself), `slot` = its place in the tree's authentication structure (descending node index, merkle_tree.rs:502-503)
struct OpenEntry {
    unsigned rel, slot;
};
static_assert(sizeof(OpenEntry) == 8, "the plan is staged as 8 bytes per structure node");

// out[tree * out_ts + slot * 5 + word] = level[tree * level_ts + rel * 5 + word] for every (tree, plan entry, word): one thread
// each, the five words of a digest on consecutive lanes, a grid stride beyond the launch's blocks.
__global__ void __launch_bounds__(256) merkle_open_emit_kernel(const u64* level, long long level_ts, const OpenEntry* plan, long long count,
                                                              long long batch, u64* out, long long out_ts) {
    const long long per_tree = count * 5, total = per_tree * batch, step = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += step) {
        const long long tree = i / per_tree, r = i - tree * per_tree, e = r / 5, w = r - 5 * e;
        const OpenEntry p = plan[e];
        out[tree * out_ts + (long long)p.slot * 5 + w] = level[tree * level_ts + (long long)p.rel * 5 + w];
    }
}

}  // namespace tfk
