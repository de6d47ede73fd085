// tf_merkle_open.hip -- MerkleTree::{sequential,par}_authentication_structure_from_leafs (util_types/merkle_tree.rs:506-542): the
// authentication structure and the root of a batch of trees from their leafs alone, no node array.
//
// The reference takes every structure node as the frugal root of its own subtree (subtree_leafs, :565-575).  Those subtrees are disjoint
// and cover almost all leafs, so on the device the work is ONE level sweep of the whole tree -- the root-only sweep of merkle_root_dev
// (tf_tip5.hip: launch_hash_pairs down to the level at which the tree narrows, merkle_narrow_levels above it) -- and the wanted nodes are
// copied out as their level goes by (merkle_open_kernels.h):
//   wide levels   ping-pong between two buffers of n / 2 and n / 4 digests per tree; a level's wanted nodes leave by a launch placed right
//                 after the launch that made the level, so stream order has them out before the buffer is written again two levels on;
//   the top       from the level of w nodes on (merkle_narrow_from) every level is built into a heap-ordered block of 2 w digests per
//                 tree (merkle_narrow_levels with a node pointer and copy_input, the form merkle_build_dev runs); all its wanted nodes
//                 leave in one launch and the root is node 1 of the block;
//   leaf level    wanted leafs are read from the caller's array (a tree that is narrow from its leafs is all top block).
// The plan (node -> slot, per level) is built on the host from the host's leaf indices and reaches the device through pinned staging, so
// the _dev form never waits for its stream.
//
// The *_sampled forms (second half of this file) take their leaf indices from DEVICE memory, n_lists lists of k u32 each as the Tip5
// sponges sample them: merkle_plan_kernel (merkle_plan_kernels.h) computes the plan where the indices lie, and the gather from a node
// array and the same sweep run from it.  The host never sees an index or a count; it sizes grids and work space by the bound
// plan_max_nodes, and what depends on the data goes to the caller's status word.
#include "tf_temp.h"
#include "merkle_open_kernels.h"
#include "merkle_plan_kernels.h"

namespace tfi {
namespace {

using tfk::OpenEntry;
constexpr size_t kMaxOpenLeafs = size_t(1) << 31;  // 32-bit plan entries: a node's index within its level

// wide levels of the sweep: levels below the one at which the trees narrow (0: narrow from the leafs)
int wide_levels(size_t n, size_t batch) {
    int j = 0;
    for (long long w = (long long)n; !merkle_narrow_from(w, batch); w /= 2) ++j;
    return j;
}

// Digests of work space the sweep of `batch` trees uses: buffer a (n / 2 per tree, with a wide level), buffer b (n / 4, with two), and the
// top block (2 w per tree, w = n >> wide levels).
struct OpenLayout {
    long long top_w = 0;
    size_t a = 0, b = 0, top = 0;  // digests, all trees together
    size_t digests() const { return a + b + top; }
};
OpenLayout open_layout(size_t n, size_t batch) {
    OpenLayout l;
    const int j = wide_levels(n, batch);
    l.top_w = (long long)(n >> j);
    l.a = j >= 1 ? batch * (n / 2) : 0;
    l.b = j >= 2 ? batch * (n / 4) : 0;
    l.top = batch * 2 * size_t(l.top_w);
    return l;
}

// Bytes the call requests from the pool.  A tree that narrows later keeps a smaller top block, so the digests in use DROP where one
// more tree adds a wide level (2^10 leafs: 16 trees are all top block, 32 n digests; 17 trees use 25.5 n).  The request is the largest
// use of any batch up to this one -- the last batch of every smaller number of wide levels, kCoopMaxCount / (w / 2) trees -- so that
// it never shrinks as the batch grows: work space sized for the largest batch of a prover covers every smaller one.  That batch is
// smaller than this one and uses at most 2 n digests per tree, so both bounds of include/tf_hip.h hold for the request as well.
size_t open_workspace_bytes(size_t n, size_t batch, size_t k_nodes) {
    if (check_leaves(n) || n > kMaxOpenLeafs || batch == 0) return 0;
    size_t digests = open_layout(n, batch).digests();
    const int j = wide_levels(n, batch);
    for (int i = 0; i < j; ++i) {
        const size_t last = size_t(kCoopMaxCount) / ((n >> i) / 2);  // the largest batch that is narrow from the level of n >> i nodes
        if (last) digests = std::max(digests, open_layout(n, last).digests());
    }
    return digests * 5 * sizeof(u64) + k_nodes * sizeof(OpenEntry);
}

int emit(const u64* level, long long level_ts, const OpenEntry* plan, size_t count, size_t batch, u64* out, long long out_ts, hipStream_t s) {
    if (count == 0) return TF_OK;
    const long long total = (long long)(count * batch) * 5;
    const long long blocks = std::min<long long>((total + 255) / 256, 1ll << 20);
    hipLaunchKernelGGL(tfk::merkle_open_emit_kernel, dim3((unsigned)blocks), dim3(256), 0, s, level, level_ts, plan, (long long)count, (long long)batch,
                       out, out_ts);
    HIPCHK(hipGetLastError());
    return TF_OK;
}

// MerkleTree::authentication_structure_node_indices (merkle_tree.rs:449-504; auth_structure_indices of tf_poly.hip restates it with the
// reference's two sets) level by level, for index lists as long as the tree is wide: a node's sibling is needed and not computable
// exactly when the sibling is not itself on a path, and both sets of a level hold nodes of that level only.  cur = the sorted nodes
// of the paths on one level; the level's structure nodes are the siblings missing from it, descending as the reference sorts them.
void structure_nodes(size_t n, const uint64_t* leaf_indices, size_t k, std::vector<unsigned long long>* out) {
    std::vector<unsigned long long> cur(k);
    for (size_t i = 0; i < k; ++i) cur[i] = leaf_indices[i] + n;
    std::sort(cur.begin(), cur.end());
    cur.erase(std::unique(cur.begin(), cur.end()), cur.end());
    out->clear();
    while (!cur.empty() && cur[0] > 1) {
        for (size_t i = cur.size(); i-- > 0;) {
            const unsigned long long sib = cur[i] ^ 1ull;
            const bool on_a_path = sib > cur[i] ? (i + 1 < cur.size() && cur[i + 1] == sib) : (i > 0 && cur[i - 1] == sib);
            if (!on_a_path) out->push_back(sib);
        }
        size_t m = 0;
        for (size_t i = 0; i < cur.size(); ++i)
            if (m == 0 || cur[m - 1] != cur[i] / 2) cur[m++] = cur[i] / 2;
        cur.resize(m);
    }
}

// Everything the entry points decide before a device is needed, in the order include/tf_hip.h gives.  *run: the call has work for the
// device (structure nodes to write, or roots).
int open_args(const void* leafs, size_t n, size_t batch, const uint64_t* leaf_indices, size_t k, const void* out, size_t capacity, size_t* out_count,
              const void* roots, std::vector<unsigned long long>* idx, bool* run) {
    *run = false;
    TRY(check_leaves(n));
    if (n > kMaxOpenLeafs) return TF_ERR_TREE_TOO_HIGH;
    if (leaf_indices)
        for (size_t i = 0; i < k; ++i)
            if (leaf_indices[i] >= n) return TF_ERR_LEAF_INDEX_INVALID;
    if (!leafs || (k && !leaf_indices) || !out_count) return TF_ERR_NULL_POINTER;
    structure_nodes(n, leaf_indices, k, idx);
    *out_count = idx->size();
    if (batch == 0 || !out || capacity == 0) return TF_OK;  // (the sizing call: only the count)
    if (capacity < idx->size()) return TF_ERR_BUFFER_TOO_SMALL;
    *run = !idx->empty() || roots;
    return TF_OK;
}

// the sweep: idx = the structure's node indices (descending), d_out = batch x idx.size() digests, d_roots = batch digests or null
int open_run(const u64* d_leafs, size_t n, size_t batch, const std::vector<unsigned long long>& idx, u64* d_out, u64* d_roots, hipStream_t s) {
    DeviceCtx* ctx = nullptr;
    TRY(current_ctx(&ctx));
    TRY(ensure_tip5(ctx));
    const int dev = (int)(ctx - g_ctx);
    const size_t count = idx.size();
    const OpenLayout lay = open_layout(n, batch);
    const long long N = (long long)n, top_w = lay.top_w, out_ts = 5 * (long long)count;

    // the plan, in slot order: descending node indices put the leaf level first, then level after level, the top block last, so the
    // wanted nodes of a level are one run of it, ending at run_end[level]
    std::vector<OpenEntry> plan(count);
    std::vector<size_t> run_end;  // end of the run of the level of n, n / 2, ... nodes (levels wider than the top block's), in that order
    {
        unsigned long long level_first = (unsigned long long)N;  // first node of the level being filled
        for (size_t slot = 0; slot < count; ++slot) {
            const unsigned long long node = idx[slot];
            while (level_first >= 2ull * (unsigned long long)top_w && node < level_first) {
                run_end.push_back(slot);
                level_first /= 2;
            }
            const bool in_top = node < 2ull * (unsigned long long)top_w;
            plan[slot] = OpenEntry{(unsigned)(in_top ? node : node - level_first), (unsigned)slot};
        }
        while (level_first >= 2ull * (unsigned long long)top_w) {
            run_end.push_back(count);
            level_first /= 2;
        }
    }
    auto run_of = [&](size_t level, size_t* first) {  // level 0 = the leafs, 1 = their parents, ...
        *first = level ? run_end[level - 1] : 0;
        return run_end[level] - *first;
    };

    DevTemp ws(s);
    if (ws.alloc_bytes(open_workspace_bytes(n, batch, count), "merkle open")) return TF_ERR_TREE_TOO_HIGH;  // as merkle_root_dev: merkle_tree.rs:405-410
    u64* a = ws.p;
    u64* b = a + 5 * lay.a;
    u64* top = b + 5 * lay.b;
    // (the plan sits behind the digests of the REQUEST, which may be more than this batch uses: open_workspace_bytes)
    const OpenEntry* d_plan = reinterpret_cast<const OpenEntry*>(reinterpret_cast<const char*>(ws.p) + open_workspace_bytes(n, batch, 0));
    TRY(StagedUpload::copy_to(dev, const_cast<OpenEntry*>(d_plan), plan.data(), count * sizeof(OpenEntry), s, "merkle open plan"));

    const u64* level = d_leafs;  // the level the top block starts from, w digests per tree
    long long w = N, level_ts = 5 * N;
    if (!merkle_narrow_from(N, batch)) {
        size_t first = 0, cnt = run_of(0, &first);
        TRY(emit(d_leafs, 5 * N, d_plan + first, cnt, batch, d_out, out_ts, s));
        w = N / 2;
        TRY(launch_hash_pairs(d_leafs, a, nullptr, w * (long long)batch, w, 5 * N, 5 * w, 0, s));
        for (size_t lv = 1; !merkle_narrow_from(w, batch); ++lv) {
            cnt = run_of(lv, &first);
            TRY(emit(a, 5 * w, d_plan + first, cnt, batch, d_out, out_ts, s));
            const long long nw = w / 2;
            TRY(launch_hash_pairs(a, b, nullptr, nw * (long long)batch, nw, 5 * w, 5 * nw, 0, s));
            std::swap(a, b);
            w = nw;
        }
        level = a;
        level_ts = 5 * w;
    }
    // w == top_w: every level from here on into the top block (the level itself copied to nodes[w .. 2 w)), the roots to d_roots
    TRY(merkle_narrow_levels(level, level_ts, w, top, 10 * w, d_roots, nullptr, batch, true, s));
    const size_t top_first = run_end.empty() ? 0 : run_end.back();
    return emit(top, 10 * w, d_plan + top_first, count - top_first, batch, d_out, out_ts, s);
}

// ------------------------------------------------------------------------------------ leaf indices in device memory
constexpr size_t kPlanMaxK = tfk::kPlanMaxIndices;
constexpr size_t kPlanMaxLists = (size_t(1) << 31) - 1;  // one workgroup per list: the grid's x dimension
constexpr size_t kPlanMaxTrees = size_t(1) << 31;

// Structure nodes on the level of w nodes, at most: they are siblings of distinct path nodes (<= k of them) and lie outside the path
// set, which holds at least as many nodes of the level as they do (<= w / 2).
size_t plan_level_bound(size_t w, size_t k) { return std::min(k, w / 2); }

// Everything the sampled entry points decide before a device is needed, in the order include/tf_hip.h gives
int sampled_args(size_t n, size_t k, size_t n_lists, size_t trees_per_list, const void* d_leaf_indices, const void* d_counts, const int* d_status) {
    TRY(check_leaves(n));
    if (n > kMaxOpenLeafs) return TF_ERR_TREE_TOO_HIGH;
    if (k > kPlanMaxK || n_lists > kPlanMaxLists || (trees_per_list && n_lists > kPlanMaxTrees / trees_per_list)) return TF_ERR_LEN_TOO_LARGE;
    if (!d_status || (n_lists && ((k && !d_leaf_indices) || !d_counts))) return TF_ERR_NULL_POINTER;
    return TF_OK;
}

// the plan of n_lists lists: `stride` u32 of node indices per list, then (sweep only) kPlanLevels run ends per list
size_t plan_words(size_t n_lists, size_t stride, bool with_ends) { return n_lists * (stride + (with_ends ? size_t(tfk::kPlanLevels) : 0)); }
size_t plan_bytes(size_t n_lists, size_t stride, bool with_ends) { return (plan_words(n_lists, stride, with_ends) * sizeof(uint32_t) + 7) & ~size_t(7); }

// One workgroup per list, sized by k: one wave up to 64 indices, 256 threads up to 1024, 1024 threads up to kPlanMaxK.
int launch_plan(size_t n, const uint32_t* d_leaf_indices, size_t k, size_t n_lists, uint32_t* d_node_indices, size_t stride, size_t capacity,
                uint32_t* d_counts, uint32_t* d_level_ends, int* d_status, hipStream_t s) {
    if (n_lists == 0) return TF_OK;
    unsigned padded = 1;
    while (padded < k) padded <<= 1;
    const int height = __builtin_ctzll((unsigned long long)n);
    const unsigned cap = (unsigned)std::min<size_t>(capacity, 0xFFFFFFFFu);  // (a count is far below 2^32: the clamp changes no verdict)
#define TF_PLAN_LAUNCH(T, CAP)                                                                                                                 \
    hipLaunchKernelGGL((tfk::merkle_plan_kernel<T, CAP>), dim3((unsigned)n_lists), dim3(T), 0, s, d_leaf_indices, (unsigned)k, padded, (unsigned)n, \
                       height, d_node_indices, (unsigned long long)stride, cap, d_counts, d_level_ends, d_status, (int)TF_ERR_LEAF_INDEX_INVALID, \
                       (int)TF_ERR_BUFFER_TOO_SMALL)
    if (k <= 64)
        TF_PLAN_LAUNCH(64, 64);
    else if (k <= 1024)
        TF_PLAN_LAUNCH(256, 1024);
    else
        TF_PLAN_LAUNCH(1024, tfk::kPlanMaxIndices);
#undef TF_PLAN_LAUNCH
    HIPCHK(hipGetLastError());
    return TF_OK;
}

unsigned plan_copy_blocks(size_t trees, size_t bound) {
    const long long total = (long long)(trees * bound) * 5;
    return (unsigned)std::min<long long>((total + 255) / 256, 1ll << 20);
}

// emit() from the device plan: level `run` of the sweep (to_count: the top block, every level from `run` up), `bound` slots per tree
int emit_sampled(const u64* level, long long level_ts, size_t first_node, const uint32_t* d_plan, size_t stride, const uint32_t* d_counts,
                 const uint32_t* d_ends, int run, bool to_count, size_t capacity, size_t trees_per_list, size_t trees, size_t bound, u64* out,
                 hipStream_t s) {
    if (bound == 0) return TF_OK;
    hipLaunchKernelGGL(tfk::merkle_plan_emit_kernel, dim3(plan_copy_blocks(trees, bound)), dim3(256), 0, s, level, level_ts, (unsigned)first_node, d_plan,
                       (long long)stride, d_counts, d_ends, run, to_count ? 1 : 0, (unsigned)std::min<size_t>(capacity, 0xFFFFFFFFu),
                       (long long)trees_per_list, (long long)trees, (long long)bound, out, 5 * (long long)capacity);
    HIPCHK(hipGetLastError());
    return TF_OK;
}

size_t sampled_workspace_bytes(size_t n, size_t trees, size_t k, size_t n_lists) {
    const size_t sweep = open_workspace_bytes(n, trees, 0);
    if (!sweep || k > kPlanMaxK || n_lists == 0 || n_lists > kPlanMaxLists) return 0;
    return sweep + plan_bytes(n_lists, merkle_plan_max_nodes(n, k), true);
}

// open_run with the plan made on the device: the same buffers, the same hashing launches, emit_sampled for emit
int open_run_sampled(const u64* d_leafs, size_t n, const uint32_t* d_leaf_indices, size_t k, size_t n_lists, size_t trees_per_list, u64* d_out,
                     size_t capacity, uint32_t* d_counts, u64* d_roots, int* d_status, hipStream_t s) {
    DeviceCtx* ctx = nullptr;
    TRY(current_ctx(&ctx));
    TRY(ensure_tip5(ctx));
    const size_t batch = n_lists * trees_per_list, stride = merkle_plan_max_nodes(n, k);
    const OpenLayout lay = open_layout(n, batch);
    const long long N = (long long)n, top_w = lay.top_w;

    DevTemp ws(s);
    if (ws.alloc_bytes(sampled_workspace_bytes(n, batch, k, n_lists), "merkle open (sampled)")) return TF_ERR_TREE_TOO_HIGH;
    u64* a = ws.p;
    u64* b = a + 5 * lay.a;
    u64* top = b + 5 * lay.b;
    // (the plan sits behind the digests of the REQUEST, as in open_run)
    uint32_t* d_plan = reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(ws.p) + open_workspace_bytes(n, batch, 0));
    uint32_t* d_ends = d_plan + n_lists * stride;
    TRY(launch_plan(n, d_leaf_indices, k, n_lists, d_plan, stride, capacity, d_counts, d_ends, d_status, s));
    if (stride == 0 && !d_roots) return TF_OK;  // no index, or a tree that is its root: the counts are all there is
    auto emit_level = [&](const u64* level, long long level_ts, long long w, int run) {
        return emit_sampled(level, level_ts, (size_t)w, d_plan, stride, d_counts, d_ends, run, false, capacity, trees_per_list, batch,
                            plan_level_bound((size_t)w, k), d_out, s);
    };

    const u64* level = d_leafs;
    long long w = N, level_ts = 5 * N;
    int run = 0;
    if (!merkle_narrow_from(N, batch)) {
        TRY(emit_level(d_leafs, 5 * N, N, run++));
        w = N / 2;
        TRY(launch_hash_pairs(d_leafs, a, nullptr, w * (long long)batch, w, 5 * N, 5 * w, 0, s));
        while (!merkle_narrow_from(w, batch)) {
            TRY(emit_level(a, 5 * w, w, run++));
            const long long nw = w / 2;
            TRY(launch_hash_pairs(a, b, nullptr, nw * (long long)batch, nw, 5 * w, 5 * nw, 0, s));
            std::swap(a, b);
            w = nw;
        }
        level = a;
        level_ts = 5 * w;
    }
    TRY(merkle_narrow_levels(level, level_ts, w, top, 10 * w, d_roots, nullptr, batch, true, s));
    size_t top_bound = 0;
    for (size_t lw = (size_t)top_w; lw > 1; lw /= 2) top_bound += plan_level_bound(lw, k);
    return emit_sampled(top, 10 * w, 0, d_plan, stride, d_counts, d_ends, run, true, capacity, trees_per_list, batch, top_bound, d_out, s);
}

}  // namespace

size_t merkle_open_workspace(size_t n, size_t batch, size_t k_nodes) { return open_workspace_bytes(n, batch, k_nodes); }

int merkle_open_dev(const u64* d_leafs, size_t n, size_t batch, const uint64_t* leaf_indices, size_t k, u64* d_out, size_t capacity, size_t* out_count,
                    u64* d_roots, hipStream_t s) {
    std::vector<unsigned long long> idx;
    bool run = false;
    TRY(open_args(d_leafs, n, batch, leaf_indices, k, d_out, capacity, out_count, d_roots, &idx, &run));
    if (!run) return TF_OK;
    return open_run(d_leafs, n, batch, idx, d_out, d_roots, s);
}

int merkle_open_host(const u64* leafs, size_t n, size_t batch, const uint64_t* leaf_indices, size_t k, u64* out, size_t capacity, size_t* out_count,
                     u64* roots) {
    std::vector<unsigned long long> idx;
    bool run = false;
    TRY(open_args(leafs, n, batch, leaf_indices, k, out, capacity, out_count, roots, &idx, &run));
    if (!run) return TF_OK;
    DeviceCtx* ctx = nullptr;
    TRY(current_ctx(&ctx));
    hipStream_t s = host_stream();
    DevTemp din(s), dout(s), droots(s);
    const size_t out_words = batch * idx.size() * 5;
    if (din.alloc(n * batch * 5, "merkle open leafs")) return TF_ERR_TREE_TOO_HIGH;
    TRY(dout.alloc(out_words, "merkle open output"));
    TRY(droots.alloc(roots ? batch * 5 : 0, "merkle open roots"));
    TRY(h2d(din.p, leafs, n * batch * 5, s));
    TRY(open_run(din.p, n, batch, idx, dout.p, droots.p, s));
    TRY(d2h(out, dout.p, out_words, s));
    if (roots) TRY(d2h(roots, droots.p, batch * 5, s));
    return sync(s);
}

size_t merkle_plan_max_nodes(size_t n, size_t k) {
    if (check_leaves(n) || n > kMaxOpenLeafs || k > kPlanMaxK) return 0;
    size_t sum = 0;
    for (size_t w = n; w > 1; w /= 2) sum += plan_level_bound(w, k);
    return sum;
}

int merkle_plan_dev(size_t n, const uint32_t* d_leaf_indices, size_t k, size_t n_lists, uint32_t* d_node_indices, size_t capacity, uint32_t* d_counts,
                    uint32_t* d_level_ends, hipStream_t s, int* d_status) {
    TRY(sampled_args(n, k, n_lists, 0, d_leaf_indices, d_counts, d_status));
    if (n_lists && capacity && !d_node_indices) return TF_ERR_NULL_POINTER;
    if (n_lists == 0) return TF_OK;
    DeviceCtx* ctx = nullptr;
    TRY(current_ctx(&ctx));
    return launch_plan(n, d_leaf_indices, k, n_lists, d_node_indices, capacity, capacity, d_counts, d_level_ends, d_status, s);
}

int merkle_nodes_sampled_dev(const u64* d_nodes, size_t n, const uint32_t* d_leaf_indices, size_t k, size_t n_lists, size_t trees_per_list,
                             u64* d_out, size_t capacity, uint32_t* d_counts, hipStream_t s, int* d_status) {
    TRY(sampled_args(n, k, n_lists, trees_per_list, d_leaf_indices, d_counts, d_status));
    if (n_lists && trees_per_list && (!d_nodes || (capacity && !d_out))) return TF_ERR_NULL_POINTER;
    if (n_lists == 0 || trees_per_list == 0) return TF_OK;
    DeviceCtx* ctx = nullptr;
    TRY(current_ctx(&ctx));
    const size_t stride = merkle_plan_max_nodes(n, k), trees = n_lists * trees_per_list;
    DevTemp plan(s);
    TRY(plan.alloc_bytes(plan_bytes(n_lists, stride, false), "merkle plan"));
    TRY(launch_plan(n, d_leaf_indices, k, n_lists, plan.as<uint32_t>(), stride, capacity, d_counts, nullptr, d_status, s));
    const size_t bound = std::min(stride, capacity);  // (a list with more nodes than `capacity` writes nothing)
    if (bound == 0) return TF_OK;
    hipLaunchKernelGGL(tfk::merkle_plan_gather_kernel, dim3(plan_copy_blocks(trees, bound)), dim3(256), 0, s, d_nodes, 10 * (long long)n,
                       plan.as<const uint32_t>(), (long long)stride, d_counts, (unsigned)std::min<size_t>(capacity, 0xFFFFFFFFu),
                       (long long)trees_per_list, (long long)trees, (long long)bound, d_out, 5 * (long long)capacity);
    HIPCHK(hipGetLastError());
    return TF_OK;
}

int merkle_open_sampled_dev(const u64* d_leafs, size_t n, const uint32_t* d_leaf_indices, size_t k, size_t n_lists, size_t trees_per_list,
                            u64* d_out, size_t capacity, uint32_t* d_counts, u64* d_roots, hipStream_t s, int* d_status) {
    TRY(sampled_args(n, k, n_lists, trees_per_list, d_leaf_indices, d_counts, d_status));
    if (n_lists && trees_per_list && (!d_leafs || (capacity && !d_out))) return TF_ERR_NULL_POINTER;
    if (n_lists == 0 || trees_per_list == 0) return TF_OK;
    return open_run_sampled(d_leafs, n, d_leaf_indices, k, n_lists, trees_per_list, d_out, capacity, d_counts, d_roots, d_status, s);
}

size_t merkle_open_sampled_workspace(size_t n, size_t trees, size_t k, size_t n_lists) { return sampled_workspace_bytes(n, trees, k, n_lists); }

}  // namespace tfi
