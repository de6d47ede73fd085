// tf_mmr.hip -- planner and launchers of the batched Merkle Mountain Range operations (mmr_kernels.h), with their host flavours:
// util_types/mmr/mmr_accumulator.rs, mmr_membership_proof.rs, shared_basic.rs.
#include "tf_internal.h"

#include <unordered_map>

// As tf_proof.hip: this unit has its own copy of the Tip5 constants, in a namespace of its own, uploaded once per device.
namespace tfm {
#include "mmr_kernels.h"
}

namespace tfi {

namespace {
using tfm::tfk::MmrChain;
constexpr u64 kMaxLeafs = 1ull << 63;  // mmr.rs:12-13

std::mutex g_consts_mu;
bool g_consts_ready[kMaxDevices];

int ensure_mmr_consts(int dev) {
    std::lock_guard<std::mutex> lk(g_consts_mu);
    if (g_consts_ready[dev]) return TF_OK;
    tfm::tfk::Tip5Consts c;
    for (int i = 0; i < 80; ++i) c.rc[i] = gl::to_mont(kRoundConstants[i]);
    HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(tfm::tfk::g_tip5), &c, sizeof(c)));
    tfm::tfk::Tip5MxConsts mx;
    tfm::tfk::fill_tip5_mx(mx, c.rc);
    HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(tfm::tfk::g_tip5_mx), &mx, sizeof(mx)));
    HIPCHK(hipDeviceSynchronize());
    g_consts_ready[dev] = true;
    return TF_OK;
}

int ctx_dev(int* dev) {
    DeviceCtx* ctx = nullptr;
    TRY(current_ctx(&ctx));
    *dev = (int)(ctx - g_ctx);
    return ensure_mmr_consts(*dev);
}

// Host-built words (descriptors, move lists) reach the device through pinned staging: the _dev forms never wait for their stream.
// The device copy is freed on the stream when the Upload goes out of scope, after the launches that read it are enqueued.
struct Upload {
    void* d = nullptr;
    hipStream_t s = nullptr;
    ~Upload() {
        if (d) (void)hipFreeAsync(d, s);
    }
    int put(int dev, const void* host, size_t bytes, hipStream_t st) {
        s = st;
        if (!bytes) return TF_OK;
        Staging stg;
        TRY(stage_acquire(dev, bytes, &stg));
        std::memcpy(stg.p, host, bytes);
        hipError_t e = pool_malloc_async(&d, bytes, s);
        if (e != hipSuccess) {
            stage_release(dev, stg, s);
            d = nullptr;
            return hip_fail(e, "pool_malloc_async(mmr descriptors)", __FILE__, __LINE__);
        }
        e = hipMemcpyAsync(d, stg.p, bytes, hipMemcpyHostToDevice, s);
        stage_release(dev, stg, s);
        if (e != hipSuccess) return hip_fail(e, "hipMemcpyAsync(mmr descriptors)", __FILE__, __LINE__);
        return TF_OK;
    }
};

struct Temp {  // stream-ordered device work space
    u64* p = nullptr;
    hipStream_t s;
    explicit Temp(hipStream_t st) : s(st) {}
    int alloc(size_t words) {
        if (!words) return TF_OK;
        const hipError_t e = pool_malloc_async(reinterpret_cast<void**>(&p), words * sizeof(u64), s);
        if (e != hipSuccess) return hip_fail(e, "pool_malloc_async(mmr work space)", __FILE__, __LINE__);
        return TF_OK;
    }
    ~Temp() {
        if (p) (void)hipFreeAsync(p, s);
    }
};

inline unsigned grid_for(long long threads, int per_block) { return (unsigned)((threads + per_block - 1) / per_block); }

template <int MODE>
int launch_chains(const MmrChain* d_chains, long long n, const u64* init, const u64* sib, const u64* sib2, u64* out, const u64* idx,
                  u64 leaf_count, long long n_peaks, int* statuses, hipStream_t s) {
    if (n == 0) return TF_OK;
    hipLaunchKernelGGL(tfm::tfk::mmr_chain_kernel<MODE>, dim3(grid_for(n, 64)), dim3(256), 0, s, d_chains, n, init, sib, sib2, out, idx,
                       leaf_count, n_peaks, statuses);
    HIPCHK(hipGetLastError());
    return TF_OK;
}

using tfm::tfk::MmrMoveArrays;
constexpr int kSel = tfm::tfk::kMmrSelShift;
int launch_moves(const MmrMoveArrays& arrays, const unsigned long long* d_moves, long long count, hipStream_t s) {
    if (count == 0) return TF_OK;
    hipLaunchKernelGGL(tfm::tfk::mmr_move_digests_kernel, dim3(grid_for(5 * count, 256)), dim3(256), 0, s, arrays, d_moves, count);
    HIPCHK(hipGetLastError());
    return TF_OK;
}
// one source and one destination array (selector 0 on both sides)
int launch_moves(const u64* src, const unsigned long long* d_moves, long long count, u64* dst, hipStream_t s) {
    return launch_moves(MmrMoveArrays{{src, nullptr, nullptr, nullptr}, {dst, nullptr, nullptr, nullptr}}, d_moves, count, s);
}

int check_offsets(const uint64_t* off, size_t n) {
    for (size_t i = 0; i < n; ++i)
        if (off[i + 1] < off[i]) return TF_ERR_INVALID_ARGUMENT;
    return TF_OK;
}

// leaf_index_to_mt_index_and_peak_index (shared_basic.rs:24-62): the peak of leaf i < n
inline u64 peak_index(u64 i, u64 n) {
    const int h = 63 - __builtin_clzll(i ^ n);
    return (u64)(__builtin_popcountll(n) - __builtin_popcountll(n & ((1ull << h) - 1)) - 1);
}
}  // namespace

// ------------------------------------------------------------------------------------ append / build
// One level sweep over the new leafs.  Level h consists of the nodes [s_h, e_h) of that level, s_h = (n >> h) & ~1, e_h = (n + k) >> h:
// the new nodes, preceded by the old peak of height h where bit h of n is set (node (n >> h) - 1, always a left child), so level
// h + 1 is the hash_pairs of level h read from its start.  Level 0 is new_leafs itself: for an even n it is hashed in place, for an
// odd n the pair (old peak, leaf 0) is hashed on its own and the rest from leaf 1.  Levels 1 .. top live in two alternating buffers.
// After each level one move launch takes what is needed from it: the proof siblings (for appended leaf L, node (L >> h) - 1), the
// new peak of that height (the last node of level h where bit h of n + k is set), and the old peak of height h + 1 into the first
// slot of the next level's buffer.  Every move list is built on the host and uploaded once.
int mmr_append_dev(u64 n, const u64* old_peaks, const u64* leafs, size_t k, u64* new_peaks, u64* proofs, hipStream_t s) {
    if (n > kMaxLeafs || k > kMaxLeafs - n) return TF_ERR_INVALID_ARGUMENT;
    if (!new_peaks || (k && !leafs) || (n && !old_peaks)) return TF_ERR_NULL_POINTER;
    const u64 N = n + k;
    const int old_count = __builtin_popcountll(n);
    // index of the peak of height h in the old / new list (peaks above it: the set bits above h; no shift by 64)
    auto old_at = [&](int h) { return h == 63 ? 0ull : (u64)__builtin_popcountll(n >> (h + 1)); };
    auto new_at = [&](int h) { return h == 63 ? 0ull : (u64)__builtin_popcountll(N >> (h + 1)); };
    if (k == 0) {
        if (old_count) HIPCHK(hipMemcpyAsync(new_peaks, old_peaks, 5 * sizeof(u64) * old_count, hipMemcpyDeviceToDevice, s));
        return TF_OK;
    }
    int dev = 0;
    TRY(ctx_dev(&dev));
    // levels with new nodes: h <= top
    int top = 0;
    while (top < 63 && (N >> (top + 1)) > (n >> (top + 1))) ++top;
    std::vector<u64> start(top + 1), end(top + 1);
    u64 even_words = 2, odd_words = 0;  // digests of the two level buffers (the even one also holds level 1's first pair for an odd n)
    for (int h = 0; h <= top; ++h) {
        start[h] = (n >> h) & ~1ull;
        end[h] = N >> h;
        if (h) (h & 1 ? odd_words : even_words) = std::max(h & 1 ? odd_words : even_words, end[h] - start[h]);
    }
    // sources and destinations of the moves
    enum : unsigned long long { S_LEAFS = 0, S_OLD = 1, S_EVEN = 2, S_ODD = 3, D_PROOFS = 0, D_PEAKS = 1, D_EVEN = 2, D_ODD = 3 };
    auto at = [](unsigned long long sel, u64 i) { return (sel << kSel) | i; };
    auto buf_src = [&](int h) { return h == 0 ? (unsigned long long)S_LEAFS : (h & 1 ? S_ODD : S_EVEN); };
    auto buf_dst = [&](int h) { return (unsigned long long)(h & 1 ? D_ODD : D_EVEN); };
    // node x of level h as a source: level 0 is new_leafs (and the old peak of height 0), the others their buffer
    auto node_src = [&](int h, u64 x) -> unsigned long long {
        if (h == 0) return x >= n ? at(S_LEAFS, x - n) : at(S_OLD, old_at(0));
        return at(buf_src(h), x - start[h]);
    };
    std::vector<u64> proof_off(proofs ? k + 1 : 0, 0);  // first digest of each append's proof
    if (proofs)
        for (u64 i = 0; i < k; ++i) proof_off[i + 1] = proof_off[i] + (u64)__builtin_ctzll(~(n + i));
    std::vector<unsigned long long> moves;
    std::vector<size_t> moves_at(top + 2, 0);
    const bool odd_pair = n & 1;  // level 1 starts with hash_pair(old peak of height 0, leaf 0)
    for (int h = 0; h <= top; ++h) {
        moves_at[h] = moves.size() / 2;
        if (h == 0 && odd_pair && top >= 1) moves.insert(moves.end(), {at(S_OLD, old_at(0)), at(D_EVEN, 0), at(S_LEAFS, 0), at(D_EVEN, 1)});
        if (proofs && h < 63) {  // the appended leafs whose proof has a digest h: bits 0 .. h of L set, L = -1 mod 2^(h + 1)
            const u64 m = 2ull << h;
            for (u64 L = n + ((m - 1 - (n & (m - 1))) & (m - 1)); L < N; L += m)
                moves.insert(moves.end(), {node_src(h, (L >> h) - 1), at(D_PROOFS, proof_off[L - n] + (u64)h)});
        }
        if ((N >> h) & 1) moves.insert(moves.end(), {node_src(h, end[h] - 1), at(D_PEAKS, new_at(h))});
        if (h < top && ((n >> (h + 1)) & 1)) moves.insert(moves.end(), {at(S_OLD, old_at(h + 1)), at(buf_dst(h + 1), 0)});
        if (h == top)  // peaks above the sweep are old peaks
            for (int g = top + 1; g < 64; ++g)
                if ((N >> g) & 1) moves.insert(moves.end(), {at(S_OLD, old_at(g)), at(D_PEAKS, new_at(g))});
    }
    moves_at[top + 1] = moves.size() / 2;
    Upload up;
    TRY(up.put(dev, moves.data(), moves.size() * sizeof(unsigned long long), s));
    const auto* dm = static_cast<const unsigned long long*>(up.d);
    Temp even(s), odd(s);
    TRY(even.alloc(5 * even_words));
    TRY(odd.alloc(5 * odd_words));
    const MmrMoveArrays arrays{{leafs, old_peaks, even.p, odd.p}, {proofs, new_peaks, even.p, odd.p}};
    auto level = [&](int h) { return h & 1 ? odd.p : even.p; };
    for (int h = 0; h <= top; ++h) {
        TRY(launch_moves(arrays, dm + 2 * moves_at[h], (long long)(moves_at[h + 1] - moves_at[h]), s));
        if (h == top) break;
        // level h + 1: its new nodes start after the old peak of height h + 1, if there is one
        u64* dst = level(h + 1) + 5 * ((n >> (h + 1)) - start[h + 1]);
        const size_t count = (size_t)(end[h + 1] - (n >> (h + 1)));
        if (h > 0) TRY(tip5_hash_pairs_dev(level(h), dst, count, s));
        else if (!odd_pair) TRY(tip5_hash_pairs_dev(leafs, dst, count, s));
        else {
            TRY(tip5_hash_pairs_dev(even.p, dst, 1, s));
            TRY(tip5_hash_pairs_dev(leafs + 5, dst + 5, count - 1, s));
        }
    }
    return TF_OK;
}

// ------------------------------------------------------------------------------------ bag_peaks
int mmr_bag_peaks_dev(const uint64_t* leaf_counts, size_t n_acc, const u64* peaks, u64* out, hipStream_t s) {
    if (n_acc == 0) return TF_OK;
    if (!leaf_counts || !out) return TF_ERR_NULL_POINTER;
    std::vector<MmrChain> ch(n_acc);
    u64 off = 0;
    for (size_t a = 0; a < n_acc; ++a) {
        if (leaf_counts[a] > kMaxLeafs) return TF_ERR_INVALID_ARGUMENT;
        ch[a] = MmrChain{leaf_counts[a], off, a, 0};
        off += __builtin_popcountll(leaf_counts[a]);
    }
    if (off && !peaks) return TF_ERR_NULL_POINTER;
    // chains of a wave end together: accumulators by peak count
    std::stable_sort(ch.begin(), ch.end(), [](const MmrChain& x, const MmrChain& y) { return __builtin_popcountll(x.a) > __builtin_popcountll(y.a); });
    int dev = 0;
    TRY(ctx_dev(&dev));
    Upload up;
    TRY(up.put(dev, ch.data(), ch.size() * sizeof(MmrChain), s));
    return launch_chains<tfm::tfk::kMmrBag>(static_cast<const MmrChain*>(up.d), (long long)n_acc, nullptr, peaks, nullptr, out, nullptr, 0, 0,
                                            nullptr, s);
}

// ------------------------------------------------------------------------------------ verify
int mmr_verify_dev(u64 leaf_count, const u64* peaks, size_t n_peaks, size_t n, const u64* idx, const u64* digests, const uint64_t* offsets,
                   const u64* paths, int* statuses, uint64_t path_base, hipStream_t s) {
    if (leaf_count > kMaxLeafs) return TF_ERR_INVALID_ARGUMENT;
    if (n == 0) return TF_OK;
    if (!offsets || !idx || !digests || !statuses) return TF_ERR_NULL_POINTER;
    TRY(check_offsets(offsets, n));
    if (offsets[0] < path_base) return TF_ERR_INVALID_ARGUMENT;
    if ((offsets[n] > offsets[0] && !paths) || (n_peaks && !peaks)) return TF_ERR_NULL_POINTER;
    std::vector<MmrChain> ch(n);
    for (size_t p = 0; p < n; ++p) ch[p] = MmrChain{p, offsets[p] - path_base, offsets[p + 1] - offsets[p], 0};
    std::stable_sort(ch.begin(), ch.end(), [](const MmrChain& x, const MmrChain& y) { return x.c > y.c; });
    int dev = 0;
    TRY(ctx_dev(&dev));
    Upload up;
    TRY(up.put(dev, ch.data(), ch.size() * sizeof(MmrChain), s));
    return launch_chains<tfm::tfk::kMmrVerify>(static_cast<const MmrChain*>(up.d), (long long)n, digests, paths, peaks, nullptr, idx, leaf_count,
                                               (long long)n_peaks, statuses, s);
}

// ------------------------------------------------------------------------------------ batch mutation
namespace {
// every argument error of a batch mutation that the host arrays decide (the host flavour checks them before it uploads anything)
int mutate_check(u64 leaf_count, size_t M, const uint64_t* midx, const uint64_t* moff, size_t P, const uint64_t* pidx, const uint64_t* poff,
                 uint64_t mbase, uint64_t pbase) {
    if (leaf_count > kMaxLeafs) return TF_ERR_INVALID_ARGUMENT;
    if ((M && (!midx || !moff)) || (P && (!pidx || !poff))) return TF_ERR_NULL_POINTER;
    if (M) TRY(check_offsets(moff, M));
    if (P) TRY(check_offsets(poff, P));
    if ((M && moff[0] < mbase) || (P && poff[0] < pbase)) return TF_ERR_INVALID_ARGUMENT;
    for (size_t j = 0; j < M; ++j) {
        if (midx[j] >= leaf_count) return TF_ERR_LEAF_INDEX_INVALID;
        if (moff[j + 1] - moff[j] > 63) return TF_ERR_INVALID_ARGUMENT;  // no node of an MMR is that high (the reference's node index overflows)
    }
    for (size_t p = 0; p < P; ++p)
        if (pidx[p] >= leaf_count) return TF_ERR_LEAF_INDEX_INVALID;
    std::vector<u64> sorted(midx, midx + M);
    std::sort(sorted.begin(), sorted.end());
    if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) return TF_ERR_INVALID_ARGUMENT;  // the reference panics
    return TF_OK;
}
}  // namespace

// The reference processes the mutations from last to first through one HashMap of node -> digest (node = (level l, index x of the
// level), the post-order node index of shared_advanced.rs being a bijection of it).  The map's state when mutation j takes its step
// l is decided by the indices alone, so the host resolves every sibling source first: the node's latest writer so far (the smallest
// j' > j that writes it), or j's own path digest.  Mutation j's digest at level l goes to row l of the accumulator table A (one
// digest per mutation and level, mutations ordered by path length so the chains of each level are a prefix); the level launches
// then only hash.  At the end each map node holds the digest of its smallest writer, which is what the own proofs are compared with.
int mmr_mutate_dev(u64 leaf_count, u64* peaks, size_t M, const uint64_t* midx, const u64* leafs, const uint64_t* moff, const u64* mpaths, size_t P,
                   const uint64_t* pidx, const uint64_t* poff, u64* ppaths, int* modified, uint64_t mbase, uint64_t pbase, hipStream_t s) {
    TRY(mutate_check(leaf_count, M, midx, moff, P, pidx, poff, mbase, pbase));
    if ((M && !leafs) || (M && moff[M] > moff[0] && !mpaths) || (P && (!modified || (poff[P] > poff[0] && !ppaths)))) return TF_ERR_NULL_POINTER;
    if (M && peaks == nullptr && P == 0) return TF_OK;  // nothing the call writes depends on the mutations
    if (M == 0 && P == 0) return TF_OK;

    int dev = 0;
    TRY(ctx_dev(&dev));
    if (P) HIPCHK(hipMemsetAsync(modified, 0, P * sizeof(int), s));
    if (M == 0) return TF_OK;

    // slots: mutations by path length, longest first
    std::vector<u64> order(M), slot(M), len(M);
    u64 Lmax = 0;
    for (size_t j = 0; j < M; ++j) {
        order[j] = j;
        len[j] = moff[j + 1] - moff[j];
        Lmax = std::max(Lmax, len[j]);
    }
    std::stable_sort(order.begin(), order.end(), [&](u64 x, u64 y) { return len[x] > len[y]; });
    for (size_t r = 0; r < M; ++r) slot[order[r]] = r;
    std::vector<u64> active(Lmax + 1, 0);  // active[l] = mutations whose step l exists (a prefix of the slots)
    for (size_t j = 0; j < M; ++j)
        for (u64 l = 0; l < len[j]; ++l) ++active[l];

    // the map, one per level: node x of level l -> its latest writer
    std::vector<std::unordered_map<u64, u64>> map(Lmax + 1);
    std::vector<std::vector<MmrChain>> steps(Lmax);
    for (u64 l = 0; l < Lmax; ++l) steps[l].resize(active[l]);
    for (size_t jj = M; jj-- > 0;) {
        const u64 x = midx[jj];
        map[0][x] = jj;
        for (u64 l = 0; l < len[jj]; ++l) {
            const auto it = map[l].find((x >> l) ^ 1);
            const u64 b = it != map[l].end() ? (tfm::tfk::kMmrFromAcc | slot[it->second]) : (moff[jj] - mbase + l);
            steps[l][slot[jj]] = MmrChain{0, b, (x >> l) & 1, 0};
            if (l + 1 < len[jj]) map[l + 1][x >> (l + 1)] = jj;
        }
    }
    // descriptors of every level, then the moves (leafs -> row 0, the peaks' tops), then the own-proof fixes, in one upload
    std::vector<unsigned long long> words;
    std::vector<size_t> step_at(Lmax + 1, 0);
    for (u64 l = 0; l < Lmax; ++l) {
        step_at[l] = words.size();
        const auto* w = reinterpret_cast<const unsigned long long*>(steps[l].data());
        words.insert(words.end(), w, w + 4 * steps[l].size());
    }
    const size_t leaf_moves_at = words.size();
    for (size_t j = 0; j < M; ++j) words.insert(words.end(), {j, slot[j]});
    const size_t peak_moves_at = words.size();
    if (peaks) {
        std::unordered_map<u64, u64> top;  // peak -> smallest mutation in it
        for (size_t j = M; j-- > 0;) top[peak_index(midx[j], leaf_count)] = j;
        for (const auto& [p, j] : top) words.insert(words.end(), {len[j] * M + slot[j], p});
    }
    const size_t fixes_at = words.size();
    for (size_t p = 0; p < P; ++p) {
        const u64 x = pidx[p];
        for (u64 e = poff[p]; e < poff[p + 1]; ++e) {
            const u64 l = e - poff[p];
            if (l > Lmax) break;
            const auto it = map[l].find((x >> l) ^ 1);
            if (it != map[l].end()) words.insert(words.end(), {e - pbase, l * M + slot[it->second], p});
        }
    }
    const size_t n_fixes = (words.size() - fixes_at) / 3;
    Upload up;
    TRY(up.put(dev, words.data(), words.size() * sizeof(unsigned long long), s));
    const auto* dw = static_cast<const unsigned long long*>(up.d);
    Temp A(s);
    TRY(A.alloc(5 * M * (Lmax + 1)));
    TRY(launch_moves(leafs, dw + leaf_moves_at, (long long)M, A.p, s));
    for (u64 l = 0; l < Lmax; ++l) {
        const u64* row = A.p + 5 * M * l;
        TRY(launch_chains<tfm::tfk::kMmrStep>(reinterpret_cast<const MmrChain*>(dw + step_at[l]), (long long)active[l], row, mpaths, row,
                                              A.p + 5 * M * (l + 1), nullptr, 0, 0, nullptr, s));
    }
    if (peaks) TRY(launch_moves(A.p, dw + peak_moves_at, (long long)((fixes_at - peak_moves_at) / 2), peaks, s));
    if (n_fixes) {
        hipLaunchKernelGGL(tfm::tfk::mmr_update_paths_kernel, dim3(grid_for((long long)n_fixes, 256)), dim3(256), 0, s, dw + fixes_at,
                           (long long)n_fixes, A.p, ppaths, modified);
        HIPCHK(hipGetLastError());
    }
    return TF_OK;
}

// ------------------------------------------------------------------------------------ host flavours
// Upload the inputs (waiting for each upload: pageable memory), run the _dev form on the thread's stream, copy back, synchronise.
namespace {
int up_words(Temp& t, const u64* h, size_t words, hipStream_t s) {
    TRY(t.alloc(words));
    return h && words ? h2d(t.p, h, words, s) : TF_OK;
}
}  // namespace

int mmr_append_host(u64 n, const u64* old_peaks, const u64* leafs, size_t k, u64* new_peaks, u64* proofs) {
    if (n > kMaxLeafs || k > kMaxLeafs - n) return TF_ERR_INVALID_ARGUMENT;
    if (!new_peaks || (k && !leafs) || (n && !old_peaks)) return TF_ERR_NULL_POINTER;
    u64 n_proof = 0;
    if (proofs)
        for (u64 i = 0; i < k; ++i) n_proof += __builtin_ctzll(~(n + i));
    DeviceCtx* ctx = nullptr;
    TRY(current_ctx(&ctx));
    hipStream_t s = host_stream();
    const size_t np_old = __builtin_popcountll(n), np_new = __builtin_popcountll(n + k);
    Temp dold(s), dl(s), dnew(s), dpr(s);
    TRY(up_words(dold, old_peaks, 5 * np_old, s));
    TRY(up_words(dl, leafs, 5 * k, s));
    TRY(dnew.alloc(5 * np_new));
    TRY(dpr.alloc(proofs ? 5 * n_proof : 0));
    u64 dummy = 0;
    TRY(mmr_append_dev(n, np_old ? dold.p : &dummy, k ? dl.p : &dummy, k, np_new ? dnew.p : &dummy, proofs ? (n_proof ? dpr.p : &dummy) : nullptr, s));
    TRY(d2h(new_peaks, dnew.p, 5 * np_new, s));
    if (proofs) TRY(d2h(proofs, dpr.p, 5 * n_proof, s));
    return sync(s);
}

int mmr_bag_peaks_host(const uint64_t* leaf_counts, size_t n_acc, const u64* peaks, u64* out) {
    if (n_acc == 0) return TF_OK;
    if (!leaf_counts || !out) return TF_ERR_NULL_POINTER;
    u64 np = 0;
    for (size_t a = 0; a < n_acc; ++a) {
        if (leaf_counts[a] > kMaxLeafs) return TF_ERR_INVALID_ARGUMENT;
        np += __builtin_popcountll(leaf_counts[a]);
    }
    if (np && !peaks) return TF_ERR_NULL_POINTER;
    DeviceCtx* ctx = nullptr;
    TRY(current_ctx(&ctx));
    hipStream_t s = host_stream();
    Temp dp(s), dout(s);
    TRY(up_words(dp, peaks, 5 * np, s));
    TRY(dout.alloc(5 * n_acc));
    TRY(mmr_bag_peaks_dev(leaf_counts, n_acc, dp.p, dout.p, s));
    TRY(d2h(out, dout.p, 5 * n_acc, s));
    return sync(s);
}

int mmr_verify_host(u64 leaf_count, const u64* peaks, size_t n_peaks, size_t n, const u64* idx, const u64* digests, const uint64_t* offsets,
                    const u64* paths, int* statuses) {
    if (leaf_count > kMaxLeafs) return TF_ERR_INVALID_ARGUMENT;
    if (n == 0) return TF_OK;
    if (!offsets || !idx || !digests || !statuses) return TF_ERR_NULL_POINTER;
    TRY(check_offsets(offsets, n));
    const size_t na = offsets[n] - offsets[0];
    if ((na && !paths) || (n_peaks && !peaks)) return TF_ERR_NULL_POINTER;
    DeviceCtx* ctx = nullptr;
    TRY(current_ctx(&ctx));
    hipStream_t s = host_stream();
    Temp dpk(s), di(s), dd(s), dpa(s), dst(s);
    TRY(up_words(dpk, peaks, 5 * n_peaks, s));
    TRY(up_words(di, idx, n, s));
    TRY(up_words(dd, digests, 5 * n, s));
    TRY(up_words(dpa, na ? paths + 5 * offsets[0] : nullptr, 5 * na, s));
    TRY(dst.alloc((n + 1) / 2));
    TRY(mmr_verify_dev(leaf_count, dpk.p, n_peaks, n, di.p, dd.p, offsets, dpa.p, reinterpret_cast<int*>(dst.p), offsets[0], s));
    HIPCHK(hipMemcpyAsync(statuses, dst.p, n * sizeof(int), hipMemcpyDeviceToHost, s));
    return sync(s);
}

int mmr_mutate_host(u64 leaf_count, u64* peaks, size_t M, const uint64_t* midx, const u64* leafs, const uint64_t* moff, const u64* mpaths, size_t P,
                    const uint64_t* pidx, const uint64_t* poff, u64* ppaths, int* modified) {
    TRY(mutate_check(leaf_count, M, midx, moff, P, pidx, poff, M ? moff[0] : 0, P ? poff[0] : 0));
    const size_t nm = M ? moff[M] - moff[0] : 0, nq = P ? poff[P] - poff[0] : 0, np = peaks ? __builtin_popcountll(leaf_count) : 0;
    if ((M && !leafs) || (nm && !mpaths) || (P && !modified) || (nq && !ppaths)) return TF_ERR_NULL_POINTER;
    DeviceCtx* ctx = nullptr;
    TRY(current_ctx(&ctx));
    hipStream_t s = host_stream();
    Temp dpk(s), dl(s), dm(s), dq(s), dmod(s);
    TRY(up_words(dpk, peaks, 5 * np, s));
    TRY(up_words(dl, leafs, 5 * M, s));
    TRY(up_words(dm, nm ? mpaths + 5 * moff[0] : nullptr, 5 * nm, s));
    TRY(up_words(dq, nq ? ppaths + 5 * poff[0] : nullptr, 5 * nq, s));
    TRY(dmod.alloc((P + 1) / 2));
    u64 dummy = 0;
    TRY(mmr_mutate_dev(leaf_count, peaks ? (np ? dpk.p : &dummy) : nullptr, M, midx, dl.p, moff, dm.p, P, pidx, poff, dq.p,
                       reinterpret_cast<int*>(dmod.p), M ? moff[0] : 0, P ? poff[0] : 0, s));
    if (np) TRY(d2h(peaks, dpk.p, 5 * np, s));
    if (nq) TRY(d2h(ppaths + 5 * poff[0], dq.p, 5 * nq, s));
    if (P) HIPCHK(hipMemcpyAsync(modified, dmod.p, P * sizeof(int), hipMemcpyDeviceToHost, s));
    return sync(s);
}

}  // namespace tfi
