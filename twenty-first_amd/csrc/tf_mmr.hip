// tf_mmr.hip -- planner and launchers of the batched Merkle Mountain Range operations (mmr_kernels.h), with their host flavours:
// util_types/mmr/mmr_accumulator.rs, mmr_membership_proof.rs, shared_basic.rs.
#include "tf_temp.h"

#include <unordered_map>

// As tf_proof.hip: this unit has its own copy of the Tip5 constants, in a namespace of its own, uploaded once per device.
namespace tfm {
#include "mmr_kernels.h"
}

namespace tfi {

namespace {
using tfm::tfk::MmrChain;
constexpr u64 kMaxLeafs = 1ull << 63;  // mmr.rs:12-13

Tip5ConstsOnce g_consts;
int ctx_dev(int* dev) { return g_consts.ensure(dev, tfm::tfk::g_tip5, tfm::tfk::g_tip5_mx); }

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
//
// The successor proof and the proof update (below) are the same sweep with other digests taken from it: a SweepWant names node `index`
// of level `level`, or with old_peak the old peak of that height, and the digest of `wanted` it goes to.  They pass no proofs, may
// pass no new_peaks (the peaks are then not written), and may pass no old_peaks: the nodes that cover old leafs then hold
// unspecified words, and no want may name one.
namespace {
struct SweepWant {
    int level;
    u64 index;
    bool old_peak;
    u64 dst;
};
int mmr_sweep(u64 n, const u64* old_peaks, const u64* leafs, size_t k, u64* new_peaks, u64* proofs, const std::vector<SweepWant>& wants, u64* wanted,
              hipStream_t s);
}  // namespace

int mmr_append_dev(u64 n, const u64* old_peaks, const u64* leafs, size_t k, u64* new_peaks, u64* proofs, hipStream_t s) {
    if (n > kMaxLeafs || k > kMaxLeafs - n) return TF_ERR_INVALID_ARGUMENT;
    if (!new_peaks || (k && !leafs) || (n && !old_peaks)) return TF_ERR_NULL_POINTER;
    return mmr_sweep(n, old_peaks, leafs, k, new_peaks, proofs, {}, nullptr, s);
}

namespace {
int mmr_sweep(u64 n, const u64* old_peaks, const u64* leafs, size_t k, u64* new_peaks, u64* proofs, const std::vector<SweepWant>& wants, u64* wanted,
              hipStream_t s) {
    const u64 N = n + k;
    const int old_count = __builtin_popcountll(n);
    // index of the peak of height h in the old / new list (peaks above it: the set bits above h; no shift by 64)
    auto old_at = [&](int h) { return h == 63 ? 0ull : (u64)__builtin_popcountll(n >> (h + 1)); };
    auto new_at = [&](int h) { return h == 63 ? 0ull : (u64)__builtin_popcountll(N >> (h + 1)); };
    if (k == 0) {
        if (old_count && new_peaks) HIPCHK(hipMemcpyAsync(new_peaks, old_peaks, 5 * sizeof(u64) * old_count, hipMemcpyDeviceToDevice, s));
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
    std::vector<std::vector<unsigned long long>> want_moves(wants.empty() ? 0 : top + 1);  // by the level whose launch makes them
    for (const SweepWant& w : wants) {
        if (!w.old_peak && (w.level > top || w.index < start[w.level] || w.index >= end[w.level])) return TF_ERR_INTERNAL;  // not a node of the sweep
        auto& list = want_moves[std::min(w.level, top)];
        list.insert(list.end(), {w.old_peak ? at(S_OLD, old_at(w.level)) : node_src(w.level, w.index), at(D_PROOFS, w.dst)});
    }
    for (int h = 0; h <= top; ++h) {
        moves_at[h] = moves.size() / 2;
        if (h == 0 && odd_pair && top >= 1) {
            if (old_peaks) moves.insert(moves.end(), {at(S_OLD, old_at(0)), at(D_EVEN, 0)});
            moves.insert(moves.end(), {at(S_LEAFS, 0), at(D_EVEN, 1)});
        }
        if (!wants.empty()) moves.insert(moves.end(), want_moves[h].begin(), want_moves[h].end());
        if (proofs && h < 63) {  // the appended leafs whose proof has a digest h: bits 0 .. h of L set, L = -1 mod 2^(h + 1)
            const u64 m = 2ull << h;
            for (u64 L = n + ((m - 1 - (n & (m - 1))) & (m - 1)); L < N; L += m)
                moves.insert(moves.end(), {node_src(h, (L >> h) - 1), at(D_PROOFS, proof_off[L - n] + (u64)h)});
        }
        if (new_peaks && ((N >> h) & 1)) moves.insert(moves.end(), {node_src(h, end[h] - 1), at(D_PEAKS, new_at(h))});
        if (old_peaks && h < top && ((n >> (h + 1)) & 1)) moves.insert(moves.end(), {at(S_OLD, old_at(h + 1)), at(buf_dst(h + 1), 0)});
        if (new_peaks && h == top)  // peaks above the sweep are old peaks
            for (int g = top + 1; g < 64; ++g)
                if ((N >> g) & 1) moves.insert(moves.end(), {at(S_OLD, old_at(g)), at(D_PEAKS, new_at(g))});
    }
    moves_at[top + 1] = moves.size() / 2;
    StagedUpload up(s);
    TRY(up.put(dev, moves.data(), moves.size() * sizeof(unsigned long long), "mmr move list"));
    const auto* dm = up.as<unsigned long long>();
    DevTemp even(s), odd(s);
    TRY(even.alloc(5 * even_words, "mmr sweep levels"));
    TRY(odd.alloc(5 * odd_words, "mmr sweep levels"));
    const MmrMoveArrays arrays{{leafs, old_peaks, even.p, odd.p}, {wants.empty() ? proofs : wanted, new_peaks, even.p, odd.p}};
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
}  // namespace

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
    StagedUpload up(s);
    TRY(up.put(dev, ch.data(), ch.size() * sizeof(MmrChain), "mmr bag chains"));
    return launch_chains<tfm::tfk::kMmrBag>(up.as<MmrChain>(), (long long)n_acc, nullptr, peaks, nullptr, out, nullptr, 0, 0,
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
    StagedUpload up(s);
    TRY(up.put(dev, ch.data(), ch.size() * sizeof(MmrChain), "mmr verify chains"));
    return launch_chains<tfm::tfk::kMmrVerify>(up.as<MmrChain>(), (long long)n, digests, paths, peaks, nullptr, idx, leaf_count,
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
    StagedUpload up(s);
    TRY(up.put(dev, words.data(), words.size() * sizeof(unsigned long long), "mmr mutation plan"));
    const auto* dw = up.as<unsigned long long>();
    DevTemp A(s);
    TRY(A.alloc(5 * M * (Lmax + 1), "mmr mutation chains"));
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

// ------------------------------------------------------------------------------------ successor proofs
// MmrSuccessorProof (mmr_successor_proof.rs).  With t = trailing_zeros(n) and H the highest bit in which n and N = n + k differ,
// the proof starts with the root of the first 2^t new leafs, node (t, n >> t) of the sweep, and climbs to level H: where the node
// (g, n >> g) is a left child its sibling (g, (n >> g) + 1) is a sweep node of new leafs only and joins the proof, where it is a
// right child the sibling is the old peak of height g, which the verifier has.
namespace {
inline int top_difference(u64 n, u64 N) { return 63 - __builtin_clzll(n ^ N); }  // n != N
}  // namespace

size_t mmr_successor_proof_len(u64 n, u64 k) {
    if (n > kMaxLeafs || k > kMaxLeafs - n || n == 0) return 0;
    const int t = __builtin_ctzll(n);
    if (k < (1ull << t)) return 0;
    const int H = top_difference(n, n + k);  // > t: the first 2^t new leafs carry into bit t + 1 or above
    return (size_t)(1 + (H - t) - __builtin_popcountll((n >> t) & ((1ull << (H - t)) - 1)));
}

int mmr_successor_new_dev(u64 n, const u64* old_peaks, const u64* leafs, size_t k, u64* paths_out, u64* new_peaks, hipStream_t s) {
    if (n > kMaxLeafs || k > kMaxLeafs - n) return TF_ERR_INVALID_ARGUMENT;
    const size_t len = mmr_successor_proof_len(n, k);
    if ((len && !paths_out) || (k && (len || new_peaks) && !leafs) || (n && new_peaks && !old_peaks)) return TF_ERR_NULL_POINTER;
    if (!len) return new_peaks ? mmr_sweep(n, old_peaks, leafs, k, new_peaks, nullptr, {}, nullptr, s) : TF_OK;
    const int t = __builtin_ctzll(n), H = top_difference(n, n + k);
    std::vector<SweepWant> wants{{t, n >> t, false, 0}};
    for (int g = t; g < H; ++g)
        if (!((n >> g) & 1)) wants.push_back({g, (n >> g) + 1, false, (u64)wants.size()});
    return mmr_sweep(n, new_peaks ? old_peaks : nullptr, leafs, k, new_peaks, nullptr, wants, paths_out, s);
}

// One chain per proof (mmr_kernels.h: mmr_successor_kernel); the host settles what the counts settle, in verify_internal's order.
int mmr_successor_verify_dev(size_t P, const uint64_t* old_counts, const uint64_t* new_counts, const uint64_t* old_off, const u64* old_peaks,
                             const uint64_t* new_off, const u64* new_peaks, const uint64_t* path_off, const u64* paths, int* statuses, uint64_t old_base,
                             uint64_t new_base, uint64_t path_base, hipStream_t s) {
    if (P == 0) return TF_OK;
    if (!old_counts || !new_counts || !old_off || !new_off || !path_off || !statuses) return TF_ERR_NULL_POINTER;
    for (size_t p = 0; p < P; ++p)
        if (old_counts[p] > kMaxLeafs || new_counts[p] > kMaxLeafs) return TF_ERR_INVALID_ARGUMENT;
    TRY(check_offsets(old_off, P));
    TRY(check_offsets(new_off, P));
    TRY(check_offsets(path_off, P));
    if (old_off[0] < old_base || new_off[0] < new_base || path_off[0] < path_base) return TF_ERR_INVALID_ARGUMENT;
    if ((old_off[P] > old_off[0] && !old_peaks) || (new_off[P] > new_off[0] && !new_peaks) || (path_off[P] > path_off[0] && !paths))
        return TF_ERR_NULL_POINTER;
    std::vector<tfm::tfk::MmrSuccessorChain> ch(P);
    for (size_t p = 0; p < P; ++p) {
        const u64 n = old_counts[p], N = new_counts[p], n_old = old_off[p + 1] - old_off[p], n_new = new_off[p + 1] - new_off[p];
        const u64 len = path_off[p + 1] - path_off[p];
        tfm::tfk::MmrSuccessorChain c{p, 0, path_off[p] - path_base, old_off[p] - old_base, new_off[p] - new_base, (unsigned)n_old, 0, 0, 0, 0};
        const unsigned empty_path = len ? TF_ERR_MMR_SUCCESSOR_PATH_TOO_LONG : TF_OK;
        if ((u64)__builtin_popcountll(n) != n_old) c.verdict = TF_ERR_MMR_INCONSISTENT_OLD;
        else if ((u64)__builtin_popcountll(N) != n_new) c.verdict = TF_ERR_MMR_INCONSISTENT_NEW;
        else if (n == 0) c.verdict = empty_path;
        else if (n == N) {
            c.cmp = (unsigned)n_old;
            c.verdict = empty_path;
        } else if (n > N) c.verdict = TF_ERR_MMR_OLD_HAS_MORE_LEAFS;
        else {
            const int t = __builtin_ctzll(n), H = top_difference(n, N);
            c.cmp = H == 63 ? 0u : (unsigned)__builtin_popcountll(n >> (H + 1));  // the peaks above the first difference
            const u64 want = mmr_successor_proof_len(n, N - n);
            if (want == 0) c.verdict = empty_path;  // the new leafs do not reach the lowest old peak
            else if (len < want) c.verdict = TF_ERR_MMR_SUCCESSOR_PATH_TOO_SHORT;
            else if (len > want) c.verdict = TF_ERR_MMR_SUCCESSOR_PATH_TOO_LONG;
            else {
                c.steps = (unsigned)(H - t);
                c.bits = n >> t;
            }
        }
        ch[p] = c;
    }
    std::stable_sort(ch.begin(), ch.end(), [](const auto& x, const auto& y) { return x.steps > y.steps; });
    int dev = 0;
    TRY(ctx_dev(&dev));
    StagedUpload up(s);
    TRY(up.put(dev, ch.data(), ch.size() * sizeof(ch[0]), "mmr successor chains"));
    hipLaunchKernelGGL(tfm::tfk::mmr_successor_kernel, dim3(grid_for((long long)P, 64)), dim3(256), 0, s,
                       up.as<tfm::tfk::MmrSuccessorChain>(), (long long)P, old_peaks, new_peaks, paths, statuses);
    HIPCHK(hipGetLastError());
    return TF_OK;
}

// ------------------------------------------------------------------------------------ membership proofs under appends
// k rounds of MmrMembershipProof::batch_update_from_append (mmr_membership_proof.rs:224-331) and append.  The proof of leaf i has
// h0 = bit_length(i ^ n) - 1 digests in the MMR of n leafs (the height of its peak) and max(h0, H) in that of N = n + k, the old
// path first.  The new digests are those of levels h0 .. H - 1: at level h0 the sweep node (h0, n >> h0), which grows beside the old
// peak; above it the sibling of node (g, n >> g), which is the old peak of height g or the sweep node (g, (n >> g) + 1).  So every
// proof under one old peak receives the same suffix: the sweep fills one list per old peak, and mmr_gather_paths_kernel writes each
// proof as its old path and its peak's list.
int mmr_update_proofs_dev(u64 n, const u64* old_peaks, const u64* leafs, size_t k, size_t P, const uint64_t* own_idx, const uint64_t* own_off,
                          const u64* own_paths, uint64_t* out_off, u64* out_paths, size_t capacity, int* modified, u64* new_peaks, uint64_t own_base,
                          hipStream_t s) {
    if (n > kMaxLeafs || k > kMaxLeafs - n) return TF_ERR_INVALID_ARGUMENT;
    if (!out_off || (P && (!own_idx || !own_off))) return TF_ERR_NULL_POINTER;
    for (size_t p = 0; p < P; ++p)
        if (own_idx[p] >= n) return TF_ERR_LEAF_INDEX_INVALID;
    for (size_t p = 0; p < P; ++p)
        if (own_off[p + 1] >= own_off[p] && own_off[p + 1] - own_off[p] != (u64)top_difference(own_idx[p], n))
            return TF_ERR_MMR_AUTH_PATH_LENGTH_MISMATCH;
    if (P) TRY(check_offsets(own_off, P));
    if (P && own_off[0] < own_base) return TF_ERR_INVALID_ARGUMENT;
    const u64 N = n + k;
    const int H = k ? top_difference(n, N) : -1;
    out_off[0] = 0;
    bool grows = false;
    for (size_t p = 0; p < P; ++p) {
        const int h0 = top_difference(own_idx[p], n);
        out_off[p + 1] = out_off[p] + (u64)std::max(h0, H);
        if (modified) modified[p] = H > h0;
        grows |= H > h0;
    }
    const u64 total = out_off[P];
    if (total && (!out_paths || capacity == 0)) return TF_OK;  // the sizing call
    if (capacity < total) return TF_ERR_BUFFER_TOO_SMALL;
    // one list per old peak below H
    std::vector<SweepWant> wants;
    u64 list_at[64] = {};
    for (int h0 = 0; h0 < H; ++h0) {
        if (!((n >> h0) & 1)) continue;
        list_at[h0] = wants.size();
        wants.push_back({h0, n >> h0, false, (u64)wants.size()});
        for (int g = h0 + 1; g < H; ++g)
            wants.push_back((n >> g) & 1 ? SweepWant{g, 0, true, (u64)wants.size()} : SweepWant{g, (n >> g) + 1, false, (u64)wants.size()});
    }
    const bool sweep = new_peaks || grows;
    if ((sweep && ((k && !leafs) || (n && !old_peaks))) || (P && own_off[P] > own_off[0] && !own_paths)) return TF_ERR_NULL_POINTER;
    if (!sweep && !total) return TF_OK;
    int dev = 0;
    TRY(ctx_dev(&dev));
    DevTemp table(s);
    if (grows) {
        TRY(table.alloc(5 * wants.size(), "mmr update wanted digests"));
        TRY(mmr_sweep(n, old_peaks, leafs, k, new_peaks, nullptr, wants, table.p, s));
    } else if (sweep) TRY(mmr_sweep(n, old_peaks, leafs, k, new_peaks, nullptr, {}, nullptr, s));
    if (!total) return TF_OK;
    std::vector<tfm::tfk::MmrGatherDesc> desc(P);
    for (size_t p = 0; p < P; ++p) {
        const int h0 = top_difference(own_idx[p], n);
        desc[p] = {own_off[p] - own_base, out_off[p], H > h0 ? list_at[h0] : 0, (unsigned)h0, (unsigned)(H > h0 ? H - h0 : 0)};
    }
    StagedUpload up(s);
    TRY(up.put(dev, desc.data(), desc.size() * sizeof(desc[0]), "mmr gather descriptors"));
    hipLaunchKernelGGL(tfm::tfk::mmr_gather_paths_kernel, dim3(grid_for(16 * (long long)P, 256)), dim3(256), 0, s,
                       up.as<tfm::tfk::MmrGatherDesc>(), (long long)P, own_paths, table.p, out_paths);
    HIPCHK(hipGetLastError());
    return TF_OK;
}

// ------------------------------------------------------------------------------------ host flavours
// Upload the inputs (waiting for each upload: pageable memory), run the _dev form on the thread's stream, copy back, synchronise.
namespace {
int up_words(DevTemp& t, const u64* h, size_t words, hipStream_t s, const char* what) {
    TRY(t.alloc(words, what));
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
    DevTemp dold(s), dl(s), dnew(s), dpr(s);
    TRY(up_words(dold, old_peaks, 5 * np_old, s, "mmr_append host buffers"));
    TRY(up_words(dl, leafs, 5 * k, s, "mmr_append host buffers"));
    TRY(dnew.alloc(5 * np_new, "mmr_append host buffers"));
    TRY(dpr.alloc(proofs ? 5 * n_proof : 0, "mmr_append host proofs"));
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
    return host_roundtrip(peaks, 5 * np, nullptr, 0, out, 5 * n_acc,
                          [&](u64* dp, u64*, u64* o, hipStream_t s) { return mmr_bag_peaks_dev(leaf_counts, n_acc, dp, o, s); });
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
    DevTemp dpk(s), di(s), dd(s), dpa(s), dst(s);
    TRY(up_words(dpk, peaks, 5 * n_peaks, s, "mmr_verify host buffers"));
    TRY(up_words(di, idx, n, s, "mmr_verify host buffers"));
    TRY(up_words(dd, digests, 5 * n, s, "mmr_verify host buffers"));
    TRY(up_words(dpa, na ? paths + 5 * offsets[0] : nullptr, 5 * na, s, "mmr_verify host buffers"));
    TRY(dst.alloc_bytes(n * sizeof(int), "mmr_verify host buffers"));
    TRY(mmr_verify_dev(leaf_count, dpk.p, n_peaks, n, di.p, dd.p, offsets, dpa.p, dst.as<int>(), offsets[0], s));
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
    DevTemp dpk(s), dl(s), dm(s), dq(s), dmod(s);
    TRY(up_words(dpk, peaks, 5 * np, s, "mmr_mutate host peaks"));  // (only with peaks)
    TRY(up_words(dl, leafs, 5 * M, s, "mmr_mutate host buffers"));
    TRY(up_words(dm, nm ? mpaths + 5 * moff[0] : nullptr, 5 * nm, s, "mmr_mutate host buffers"));
    TRY(up_words(dq, nq ? ppaths + 5 * poff[0] : nullptr, 5 * nq, s, "mmr_mutate host buffers"));
    TRY(dmod.alloc_bytes(P * sizeof(int), "mmr_mutate host buffers"));
    u64 dummy = 0;
    TRY(mmr_mutate_dev(leaf_count, peaks ? (np ? dpk.p : &dummy) : nullptr, M, midx, dl.p, moff, dm.p, P, pidx, poff, dq.p,
                       dmod.as<int>(), M ? moff[0] : 0, P ? poff[0] : 0, s));
    if (np) TRY(d2h(peaks, dpk.p, 5 * np, s));
    if (nq) TRY(d2h(ppaths + 5 * poff[0], dq.p, 5 * nq, s));
    if (P) HIPCHK(hipMemcpyAsync(modified, dmod.p, P * sizeof(int), hipMemcpyDeviceToHost, s));
    return sync(s);
}

int mmr_successor_new_host(u64 n, const u64* old_peaks, const u64* leafs, size_t k, u64* paths_out, u64* new_peaks) {
    if (n > kMaxLeafs || k > kMaxLeafs - n) return TF_ERR_INVALID_ARGUMENT;
    const size_t len = mmr_successor_proof_len(n, k);
    if ((len && !paths_out) || (k && (len || new_peaks) && !leafs) || (n && new_peaks && !old_peaks)) return TF_ERR_NULL_POINTER;
    if (!len && !new_peaks) return TF_OK;
    DeviceCtx* ctx = nullptr;
    TRY(current_ctx(&ctx));
    hipStream_t s = host_stream();
    const size_t np_old = new_peaks ? __builtin_popcountll(n) : 0, np_new = new_peaks ? __builtin_popcountll(n + k) : 0;
    DevTemp dold(s), dl(s), dnew(s), dpa(s);
    TRY(up_words(dold, old_peaks, 5 * np_old, s, "mmr_successor_new host peaks"));  // (only with new_peaks, as dnew)
    TRY(up_words(dl, leafs, 5 * k, s, "mmr_successor_new host buffers"));
    TRY(dnew.alloc(5 * np_new, "mmr_successor_new host peaks"));
    TRY(dpa.alloc(5 * len, "mmr_successor_new host buffers"));
    u64 dummy = 0;
    TRY(mmr_successor_new_dev(n, np_old ? dold.p : (new_peaks ? &dummy : nullptr), k ? dl.p : &dummy, k, dpa.p,
                              new_peaks ? (np_new ? dnew.p : &dummy) : nullptr, s));
    if (len) TRY(d2h(paths_out, dpa.p, 5 * len, s));
    if (np_new) TRY(d2h(new_peaks, dnew.p, 5 * np_new, s));
    return sync(s);
}

int mmr_successor_verify_host(size_t P, const uint64_t* old_counts, const uint64_t* new_counts, const uint64_t* old_off, const u64* old_peaks,
                              const uint64_t* new_off, const u64* new_peaks, const uint64_t* path_off, const u64* paths, int* statuses) {
    if (P == 0) return TF_OK;
    if (!old_counts || !new_counts || !old_off || !new_off || !path_off || !statuses) return TF_ERR_NULL_POINTER;
    for (size_t p = 0; p < P; ++p)
        if (old_counts[p] > kMaxLeafs || new_counts[p] > kMaxLeafs) return TF_ERR_INVALID_ARGUMENT;
    TRY(check_offsets(old_off, P));
    TRY(check_offsets(new_off, P));
    TRY(check_offsets(path_off, P));
    const size_t no = old_off[P] - old_off[0], nn = new_off[P] - new_off[0], na = path_off[P] - path_off[0];
    if ((no && !old_peaks) || (nn && !new_peaks) || (na && !paths)) return TF_ERR_NULL_POINTER;
    DeviceCtx* ctx = nullptr;
    TRY(current_ctx(&ctx));
    hipStream_t s = host_stream();
    DevTemp dold(s), dnew(s), dpa(s), dst(s);
    TRY(up_words(dold, no ? old_peaks + 5 * old_off[0] : nullptr, 5 * no, s, "mmr_successor_verify host buffers"));
    TRY(up_words(dnew, nn ? new_peaks + 5 * new_off[0] : nullptr, 5 * nn, s, "mmr_successor_verify host buffers"));
    TRY(up_words(dpa, na ? paths + 5 * path_off[0] : nullptr, 5 * na, s, "mmr_successor_verify host buffers"));
    TRY(dst.alloc_bytes(P * sizeof(int), "mmr_successor_verify host buffers"));
    u64 dummy = 0;
    TRY(mmr_successor_verify_dev(P, old_counts, new_counts, old_off, no ? dold.p : &dummy, new_off, nn ? dnew.p : &dummy, path_off, na ? dpa.p : &dummy,
                                 dst.as<int>(), old_off[0], new_off[0], path_off[0], s));
    HIPCHK(hipMemcpyAsync(statuses, dst.p, P * sizeof(int), hipMemcpyDeviceToHost, s));
    return sync(s);
}

int mmr_update_proofs_host(u64 n, const u64* old_peaks, const u64* leafs, size_t k, size_t P, const uint64_t* own_idx, const uint64_t* own_off,
                           const u64* own_paths, uint64_t* out_off, u64* out_paths, size_t capacity, int* modified, u64* new_peaks) {
    // the argument errors, the offsets, the flags and the sizing rule are the _dev form's, which touches no device for them
    TRY(mmr_update_proofs_dev(n, nullptr, nullptr, k, P, own_idx, own_off, nullptr, out_off, nullptr, 0, modified, nullptr, 0, nullptr));
    const u64 total = out_off[P];
    if (total && (!out_paths || capacity == 0)) return TF_OK;
    if (capacity < total) return TF_ERR_BUFFER_TOO_SMALL;
    if (!total && !new_peaks) return TF_OK;
    const size_t nq = P ? own_off[P] - own_off[0] : 0;
    // what the device call will need (it repeats the check on the device copies)
    const bool grows = total > nq, sweep = new_peaks || grows;
    if ((sweep && ((k && !leafs) || (n && !old_peaks))) || (nq && !own_paths)) return TF_ERR_NULL_POINTER;
    DeviceCtx* ctx = nullptr;
    TRY(current_ctx(&ctx));
    hipStream_t s = host_stream();
    const size_t np_old = sweep ? __builtin_popcountll(n) : 0, np_new = new_peaks ? __builtin_popcountll(n + k) : 0;
    DevTemp dold(s), dl(s), dq(s), dout(s), dnew(s);
    TRY(up_words(dold, old_peaks, 5 * np_old, s, "mmr_update_proofs host sweep inputs"));  // (only where the call sweeps)
    TRY(up_words(dl, sweep ? leafs : nullptr, sweep ? 5 * k : 0, s, "mmr_update_proofs host sweep inputs"));
    TRY(up_words(dq, nq ? own_paths + 5 * own_off[0] : nullptr, 5 * nq, s, "mmr_update_proofs host buffers"));
    TRY(dout.alloc(5 * total, "mmr_update_proofs host buffers"));
    TRY(dnew.alloc(5 * np_new, "mmr_update_proofs host new peaks"));  // (only with new_peaks)
    u64 dummy = 0;
    TRY(mmr_update_proofs_dev(n, np_old ? dold.p : &dummy, k && sweep ? dl.p : &dummy, k, P, own_idx, own_off, nq ? dq.p : &dummy, out_off,
                              total ? dout.p : &dummy, total ? (size_t)total : 1, modified, new_peaks ? (np_new ? dnew.p : &dummy) : nullptr,
                              P ? own_off[0] : 0, s));
    if (total) TRY(d2h(out_paths, dout.p, 5 * total, s));
    if (np_new) TRY(d2h(new_peaks, dnew.p, 5 * np_new, s));
    return sync(s);
}

}  // namespace tfi
