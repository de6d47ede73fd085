// mmr_successor_selftest.cpp -- MmrSuccessorProof and MmrMembershipProof::batch_update_from_append of the C++ mirror
// (twenty_first.hpp): the reference's example (42 leafs, 8 more: two digests, the roots of the new leafs 0..1 and 2..5,
// util_types/mmr/mmr_successor_proof.rs:353-383), every (n, m) below 18 verified in one call, the statuses of a few broken triples,
// and membership proofs carried over appends, one leaf at a time against all at once.
// Exit code 0 = all passed; 77 = no GPU (skipped); anything else = failure.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "twenty_first.hpp"

using namespace twenty_first;

#define EXPECT(c)                                                      \
    do {                                                               \
        if (!(c)) {                                                    \
            std::fprintf(stderr, "FAILED %s (line %d)\n", #c, __LINE__); \
            return 1;                                                  \
        }                                                              \
    } while (0)

static std::vector<Digest> some_leafs(size_t first, size_t n) {
    std::vector<Digest> leafs(n);
    for (size_t i = 0; i < n; ++i)
        for (size_t w = 0; w < 5; ++w) leafs[i].values[w] = BFieldElement::new_(1000 * (first + i) + w + 1);
    return leafs;
}

int main() {
    EXPECT(tf_mmr_successor_proof_len(42, 8) == 2 && tf_mmr_successor_proof_len(8, 3) == 0 && tf_mmr_successor_proof_len(0, 1) == 0);
    if (tf_device_count() == 0) {
        std::printf("no GPU: skipped\n");
        return 77;
    }
    {  // 42 + 8
        const std::vector<Digest> old_leafs = some_leafs(0, 42), new_leafs = some_leafs(42, 8);
        const MmrAccumulator old_mmra = MmrAccumulator::new_from_leafs(old_leafs);
        MmrAccumulator new_mmra = old_mmra;
        new_mmra.append_many(new_leafs, false);
        const MmrSuccessorProof proof = MmrSuccessorProof::new_from_batch_append(old_mmra, new_leafs);
        EXPECT(proof.paths.size() == 2);
        EXPECT(proof.paths[0] == MerkleTree::par_new({new_leafs[0], new_leafs[1]}).root());
        EXPECT(proof.paths[1] == MerkleTree::par_new({new_leafs[2], new_leafs[3], new_leafs[4], new_leafs[5]}).root());
        EXPECT(proof.verify(old_mmra, new_mmra));
        // broken triples, all in one call
        MmrSuccessorProof corrupt = proof, shorter = proof, longer = proof;
        corrupt.paths[1].values[2] = BFieldElement::new_(7);
        shorter.paths.pop_back();
        longer.paths.push_back(proof.paths[0]);
        MmrAccumulator other_shared = new_mmra, fewer_peaks = old_mmra;
        other_shared.peaks[0].values[0] = BFieldElement::new_(7);
        fewer_peaks.peaks.pop_back();
        const std::vector<int> st = MmrSuccessorProof::verify_statuses({proof, corrupt, shorter, longer, proof, proof, proof, proof},
                                                                       {old_mmra, old_mmra, old_mmra, old_mmra, old_mmra, fewer_peaks, new_mmra, old_mmra},
                                                                       {new_mmra, new_mmra, new_mmra, new_mmra, other_shared, new_mmra, old_mmra, old_mmra});
        const std::vector<int> want{TF_OK, TF_ERR_MMR_DIFFERENT_UNSHARED_PEAK, TF_ERR_MMR_SUCCESSOR_PATH_TOO_SHORT, TF_ERR_MMR_SUCCESSOR_PATH_TOO_LONG,
                                    TF_ERR_MMR_DIFFERENT_SHARED_PEAK, TF_ERR_MMR_INCONSISTENT_OLD, TF_ERR_MMR_OLD_HAS_MORE_LEAFS,
                                    TF_ERR_MMR_SUCCESSOR_PATH_TOO_LONG};
        EXPECT(st == want);
    }
    {  // unit_tests (:385-392): every (n, m) below 18
        std::vector<MmrSuccessorProof> proofs;
        std::vector<MmrAccumulator> olds, news;
        for (size_t n = 0; n < 18; ++n)
            for (size_t m = 0; m < 18; ++m) {
                const MmrAccumulator old_mmra = MmrAccumulator::new_from_leafs(some_leafs(0, n));
                MmrAccumulator new_mmra = old_mmra;
                new_mmra.append_many(some_leafs(n, m), false);
                proofs.push_back(MmrSuccessorProof::new_from_batch_append(old_mmra, some_leafs(n, m)));
                EXPECT(proofs.back().paths.size() == tf_mmr_successor_proof_len(n, m));
                olds.push_back(old_mmra);
                news.push_back(new_mmra);
            }
        for (int s : MmrSuccessorProof::verify_statuses(proofs, olds, news)) EXPECT(s == TF_OK);
    }
    {  // membership proofs under appends: 21 leafs, 11 more, one at a time and all at once
        const std::vector<Digest> old_leafs = some_leafs(0, 21), new_leafs = some_leafs(21, 11);
        MmrAccumulator acc;
        std::vector<MmrMembershipProof> step, all;
        std::vector<uint64_t> indices;
        for (size_t i = 0; i < old_leafs.size(); ++i) {  // the proofs of 21 leafs, by the same means
            MmrMembershipProof::batch_update_from_append(step, indices, acc.leaf_count, old_leafs[i], acc.peaks);
            step.push_back(acc.append(old_leafs[i]));
            indices.push_back(i);
        }
        std::vector<int> st = MmrMembershipProof::verify_statuses(step, indices, old_leafs, acc.peaks, acc.leaf_count);
        for (int s : st) EXPECT(s == TF_OK);
        all = step;
        const MmrAccumulator old_mmra = acc;
        std::vector<bool> grew(step.size(), false);
        for (const Digest& leaf : new_leafs) {
            for (size_t p : MmrMembershipProof::batch_update_from_append(step, indices, acc.leaf_count, leaf, acc.peaks)) grew[p] = true;
            acc.append(leaf);
        }
        const std::vector<size_t> grown = MmrMembershipProof::batch_update_from_append_many(all, indices, old_mmra.leaf_count, new_leafs, old_mmra.peaks);
        EXPECT(all == step);
        std::vector<bool> grew_all(step.size(), false);
        for (size_t p : grown) grew_all[p] = true;
        EXPECT(grew_all == grew);
        st = MmrMembershipProof::verify_statuses(all, indices, old_leafs, acc.peaks, acc.leaf_count);
        for (int s : st) EXPECT(s == TF_OK);
    }
    std::printf("mmr successor: PASS (42 + 8 as the reference, 324 triples, statuses, proofs carried over appends)\n");
    return 0;
}
