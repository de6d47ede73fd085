// mmr_selftest.cpp -- MmrAccumulator / MmrMembershipProof of the C++ mirror (twenty_first.hpp): the reference's bag_peaks snapshot of
// the empty accumulator (util_types/mmr/mmr_accumulator.rs:1038-1046), appends against new_from_leafs, proofs that verify, and a batch
// mutation that keeps every own proof valid.
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

int main() {
    if (tf_device_count() == 0) {
        std::printf("no GPU: skipped\n");
        return 77;
    }
    EXPECT(MmrAccumulator::new_from_leafs({}).bag_peaks().to_hex() ==
           "cd65052100640f0d27e5654f97c47e49899add2f265967ccbefee7264e9bc08f588542d9dc3d5ac5");
    std::vector<Digest> leafs(45);
    for (size_t i = 0; i < leafs.size(); ++i)
        for (size_t w = 0; w < 5; ++w) leafs[i].values[w] = BFieldElement::new_(7919 * i + w);
    MmrAccumulator acc = MmrAccumulator::new_from_leafs(std::vector<Digest>(leafs.begin(), leafs.begin() + 20));
    const std::vector<MmrMembershipProof> proofs = acc.append_many(std::vector<Digest>(leafs.begin() + 20, leafs.end()));
    const MmrAccumulator all = MmrAccumulator::new_from_leafs(leafs);
    EXPECT(acc.num_leafs() == 45 && acc.peaks == all.peaks && acc.bag_peaks() == all.bag_peaks());
    EXPECT(proofs.size() == 25 && proofs.back().verify(44, leafs[44], acc.peaks, 45));
    EXPECT(!proofs.back().verify(44, leafs[43], acc.peaks, 45));

    // 45 = 32 + 8 + 4 + 1 leafs: the proof of a leaf is its authentication path in its peak's Merkle tree
    auto proof_of = [&](size_t i) {
        size_t start = i < 32 ? 0 : (i < 40 ? 32 : 40), size = i < 32 ? 32 : (i < 40 ? 8 : 4);
        const MerkleTree t = MerkleTree::par_new(std::vector<Digest>(leafs.begin() + (long)start, leafs.begin() + (long)(start + size)));
        return MmrMembershipProof{t.inclusion_proof_for_leaf_indices({i - start}).into_authentication_paths()[0]};
    };
    std::vector<MmrMembershipProof> own = {proof_of(3), proof_of(40)};
    EXPECT(own[0].verify(3, leafs[3], all.peaks, 45) && own[1].verify(40, leafs[40], all.peaks, 45));
    Digest a5 = leafs[5], a41 = leafs[41];
    a5.values[0] = BFieldElement::new_(1);
    a41.values[4] = BFieldElement::new_(2);
    MmrAccumulator mut = all;
    const std::vector<size_t> changed = mut.batch_mutate_leaf_and_update_mps(own, {3, 40}, {{5, a5, proof_of(5)}, {41, a41, proof_of(41)}});
    std::vector<Digest> after = leafs;
    after[5] = a5;
    after[41] = a41;
    EXPECT(mut.peaks == MmrAccumulator::new_from_leafs(after).peaks);
    EXPECT(changed.size() == 2 && own[0].verify(3, leafs[3], mut.peaks, 45) && own[1].verify(40, leafs[40], mut.peaks, 45));
    std::printf("mmr: bag_peaks snapshot / append / new_from_leafs / verify / batch mutation all as the reference\n");
    return 0;
}
