// proof_selftest.cpp -- MerkleTreeInclusionProof of the C++ mirror (twenty_first.hpp) against the reference's own examples:
// the documented proof of leafs 0 and 2 of an 8-leaf tree (util_types/merkle_tree.rs:1518-1535) and the error variants of try_verify.
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

template <class F>
static int variant_of(F&& f) {
    try {
        f();
    } catch (const MerkleTreeError& e) {
        return e.variant;
    }
    return 0;
}

int main() {
    if (tf_device_count() == 0) {
        std::printf("no GPU: skipped\n");
        return 77;
    }
    std::vector<Digest> leafs(8);
    for (size_t i = 0; i < leafs.size(); ++i)
        for (size_t w = 0; w < 5; ++w) leafs[i].values[w] = BFieldElement::new_(1000 * i + w);
    const MerkleTree tree = MerkleTree::par_new(leafs);
    const MerkleTreeInclusionProof p = tree.inclusion_proof_for_leaf_indices({0, 2});
    EXPECT(p.tree_height == 3 && p.authentication_structure.size() == 3);
    EXPECT(p.authentication_structure[0] == tree.nodes[11] && p.authentication_structure[1] == tree.nodes[9] &&
           p.authentication_structure[2] == tree.nodes[3]);
    EXPECT(p.verify(tree.root()));
    const auto paths = p.into_authentication_paths();
    EXPECT(paths.size() == 2 && paths[0].size() == 3);
    EXPECT(paths[0][0] == tree.nodes[9] && paths[0][1] == tree.nodes[5] && paths[0][2] == tree.nodes[3]);
    EXPECT(paths[1][0] == tree.nodes[11] && paths[1][1] == tree.nodes[4] && paths[1][2] == tree.nodes[3]);

    EXPECT(variant_of([&] { p.try_verify(tree.nodes[2]); }) == MerkleTreeError::RootMismatch);
    MerkleTreeInclusionProof q = p;
    q.authentication_structure.pop_back();
    EXPECT(variant_of([&] { q.try_verify(tree.root()); }) == MerkleTreeError::AuthenticationStructureLengthMismatch);
    q = p;
    q.indexed_leafs.push_back({0, tree.nodes[9]});
    EXPECT(variant_of([&] { q.try_verify(tree.root()); }) == MerkleTreeError::RepeatedLeafDigestMismatch);
    q = p;
    q.indexed_leafs[1].first = 8;
    EXPECT(variant_of([&] { q.try_verify(tree.root()); }) == MerkleTreeError::LeafIndexInvalid);
    q = p;
    q.tree_height = 64;
    EXPECT(variant_of([&] { q.try_verify(tree.root()); }) == MerkleTreeError::TreeTooHigh);
    EXPECT(variant_of([&] { tree.inclusion_proof_for_leaf_indices({8}); }) == MerkleTreeError::LeafIndexInvalid);

    const std::vector<bool> ok = MerkleTreeInclusionProof::verify_batch({p, p, MerkleTreeInclusionProof{}}, {tree.root(), tree.nodes[1], tree.nodes[5]});
    EXPECT(ok.size() == 3 && ok[0] && ok[1] && ok[2]);  // the last one is trivial: no leafs, no structure
    std::printf("inclusion proofs: verify / try_verify / into_authentication_paths / verify_batch all as the reference\n");
    return 0;
}
