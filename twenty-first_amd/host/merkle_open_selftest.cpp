// merkle_open_selftest.cpp -- MerkleTree::{par,sequential}_authentication_structure_from_leafs of the C++ mirror (twenty_first.hpp):
// the reference's documented example (8 leafs, indices {0, 2} -> the digests of nodes 11, 9 and 3, util_types/merkle_tree.rs:584-602)
// and one tree of height 10 against MerkleTree::par_new + authentication_structure, with the root the same sweep returns.
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

static std::vector<Digest> some_leafs(size_t n) {
    std::vector<Digest> leafs(n);
    for (size_t i = 0; i < n; ++i)
        for (size_t w = 0; w < 5; ++w) leafs[i].values[w] = BFieldElement::new_(1000 * i + w + n);
    return leafs;
}

int main() {
    // argument errors come before any device is needed
    const std::vector<Digest> eight = some_leafs(8);
    EXPECT(variant_of([&] { MerkleTree::par_authentication_structure_from_leafs(eight, {8}); }) == MerkleTreeError::LeafIndexInvalid);
    EXPECT(variant_of([&] { MerkleTree::par_authentication_structure_from_leafs(some_leafs(6), {0}); }) == MerkleTreeError::IncorrectNumberOfLeafs);
    EXPECT(variant_of([&] { MerkleTree::sequential_authentication_structure_from_leafs({}, {}); }) == MerkleTreeError::TooFewLeafs);
    if (tf_device_count() == 0) {
        std::printf("no GPU: skipped\n");
        return 77;
    }
    const MerkleTree small = MerkleTree::par_new(eight);
    Digest root;
    const std::vector<Digest> s = MerkleTree::par_authentication_structure_from_leafs(eight, {0, 2}, &root);
    EXPECT(s.size() == 3 && s[0] == small.nodes[11] && s[1] == small.nodes[9] && s[2] == small.nodes[3]);
    EXPECT(root == small.root());
    EXPECT(MerkleTree::sequential_authentication_structure_from_leafs(eight, {0, 2}) == s);

    const std::vector<Digest> leafs = some_leafs(1 << 10);
    const MerkleTree tree = MerkleTree::par_new(leafs);
    std::vector<size_t> indices;
    for (size_t i = 0; i < 17; ++i) indices.push_back((i * i * 37 + 5 * i + 3) % leafs.size());
    indices.push_back(indices[4]);  // a repeat
    Digest root10;
    const std::vector<Digest> got = MerkleTree::par_authentication_structure_from_leafs(leafs, indices, &root10);
    EXPECT(got == tree.authentication_structure(indices) && !got.empty());
    EXPECT(root10 == tree.root());
    // every leaf opened: nothing to send, the root alone
    std::vector<size_t> all(leafs.size());
    for (size_t i = 0; i < all.size(); ++i) all[i] = i;
    Digest root_all;
    EXPECT(MerkleTree::par_authentication_structure_from_leafs(leafs, all, &root_all).empty() && root_all == tree.root());
    std::printf("merkle open: structures and roots from the leafs as par_new + authentication_structure (8 leafs, 2^10 leafs)\n");
    return 0;
}
