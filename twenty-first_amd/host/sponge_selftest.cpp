// sponge_selftest.cpp -- the sponge of the C++ mirror (twenty_first.hpp): pad_and_absorb_all in one call against hash_varlen and
// against the chunk-by-chunk absorb, sample_scalars against the squeezes it stands for (tip5/mod.rs:664-674), sample_indices
// against the reference's loop (:636-656) restated on squeeze(), its skip of BFieldElement::MAX, and its panic.
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

static std::vector<uint32_t> indices_by_squeezing(Tip5& sponge, uint32_t upper_bound, size_t num_indices) {
    std::vector<uint32_t> indices;
    std::array<BFieldElement, Tip5::RATE> buffer{};
    size_t next_in_buffer = Tip5::RATE;
    while (indices.size() < num_indices) {
        if (next_in_buffer == Tip5::RATE) {
            buffer = sponge.squeeze();
            next_in_buffer = 0;
        }
        const BFieldElement element = buffer[next_in_buffer++];
        if (element.value() != 0xffffffff00000000ULL) indices.push_back((uint32_t)element.value() % upper_bound);
    }
    return indices;
}

int main() {
    // the panic is an argument error: reported with or without a GPU
    try {
        Tip5::init().sample_indices(12, 3);
        EXPECT(!"sample_indices(12, ..) must throw");
    } catch (const BackendError&) {
    }
    if (tf_device_count() == 0) {
        std::printf("no GPU: skipped\n");
        return 77;
    }
    for (size_t len : {size_t(0), size_t(1), size_t(9), size_t(10), size_t(11), size_t(33), size_t(330)}) {
        std::vector<BFieldElement> in(len);
        for (size_t i = 0; i < len; ++i) in[i] = BFieldElement::new_(1000003 * i + len);
        Tip5 one = Tip5::init();
        one.pad_and_absorb_all(in);
        const Digest d = Tip5::hash_varlen(in);
        for (size_t w = 0; w < 5; ++w) EXPECT(one.state[w] == d.values[w]);
        // chunk by chunk, as sponge.rs:41-55 spells it
        Tip5 steps = Tip5::init();
        std::array<BFieldElement, Tip5::RATE> chunk;
        size_t i = 0;
        for (; i + Tip5::RATE <= len; i += Tip5::RATE) {
            for (size_t k = 0; k < Tip5::RATE; ++k) chunk[k] = in[i + k];
            steps.absorb(chunk);
        }
        chunk.fill(BFieldElement{});
        for (size_t k = 0; i + k < len; ++k) chunk[k] = in[i + k];
        chunk[len - i] = BFieldElement::from_raw_u64(0xffffffffULL);
        steps.absorb(chunk);
        EXPECT(steps.state == one.state);
    }
    Tip5 a = Tip5::init();
    a.pad_and_absorb_all({BFieldElement::new_(1), BFieldElement::new_(2), BFieldElement::new_(3)});
    for (size_t n : {size_t(0), size_t(1), size_t(3), size_t(4), size_t(10), size_t(100)}) {
        Tip5 b = a;
        const std::vector<XFieldElement> scalars = a.sample_scalars(n);
        std::vector<BFieldElement> words;
        for (size_t s = 0; s < (3 * n + 9) / 10; ++s)
            for (const BFieldElement& e : b.squeeze()) words.push_back(e);
        EXPECT(scalars.size() == n && a.state == b.state);
        for (size_t e = 0; e < n; ++e)
            for (size_t w = 0; w < 3; ++w) EXPECT(scalars[e].coefficients[w] == words[3 * e + w]);
    }
    const std::pair<uint32_t, size_t> cases[] = {{2, 0}, {4, 1}, {8, 9}, {16, 10}, {32, 11}, {64, 19}, {128, 20}, {256, 21}, {512, 65}, {1u << 31, 40}, {1, 5}};
    for (const auto& c : cases) {
        Tip5 b = a;
        const std::vector<uint32_t> got = a.sample_indices(c.first, c.second);
        EXPECT(got == indices_by_squeezing(b, c.first, c.second) && a.state == b.state);
        for (uint32_t v : got) EXPECT(v < c.first);
    }
    // the skip rule: the first squeeze returns the caller's rate words; MAX in positions 0, 4 and 9 turns one squeeze into two
    Tip5 m = a;
    for (size_t k : {size_t(0), size_t(4), size_t(9)}) m.state[k] = BFieldElement::new_(0xffffffff00000000ULL);
    EXPECT(m.state[0].raw_u64() == 0xfffffffe00000002ULL);
    Tip5 m2 = m, two = m;
    two.squeeze();
    two.squeeze();
    const std::vector<uint32_t> skipped = m.sample_indices(1u << 20, 10);
    EXPECT(skipped == indices_by_squeezing(m2, 1u << 20, 10) && m.state == m2.state && m.state == two.state);
    std::printf("sponge: pad_and_absorb_all / sample_scalars / sample_indices (skip of MAX, panic) all as the reference\n");
    return 0;
}
