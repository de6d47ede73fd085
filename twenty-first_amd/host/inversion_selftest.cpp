// inversion_selftest.cpp -- batch_inversion / inverse_or_zero of the C++ mirror (twenty_first.hpp) against the reference's own
// tests: empty_batch_inversion and batch_inversion (math/b_field_element.rs:1157-1170), the batch inversion part of the
// XFieldElement inversion test (math/x_field_element.rs:1100-1126): empty, [1], [2], [x], [2, x], and the inverses of the inverses.
// One PASS line per case.  Exit code 0 = all passed; 77 = no GPU (skipped); anything else = failure.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "twenty_first.hpp"

using namespace twenty_first;
using B = BFieldElement;
using X = XFieldElement;

#define EXPECT(c)                                                      \
    do {                                                               \
        if (!(c)) {                                                    \
            std::fprintf(stderr, "FAILED %s (line %d)\n", #c, __LINE__); \
            return 1;                                                  \
        }                                                              \
    } while (0)

static B b(long long v) { return B::new_(v >= 0 ? (uint64_t)v : B::P - (uint64_t)(-v)); }
static X xfe(long long c0, long long c1, long long c2) { return X{{b(c0), b(c1), b(c2)}}; }
static B bmul(B a, B c) { return B{B::montyred((unsigned __int128)a.raw * c.raw)}; }
static B badd(B a, B c) {
    const unsigned __int128 s = (unsigned __int128)a.raw + c.raw;
    return B{(uint64_t)(s >= B::P ? s - B::P : s)};
}
static B bsub(B a, B c) { return B{a.raw >= c.raw ? a.raw - c.raw : a.raw + (B::P - c.raw)}; }
// x_field_element.rs:512-536: F_p[x] / (x^3 - x + 1), self = [c, b, a], other = [f, e, d]
static X xmul(const X& s, const X& o) {
    const B c = s.coefficients[0], bb = s.coefficients[1], a = s.coefficients[2];
    const B f = o.coefficients[0], e = o.coefficients[1], d = o.coefficients[2];
    const B ae = bmul(a, e), bd = bmul(bb, d), ad = bmul(a, d);
    return X{{bsub(bsub(bmul(c, f), ae), bd), badd(badd(bsub(badd(bmul(bb, f), bmul(c, e)), ad), ae), bd),
              badd(badd(badd(bmul(a, f), bmul(bb, e)), bmul(c, d)), ad)}};
}

int main() {
    if (tf_device_count() == 0) {
        std::printf("no GPU: skipped\n");
        return 77;
    }
    const B one = b(1), two = b(2), two_inv = b((long long)((B::P + 1) / 2));
    // empty_batch_inversion (b_field_element.rs:1157-1160)
    EXPECT(batch_inversion(std::vector<B>{}).empty() && batch_inversion(std::vector<X>{}).empty());
    std::printf("PASS empty batch_inversion bfe / xfe\n");
    // batch_inversion (:1162-1169): every element times its inverse is one
    std::vector<B> bfes;
    for (long long v = 1; v <= 1000; ++v) bfes.push_back(b(v * 7919 + v * v * 104729));
    const std::vector<B> bfes_inv = batch_inversion(bfes);
    EXPECT(bfes_inv.size() == bfes.size());
    for (size_t i = 0; i < bfes.size(); ++i) EXPECT(bmul(bfes[i], bfes_inv[i]) == one);
    std::printf("PASS batch_inversion bfe: x * x^-1 == 1 for 1000 elements\n");
    // x_field_element.rs:1100-1126
    const X xone = xfe(1, 0, 0), xtwo = xfe(2, 0, 0), xthree = xfe(3, 0, 0), xhundred = xfe(100, 0, 0), x = xfe(0, 1, 0);
    const X xtwo_inv = X{{two_inv, B{}, B{}}}, x_inv = xfe(1, 0, -1);  // x (x^2 - 1) = -1  ->  x^-1 = 1 - x^2
    EXPECT(xmul(x, x_inv) == xone);
    std::vector<X> inv = batch_inversion(std::vector<X>{xone});
    EXPECT(inv.size() == 1 && inv[0] == xone);
    inv = batch_inversion(std::vector<X>{xtwo});
    EXPECT(inv.size() == 1 && inv[0] == xtwo_inv);
    inv = batch_inversion(std::vector<X>{x});
    EXPECT(inv.size() == 1 && inv[0] == x_inv);
    inv = batch_inversion(std::vector<X>{xtwo, x});
    EXPECT(inv.size() == 2 && inv[0] == xtwo_inv && inv[1] == x_inv);
    std::printf("PASS batch_inversion xfe [1], [2], [x], [2, x]\n");
    const std::vector<X> input{xone, xtwo, xthree, xhundred, x};
    const std::vector<X> inverses = batch_inversion(input);
    const std::vector<X> inverses_inverses = batch_inversion(inverses);
    EXPECT(inverses.size() == input.size());
    for (size_t i = 0; i < input.size(); ++i) EXPECT(xmul(inverses[i], input[i]) == xone && inverses_inverses[i] == input[i]);
    std::printf("PASS batch_inversion xfe: inverses of the inverses\n");
    // a zero element panics (traits.rs:106); inverse_or_zero maps it to zero (traits.rs:39-45)
    int code = 0;
    try {
        (void)batch_inversion(std::vector<B>{two, B{}, one});
    } catch (const NttPanic& e) {
        code = e.code;
    }
    EXPECT(code == TF_ERR_INVERSE_OF_ZERO);
    EXPECT(inverse_or_zero(std::vector<B>{two, B{}, one}) == (std::vector<B>{two_inv, B{}, one}));
    EXPECT(inverse_or_zero(std::vector<X>{xtwo, X{}, x}) == (std::vector<X>{xtwo_inv, X{}, x_inv}));
    std::printf("PASS a zero panics batch_inversion (code 12), inverse_or_zero keeps it zero\n");
    return 0;
}
