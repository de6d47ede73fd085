// divide_selftest.cpp -- division with remainder and the power-series inverse of the C++ mirror (twenty_first.hpp) against small
// divisions worked by hand: Polynomial::divide / Div / Rem / reduce (math/polynomial.rs:539-600, :989-1048, :2502-2524) and
// formal_power_series_inverse_newton (:1281-1366).  One PASS line per case.
// Exit code 0 = all passed; 77 = no GPU (skipped); anything else = failure.
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
static X lift(long long v) { return X{{b(v), B{}, B{}}}; }

int main() {
    if (tf_device_count() == 0) {
        std::printf("no GPU: skipped\n");
        return 77;
    }
    // (x^3 + 2x + 5) / (x + 1) = x^2 - x + 3, remainder 2
    const Polynomial<B> a({b(5), b(2), b(0), b(1)}), d({b(1), b(1)});
    const auto qr = a.divide(d);
    EXPECT(qr.first.coefficients == (std::vector<B>{b(3), b(-1), b(1)}));
    EXPECT(qr.second.coefficients == (std::vector<B>{b(2)}));
    std::printf("PASS divide bfe (x^3 + 2x + 5) / (x + 1)\n");
    EXPECT((a / d).coefficients == qr.first.coefficients && (a % d).coefficients == qr.second.coefficients &&
           a.reduce(d).coefficients == qr.second.coefficients);
    std::printf("PASS Div / Rem / reduce agree with divide\n");
    // a non-monic divisor: (6x^2 + 7x + 2) / (2x + 1) = 3x + 2, remainder 0; a dividend shorter than the divisor: (zero, self)
    const auto qr2 = Polynomial<B>({b(2), b(7), b(6)}).divide(Polynomial<B>({b(1), b(2)}));
    EXPECT(qr2.first.coefficients == (std::vector<B>{b(2), b(3)}) && qr2.second.coefficients.empty());
    const auto qr3 = d.divide(a);
    EXPECT(qr3.first.coefficients.empty() && qr3.second.coefficients == d.coefficients);
    std::printf("PASS divide bfe non-monic divisor, short dividend\n");
    // XFieldElement: (x^2 - 1) / (x - 1) = x + 1
    const auto qx = Polynomial<X>({lift(-1), lift(0), lift(1)}).divide(Polynomial<X>({lift(-1), lift(1)}));
    EXPECT(qx.first.coefficients == (std::vector<X>{lift(1), lift(1)}) && qx.second.coefficients.empty());
    std::printf("PASS divide xfe (x^2 - 1) / (x - 1)\n");
    bool panicked = false;
    try {
        (void)(a / Polynomial<B>({}));
    } catch (const NttPanic& e) {
        panicked = e.code == TF_ERR_DIVISION_BY_ZERO;
    }
    EXPECT(panicked);
    std::printf("PASS a zero divisor panics (code 15)\n");
    // 1 / (1 - x) at precision 4: two Newton steps, 1 -> 1 + x -> 1 + x + x^2 + x^3
    const Polynomial<B> inv = Polynomial<B>({b(1), b(-1)}).formal_power_series_inverse_newton(4);
    EXPECT(inv.coefficients == (std::vector<B>{b(1), b(1), b(1), b(1)}));
    const Polynomial<X> invx = Polynomial<X>({lift(1), lift(-1)}).formal_power_series_inverse_newton(3);
    EXPECT(invx.coefficients == (std::vector<X>{lift(1), lift(1), lift(1), lift(1)}));
    int code = 0;  // the zero polynomial: the reference panics indexing coefficients[0] -> TF_ERR_INVERSE_OF_ZERO
    try {
        (void)Polynomial<B>({}).formal_power_series_inverse_newton(8);
    } catch (const NttPanic& e) {
        code = e.code;
    }
    EXPECT(code == TF_ERR_INVERSE_OF_ZERO);
    std::printf("PASS formal_power_series_inverse_newton bfe / xfe, zero polynomial panics (code 12)\n");
    return 0;
}
