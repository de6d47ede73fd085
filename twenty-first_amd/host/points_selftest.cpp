// points_selftest.cpp -- are_colinear / get_colinear_y, mod_pow and powers of the C++ mirror (twenty_first.hpp) against the reference's
// own doc examples: (0,0), (1,1), (2,2) are colinear and (0,0), (1,1), (2,3) are not (math/polynomial.rs:340-346);
// get_colinear_y((0,0), (2,4), 1) == 2 and that triple is colinear (:376-384).  One PASS line per case.
// Exit code 0 = all passed; 77 = no GPU (skipped); anything else = failure.
#include <cstdio>
#include <cstdlib>
#include <utility>
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

static B b(uint64_t v) { return B::new_(v); }
static X x(uint64_t c0, uint64_t c1, uint64_t c2) { return X{{b(c0), b(c1), b(c2)}}; }
static B bmul(B a, B c) { return B{B::montyred((unsigned __int128)a.raw * c.raw)}; }

int main() {
    if (tf_device_count() == 0) {
        std::printf("no GPU: skipped\n");
        return 77;
    }
    using PB = Polynomial<B>;
    using PX = Polynomial<X>;
    // polynomial.rs:340-346
    const std::vector<std::pair<B, B>> on_line{{b(0), b(0)}, {b(1), b(1)}, {b(2), b(2)}};
    const std::vector<std::pair<B, B>> off_line{{b(0), b(0)}, {b(1), b(1)}, {b(2), b(3)}};
    EXPECT(PB::are_colinear(on_line));
    EXPECT(!PB::are_colinear(off_line));
    std::printf("PASS are_colinear: (0,0),(1,1),(2,2) on a line, (2,3) off it\n");
    // :349-355: fewer than three points, a repeated x-coordinate
    EXPECT(!PB::are_colinear({}) && !PB::are_colinear({on_line[0], on_line[1]}));
    EXPECT(!PB::are_colinear({on_line[0], on_line[1], on_line[2], on_line[1]}));
    std::printf("PASS are_colinear: two points and a repeated x are not colinear\n");
    // :376-384
    const std::pair<B, B> point_0{b(0), b(0)}, point_1{b(2), b(4)};
    const B point_2_x = b(1);
    const B point_2_y = PB::get_colinear_y(point_0, point_1, point_2_x);
    EXPECT(point_2_y == b(2));
    EXPECT(PB::are_colinear({point_0, point_1, {point_2_x, point_2_y}}));
    std::printf("PASS get_colinear_y((0,0),(2,4),1) == 2, and the three points are colinear\n");
    // the same over XFieldElements: y = (1, 2, 3) x + (4, 5, 6) through three points that differ in one limb only
    const X x0 = x(7, 1, 2), x1 = x(7, 1, 3), x2 = x(7, 1, 4);
    const X y0 = PX::get_colinear_y({x(0, 0, 0), x(4, 5, 6)}, {x(1, 0, 0), x(5, 7, 9)}, x0);
    const X y1 = PX::get_colinear_y({x(0, 0, 0), x(4, 5, 6)}, {x(1, 0, 0), x(5, 7, 9)}, x1);
    const X y2 = PX::get_colinear_y({x0, y0}, {x1, y1}, x2);
    EXPECT(PX::are_colinear({{x(0, 0, 0), x(4, 5, 6)}, {x(1, 0, 0), x(5, 7, 9)}, {x0, y0}, {x1, y1}, {x2, y2}}));
    EXPECT(!PX::are_colinear({{x0, y0}, {x1, y1}, {x2, y1}}));
    EXPECT(!PX::are_colinear({{x0, y0}, {x1, y1}, {x0, y0}}));
    std::printf("PASS get_colinear_y / are_colinear over XFieldElements\n");
    // x0 == x1 panics (:387)
    int code = 0;
    try {
        (void)PB::get_colinear_y({b(5), b(1)}, {b(5), b(2)}, b(7));
    } catch (const NttPanic& e) {
        code = e.code;
    }
    EXPECT(code == TF_ERR_INVERSE_OF_ZERO);
    std::printf("PASS get_colinear_y panics on a vertical line (code 12)\n");
    // mod_pow: 2^10 = 1024, x^0 = 1 for zero too, 7^(p-1) = 1; a broadcast base against a product chain
    const std::vector<B> pw = mod_pow_u64(std::vector<B>{b(2), b(0), b(7)}, std::vector<uint64_t>{10, 0, B::P - 1});
    EXPECT(pw.size() == 3 && pw[0] == b(1024) && pw[1] == b(1) && pw[2] == b(1));
    const std::vector<B> p3 = mod_pow_u32(std::vector<B>{b(3)}, std::vector<uint32_t>{0, 1, 2, 3, 4});
    const std::vector<B> seq = powers(b(1), b(3), 5);
    EXPECT(p3 == seq && seq[4] == b(81));
    B acc = b(5);
    const std::vector<B> geo = powers(b(5), b(11), 300);
    for (size_t i = 0; i < geo.size(); ++i) {
        EXPECT(geo[i] == acc);
        acc = bmul(acc, b(11));
    }
    std::printf("PASS mod_pow_u64 / mod_pow_u32 / powers\n");
    return 0;
}
