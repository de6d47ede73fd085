// twenty_first.hpp -- C++ host-side mirror of the reference's Rust API for the hot path, on top of the
// C ABI of libtf_hip.so (include/tf_hip.h).  The reference is a Rust crate; no Rust toolchain exists in
// the build image, so the host layer a Rust maintainer would write as an `extern "C"` shim
//  is provided here in C++ with the same names, argument meaning and error behaviour:
//
//   twenty_first::ntt / intt                          math/ntt.rs:67-82, :109-125   (panics -> NttPanic)
//   twenty_first::Polynomial<FF>::fast_coset_evaluate math/polynomial.rs:1374-1399
//   twenty_first::Tip5::{hash_10, hash_pair, hash_varlen, permutation}   tip5/mod.rs:529-623
//   twenty_first::MerkleTree::{par_new, sequential_new, par_frugal_root, sequential_frugal_root}
//                                                     util_types/merkle_tree.rs:149-364
//   twenty_first::MerkleTree::{par,sequential}_authentication_structure_from_leafs   util_types/merkle_tree.rs:506-542
//   twenty_first::MerkleTreeError                     util_types/merkle_tree.rs:933-965
//
// Everything executes on the GPU through the C ABI; there is no CPU fallback in this header.
#pragma once

#include <algorithm>
#include <array>
#include <utility>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/tf_hip.h"

namespace twenty_first {

// #[repr(transparent)] over one u64 in Montgomery form (math/b_field_element.rs:84-86)
struct BFieldElement {
    uint64_t raw = 0;
    static constexpr uint64_t P = 0xffffffff00000001ULL;  // :225
    static constexpr uint64_t MAX = P - 1;

    static uint64_t montyred(unsigned __int128 x) {  // :357-370
        uint64_t xl = (uint64_t)x, xh = (uint64_t)(x >> 64);
        uint64_t a = xl + (xl << 32);
        uint64_t e = a < xl;
        uint64_t b = a - (a >> 32) - e;
        uint64_t r = xh - b;
        return xh < b ? r - 0xffffffffULL : r;
    }
    static BFieldElement new_(uint64_t value) {  // BFieldElement::new, :235-237
        return BFieldElement{montyred((unsigned __int128)value * 0xfffffffe00000001ULL)};
    }
    static BFieldElement from_raw_u64(uint64_t r) { return BFieldElement{r}; }
    uint64_t value() const { return montyred((unsigned __int128)raw); }  // :248-250
    uint64_t raw_u64() const { return raw; }
    static BFieldElement generator() { return new_(7); }  // :312-314
    bool operator==(const BFieldElement& o) const { return raw == o.raw; }
    bool operator!=(const BFieldElement& o) const { return raw != o.raw; }
};
static_assert(sizeof(BFieldElement) == 8, "layout contract of the C ABI");

// #[repr(transparent)] over [BFieldElement; 3] (math/x_field_element.rs:56-59)
struct XFieldElement {
    std::array<BFieldElement, 3> coefficients{};
    bool operator==(const XFieldElement& o) const { return coefficients == o.coefficients; }
};
static_assert(sizeof(XFieldElement) == 24, "layout contract of the C ABI");

struct Digest {  // tip5/digest.rs:29
    std::array<BFieldElement, 5> values{};
    static constexpr size_t LEN = 5;
    bool operator==(const Digest& o) const { return values == o.values; }
    std::string to_hex() const {  // canonical values, little-endian bytes (digest.rs:85-90, :144-153)
        static const char* hx = "0123456789abcdef";
        std::string s;
        for (auto& v : values) {
            uint64_t c = v.value();
            for (int b = 0; b < 8; ++b) {
                unsigned byte = (c >> (8 * b)) & 0xff;
                s.push_back(hx[byte >> 4]);
                s.push_back(hx[byte & 15]);
            }
        }
        return s;
    }
};
static_assert(sizeof(Digest) == 40, "layout contract of the C ABI");

// ---- errors -------------------------------------------------------------------------------------
struct BackendError : std::runtime_error {
    int code;
    BackendError(int c, const std::string& where)
        : std::runtime_error(where + ": " + tf_status_string(c) +
                             (((c >= TF_ERR_NO_DEVICE && c <= TF_ERR_OUT_OF_MEMORY) || c == TF_ERR_INTERNAL) ? std::string(" (") + tf_last_error() + ")" : "")),
          code(c) {}  // tf_last_error() belongs to the HIP failures (codes 8..10) and to an exception caught at the ABI (18) only
};
// where the reference panics (math/ntt.rs:135-140, math/polynomial.rs:1388-1392)
struct NttPanic : BackendError {
    using BackendError::BackendError;
};
// util_types/merkle_tree.rs:933-965
struct MerkleTreeError : BackendError {
    enum Variant {
        TooFewLeafs = 1,
        IncorrectNumberOfLeafs = 2,
        TreeTooHigh = 3,
        LeafIndexInvalid = 11,
        AuthenticationStructureLengthMismatch = 19,
        RepeatedLeafDigestMismatch = 20,
        RootMismatch = 21
    } variant;
    MerkleTreeError(int c, const std::string& where) : BackendError(c, where), variant((Variant)c) {}
};

inline void check(int rc, const char* where) {
    if (rc == TF_OK) return;
    if ((rc >= 1 && rc <= 3) || rc == TF_ERR_LEAF_INDEX_INVALID || (rc >= TF_ERR_AUTH_STRUCTURE_LENGTH_MISMATCH && rc <= TF_ERR_ROOT_MISMATCH))
        throw MerkleTreeError(rc, where);  // merkle_tree.rs:933-965
    if ((rc >= 4 && rc <= 6) || rc == TF_ERR_INVERSE_OF_ZERO || (rc >= TF_ERR_EMPTY_DOMAIN && rc <= TF_ERR_DIVISION_NOT_CLEAN)) throw NttPanic(rc, where);  // the reference panics here
    throw BackendError(rc, where);
}

// ---- ntt / intt (math/ntt.rs:67-82, :109-125) ----------------------------------------------------
inline void ntt(std::vector<BFieldElement>& x) { check(tf_ntt_bfe(reinterpret_cast<uint64_t*>(x.data()), x.size(), 1, 0), "ntt"); }
inline void intt(std::vector<BFieldElement>& x) { check(tf_ntt_bfe(reinterpret_cast<uint64_t*>(x.data()), x.size(), 1, 1), "intt"); }
inline void ntt(std::vector<XFieldElement>& x) { check(tf_ntt_xfe(reinterpret_cast<uint64_t*>(x.data()), x.size(), 1, 0), "ntt"); }
inline void intt(std::vector<XFieldElement>& x) { check(tf_ntt_xfe(reinterpret_cast<uint64_t*>(x.data()), x.size(), 1, 1), "intt"); }
// many equal-length slices in one call (what a rayon caller of ntt() does, ntt.rs:250-274)
inline void ntt_batch(BFieldElement* x, size_t n, size_t batch, bool inverse = false) {
    check(tf_ntt_bfe(reinterpret_cast<uint64_t*>(x), n, batch, inverse), inverse ? "intt" : "ntt");
}
// ... and the same batch over several GPUs of the node: `devices` empty = every visible device (tf_ntt_bfe_multi: contiguous
// slices of the batch, one worker thread + stream per listed device, results in place at each slice's offset)
inline void ntt_batch_multi(BFieldElement* x, size_t n, size_t batch, const std::vector<int>& devices = {}, bool inverse = false) {
    check(tf_ntt_bfe_multi(reinterpret_cast<uint64_t*>(x), n, batch, inverse, devices.empty() ? nullptr : devices.data(), (int)devices.size()),
          inverse ? "intt" : "ntt");
}
inline void ntt_batch_multi(XFieldElement* x, size_t n, size_t batch, const std::vector<int>& devices = {}, bool inverse = false) {
    check(tf_ntt_xfe_multi(reinterpret_cast<uint64_t*>(x), n, batch, inverse, devices.empty() ? nullptr : devices.data(), (int)devices.size()),
          inverse ? "intt" : "ntt");
}

// ---- FiniteField::batch_inversion (math/traits.rs:93-121) / Inverse::inverse_or_zero (:39-45) over a whole vector --------------
// batch_inversion consumes its input and returns it inverted, as the reference does; a zero element panics (NttPanic, code 12, :106)
inline std::vector<BFieldElement> batch_inversion(std::vector<BFieldElement> input) {
    uint64_t* p = reinterpret_cast<uint64_t*>(input.data());
    check(tf_batch_inversion_bfe(p, input.size(), p), "batch_inversion");
    return input;
}
inline std::vector<XFieldElement> batch_inversion(std::vector<XFieldElement> input) {
    uint64_t* p = reinterpret_cast<uint64_t*>(input.data());
    check(tf_batch_inversion_xfe(p, input.size(), p), "batch_inversion");
    return input;
}
// every element's inverse_or_zero: zero stays zero
inline std::vector<BFieldElement> inverse_or_zero(std::vector<BFieldElement> input) {
    uint64_t* p = reinterpret_cast<uint64_t*>(input.data());
    check(tf_inverse_or_zero_bfe(p, input.size(), p), "inverse_or_zero");
    return input;
}
inline std::vector<XFieldElement> inverse_or_zero(std::vector<XFieldElement> input) {
    uint64_t* p = reinterpret_cast<uint64_t*>(input.data());
    check(tf_inverse_or_zero_xfe(p, input.size(), p), "inverse_or_zero");
    return input;
}

// ---- element-wise powers and geometric sequences ----------------------------------------------------------------------------
// mod_pow_u64 (b_field_element.rs:340-353, :809; x_field_element.rs:654-680): out[i] = bases[i] ^ exps[i]; either vector may hold a
// single element, which then serves every element of the other.  x^0 = 1, zero included.
template <class FF>
inline std::vector<FF> mod_pow_u64(const std::vector<FF>& bases, const std::vector<uint64_t>& exps) {
    const size_t n = bases.empty() || exps.empty() ? 0 : std::max(bases.size(), exps.size());
    std::vector<FF> out(n);
    check(tf_mod_pow(reinterpret_cast<const uint64_t*>(bases.data()), bases.size(), exps.data(), exps.size(), sizeof(FF) / 8,
                     reinterpret_cast<uint64_t*>(out.data()), n), "mod_pow_u64");
    return out;
}
// mod_pow_u32 (b_field_element.rs:650; x_field_element.rs:654-667)
template <class FF>
inline std::vector<FF> mod_pow_u32(const std::vector<FF>& bases, const std::vector<uint32_t>& exps) {
    return mod_pow_u64(bases, std::vector<uint64_t>(exps.begin(), exps.end()));
}
// first * ratio^i for i < n: the elements of a cyclic group (first = 1, n = the order of ratio; b_field_element.rs:656-668,
// x_field_element.rs:423-435), the powers inside Polynomial::scale, the points of an evaluation domain
template <class FF>
inline std::vector<FF> powers(FF first, FF ratio, size_t n) {
    std::vector<FF> out(n);
    check(tf_powers(reinterpret_cast<const uint64_t*>(&first), reinterpret_cast<const uint64_t*>(&ratio), sizeof(FF) / 8,
                    reinterpret_cast<uint64_t*>(out.data()), n), "powers");
    return out;
}

// ---- tables between the column-major and the row-major layout (include/tf_hip.h, "Tables") ---------------------------------
// column-major: n_cols columns of n_rows elements back to back (what hash_table_rows / MerkleTree::from_columns read);
// row-major: n_rows rows of n_cols elements back to back (what hash_varlen_rows reads); `batch` tables one after the other
template <class FF>
inline std::vector<FF> table_columns_to_rows(const std::vector<FF>& table, size_t n_rows, size_t n_cols, size_t batch = 1) {
    if (table.size() != batch * n_rows * n_cols) throw std::invalid_argument("table_columns_to_rows: the table is not batch x n_cols x n_rows");
    constexpr int W = sizeof(FF) / 8;
    std::vector<FF> rows(table.size());
    check(tf_table_transpose(reinterpret_cast<const uint64_t*>(table.data()), n_cols, n_rows, W, n_rows * W, reinterpret_cast<uint64_t*>(rows.data()),
                             n_cols * W, batch), "table_columns_to_rows");
    return rows;
}
template <class FF>
inline std::vector<FF> table_rows_to_columns(const std::vector<FF>& rows, size_t n_rows, size_t n_cols, size_t batch = 1) {
    if (rows.size() != batch * n_rows * n_cols) throw std::invalid_argument("table_rows_to_columns: the table is not batch x n_rows x n_cols");
    constexpr int W = sizeof(FF) / 8;
    std::vector<FF> table(rows.size());
    check(tf_table_transpose(reinterpret_cast<const uint64_t*>(rows.data()), n_rows, n_cols, W, n_cols * W, reinterpret_cast<uint64_t*>(table.data()),
                             n_rows * W, batch), "table_rows_to_columns");
    return table;
}
// rows indices[q] of every table, k rows of n_cols elements per table; layout is TF_TABLE_COLUMN_MAJOR or TF_TABLE_ROW_MAJOR.  An
// index >= n_rows throws (BackendError, code 17)
template <class FF>
inline std::vector<FF> table_gather_rows(const std::vector<FF>& table, int layout, size_t n_rows, size_t n_cols, const std::vector<uint32_t>& indices,
                                         size_t batch = 1) {
    if (table.size() != batch * n_rows * n_cols) throw std::invalid_argument("table_gather_rows: the table is not batch x n_rows x n_cols");
    constexpr int W = sizeof(FF) / 8;
    std::vector<FF> out(batch * indices.size() * n_cols);
    check(tf_table_gather_rows(reinterpret_cast<const uint64_t*>(table.data()), layout, n_rows, n_cols, W,
                               (layout == TF_TABLE_ROW_MAJOR ? n_cols : n_rows) * W, indices.data(), indices.size(),
                               reinterpret_cast<uint64_t*>(out.data()), n_cols * W, batch), "table_gather_rows");
    return out;
}

// the field a product of an A and a B lives in (x_field_element.rs:491-556): the extension field if either is
template <class A, class B>
using ProductField = std::conditional_t<(sizeof(A) >= sizeof(B)), A, B>;

// ---- Polynomial (math/polynomial.rs:78-84): only the hot-path members ------------------------------
template <class FF>
struct Polynomial {
    std::vector<FF> coefficients;  // low -> high degree
  private:
    std::pair<Polynomial, Polynomial> divide_impl(const Polynomial& divisor, bool want_q) const {
        const size_t na = coefficients.size(), nb = divisor.coefficients.size();
        std::vector<FF> q(want_q && na >= nb ? na - nb + 1 : 0), r(nb ? nb - 1 : 0);
        const uint64_t* a = reinterpret_cast<const uint64_t*>(coefficients.data());
        const uint64_t* b = reinterpret_cast<const uint64_t*>(divisor.coefficients.data());
        uint64_t dummy[3] = {0, 0, 0};  // stands for an empty output (never written) and an empty dividend (never read)
        uint64_t* qp = want_q ? (q.empty() ? dummy : reinterpret_cast<uint64_t*>(q.data())) : nullptr;
        uint64_t* rp = r.empty() ? dummy : reinterpret_cast<uint64_t*>(r.data());
        if (!na) a = dummy;
        if constexpr (sizeof(FF) == 8) check(tf_poly_divide_bfe(a, na, 1, b, nb, qp, rp), "divide");
        else check(tf_poly_divide_xfe(a, na, 1, b, nb, qp, rp), "divide");
        return {Polynomial(std::move(q)), Polynomial(std::move(r))};
    }

  public:
    explicit Polynomial(std::vector<FF> c) : coefficients(std::move(c)) {
        while (!coefficients.empty() && coefficients.back() == FF{}) coefficients.pop_back();  // Polynomial::new normalises
    }
    long degree() const { return (long)coefficients.size() - 1; }
    // fast_coset_evaluate (polynomial.rs:1374-1399); offset is a BFieldElement (the documented fast case, :1366-1368)
    std::vector<FF> fast_coset_evaluate(BFieldElement offset, size_t order) const {
        if ((long)order <= degree()) throw NttPanic(TF_ERR_ORDER_NOT_ABOVE_DEGREE, "fast_coset_evaluate");  // :1388-1392
        std::vector<FF> out(order);
        const uint64_t* c = reinterpret_cast<const uint64_t*>(coefficients.data());
        uint64_t* o = reinterpret_cast<uint64_t*>(out.data());
        if constexpr (sizeof(FF) == 8)
            check(tf_coset_eval_bfe(c, coefficients.size(), offset.raw, o, order, 1), "fast_coset_evaluate");
        else
            check(tf_coset_eval_xfe(c, coefficients.size(), offset.raw, o, order, 1), "fast_coset_evaluate");
        return out;
    }
    // fast_coset_interpolate (polynomial.rs:1907-1918): values on {offset * w^i} -> the interpolant; panics unless the
    // number of values is a power of two
    static Polynomial fast_coset_interpolate(BFieldElement offset, const std::vector<FF>& values) {
        std::vector<FF> c(values.size());
        const uint64_t* v = reinterpret_cast<const uint64_t*>(values.data());
        uint64_t* o = reinterpret_cast<uint64_t*>(c.data());
        if constexpr (sizeof(FF) == 8)
            check(tf_coset_interpolate_bfe(v, values.size(), offset.raw, o, 1), "fast_coset_interpolate");
        else
            check(tf_coset_interpolate_xfe(v, values.size(), offset.raw, o, 1), "fast_coset_interpolate");
        return Polynomial(std::move(c));
    }
    // fast_multiply (polynomial.rs:900-932), same field on both sides; the zero polynomial annihilates
    Polynomial fast_multiply(const Polynomial& other) const {
        if (degree() < 0 || other.degree() < 0) return Polynomial({});
        std::vector<FF> out(coefficients.size() + other.coefficients.size() - 1);
        const uint64_t* a = reinterpret_cast<const uint64_t*>(coefficients.data());
        const uint64_t* b = reinterpret_cast<const uint64_t*>(other.coefficients.data());
        uint64_t* o = reinterpret_cast<uint64_t*>(out.data());
        if constexpr (sizeof(FF) == 8)
            check(tf_poly_mul_bfe(a, coefficients.size(), b, other.coefficients.size(), o, 1), "fast_multiply");
        else
            check(tf_poly_mul_xfe(a, coefficients.size(), b, other.coefficients.size(), o, 1), "fast_multiply");
        return Polynomial(std::move(out));
    }
    // Add (polynomial.rs:2526-2563), Sub (:2565-), Neg (:2700-): Polynomial<FF> with Polynomial<FF>
  private:
    Polynomial add_sub(const Polynomial& other, bool sub) const {
        const size_t na = coefficients.size(), nb = other.coefficients.size();
        std::vector<FF> out(std::max(na, nb));
        const uint64_t* a = reinterpret_cast<const uint64_t*>(coefficients.data());
        const uint64_t* b = reinterpret_cast<const uint64_t*>(other.coefficients.data());
        uint64_t* o = reinterpret_cast<uint64_t*>(out.data());
        check(sub ? tf_poly_sub(a, na, b, nb, sizeof(FF) / 8, o, 1) : tf_poly_add(a, na, b, nb, sizeof(FF) / 8, o, 1), sub ? "sub" : "add");
        return Polynomial(std::move(out));
    }
    template <class S>
    Polynomial<ProductField<FF, S>> by_scalar(S scalar, bool scale) const {
        std::vector<ProductField<FF, S>> out(coefficients.size());
        const uint64_t* a = reinterpret_cast<const uint64_t*>(coefficients.data());
        const uint64_t* sc = reinterpret_cast<const uint64_t*>(&scalar);
        uint64_t* o = reinterpret_cast<uint64_t*>(out.data());
        if (scale) check(tf_poly_scale(a, coefficients.size(), sizeof(FF) / 8, sc, sizeof(S) / 8, o, 1), "scale");
        else check(tf_poly_scalar_mul(a, coefficients.size(), sizeof(FF) / 8, sc, sizeof(S) / 8, o, 1), "scalar_mul");
        return Polynomial<ProductField<FF, S>>(std::move(out));
    }

  public:
    Polynomial operator+(const Polynomial& other) const { return add_sub(other, false); }
    Polynomial operator-(const Polynomial& other) const { return add_sub(other, true); }
    Polynomial operator-() const {
        std::vector<FF> out(coefficients.size());
        check(tf_poly_neg(reinterpret_cast<const uint64_t*>(coefficients.data()), coefficients.size(), sizeof(FF) / 8,
                          reinterpret_cast<uint64_t*>(out.data()), 1), "neg");
        return Polynomial(std::move(out));
    }
    // scalar_mul (polynomial.rs:498-532, Mul<S> :2650-2686): every coefficient times a BFieldElement or an XFieldElement
    template <class S>
    Polynomial<ProductField<FF, S>> scalar_mul(S scalar) const { return by_scalar(scalar, false); }
    // scale (polynomial.rs:760-773): P(alpha x), coefficient j times alpha^j
    template <class S>
    Polynomial<ProductField<FF, S>> scale(S alpha) const { return by_scalar(alpha, true); }
    // formal_derivative (polynomial.rs:275-285)
    Polynomial formal_derivative() const {
        std::vector<FF> out(coefficients.empty() ? 0 : coefficients.size() - 1);
        check(tf_poly_formal_derivative(reinterpret_cast<const uint64_t*>(coefficients.data()), coefficients.size(), sizeof(FF) / 8,
                                        reinterpret_cast<uint64_t*>(out.data()), 1), "formal_derivative");
        return Polynomial(std::move(out));
    }
    // are_colinear (polynomial.rs:348-364): fewer than three points, or two equal x-coordinates, are not colinear
    static bool are_colinear(const std::vector<std::pair<FF, FF>>& points) {
        std::vector<FF> xs, ys;
        for (const auto& p : points) xs.push_back(p.first), ys.push_back(p.second);
        int flag = 0;
        check(tf_are_colinear(reinterpret_cast<const uint64_t*>(xs.data()), reinterpret_cast<const uint64_t*>(ys.data()), 1, points.size(),
                              sizeof(FF) / 8, sizeof(FF) / 8, &flag), "are_colinear");
        return flag != 0;
    }
    // get_colinear_y (polynomial.rs:386-394); panics if p0 and p1 share their x-coordinate (NttPanic, code 12, :387)
    static FF get_colinear_y(std::pair<FF, FF> p0, std::pair<FF, FF> p1, FF p2_x) {
        FF out{};
        check(tf_get_colinear_y(reinterpret_cast<const uint64_t*>(&p0.first), reinterpret_cast<const uint64_t*>(&p0.second),
                                reinterpret_cast<const uint64_t*>(&p1.first), reinterpret_cast<const uint64_t*>(&p1.second), 1,
                                reinterpret_cast<const uint64_t*>(&p2_x), 1, sizeof(FF) / 8, sizeof(FF) / 8, reinterpret_cast<uint64_t*>(&out)),
              "get_colinear_y");
        return out;
    }
    // batch_evaluate (polynomial.rs:1840-1852): f at every point of `domain`
    std::vector<FF> batch_evaluate(const std::vector<FF>& domain) const {
        std::vector<FF> out(domain.size());
        const uint64_t* c = reinterpret_cast<const uint64_t*>(coefficients.data());
        const uint64_t* d = reinterpret_cast<const uint64_t*>(domain.data());
        uint64_t* o = reinterpret_cast<uint64_t*>(out.data());
        if constexpr (sizeof(FF) == 8)
            check(tf_poly_batch_evaluate_bfe(c, coefficients.size(), d, domain.size(), o), "batch_evaluate");
        else
            check(tf_poly_batch_evaluate_xfe(c, coefficients.size(), d, domain.size(), o), "batch_evaluate");
        return out;
    }
    // clean_divide (polynomial.rs:2358-2411, BFieldElement only): self / divisor for a division known to be clean; panics on a
    // zero divisor and on an unclean division
    Polynomial clean_divide(const Polynomial& divisor) const {
        static_assert(sizeof(FF) == 8, "clean_divide is defined for Polynomial<BFieldElement> (polynomial.rs:2333)");
        const size_t na = coefficients.size(), nb = divisor.coefficients.size();
        std::vector<FF> out(na >= nb ? na - nb + 1 : 0);
        check(tf_poly_clean_divide_bfe(reinterpret_cast<const uint64_t*>(coefficients.data()), na,
                                       reinterpret_cast<const uint64_t*>(divisor.coefficients.data()), nb, reinterpret_cast<uint64_t*>(out.data())),
              "clean_divide");
        if (na < nb) out.clear();
        return Polynomial(std::move(out));
    }
    // divide / naive_divide (polynomial.rs:539-600): (quotient, remainder); a zero divisor panics (NttPanic, code 15)
    std::pair<Polynomial, Polynomial> divide(const Polynomial& divisor) const {
        return divide_impl(divisor, true);
    }
    Polynomial operator/(const Polynomial& divisor) const { return divide(divisor).first; }   // Div (:2502-2512)
    Polynomial operator%(const Polynomial& divisor) const { return reduce(divisor); }         // Rem (:2514-2524)
    // reduce / fast_reduce (polynomial.rs:989-1048): the remainder only
    Polynomial reduce(const Polynomial& modulus) const { return divide_impl(modulus, false).second; }
    // formal_power_series_inverse_newton (polynomial.rs:1281-1366): the untruncated Newton iterate the reference returns
    Polynomial formal_power_series_inverse_newton(size_t precision) const {
        const size_t nf = coefficients.size();
        std::vector<FF> out(nf ? tf_poly_fps_inverse_newton_len(nf, precision) : 0);
        const uint64_t* f = reinterpret_cast<const uint64_t*>(coefficients.data());
        uint64_t dummy[3] = {0, 0, 0};  // an empty output (the zero polynomial, or a length above the limit): never written
        uint64_t* o = out.empty() ? dummy : reinterpret_cast<uint64_t*>(out.data());
        if constexpr (sizeof(FF) == 8) check(tf_poly_fps_inverse_newton_bfe(f, nf, precision, o), "formal_power_series_inverse_newton");
        else check(tf_poly_fps_inverse_newton_xfe(f, nf, precision, o), "formal_power_series_inverse_newton");
        return Polynomial(std::move(out));
    }
    // zerofier (polynomial.rs:1435-1441, par_zerofier :1444-1459): the monic polynomial with exactly these roots
    static Polynomial zerofier(const std::vector<FF>& roots) {
        std::vector<FF> out(roots.size() + 1);
        const uint64_t* r = reinterpret_cast<const uint64_t*>(roots.data());
        uint64_t* o = reinterpret_cast<uint64_t*>(out.data());
        if constexpr (sizeof(FF) == 8) check(tf_poly_zerofier_bfe(r, roots.size(), o), "zerofier");
        else check(tf_poly_zerofier_xfe(r, roots.size(), o), "zerofier");
        return Polynomial(std::move(out));
    }
    // batch_fast_interpolate (polynomial.rs:1703-1731): one interpolant per value row over the same domain
    static std::vector<Polynomial> batch_fast_interpolate(const std::vector<FF>& domain, const std::vector<std::vector<FF>>& values_matrix) {
        if (domain.empty()) throw NttPanic(TF_ERR_EMPTY_DOMAIN, "interpolate");  // :1503-1506
        std::vector<FF> flat;
        flat.reserve(values_matrix.size() * domain.size());
        for (auto& row : values_matrix) {
            if (row.size() != domain.size()) throw NttPanic(TF_ERR_EMPTY_DOMAIN, "interpolate: the domain and values lists have to be of equal length");  // :1507-1511
            flat.insert(flat.end(), row.begin(), row.end());
        }
        std::vector<FF> out(flat.size());
        const uint64_t* d = reinterpret_cast<const uint64_t*>(domain.data());
        const uint64_t* v = reinterpret_cast<const uint64_t*>(flat.data());
        uint64_t* o = reinterpret_cast<uint64_t*>(out.data());
        if constexpr (sizeof(FF) == 8) check(tf_poly_interpolate_bfe(d, v, domain.size(), values_matrix.size(), o), "interpolate");
        else check(tf_poly_interpolate_xfe(d, v, domain.size(), values_matrix.size(), o), "interpolate");
        std::vector<Polynomial> polys;
        for (size_t r = 0; r < values_matrix.size(); ++r)
            polys.emplace_back(std::vector<FF>(out.begin() + r * domain.size(), out.begin() + (r + 1) * domain.size()));
        return polys;
    }
    // interpolate (polynomial.rs:1502-1520; par_interpolate :1525-1545): panics on an empty domain, unequal lengths, repeated points
    static Polynomial interpolate(const std::vector<FF>& domain, const std::vector<FF>& values) {
        return batch_fast_interpolate(domain, {values})[0];
    }
    // evaluate::<XFieldElement, XFieldElement> (polynomial.rs:309-320) of a base-field polynomial at extension-field points
    std::vector<XFieldElement> evaluate_at(const std::vector<XFieldElement>& points) const {
        static_assert(sizeof(FF) == 8, "the mixed-field evaluation is for Polynomial<BFieldElement>; use batch_evaluate otherwise");
        std::vector<XFieldElement> out(points.size());
        check(tf_poly_evaluate_bfe_at_xfe(reinterpret_cast<const uint64_t*>(coefficients.data()), coefficients.size(), 1,
                                          reinterpret_cast<const uint64_t*>(points.data()), points.size(), reinterpret_cast<uint64_t*>(out.data())),
              "evaluate");
        return out;
    }
    // batch_coset_extrapolate (polynomial.rs:2196-2208, par_ :2262): codeword-major values of every interpolant at
    // every point; panics unless codeword_length is a power of two
    static std::vector<FF> batch_coset_extrapolate(BFieldElement domain_offset, size_t codeword_length, const std::vector<FF>& codewords,
                                                   const std::vector<FF>& points) {
        const size_t batch = codeword_length ? codewords.size() / codeword_length : 0;
        std::vector<FF> out(batch * points.size());
        const uint64_t* c = reinterpret_cast<const uint64_t*>(codewords.data());
        const uint64_t* p = reinterpret_cast<const uint64_t*>(points.data());
        uint64_t* o = reinterpret_cast<uint64_t*>(out.data());
        if constexpr (sizeof(FF) == 8)
            check(tf_coset_extrapolate_bfe(domain_offset.raw, c, codeword_length, batch, p, points.size(), o), "batch_coset_extrapolate");
        else
            check(tf_coset_extrapolate_xfe(domain_offset.raw, c, codeword_length, batch, p, points.size(), o), "batch_coset_extrapolate");
        return out;
    }
    static std::vector<FF> coset_extrapolate(BFieldElement domain_offset, const std::vector<FF>& codeword, const std::vector<FF>& points) {  // :2117-2128
        return batch_coset_extrapolate(domain_offset, codeword.size(), codeword, points);
    }
};

// ---- barycentric_evaluate (math/polynomial.rs:2609-2637): every codeword of a batch at one indeterminate ------------------
// sum_j weights[j] * column j, "scalar_mul each, then Add them all" in one pass: `columns` holds weights.size() packed columns of n
// elements (the column-major table MerkleTree::from_columns takes); no column gives n zeros (the reference's empty Sum)
template <class FF, class S>
inline std::vector<ProductField<FF, S>> linear_combination(const std::vector<FF>& columns, size_t n, const std::vector<S>& weights) {
    if (columns.size() != n * weights.size()) throw std::invalid_argument("linear_combination: columns must hold weights.size() columns of n elements");
    std::vector<ProductField<FF, S>> out(n);
    check(tf_poly_linear_combination(reinterpret_cast<const uint64_t*>(columns.data()), n, sizeof(FF) / 8, n * (sizeof(FF) / 8), weights.size(),
                                     reinterpret_cast<const uint64_t*>(weights.data()), sizeof(S) / 8, reinterpret_cast<uint64_t*>(out.data())),
          "linear_combination");
    return out;
}

template <class Coeff>
inline std::vector<XFieldElement> barycentric_evaluate(const std::vector<Coeff>& codewords, size_t codeword_length, XFieldElement indeterminate) {
    const size_t batch = codeword_length ? codewords.size() / codeword_length : 0;
    std::vector<XFieldElement> out(batch);
    const uint64_t* c = reinterpret_cast<const uint64_t*>(codewords.data());
    const uint64_t* x = reinterpret_cast<const uint64_t*>(&indeterminate);
    uint64_t* o = reinterpret_cast<uint64_t*>(out.data());
    if constexpr (sizeof(Coeff) == 8) check(tf_barycentric_evaluate_bfe(c, codeword_length, batch, x, o), "barycentric_evaluate");
    else check(tf_barycentric_evaluate_xfe(c, codeword_length, batch, x, o), "barycentric_evaluate");
    return out;
}

// ---- ZerofierTree (math/zerofier_tree.rs): the tree of a domain, built once and kept in HBM -----------------------------
template <class FF>
struct ZerofierTree {
    tf_zerofier_tree* handle = nullptr;
    size_t num_points = 0;
    ZerofierTree() = default;
    ZerofierTree(const ZerofierTree&) = delete;
    ZerofierTree& operator=(const ZerofierTree&) = delete;
    ZerofierTree(ZerofierTree&& o) noexcept : handle(o.handle), num_points(o.num_points) { o.handle = nullptr; }
    ~ZerofierTree() { tf_zerofier_tree_free(handle); }
    static ZerofierTree new_from_domain(const std::vector<FF>& domain) {  // :66-87
        ZerofierTree t;
        const uint64_t* d = reinterpret_cast<const uint64_t*>(domain.data());
        if constexpr (sizeof(FF) == 8) check(tf_zerofier_tree_new_bfe(d, domain.size(), &t.handle), "ZerofierTree::new_from_domain");
        else check(tf_zerofier_tree_new_xfe(d, domain.size(), &t.handle), "ZerofierTree::new_from_domain");
        t.num_points = domain.size();
        return t;
    }
    Polynomial<FF> zerofier() const {  // :93-99
        std::vector<FF> out(num_points + 1);
        check(tf_zerofier_tree_zerofier(handle, reinterpret_cast<uint64_t*>(out.data())), "ZerofierTree::zerofier");
        return Polynomial<FF>(std::move(out));
    }
    // polynomial.divide_and_conquer_batch_evaluate(&tree) (polynomial.rs:1882-1894)
    std::vector<FF> batch_evaluate(const Polynomial<FF>& f) const {
        std::vector<FF> out(num_points);
        check(tf_zerofier_tree_batch_evaluate(handle, reinterpret_cast<const uint64_t*>(f.coefficients.data()), f.coefficients.size(), 1,
                                              reinterpret_cast<uint64_t*>(out.data())),
              "divide_and_conquer_batch_evaluate");
        return out;
    }
    // the interpolant of `values` over the tree's domain (weights cached after the first call)
    Polynomial<FF> interpolate(const std::vector<FF>& values) {
        if (values.size() != num_points || num_points == 0) throw NttPanic(TF_ERR_EMPTY_DOMAIN, "interpolate");
        std::vector<FF> out(num_points);
        check(tf_zerofier_tree_interpolate(handle, reinterpret_cast<const uint64_t*>(values.data()), 1, reinterpret_cast<uint64_t*>(out.data())), "interpolate");
        return Polynomial<FF>(std::move(out));
    }
};

// ---- Tip5 (tip5/mod.rs) ---------------------------------------------------------------------------
struct Tip5 {
    std::array<BFieldElement, 16> state{};  // :159-165
    static constexpr size_t RATE = 10;
    void permutation() { check(tf_tip5_permute(reinterpret_cast<uint64_t*>(state.data()), 1), "Tip5::permutation"); }  // :529-533
    std::array<std::array<BFieldElement, 16>, 6> trace() {  // :538-548: the state before the permutation and after each round
        std::array<std::array<BFieldElement, 16>, 6> t;
        check(tf_tip5_trace(reinterpret_cast<uint64_t*>(state.data()), reinterpret_cast<uint64_t*>(t.data()), 1), "Tip5::trace");
        return t;
    }
    static std::array<BFieldElement, 5> hash_10(const std::array<BFieldElement, 10>& in) {  // :559-569
        std::array<BFieldElement, 5> out;
        check(tf_tip5_hash_pairs(reinterpret_cast<const uint64_t*>(in.data()), reinterpret_cast<uint64_t*>(out.data()), 1), "Tip5::hash_10");
        return out;
    }
    static Digest hash_pair(const Digest& l, const Digest& r) {  // :577-586
        std::array<BFieldElement, 10> in;
        for (int i = 0; i < 5; ++i) { in[i] = l.values[i]; in[5 + i] = r.values[i]; }
        return Digest{hash_10(in)};
    }
    static Digest hash_varlen(const std::vector<BFieldElement>& in) {  // :617-623
        Digest d;
        check(tf_tip5_hash_varlen_rows(reinterpret_cast<const uint64_t*>(in.data()), in.size(), 1, reinterpret_cast<uint64_t*>(d.values.data())), "Tip5::hash_varlen");
        return d;
    }
    // impl Sponge for Tip5 (:677-699) and Sponge::pad_and_absorb_all (util_types/sponge.rs:41-55)
    static Tip5 init() { return Tip5{}; }  // Domain::VariableLength: the all-zero state
    void absorb(const std::array<BFieldElement, RATE>& input) {
        for (size_t i = 0; i < RATE; ++i) state[i] = input[i];
        permutation();
    }
    std::array<BFieldElement, RATE> squeeze() {
        std::array<BFieldElement, RATE> produce;
        for (size_t i = 0; i < RATE; ++i) produce[i] = state[i];
        permutation();
        return produce;
    }
    void pad_and_absorb_all(const std::vector<BFieldElement>& input) {  // one library call (one launch) for all chunks and the padding
        check(tf_tip5_sponge_pad_and_absorb_all(reinterpret_cast<uint64_t*>(state.data()), 1, reinterpret_cast<const uint64_t*>(input.data()),
                                                input.size(), nullptr),
              "Sponge::pad_and_absorb_all");
    }
    // :636-656.  Panics in the reference if upper_bound is not a power of two: BackendError(TF_ERR_UPPER_BOUND_NOT_POWER_OF_TWO) here.
    std::vector<uint32_t> sample_indices(uint32_t upper_bound, size_t num_indices) {
        std::vector<uint32_t> indices(num_indices);
        check(tf_tip5_sponge_sample_indices(reinterpret_cast<uint64_t*>(state.data()), 1, upper_bound, num_indices, indices.data()),
              "Tip5::sample_indices");
        return indices;
    }
    std::vector<XFieldElement> sample_scalars(size_t num_elements) {  // :664-674
        std::vector<XFieldElement> scalars(num_elements);
        check(tf_tip5_sponge_sample_scalars(reinterpret_cast<uint64_t*>(state.data()), 1, num_elements, reinterpret_cast<uint64_t*>(scalars.data())),
              "Tip5::sample_scalars");
        return scalars;
    }
    // batched forms -- the reason to cross the boundary at all
    static std::vector<Digest> hash_pairs(const std::vector<Digest>& pairs) {  // pairs.size() even: (l0, r0, l1, r1, ...)
        std::vector<Digest> out(pairs.size() / 2);
        check(tf_tip5_hash_pairs(reinterpret_cast<const uint64_t*>(pairs.data()), reinterpret_cast<uint64_t*>(out.data()), out.size()), "Tip5::hash_pair");
        return out;
    }
};

// ---- MerkleTree (util_types/merkle_tree.rs:85-88) -----------------------------------------------------
struct MerkleTree {
    std::vector<Digest> nodes;  // nodes[0] dummy, nodes[1] root, leaves at nodes[n..2n)
    static MerkleTree par_new(const std::vector<Digest>& leafs) {  // :165-212
        MerkleTree t;
        t.nodes.resize(2 * leafs.size() + (leafs.empty() ? 1 : 0));
        check(tf_merkle_build(reinterpret_cast<const uint64_t*>(leafs.data()), leafs.size(), reinterpret_cast<uint64_t*>(t.nodes.data()), 1), "MerkleTree::par_new");
        return t;
    }
    static MerkleTree sequential_new(const std::vector<Digest>& leafs) { return par_new(leafs); }  // :149-153, same result
    // `batch` trees of n_leafs leaves each, split over the GPUs of the node (tf_merkle_root_multi); devices empty = all
    static std::vector<Digest> roots_multi(const std::vector<Digest>& leafs, size_t n_leafs, const std::vector<int>& devices = {}) {
        const size_t batch = n_leafs ? leafs.size() / n_leafs : 0;
        std::vector<Digest> roots(batch);
        check(tf_merkle_root_multi(reinterpret_cast<const uint64_t*>(leafs.data()), n_leafs, reinterpret_cast<uint64_t*>(roots.data()), batch,
                                   devices.empty() ? nullptr : devices.data(), (int)devices.size()), "MerkleTree::par_frugal_root");
        return roots;
    }
    static Digest sequential_frugal_root(const std::vector<Digest>& leafs) {  // :299-309
        Digest r;
        check(tf_merkle_root(reinterpret_cast<const uint64_t*>(leafs.data()), leafs.size(), reinterpret_cast<uint64_t*>(r.values.data()), 1), "MerkleTree::sequential_frugal_root");
        return r;
    }
    static Digest par_frugal_root(const std::vector<Digest>& leafs) {  // :332-364
        if (leafs.empty()) throw MerkleTreeError(TF_ERR_INCORRECT_NUMBER_OF_LEAFS, "MerkleTree::par_frugal_root");  // :333-335
        return sequential_frugal_root(leafs);
    }
    // hash_varlen of every row -> leaves -> tree in one device pipeline (the producer idiom of tip5/mod.rs:617-623)
    static MerkleTree from_rows(const std::vector<BFieldElement>& rows, size_t row_len) {
        const size_t n_rows = row_len ? rows.size() / row_len : 0;
        MerkleTree t;
        t.nodes.resize(2 * n_rows + (n_rows ? 0 : 1));
        check(tf_merkle_from_rows(reinterpret_cast<const uint64_t*>(rows.data()), row_len, n_rows, reinterpret_cast<uint64_t*>(t.nodes.data()), 1), "MerkleTree::par_new");
        return t;
    }
    // rows taken across a column-major table: `columns` = n_cols columns of n_rows elements back to back (one codeword each)
    template <class FF>
    static MerkleTree from_columns(const std::vector<FF>& columns, size_t n_rows) {
        constexpr int width = sizeof(FF) / 8;
        const size_t n_cols = n_rows ? columns.size() / n_rows : 0;
        MerkleTree t;
        t.nodes.resize(2 * n_rows + (n_rows ? 0 : 1));
        check(tf_merkle_from_columns(reinterpret_cast<const uint64_t*>(columns.data()), n_rows, n_cols, width, n_rows * width,
                                     reinterpret_cast<uint64_t*>(t.nodes.data()), 1), "MerkleTree::par_new");
        return t;
    }
    // authentication_structure (:614-622) over authentication_structure_node_indices (:449-504)
    std::vector<Digest> authentication_structure(const std::vector<size_t>& leaf_indices) const {
        std::vector<uint64_t> li(leaf_indices.begin(), leaf_indices.end()), idx(leaf_indices.size() * 64 + 1);
        size_t count = 0;
        check(tf_merkle_auth_structure_indices(num_leafs(), li.data(), li.size(), idx.data(), idx.size(), &count), "MerkleTree::authentication_structure");
        std::vector<Digest> out(count);
        for (size_t i = 0; i < count; ++i) out[i] = nodes[idx[i]];
        return out;
    }
    // the authentication structure from the leafs alone, no node array (:532-542): one level sweep on the device; root_out, when given,
    // receives the root the same sweep ends in
    static std::vector<Digest> par_authentication_structure_from_leafs(const std::vector<Digest>& leafs, const std::vector<size_t>& leaf_indices,
                                                                       Digest* root_out = nullptr) {
        const char* where = "MerkleTree::par_authentication_structure_from_leafs";
        const std::vector<uint64_t> li(leaf_indices.begin(), leaf_indices.end());
        const uint64_t* lp = reinterpret_cast<const uint64_t*>(leafs.data());
        size_t count = 0;
        check(tf_merkle_auth_structure_from_leafs(lp, leafs.size(), 1, li.data(), li.size(), nullptr, 0, &count, nullptr), where);
        std::vector<Digest> out(count + 1);  // (one digest of room: an empty buffer is the sizing call)
        if (count || root_out)
            check(tf_merkle_auth_structure_from_leafs(lp, leafs.size(), 1, li.data(), li.size(), reinterpret_cast<uint64_t*>(out.data()), out.size(),
                                                      &count, root_out ? reinterpret_cast<uint64_t*>(root_out->values.data()) : nullptr), where);
        out.resize(count);
        return out;
    }
    static std::vector<Digest> sequential_authentication_structure_from_leafs(const std::vector<Digest>& leafs, const std::vector<size_t>& leaf_indices,
                                                                              Digest* root_out = nullptr) {  // :514-522, same result
        return par_authentication_structure_from_leafs(leafs, leaf_indices, root_out);
    }
    const Digest& root() const { return nodes[1]; }            // :624-626
    size_t num_leafs() const { return nodes.size() / 2; }       // :628-631
    unsigned height() const { unsigned h = 0; for (size_t n = num_leafs(); n > 1; n >>= 1) ++h; return h; }  // :633-636
    const Digest* node(size_t i) const { return i < nodes.size() ? &nodes[i] : nullptr; }  // :638-645
    const Digest* leaf(size_t i) const { return i < num_leafs() ? &nodes[num_leafs() + i] : nullptr; }  // :654-661
    std::vector<std::pair<size_t, Digest>> indexed_leafs(const std::vector<size_t>& indices) const {  // :665-674
        std::vector<std::pair<size_t, Digest>> out;
        for (size_t i : indices) {
            const Digest* d = leaf(i);
            if (!d) throw MerkleTreeError(TF_ERR_LEAF_INDEX_INVALID, "MerkleTree::indexed_leafs");
            out.emplace_back(i, *d);
        }
        return out;
    }
    struct MerkleTreeInclusionProof inclusion_proof_for_leaf_indices(const std::vector<size_t>& indices) const;  // :684-709
};

// ---- MerkleTreeInclusionProof (util_types/merkle_tree.rs:90-113, :712-777), verified on the GPU in batches ----------------------
struct MerkleTreeInclusionProof {
    uint32_t tree_height = 0;
    std::vector<std::pair<size_t, Digest>> indexed_leafs;
    std::vector<Digest> authentication_structure;

    // statuses of try_verify for every proof, one device call (0 = Ok, else a MerkleTreeError code)
    static std::vector<int> try_verify_statuses(const std::vector<MerkleTreeInclusionProof>& proofs, const std::vector<Digest>& roots) {
        if (roots.size() != proofs.size()) throw std::invalid_argument("one root per proof");
        Packed p(proofs);
        std::vector<int> st(proofs.size());
        check(tf_merkle_verify_proofs(p.heights.data(), proofs.size(), p.leaf_off.data(), p.idx.data(), p.dig(), p.auth_off.data(), p.auth(),
                                      reinterpret_cast<const uint64_t*>(roots.data()), st.data()),
              "MerkleTreeInclusionProof::verify");
        return st;
    }
    static std::vector<bool> verify_batch(const std::vector<MerkleTreeInclusionProof>& proofs, const std::vector<Digest>& roots) {
        std::vector<int> st = try_verify_statuses(proofs, roots);
        return flip_ok(st);
    }
    void try_verify(const Digest& root) const {  // :736-748
        const int st = try_verify_statuses({*this}, {root})[0];
        if (st) throw MerkleTreeError(st, "MerkleTreeInclusionProof::try_verify");
    }
    bool verify(const Digest& root) const { return try_verify_statuses({*this}, {root})[0] == TF_OK; }  // :727-729
    // :773-777: for every entry of indexed_leafs (duplicates included) its tree_height siblings, bottom first
    std::vector<std::vector<Digest>> into_authentication_paths() const {
        Packed p({*this});
        const size_t h = tree_height < 64 ? tree_height : 0, k = indexed_leafs.size();
        std::vector<Digest> out(k * h + 1);
        int st = 0;
        check(tf_merkle_authentication_paths(p.heights.data(), 1, p.leaf_off.data(), p.idx.data(), p.dig(), p.auth_off.data(), p.auth(),
                                             reinterpret_cast<uint64_t*>(out.data()), &st),
              "MerkleTreeInclusionProof::into_authentication_paths");
        if (st) throw MerkleTreeError(st, "MerkleTreeInclusionProof::into_authentication_paths");
        std::vector<std::vector<Digest>> paths(k);
        for (size_t e = 0; e < k; ++e) paths[e].assign(out.begin() + (long)(e * h), out.begin() + (long)((e + 1) * h));
        return paths;
    }

  private:
    static std::vector<bool> flip_ok(const std::vector<int>& st) {
        std::vector<bool> ok(st.size());
        for (size_t i = 0; i < st.size(); ++i) ok[i] = st[i] == TF_OK;
        return ok;
    }
    // the CSR layout of include/tf_hip.h ("Inclusion proofs")
    struct Packed {
        std::vector<uint32_t> heights;
        std::vector<uint64_t> leaf_off{0}, auth_off{0}, idx;
        std::vector<Digest> digs, auths;
        explicit Packed(const std::vector<MerkleTreeInclusionProof>& proofs) {
            for (const auto& q : proofs) {
                heights.push_back(q.tree_height);
                for (const auto& [i, d] : q.indexed_leafs) {
                    idx.push_back(i);
                    digs.push_back(d);
                }
                auths.insert(auths.end(), q.authentication_structure.begin(), q.authentication_structure.end());
                leaf_off.push_back(idx.size());
                auth_off.push_back(auths.size());
            }
        }
        const uint64_t* dig() const { return reinterpret_cast<const uint64_t*>(digs.data()); }
        const uint64_t* auth() const { return reinterpret_cast<const uint64_t*>(auths.data()); }
    };
};

inline MerkleTreeInclusionProof MerkleTree::inclusion_proof_for_leaf_indices(const std::vector<size_t>& indices) const {
    MerkleTreeInclusionProof p;
    p.tree_height = height();
    p.indexed_leafs = indexed_leafs(indices);
    p.authentication_structure = authentication_structure(indices);
    return p;
}

// ---- Merkle Mountain Range (util_types/mmr/), every operation on the GPU -----------------------------------------------------------
struct MmrMembershipProof {  // mmr_membership_proof.rs:23-34
    std::vector<Digest> authentication_path;
    bool operator==(const MmrMembershipProof& o) const { return authentication_path == o.authentication_path; }

    // verify (:36-77) of many proofs against one accumulator: 0 = true, else the first reason it is false (TF_ERR_MMR_*)
    static std::vector<int> verify_statuses(const std::vector<MmrMembershipProof>& proofs, const std::vector<uint64_t>& leaf_indices,
                                            const std::vector<Digest>& leafs, const std::vector<Digest>& peaks, uint64_t num_leafs) {
        if (leaf_indices.size() != proofs.size() || leafs.size() != proofs.size()) throw std::invalid_argument("one leaf per proof");
        std::vector<uint64_t> off;
        std::vector<Digest> paths;
        pack(proofs, off, paths);
        std::vector<int> st(proofs.size());
        check(tf_mmr_verify_membership_proofs(num_leafs, reinterpret_cast<const uint64_t*>(peaks.data()), peaks.size(), proofs.size(),
                                              leaf_indices.data(), reinterpret_cast<const uint64_t*>(leafs.data()), off.data(),
                                              reinterpret_cast<const uint64_t*>(paths.data()), st.data()),
              "MmrMembershipProof::verify");
        return st;
    }
    bool verify(uint64_t leaf_index, const Digest& leaf, const std::vector<Digest>& peaks, uint64_t num_leafs) const {
        return verify_statuses({*this}, {leaf_index}, {leaf}, peaks, num_leafs)[0] == TF_OK;
    }
    // the CSR layout of include/tf_hip.h (Merkle Mountain Range calls)
    static void pack(const std::vector<MmrMembershipProof>& proofs, std::vector<uint64_t>& off, std::vector<Digest>& paths) {
        off.assign(1, 0);
        for (const auto& p : proofs) {
            paths.insert(paths.end(), p.authentication_path.begin(), p.authentication_path.end());
            off.push_back(paths.size());
        }
    }
    // batch_update_from_append (:224-331) and append, once per digest of new_leafs, in one call: the proofs are extended in place to the
    // accumulator of old_leaf_count + new_leafs.size() leafs; returns the indices of those that grew, which is the union of what the
    // reference's calls return.  A proof whose length is not the height of its leaf's peak is an error (include/tf_hip.h).
    static std::vector<size_t> batch_update_from_append_many(std::vector<MmrMembershipProof>& proofs, const std::vector<uint64_t>& leaf_indices,
                                                             uint64_t old_leaf_count, const std::vector<Digest>& new_leafs,
                                                             const std::vector<Digest>& old_peaks) {
        if (leaf_indices.size() != proofs.size()) throw std::invalid_argument("Lists must have same length");
        std::vector<uint64_t> off, out_off(proofs.size() + 1);
        std::vector<Digest> paths;
        pack(proofs, off, paths);
        std::vector<int> mod(proofs.size() + 1);
        auto call = [&](Digest* out, size_t capacity) {
            check(tf_mmr_update_proofs_from_append(old_leaf_count, reinterpret_cast<const uint64_t*>(old_peaks.data()),
                                                   reinterpret_cast<const uint64_t*>(new_leafs.data()), new_leafs.size(), proofs.size(),
                                                   leaf_indices.data(), off.data(), reinterpret_cast<const uint64_t*>(paths.data()), out_off.data(),
                                                   reinterpret_cast<uint64_t*>(out), capacity, mod.data(), nullptr),
                  "MmrMembershipProof::batch_update_from_append");
        };
        call(nullptr, 0);  // sizes
        std::vector<Digest> out(out_off.back() + 1);
        if (out_off.back()) call(out.data(), out_off.back());
        std::vector<size_t> grown;
        for (size_t p = 0; p < proofs.size(); ++p) {
            proofs[p].authentication_path.assign(out.begin() + (long)out_off[p], out.begin() + (long)out_off[p + 1]);
            if (mod[p]) grown.push_back(p);
        }
        return grown;
    }
    static std::vector<size_t> batch_update_from_append(std::vector<MmrMembershipProof>& proofs, const std::vector<uint64_t>& leaf_indices,
                                                        uint64_t old_leaf_count, const Digest& new_leaf, const std::vector<Digest>& old_peaks) {
        return batch_update_from_append_many(proofs, leaf_indices, old_leaf_count, {new_leaf}, old_peaks);
    }
};

struct LeafMutation {  // mmr_trait.rs
    uint64_t leaf_index = 0;
    Digest new_leaf;
    MmrMembershipProof membership_proof;
};

// batch_mutate_leaf_and_update_mps, or with peaks == nullptr batch_update_from_batch_leaf_mutation: the proofs are updated in place and
// the indices of those that changed are returned
inline std::vector<size_t> mmr_batch_mutate(uint64_t leaf_count, std::vector<Digest>* peaks, std::vector<MmrMembershipProof>& proofs,
                                            const std::vector<uint64_t>& proof_indices, const std::vector<LeafMutation>& mutations) {
    if (proof_indices.size() != proofs.size()) throw std::invalid_argument("Lists must have same length");
    std::vector<uint64_t> midx, moff, poff;
    std::vector<Digest> leafs, mpaths, ppaths;
    std::vector<MmrMembershipProof> mp;
    for (const auto& m : mutations) {
        midx.push_back(m.leaf_index);
        leafs.push_back(m.new_leaf);
        mp.push_back(m.membership_proof);
    }
    MmrMembershipProof::pack(mp, moff, mpaths);
    MmrMembershipProof::pack(proofs, poff, ppaths);
    std::vector<int> mod(proofs.size() + 1);
    check(tf_mmr_batch_mutate_leafs(leaf_count, peaks ? reinterpret_cast<uint64_t*>(peaks->data()) : nullptr, mutations.size(), midx.data(),
                                    reinterpret_cast<const uint64_t*>(leafs.data()), moff.data(), reinterpret_cast<const uint64_t*>(mpaths.data()),
                                    proofs.size(), proof_indices.data(), poff.data(), reinterpret_cast<uint64_t*>(ppaths.data()), mod.data()),
          "batch_mutate_leaf_and_update_mps");
    std::vector<size_t> changed;
    for (size_t p = 0; p < proofs.size(); ++p) {
        proofs[p].authentication_path.assign(ppaths.begin() + (long)poff[p], ppaths.begin() + (long)poff[p + 1]);
        if (mod[p]) changed.push_back(p);
    }
    return changed;
}

struct MmrAccumulator {  // mmr_accumulator.rs
    uint64_t leaf_count = 0;
    std::vector<Digest> peaks;  // highest first

    static MmrAccumulator new_from_leafs(const std::vector<Digest>& leafs) {  // :29-115
        MmrAccumulator a;
        a.append_many(leafs, false);
        return a;
    }
    uint64_t num_leafs() const { return leaf_count; }
    Digest bag_peaks() const {  // :379-391
        Digest out;
        check(tf_mmr_bag_peaks(&leaf_count, 1, reinterpret_cast<const uint64_t*>(peaks.data()), reinterpret_cast<uint64_t*>(&out)), "bag_peaks");
        return out;
    }
    // k successive appends (:149-159) in one call; their membership proofs if `proofs`
    std::vector<MmrMembershipProof> append_many(const std::vector<Digest>& leafs, bool proofs = true) {
        const uint64_t n = leaf_count, k = leafs.size();
        std::vector<size_t> lens;
        size_t total = 0;
        for (uint64_t i = 0; i < k; ++i) total += lens.emplace_back(__builtin_ctzll(~(n + i)));
        std::vector<Digest> next(__builtin_popcountll(n + k) + 1), flat(total + 1);  // (+ 1: never an empty buffer)
        check(tf_mmr_append(n, reinterpret_cast<const uint64_t*>(peaks.data()), reinterpret_cast<const uint64_t*>(leafs.data()), k,
                            reinterpret_cast<uint64_t*>(next.data()), proofs ? reinterpret_cast<uint64_t*>(flat.data()) : nullptr),
              "MmrAccumulator::append");
        next.pop_back();
        peaks = next;
        leaf_count = n + k;
        std::vector<MmrMembershipProof> out;
        if (!proofs) return out;
        size_t off = 0;
        for (size_t L : lens) {
            out.push_back({std::vector<Digest>(flat.begin() + (long)off, flat.begin() + (long)(off + L))});
            off += L;
        }
        return out;
    }
    MmrMembershipProof append(const Digest& leaf) { return append_many({leaf})[0]; }
    void mutate_leaf(const LeafMutation& m) {  // :164-175
        std::vector<MmrMembershipProof> none;
        mmr_batch_mutate(leaf_count, &peaks, none, {}, {m});
    }
    std::vector<size_t> batch_mutate_leaf_and_update_mps(std::vector<MmrMembershipProof>& proofs, const std::vector<uint64_t>& indices,
                                                         const std::vector<LeafMutation>& mutations) {  // :180-302
        return mmr_batch_mutate(leaf_count, &peaks, proofs, indices, mutations);
    }
};

struct MmrSuccessorProof {  // mmr_successor_proof.rs:15-18
    std::vector<Digest> paths;
    bool operator==(const MmrSuccessorProof& o) const { return paths == o.paths; }

    static MmrSuccessorProof new_from_batch_append(const MmrAccumulator& mmra, const std::vector<Digest>& new_leafs) {  // :34-91
        MmrSuccessorProof p;
        p.paths.resize(tf_mmr_successor_proof_len(mmra.leaf_count, new_leafs.size()) + 1);  // (+ 1: never an empty buffer)
        check(tf_mmr_successor_proof_new(mmra.leaf_count, nullptr, reinterpret_cast<const uint64_t*>(new_leafs.data()), new_leafs.size(),
                                         reinterpret_cast<uint64_t*>(p.paths.data()), nullptr),
              "MmrSuccessorProof::new_from_batch_append");
        p.paths.pop_back();
        return p;
    }
    // verify_internal (:142-223) of many (proof, old, new) triples: 0, or its first error (TF_ERR_MMR_INCONSISTENT_OLD ..)
    static std::vector<int> verify_statuses(const std::vector<MmrSuccessorProof>& proofs, const std::vector<MmrAccumulator>& olds,
                                            const std::vector<MmrAccumulator>& news) {
        if (olds.size() != proofs.size() || news.size() != proofs.size()) throw std::invalid_argument("one old and one new accumulator per proof");
        std::vector<uint64_t> oc, nc, oo(1, 0), no(1, 0), po(1, 0);
        std::vector<Digest> od, nd, pd;
        for (size_t p = 0; p < proofs.size(); ++p) {
            oc.push_back(olds[p].leaf_count);
            nc.push_back(news[p].leaf_count);
            od.insert(od.end(), olds[p].peaks.begin(), olds[p].peaks.end());
            nd.insert(nd.end(), news[p].peaks.begin(), news[p].peaks.end());
            pd.insert(pd.end(), proofs[p].paths.begin(), proofs[p].paths.end());
            oo.push_back(od.size());
            no.push_back(nd.size());
            po.push_back(pd.size());
        }
        std::vector<int> st(proofs.size());
        check(tf_mmr_verify_successor_proofs(proofs.size(), oc.data(), nc.data(), oo.data(), reinterpret_cast<const uint64_t*>(od.data()), no.data(),
                                             reinterpret_cast<const uint64_t*>(nd.data()), po.data(), reinterpret_cast<const uint64_t*>(pd.data()),
                                             st.data()),
              "MmrSuccessorProof::verify");
        return st;
    }
    bool verify(const MmrAccumulator& old_mmra, const MmrAccumulator& new_mmra) const {  // :94-96
        return verify_statuses({*this}, {old_mmra}, {new_mmra})[0] == TF_OK;
    }
};

}  // namespace twenty_first
