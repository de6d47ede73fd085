// tf_divide.hip -- polynomial division with remainder (Polynomial::divide / naive_divide, Div, Rem, reduce / fast_reduce;
// math/polynomial.rs:539-600, :989-1048, :2502-2524) and formal_power_series_inverse_newton (:1281-1366): the planner over
// divide_kernels.h and the library's transforms (run_ntt), and the entry points of include/tf_hip.h.
#include "tf_temp.h"
#include "divide_kernels.h"

#include <deque>

namespace tfi {
namespace {

constexpr size_t kMaxDivideBatch = 65535;          // dividends per call
constexpr size_t kMaxDivideLen = size_t(1) << 30;  // na, nb (the quotient's product has order <= 2^31, the transforms' limit)
constexpr size_t kMaxFpsLen = size_t(1) << 30;     // coefficients of a power-series inverse

size_t next_pow2(size_t v) {
    size_t n = 1;
    while (n < v) n <<= 1;
    return n;
}

// stream-ordered work space of one call: one DevTemp per block, all given back (in stream order) when the call has enqueued its work.
// An empty piece is still a block of one word, so every kernel gets a valid pointer for it.
struct WorkSpace {
    hipStream_t s;
    std::deque<DevTemp> blocks;
    explicit WorkSpace(hipStream_t st) : s(st) {}
    int get(u64** p, size_t words, const char* what) {
        blocks.emplace_back(s);
        TRY(blocks.back().alloc(std::max<size_t>(words, 1), what));
        *p = blocks.back().p;
        return TF_OK;
    }
};

// grid-stride kernels of divide_kernels.h: 256-thread blocks, at most 8192 of them
template <class K, class... Args>
int launch(K kernel, long long threads, hipStream_t s, Args... args) {
    if (threads <= 0) return TF_OK;
    const long long blocks = std::min<long long>((threads + 255) / 256, 256 * 32);
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(256), 0, s, args...);
    HIPCHK(hipGetLastError());
    return TF_OK;
}
int copy_pad(const u64* src, long long src_bs, long long n_src, u64* dst, long long dst_bs, long long n_dst, long long batch, hipStream_t s) {
    return launch(tfk::copy_pad_kernel, n_dst * batch, s, src, src_bs, n_src, dst, dst_bs, n_dst, batch);
}
template <int L>
int bcast_mul(u64* A, const u64* B, long long period, long long total, hipStream_t s) {
    return launch(tfk::bcast_mul_kernel<L>, total, s, A, (const u64*)B, period, total);
}

// a transform of order n of `batch` slices whose first n_coeffs elements are read (the rest as zero; n_coeffs >= n: all)
int xform(DeviceCtx* ctx, const u64* in, long long in_bs, long long n_coeffs, u64* out, long long out_bs, size_t n, size_t batch, int L,
          bool inverse, hipStream_t s) {
    if (n == 1) return copy_pad(in, in_bs, (n_coeffs < 0 ? 1 : std::min<long long>(n_coeffs, 1)) * L, out, out_bs, L, (long long)batch, s);
    NttCall c(in, out, n, batch, L, inverse);
    c.in_bs = in_bs, c.out_bs = out_bs, c.n_coeffs = n_coeffs < (long long)n ? n_coeffs : -1;
    return run_ntt(ctx, c, s);
}

// dst (batch x N elements) = the rows of src (len elements each, src_bs words apart) folded modulo x^N - 1; long rows fold in steps
// of at most 64 terms per thread, so the first step fills the chip however short the modulus is
template <int L>
int fold(const u64* src, size_t len, long long src_bs, u64* dst, size_t N, size_t batch, hipStream_t s, WorkSpace& tmp) {
    if (len <= N) return copy_pad(src, src_bs, (long long)(len * L), dst, (long long)(N * L), (long long)(N * L), (long long)batch, s);
    const u64* cur = src;
    size_t cur_len = len;
    long long cur_bs = src_bs;
    for (;;) {
        const size_t M = cur_len > 64 * N ? next_pow2((cur_len + 63) / 64) : N;
        u64* target = dst;
        if (M != N) TRY(tmp.get(&target, batch * M * L, "divide fold step"));
        TRY(launch(tfk::fold_kernel, (long long)(batch * M * L), s, cur, (long long)(cur_len * L), cur_bs, target, (long long)(M * L),
                   (long long)batch));
        if (M == N) return TF_OK;
        cur = target, cur_len = M, cur_bs = (long long)(M * L);
    }
}

template <int L, int LOGN>
int launch_newton_lds(DeviceCtx* ctx, tfk::NewtonArgs A, hipStream_t s) {
    using G = tfk::NewtonGeom<L, LOGN>;
    TRY(get_lat_table(ctx, LOGN, false, &A.tw_f, -1));
    TRY(get_lat_table(ctx, LOGN, true, &A.tw_i, -1));
    A.ninv = gl::mont_inverse(gl::to_mont(u64(1) << LOGN));
    constexpr size_t lds = size_t(G::LDS_WORDS) * sizeof(u64);
    static_assert(lds <= 160 * 1024, "Newton lines must fit one workgroup's LDS");
    if constexpr (lds > 48 * 1024) {
        static std::atomic<unsigned long long> done_mask{0};
        TRY(ensure_dynamic_lds(reinterpret_cast<const void*>(&tfk::newton_lds_kernel<L, LOGN>), (int)lds, done_mask));
    }
    hipLaunchKernelGGL((tfk::newton_lds_kernel<L, LOGN>), dim3(1), dim3(G::WG), lds, s, A);
    HIPCHK(hipGetLastError());
    return TF_OK;
}

// H (k elements) = rev(b)^-1 mod x^k, b of m + 1 coefficients.  Doublings up to NewtonMax<L>::PMAX in one launch of
// newton_lds_kernel, each further one as two forward transforms, newton_point_kernel and an inverse transform.
template <int L>
int inverse_of_reversed(DeviceCtx* ctx, const u64* b, size_t m, size_t k, u64* H, int* status, hipStream_t s, WorkSpace& tmp) {
    using G = tfk::NewtonMax<L>;
    tfk::NewtonArgs A{};
    A.b = b;
    A.m = (long long)m;
    A.prec = (long long)std::min<size_t>(k, G::PMAX);
    A.h = H;
    A.status = status;
    int logn = 6;  // the order of the launch's last doubling p -> prec: 4p
    for (long long p = tfk::kNewtonSerial; p < A.prec; p *= 2) logn = std::max(logn, ilog2((size_t)p) + 2);
    int rc = TF_ERR_INTERNAL;
    switch (logn) {  // (orders above NewtonMax<L>::LOGN are never reached, and never instantiated: they would spill)
        case 6: rc = launch_newton_lds<L, 6>(ctx, A, s); break;
        case 7: rc = launch_newton_lds<L, 7>(ctx, A, s); break;
        case 8: rc = launch_newton_lds<L, 8>(ctx, A, s); break;
        case 9: rc = launch_newton_lds<L, 9>(ctx, A, s); break;
        case 10:
            if constexpr (G::LOGN >= 10) rc = launch_newton_lds<L, 10>(ctx, A, s);
            break;
        case 11:
            if constexpr (G::LOGN >= 11) rc = launch_newton_lds<L, 11>(ctx, A, s);
            break;
        case 12:
            if constexpr (G::LOGN >= 12) rc = launch_newton_lds<L, 12>(ctx, A, s);
            break;
    }
    TRY(rc);
    if (k <= (size_t)G::PMAX) return TF_OK;
    const size_t nb = m + 1;
    size_t nmax = 0;
    for (size_t p = G::PMAX; p < k; p = std::min(2 * p, k)) nmax = next_pow2(2 * p + std::min(2 * p, k) - 1);
    TRY(check_len(nmax));
    u64 *rb = nullptr, *X = nullptr, *Y = nullptr;
    TRY(tmp.get(&rb, nb * L, "divide newton work"));
    TRY(tmp.get(&X, nmax * L, "divide newton work"));
    TRY(tmp.get(&Y, nmax * L, "divide newton work"));
    TRY(launch(tfk::reverse_kernel<L>, (long long)nb, s, b, (long long)nb, rb));
    for (size_t p = G::PMAX; p < k;) {
        const size_t p2 = std::min(2 * p, k), N = next_pow2(2 * p + p2 - 1);
        const long long w = (long long)(N * L);
        TRY(xform(ctx, H, w, (long long)p, X, w, N, 1, L, false, s));
        TRY(xform(ctx, rb, w, (long long)std::min(p2, nb), Y, w, N, 1, L, false, s));
        TRY(launch(tfk::newton_point_kernel<L>, (long long)N, s, X, (const u64*)Y, (long long)N));
        TRY(xform(ctx, X, w, -1, X, w, N, 1, L, true, s));
        TRY(copy_pad(X, w, (long long)(p2 * L), H, (long long)(k * L), (long long)(p2 * L), 1, s));
        p = p2;
    }
    return TF_OK;
}

// Everything but the host-side argument checks (the entry points do those, before any HIP call).
template <int L>
int divide_dev_t(const u64* a, size_t na, size_t batch, const u64* b, size_t nb, u64* q, u64* r, hipStream_t s, int* status) {
    DeviceCtx* ctx = nullptr;
    TRY(current_ctx(&ctx));
    WorkSpace tmp(s);
    const size_t m = nb - 1;
    if (na < nb) {  // (zero, self): polynomial.rs:560-563
        if (status) TRY(launch(tfk::head_inverse_kernel<L>, 1, s, b + m * L, (const u64*)nullptr, (u64*)nullptr, status, 17, 0));
        if (r && m) TRY(copy_pad(a, (long long)(na * L), (long long)(na * L), r, (long long)(m * L), (long long)(m * L), (long long)batch, s));
        return TF_OK;
    }
    const size_t k = na - m;
    if (m == 0) {  // a constant divisor: q = a lc^-1, no remainder
        u64* w = nullptr;
        TRY(tmp.get(&w, L, "divide constant divisor"));
        TRY(launch(tfk::head_inverse_kernel<L>, 1, s, b, (const u64*)nullptr, w, status, 17, 0));
        if (q) TRY(launch(tfk::scale_kernel<L>, (long long)(batch * na), s, a, (const u64*)w, q, (long long)(batch * na)));
        return TF_OK;
    }
    // 1. h = rev(b)^-1 mod x^k, once for the batch
    u64* H = nullptr;
    TRY(tmp.get(&H, k * L, "divide quotient work"));
    TRY(inverse_of_reversed<L>(ctx, b, m, k, H, status, s, tmp));
    // 2. q = coefficients k - 1 .. 2k - 2 of a[m ..] * rev_k(h), every dividend against ONE transform of rev_k(h)
    const size_t M = next_pow2(2 * k - 1);
    TRY(check_len(M));
    const long long wm = (long long)(M * L);
    u64 *HR = nullptr, *Hh = nullptr, *C = nullptr;
    TRY(tmp.get(&HR, k * L, "divide quotient work"));
    TRY(tmp.get(&Hh, M * L, "divide quotient work"));
    TRY(tmp.get(&C, batch * M * L, "divide quotient work"));
    TRY(launch(tfk::reverse_kernel<L>, (long long)k, s, (const u64*)H, (long long)k, HR));
    TRY(xform(ctx, HR, wm, (long long)k, Hh, wm, M, 1, L, false, s));
    TRY(xform(ctx, a + m * L, (long long)(na * L), (long long)k, C, wm, M, batch, L, false, s));
    TRY(bcast_mul<L>(C, Hh, (long long)M, (long long)(batch * M), s));
    TRY(xform(ctx, C, wm, -1, C, wm, M, batch, L, true, s));
    u64* Q = q;
    if (!Q) TRY(tmp.get(&Q, batch * k * L, "divide unwanted quotient"));
    TRY(copy_pad(C + (k - 1) * L, wm, (long long)(k * L), Q, (long long)(k * L), (long long)(k * L), (long long)batch, s));
    if (!r) return TF_OK;
    // 3. r = fold(a) - fold(q) fold(b) modulo x^N - 1, low m coefficients: one cyclic product of order N = next_power_of_two(m)
    const size_t N = next_pow2(m);
    const long long wn = (long long)(N * L);
    u64 *FA = nullptr, *FQ = nullptr, *FB = nullptr;
    TRY(tmp.get(&FA, batch * N * L, "divide remainder work"));
    TRY(tmp.get(&FQ, batch * N * L, "divide remainder work"));
    TRY(tmp.get(&FB, N * L, "divide remainder work"));
    TRY(fold<L>(a, na, (long long)(na * L), FA, N, batch, s, tmp));
    TRY(fold<L>(Q, k, (long long)(k * L), FQ, N, batch, s, tmp));
    TRY(fold<L>(b, nb, (long long)(nb * L), FB, N, 1, s, tmp));
    TRY(xform(ctx, FQ, wn, -1, FQ, wn, N, batch, L, false, s));
    TRY(xform(ctx, FB, wn, -1, FB, wn, N, 1, L, false, s));
    TRY(bcast_mul<L>(FQ, FB, (long long)N, (long long)(batch * N), s));
    TRY(xform(ctx, FQ, wn, -1, FQ, wn, N, batch, L, true, s));
    return launch(tfk::sub_low_kernel<L>, (long long)(batch * m * L), s, (const u64*)FA, (const u64*)FQ, r, (long long)N, (long long)m,
                  (long long)batch);
}

// the checks every flavour returns before any HIP call
int divide_args(const u64* a, size_t na, size_t batch, const u64* b, size_t nb, const u64* q, const u64* r) {
    if (!q && !r) return TF_ERR_NULL_POINTER;
    if (nb == 0) return TF_ERR_DIVISION_BY_ZERO;  // "divisor should be non-zero", polynomial.rs:556-559
    if (!b || (na && batch && !a)) return TF_ERR_NULL_POINTER;
    if (batch > kMaxDivideBatch || na > kMaxDivideLen || nb > kMaxDivideLen) return TF_ERR_LEN_TOO_LARGE;
    return TF_OK;
}

}  // namespace

int divide_dev(const u64* a, size_t na, size_t batch, const u64* b, size_t nb, u64* q, u64* r, void* stream, int* status, int L) {
    TRY(divide_args(a, na, batch, b, nb, q, r));
    if (batch == 0) return TF_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return L == 1 ? divide_dev_t<1>(a, na, batch, b, nb, q, r, s, status) : divide_dev_t<3>(a, na, batch, b, nb, q, r, s, status);
}

static bool is_zero(const u64* x, int L) {
    u64 o = 0;
    for (int k = 0; k < L; ++k) o |= x[k];
    return o == 0;
}

int divide_host(const u64* a, size_t na, size_t batch, const u64* b, size_t nb, u64* q, u64* r, int L) {
    TRY(divide_args(a, na, batch, b, nb, q, r));
    if (is_zero(b + (nb - 1) * L, L)) return TF_ERR_INVALID_ARGUMENT;  // b not normalised
    if (batch == 0) return TF_OK;
    const size_t m = nb - 1, k = na >= nb ? na - m : 0;
    const size_t wa = batch * na * L, wq = q ? batch * k * L : 0, wr = r ? batch * m * L : 0;
    if (wq + wr == 0) return TF_OK;  // nothing to write (only empty outputs were asked for)
    DeviceCtx* ctx = nullptr;
    TRY(current_ctx(&ctx));
    hipStream_t s = host_stream();
    WorkSpace tmp(s);
    u64 *da = nullptr, *db = nullptr, *dq = nullptr, *dr = nullptr;
    TRY(tmp.get(&da, wa, "divide host inputs"));
    TRY(tmp.get(&db, nb * L, "divide host inputs"));
    if (wq) TRY(tmp.get(&dq, wq, "divide host quotient"));
    if (wr) TRY(tmp.get(&dr, wr, "divide host remainder"));
    TRY(h2d(da, a, wa, s));
    TRY(h2d(db, b, nb * L, s));
    TRY(divide_dev(da, na, batch, db, nb, dq, dr, s, nullptr, L));
    if (wq) TRY(d2h(q, dq, wq, s));
    if (wr) TRY(d2h(r, dr, wr, s));
    return sync(s);
}

// ---- formal_power_series_inverse_newton -----------------------------------------------------------------------------------
// The R-th Newton iterate f <- 2 f - f^2 g from f = g(0)^-1, R = ilog2(next_power_of_two(precision)), untruncated: deg f_R =
// (2^R - 1) d, d = deg g.  The reference's schedule (:1322-1365): g transformed ONCE at the final order F, every step pointwise
// against g^ read at stride F / D, and a low-degree extension (inverse transform, forward transform of the larger order) whenever
// the degree bound 2 deg + d reaches the domain D.  Every step is exact, so the words are the reference's.
size_t fps_len(size_t nf, size_t precision) {
    if (nf == 0 || precision > (size_t(1) << 62)) return 0;
    const size_t d = nf - 1;
    if (d == 0) return 1;
    const int R = ilog2(next_pow2(std::max<size_t>(precision, 1)));
    if (R >= 62) return 0;
    const size_t pw = (size_t(1) << R) - 1;
    if (pw && d > (kMaxFpsLen - 1) / pw) return 0;
    const size_t len = pw * d + 1;
    return len <= kMaxFpsLen ? len : 0;
}

namespace {
template <int L>
int fps_dev_t(const u64* f, size_t nf, size_t precision, u64* out, hipStream_t s, int* status) {
    DeviceCtx* ctx = nullptr;
    TRY(current_ctx(&ctx));
    const size_t d = nf - 1, len = fps_len(nf, precision);
    const u64* lead = f + d * L;
    if (len == 1)  // a constant, or precision <= 1: f_0 = g(0)^-1
        return launch(tfk::head_inverse_kernel<L>, 1, s, f, lead, out, status, (int)TF_ERR_INVERSE_OF_ZERO, (int)TF_ERR_INVALID_ARGUMENT);
    const int R = ilog2(next_pow2(std::max<size_t>(precision, 1)));
    const size_t F = next_pow2(len);
    TRY(check_len(F));
    WorkSpace tmp(s);
    u64 *Gh = nullptr, *X = nullptr, *Y = nullptr;
    TRY(tmp.get(&Gh, F * L, "fps_inverse work"));
    TRY(tmp.get(&X, F * L, "fps_inverse work"));
    TRY(tmp.get(&Y, F * L, "fps_inverse work"));
    TRY(xform(ctx, f, (long long)(F * L), (long long)nf, Gh, (long long)(F * L), F, 1, L, false, s));
    TRY(launch(tfk::head_inverse_kernel<L>, 1, s, f, lead, X, status, (int)TF_ERR_INVERSE_OF_ZERO, (int)TF_ERR_INVALID_ARGUMENT));
    size_t D = 1, deg = 0;
    for (int round = 0; round < R; ++round) {
        deg = 2 * deg + d;
        if (deg >= D) {  // lde: the iterate outgrows the domain
            const size_t D2 = next_pow2(deg + 1);
            TRY(xform(ctx, X, (long long)(D * L), -1, X, (long long)(D * L), D, 1, L, true, s));
            TRY(xform(ctx, X, (long long)(D2 * L), (long long)D, Y, (long long)(D2 * L), D2, 1, L, false, s));
            std::swap(X, Y);
            D = D2;
        }
        TRY(launch(tfk::fps_point_kernel<L>, (long long)D, s, X, (const u64*)Gh, (long long)(F / D), (long long)D));
    }
    TRY(xform(ctx, X, (long long)(D * L), -1, X, (long long)(D * L), D, 1, L, true, s));
    return copy_pad(X, (long long)(D * L), (long long)(len * L), out, (long long)(len * L), (long long)(len * L), 1, s);
}

// (a caller that sizes `out` from tf_poly_fps_inverse_newton_len, which is 0 for both of the first two cases, may pass NULL there:
// the reference's panic and the size limit come before the pointer checks)
int fps_args(const u64* f, size_t nf, size_t precision, const u64* out) {
    if (nf == 0) return TF_ERR_INVERSE_OF_ZERO;  // the reference indexes coefficients[0] of the zero polynomial
    if (fps_len(nf, precision) == 0) return TF_ERR_LEN_TOO_LARGE;
    if (!out || !f) return TF_ERR_NULL_POINTER;
    return TF_OK;
}

}  // namespace

int fps_dev(const u64* f, size_t nf, size_t precision, u64* out, void* stream, int* status, int L) {
    TRY(fps_args(f, nf, precision, out));
    hipStream_t s = static_cast<hipStream_t>(stream);
    return L == 1 ? fps_dev_t<1>(f, nf, precision, out, s, status) : fps_dev_t<3>(f, nf, precision, out, s, status);
}

int fps_host(const u64* f, size_t nf, size_t precision, u64* out, int L) {
    TRY(fps_args(f, nf, precision, out));
    if (is_zero(f, L)) return TF_ERR_INVERSE_OF_ZERO;
    if (is_zero(f + (nf - 1) * L, L)) return TF_ERR_INVALID_ARGUMENT;
    const size_t len = fps_len(nf, precision);
    return host_roundtrip(f, nf * L, nullptr, 0, out, len * L, [&](u64* df, u64*, u64* dout, hipStream_t s) { return fps_dev(df, nf, precision, dout, s, nullptr, L); });
}

}  // namespace tfi
