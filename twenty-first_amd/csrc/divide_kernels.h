// divide_kernels.h -- device side of polynomial division with remainder and of the power-series inverse (launchers: tf_divide.hip).
//
// Division of a by b (math/polynomial.rs:539-600), k = na - nb + 1 quotient coefficients, m = nb - 1 = deg b:
//   h = rev(b)^-1 mod x^k            Newton doublings h <- h (2 - rev(b) h); every doubling whose transforms fit one workgroup's LDS
//                                    runs inside ONE launch (newton_lds_kernel), the larger ones on the library's transforms with
//                                    newton_point_kernel between them
//   rev(q) = (rev(a) mod x^k) h mod x^k, taken as the coefficients k - 1 .. 2k - 2 of a[m ..] * rev_k(h): the dividends are read
//                                    in place (no reversal), h is reversed once per call
//   r = (a - q b) mod (x^N - 1), N = next_power_of_two(m): deg(a - q b) < m <= N, so the remainder is the low m coefficients of
//                                    fold(a) - fold(q) * fold(b) with ONE cyclic product of order N (fold_kernel folds modulo x^N - 1)
// Field elements are L words (1 BFieldElement, 3 XFieldElement); every store is an ordinary vector store.
#pragma once

#include "lat_kernels.h"

namespace tfk {

// ---- field element helpers (poly_kernels.h has twins; that header's plain kernels belong to tf_poly.hip's unit alone)
__device__ __forceinline__ void dv_xfe_mul(const u64 (&s)[3], const u64 (&o)[3], u64 (&r)[3]) {
    // x_field_element.rs:512-536 with self = [c, b, a], other = [f, e, d]
    const u64 c = s[0], b = s[1], a = s[2], f = o[0], e = o[1], d = o[2];
    const u64 ae = gl::mont_mul(a, e), bd = gl::mont_mul(b, d), ad = gl::mont_mul(a, d);
    r[0] = gl::sub(gl::sub(gl::mont_mul(c, f), ae), bd);
    r[1] = gl::add(gl::add(gl::sub(gl::add(gl::mont_mul(b, f), gl::mont_mul(c, e)), ad), ae), bd);
    r[2] = gl::add(gl::add(gl::add(gl::mont_mul(a, f), gl::mont_mul(b, e)), gl::mont_mul(c, d)), ad);
}
template <int L>
__device__ __forceinline__ void dv_mul(const u64 (&a)[L], const u64 (&b)[L], u64 (&r)[L]) {
    if constexpr (L == 1) r[0] = gl::mont_mul(a[0], b[0]);
    else dv_xfe_mul(a, b, r);
}
// a^-1 (zero -> zero, and false); the extension field by the cofactors of the multiplication matrix (poly_kernels.h: xfe_inverse)
template <int L>
__device__ __forceinline__ bool dv_inv(const u64 (&a)[L], u64 (&r)[L]) {
    if constexpr (L == 1) {
        r[0] = gl::mont_inverse(a[0]);
        return a[0] != 0;
    } else {
        const u64 s = gl::add(a[0], a[2]), dd = gl::sub(a[1], a[2]);
        const u64 c0 = gl::sub(gl::mont_mul(s, s), gl::mont_mul(dd, a[1]));
        const u64 c1 = gl::sub(gl::mont_mul(dd, a[2]), gl::mont_mul(a[1], s));
        const u64 c2 = gl::sub(gl::mont_mul(a[1], a[1]), gl::mont_mul(s, a[2]));
        const u64 det = gl::sub(gl::sub(gl::mont_mul(a[0], c0), gl::mont_mul(a[2], c1)), gl::mont_mul(a[1], c2));
        const u64 di = gl::mont_inverse(det);
        r[0] = gl::mont_mul(c0, di);
        r[1] = gl::mont_mul(c1, di);
        r[2] = gl::mont_mul(c2, di);
        return det != 0;
    }
}
template <int L>
__device__ __forceinline__ bool dv_is_zero(const u64 (&a)[L]) {
    u64 o = 0;
#pragma unroll
    for (int k = 0; k < L; ++k) o |= a[k];
    return o == 0;
}
template <int L>
__device__ __forceinline__ void dv_load(const u64* p, u64 (&r)[L]) {
#pragma unroll
    for (int k = 0; k < L; ++k) r[k] = p[k];
}
template <int L>
__device__ __forceinline__ void dv_store(u64* p, const u64 (&r)[L]) {
#pragma unroll
    for (int k = 0; k < L; ++k) p[k] = r[k];
}
// status word of the _dev calls: the first non-zero code written wins (include/tf_hip.h, the *_dev_async convention)
__device__ __forceinline__ void dv_report(int* status, int code) {
    if (status) atomicCAS(status, 0, code);
}

// inv = x^-1 (one element).  x zero -> code_x; otherwise `other` (may be null) zero -> code_other.  One thread.
template <int L>
__global__ void __launch_bounds__(256) head_inverse_kernel(const u64* x, const u64* other, u64* inv, int* status, int code_x, int code_other) {
    if (threadIdx.x != 0) return;
    u64 a[L], r[L];
    dv_load<L>(x, a);
    const bool ok = dv_inv<L>(a, r);
    if (!ok) dv_report(status, code_x);
    if (ok && other) {
        u64 o[L];
        dv_load<L>(other, o);
        if (dv_is_zero<L>(o)) dv_report(status, code_other);
    }
    if (inv) dv_store<L>(inv, r);
}

// out[i] = in[i] * s[0], i < count elements (the quotient by a constant divisor: q = a lc^-1)
template <int L>
__global__ void __launch_bounds__(256) scale_kernel(const u64* in, const u64* s, u64* out, long long count) {
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long stride = (long long)gridDim.x * blockDim.x;
    u64 c[L];
    dv_load<L>(s, c);
    for (; i < count; i += stride) {
        u64 a[L], r[L];
        dv_load<L>(in + i * L, a);
        dv_mul<L>(a, c, r);
        dv_store<L>(out + i * L, r);
    }
}

// dst[b * dst_bs + w] = w < n_src ? src[b * src_bs + w] : 0, w < n_dst (words; every copy, truncation and zero padding of the calls)
__global__ void __launch_bounds__(256) copy_pad_kernel(const u64* src, long long src_bs, long long n_src, u64* dst, long long dst_bs, long long n_dst,
                                                       long long batch) {
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (; i < n_dst * batch; i += stride) {
        const long long b = i / n_dst, w = i - b * n_dst;
        dst[b * dst_bs + w] = w < n_src ? src[b * src_bs + w] : 0;
    }
}

// dst[b][w] = sum over u = w (mod m_words), u < n_words of src[b][u]: polynomials of n_words / L coefficients folded modulo x^M - 1
// (m_words = M L, so the limbs stay apart).  One thread per output word and row; the host folds in steps of at most 64 terms.
__global__ void __launch_bounds__(256) fold_kernel(const u64* src, long long n_words, long long src_bs, u64* dst, long long m_words, long long batch) {
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (; i < m_words * batch; i += stride) {
        const long long b = i / m_words, w = i - b * m_words;
        const u64* s = src + b * src_bs;
        u64 acc = 0;
        for (long long u = w; u < n_words; u += m_words) acc = gl::add(acc, s[u]);
        dst[i] = acc;
    }
}

// dst[i] = src[n - 1 - i], i < n elements (rev(b) for the large Newton doublings; rev_k(h) for the quotient's product)
template <int L>
__global__ void __launch_bounds__(256) reverse_kernel(const u64* src, long long n, u64* dst) {
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (; i < n; i += stride) {
        u64 a[L];
        dv_load<L>(src + (n - 1 - i) * L, a);
        dv_store<L>(dst + i * L, a);
    }
}

// A[i] = A[i] * B[i mod period]: every dividend's transform times the shared one
template <int L>
__global__ void __launch_bounds__(256) bcast_mul_kernel(u64* A, const u64* B, long long period, long long total) {
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (; i < total; i += stride) {
        u64 a[L], b[L], r[L];
        dv_load<L>(A + i * L, a);
        dv_load<L>(B + (i % period) * L, b);
        dv_mul<L>(a, b, r);
        dv_store<L>(A + i * L, r);
    }
}

// H[i] = H[i] (2 - R[i] H[i]): one Newton doubling of the inverse of rev(b) in the transform domain
template <int L>
__device__ __forceinline__ void dv_newton(const u64 (&h)[L], const u64 (&r)[L], u64 (&out)[L]) {
    u64 t[L];
    dv_mul<L>(r, h, t);
#pragma unroll
    for (int k = 0; k < L; ++k) t[k] = gl::neg(t[k]);
    t[0] = gl::add(t[0], gl::add(gl::ONE, gl::ONE));
    dv_mul<L>(h, t, out);
}
template <int L>
__global__ void __launch_bounds__(256) newton_point_kernel(u64* H, const u64* R, long long n) {
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (; i < n; i += stride) {
        u64 h[L], r[L], o[L];
        dv_load<L>(H + i * L, h);
        dv_load<L>(R + i * L, r);
        dv_newton<L>(h, r, o);
        dv_store<L>(H + i * L, o);
    }
}

// F[j] = 2 F[j] - F[j]^2 G[j * stride]: the step of formal_power_series_inverse_newton (math/polynomial.rs:1349-1359), G the
// transform of the series at the final order, read at the stride of the current domain
template <int L>
__global__ void __launch_bounds__(256) fps_point_kernel(u64* F, const u64* G, long long stride, long long n) {
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long st = (long long)gridDim.x * blockDim.x;
    for (; i < n; i += st) {
        u64 f[L], g[L], o[L];
        dv_load<L>(F + i * L, f);
        dv_load<L>(G + i * stride * L, g);
        dv_newton<L>(f, g, o);
        dv_store<L>(F + i * L, o);
    }
}

// r[b][i] = fa[b][i] - c[b][i], i < m   (fa, c: rows of n elements; r: rows of m)
template <int L>
__global__ void __launch_bounds__(256) sub_low_kernel(const u64* fa, const u64* c, u64* r, long long n, long long m, long long batch) {
    long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (; i < m * batch * L; i += stride) {
        const long long b = i / (m * L), w = i - b * m * L;
        r[i] = gl::sub(fa[b * n * L + w], c[b * n * L + w]);
    }
}

// ---- the small Newton doublings in ONE launch --------------------------------------------------------------------------------
// One workgroup computes h = rev(b)^-1 mod x^prec, prec <= N / 2: thread 0 runs the first 16 coefficients by the recurrence
// h_i = -lc^-1 sum_(j=1..i) b_(m-j) h_(i-j); then every doubling p -> 2p is three transforms of order N (N >= 4p > deg h^2 rev(b):
// exact) with the stages of ntt_lat_kernel as a device function (lat_xform, as tree_down_level_kernel runs them), h kept in LDS:
//   r^ = NTT(rev(b) mod x^2p)  (the reversal and truncation are the first stage's load), read into registers at this thread's
//   first-stage indices;  h^ = NTT(h);  h = iNTT(h^ (2 - r^ h^)) mod x^2p  (the pointwise step is the inverse's load).
// N is the order the LAST doubling needs (the host picks the instantiation); the earlier doublings run at that order too: one
// transform length per kernel keeps the stages within the register budget (several orders inlined into one kernel spill).
// LDS: two line buffers of L x N words and h.  BFieldElement: N <= 2^12 (512 threads, 90 KiB).  XFieldElement: N <= 2^9 (192
// threads, 33 KiB): the three limb lines of 2^11 would fit LDS twice, but the registers bound it first -- with the extension-field
// step in the inverse's load, 2^11 (768 threads, 170 VGPRs per lane) spills ~500 bytes per lane and 2^10 (384 threads, 256 VGPRs)
// 80 bytes; 2^9 runs spill-free.
template <int L, int LOGN>
struct NewtonGeom {
    static constexpr int N = 1 << LOGN;
    static constexpr int WG = L * N / 8;        // one thread group of N / 8 per limb line
    static constexpr int BUF = lat_pad(L * N) + 8;
    static constexpr int PMAX = N / 2;          // precision after a doubling at this order
    static constexpr int LDS_WORDS = 2 * BUF + PMAX * L;
};
template <int L>
struct NewtonMax {
    static constexpr int LOGN = L == 1 ? 12 : 9;
    static constexpr int PMAX = (1 << LOGN) / 2;  // the precision one launch reaches: 2048 (BFieldElement), 256 (XFieldElement)
};
constexpr int kNewtonSerial = 16;  // coefficients of the serial start (the first transform has order 64 at least)
struct NewtonArgs {
    const u64* b;      // the divisor, m + 1 coefficients
    long long m;
    long long prec;    // coefficients of h to produce (<= N / 2)
    u64* h;            // out: prec coefficients
    int* status;       // or null: TF_ERR_INVALID_ARGUMENT (17) when b[m] == 0
    const u64* tw_f;   // ntt_lat_kernel's tables of order N, forward / inverse (tf_lat.hip: get_lat_table)
    const u64* tw_i;
    u64 ninv;
};

template <int L, int LOGN>
__global__ void __launch_bounds__((NewtonGeom<L, LOGN>::WG)) newton_lds_kernel(const NewtonArgs A) {
    using G = NewtonGeom<L, LOGN>;
    constexpr int N = G::N, TPT = N / 8;
    extern __shared__ __attribute__((aligned(16))) u64 lds[];
    u64* hb = lds + 2 * G::BUF;
    const int t = threadIdx.x, g = t / TPT, j = t - g * TPT, limb = g;  // thread group g transforms limb line g
    const long long m = A.m;
    const u64* b = A.b;
    const int prec = (int)A.prec, p0 = prec < kNewtonSerial ? prec : kNewtonSerial;
    if (t == 0) {
        u64 lc[L], inv[L];
        dv_load<L>(b + m * L, lc);
        if (!dv_inv<L>(lc, inv)) dv_report(A.status, 17);
        dv_store<L>(hb, inv);
        for (int i = 1; i < p0; ++i) {
            u64 acc[L];
#pragma unroll
            for (int k = 0; k < L; ++k) acc[k] = 0;
            for (int jj = 1; jj <= i && jj <= m; ++jj) {
                u64 c[L], x[L], pr[L];
                dv_load<L>(b + (m - jj) * L, c);
                dv_load<L>(hb + (i - jj) * L, x);
                dv_mul<L>(c, x, pr);
#pragma unroll
                for (int k = 0; k < L; ++k) acc[k] = gl::add(acc[k], pr[k]);
            }
            u64 hi[L];
            dv_mul<L>(acc, inv, hi);
#pragma unroll
            for (int k = 0; k < L; ++k) hi[k] = gl::neg(hi[k]);
            dv_store<L>(hb + i * L, hi);
        }
    }
    __syncthreads();
    for (int p = p0; p < prec;) {
        const int p2 = 2 * p < prec ? 2 * p : prec;
        LatChain<LOGN> ch{lds, lds + G::BUF};
        u64* o = ch.out();
        lat_xform<LOGN, false>(A.tw_f, 0, g, j, ch.first, ch.second,
                               [&](int, int idx) __attribute__((always_inline)) -> u64 { return (idx < p2 && idx <= m) ? b[(m - idx) * L + limb] : 0; },
                               [&](int idx, u64 v) __attribute__((always_inline)) { o[lat_pad(g * N + idx)] = v; });
        __syncthreads();
        u64 rv[8][L];
#pragma unroll
        for (int r = 0; r < 8; ++r)
#pragma unroll
            for (int k = 0; k < L; ++k) rv[r][k] = o[lat_pad(k * N + j + r * TPT)];
        ch.next(), o = ch.out();  // the buffer holding r^ is written again only after the barrier inside the next transform
        lat_xform<LOGN, false>(A.tw_f, 0, g, j, ch.first, ch.second,
                               [&](int, int idx) __attribute__((always_inline)) -> u64 { return idx < p ? hb[idx * L + limb] : 0; },
                               [&](int idx, u64 v) __attribute__((always_inline)) { o[lat_pad(g * N + idx)] = v; });
        __syncthreads();
        const u64* in = o;
        ch.next();
        lat_xform<LOGN, true>(A.tw_i, A.ninv, g, j, ch.first, ch.second,
                              [&](int r, int idx) __attribute__((always_inline)) -> u64 {
                                  u64 hh[L], rr[L], e[L];
#pragma unroll
                                  for (int k = 0; k < L; ++k) hh[k] = in[lat_pad(k * N + idx)], rr[k] = rv[r][k];
                                  dv_newton<L>(hh, rr, e);
                                  return e[limb];
                              },
                              [&](int idx, u64 v) __attribute__((always_inline)) { if (idx < p2) hb[idx * L + limb] = v; });
        __syncthreads();
        p = p2;
    }
    for (int w = t; w < prec * L; w += G::WG) A.h[w] = hb[w];
}

}  // namespace tfk
