// points_kernels.h -- what a FRI query round does with points, kept in device memory:
//   Polynomial::get_colinear_y   math/polynomial.rs:386-394   out = (dy (p2x - x0) + dx y0) / dx, dx = x0 - x1, dy = y0 - y1
//   Polynomial::are_colinear     math/polynomial.rs:348-364   one verdict per group of k points
//   mod_pow / ModPowU32 / ModPowU64   b_field_element.rs:340-353, :650, :809, x_field_element.rs:654-680, element by element
//   first * ratio^i              CyclicGroupGenerator (b_field_element.rs:656-668, x_field_element.rs:423-435), the powers of scale
//   out[i] = src[indices[i]]     elements of 1..16 words
// A field element is W words (1 BFieldElement, 3 XFieldElement [c0, c1, c2]); words are canonical raw Montgomery words in and out,
// so every result is THE representative of its field element, however a quotient or a power is formed.
// WX is the width of the x-coordinates and WY that of the y-coordinates, (WX, WY) in {(1, 1), (3, 3), (1, 3)}: in the mixed form
// a BFieldElement x stands for its lift (x, 0, 0) (x_field_element.rs:491-556) and every product with it is three base-field
// products, so the result is word for word that of the (3, 3) form on the lifted x-coordinates.
#pragma once

#include "gl64.h"
#include "inverse_kernels.h"  // inv_mul, inv_single, inv_set_one, inv_is_zero
#include "pt_elements.h"      // pt_load, pt_store, pt_add, pt_sub, pt_eq, pt_sub_lift, pt_mul_xy

namespace tfk {

using gl::u32;
using gl::u64;

constexpr int kPtThreads = 256;

// one field element passed to a kernel by value: W words, the rest unused
struct PtScalar {
    u64 v[3];
};
// ratio^(2^j) for j <= 30, built on the host (tf_points.hip) and passed by value
constexpr int kPowersTableLen = 31;
struct PowersTable {
    u64 v[kPowersTableLen][3];
};

// ---- get_colinear_y ------------------------------------------------------------------------------------------------------------
// One pass, no work space, no LDS.  The division is Montgomery's trick per wave, laid out as inverse_kernels.h lays out the plain
// inversion: a wave owns a chunk of 64 K consecutive triples, lane l takes the triples l + 64 j (j < K) and keeps for each of them
// dx (WX words), the running product of the dx before it (WX words) and the numerator dy (p2x - x0) + dx y0 (WY words).  The wave
// then does ONE prefix / suffix product over the 64 lane totals and ONE inversion -- all of it in the field of dx, the base field
// in the mixed form -- and on the way back every triple costs two products in that field and one numerator * dx^-1.
// A missing tail triple and a triple with dx = 0 (the reference's assert_ne!, :387) enter the products as ONE; the latter makes its
// wave write `code` to *status (the first non-zero code stays) and leaves its own slot unspecified, the other triples of the wave
// keep their quotients.  K is chosen so that the (3, 3) form keeps everything in registers.
template <int WX, int WY>
struct ColinearGeom {
    static constexpr int K = WY == 1 ? 8 : WX == 1 ? 8 : 4;  // triples per lane
    static constexpr long long CHUNK = 64LL * K;              // triples one wave covers per step
};

template <int WX, int WY>
__global__ void __launch_bounds__(kPtThreads) get_colinear_y_kernel(const u64* x0, const u64* y0, const u64* x1, const u64* y1, long long n,
                                                                      const u64* p2x, int p2x_each, u64* out, int* status, int code) {
    constexpr int K = ColinearGeom<WX, WY>::K;
    constexpr long long CHUNK = ColinearGeom<WX, WY>::CHUNK;
    const int lane = threadIdx.x & 63;
    const long long waves = (long long)gridDim.x * (kPtThreads >> 6);
    const long long chunks = (n + CHUNK - 1) / CHUNK;
    u64 q0[WY];  // the one p2x of a broadcast call
    pt_load<WY>(p2x, 0, q0);
    // (the loop bound is the same for every lane of a wave: the shuffles below always run with the whole wave)
    for (long long c = (long long)blockIdx.x * (kPtThreads >> 6) + (threadIdx.x >> 6); c < chunks; c += waves) {
        const long long base = c * CHUNK + lane;
        u64 dx[K][WX], s[K][WX], num[K][WY], acc[WX];
        bool zero = false;
        inv_set_one<WX>(acc);
#pragma unroll
        for (int j = 0; j < K; ++j) {
            const long long i = base + 64LL * j;
            if (i < n) {
                u64 a[WX], b[WX], ya[WY], yb[WY], q[WY], dy[WY], t[WY];
                pt_load<WX>(x0, i, a);
                pt_load<WX>(x1, i, b);
                pt_load<WY>(y0, i, ya);
                pt_load<WY>(y1, i, yb);
                if (p2x_each) {
                    pt_load<WY>(p2x, i, q);
                } else {
#pragma unroll
                    for (int k = 0; k < WY; ++k) q[k] = q0[k];
                }
                pt_sub<WX>(a, b, dx[j]);
                pt_sub<WY>(ya, yb, dy);
                pt_sub_lift<WX, WY>(q, a, t);       // p2x - x0
                inv_mul<WY>(dy, t, t);              // dy (p2x - x0)
                pt_mul_xy<WX, WY>(dx[j], ya, num[j]);  // dx y0
                pt_add<WY>(t, num[j], num[j]);
                if (inv_is_zero<WX>(dx[j])) {
                    zero = true;
                    inv_set_one<WX>(dx[j]);
                }
            } else {
                inv_set_one<WX>(dx[j]);
#pragma unroll
                for (int k = 0; k < WY; ++k) num[j][k] = 0;
            }
#pragma unroll
            for (int k = 0; k < WX; ++k) s[j][k] = acc[k];
            inv_mul<WX>(acc, dx[j], acc);
        }
        // the lane totals: inclusive prefix and suffix products over the wave, one inversion, as batch_inverse_kernel
        u64 pre[WX], suf[WX];
#pragma unroll
        for (int k = 0; k < WX; ++k) pre[k] = suf[k] = acc[k];
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            u64 up[WX], dn[WX];
#pragma unroll
            for (int k = 0; k < WX; ++k) {
                up[k] = __shfl_up(pre[k], d, 64);
                dn[k] = __shfl_down(suf[k], d, 64);
            }
            if (lane >= d) inv_mul<WX>(up, pre, pre);
            if (lane + d < 64) inv_mul<WX>(suf, dn, suf);
        }
        u64 w[WX], wi[WX], ex_pre[WX], ex_suf[WX];
#pragma unroll
        for (int k = 0; k < WX; ++k) {
            w[k] = __shfl(pre[k], 63, 64);
            ex_pre[k] = __shfl_up(pre[k], 1, 64);
            ex_suf[k] = __shfl_down(suf[k], 1, 64);
        }
        if (lane == 0) inv_set_one<WX>(ex_pre);
        if (lane == 63) inv_set_one<WX>(ex_suf);
        inv_single<WX>(w, wi);  // W != 0: every zero was replaced by ONE
        inv_mul<WX>(wi, ex_pre, acc);
        inv_mul<WX>(acc, ex_suf, acc);  // (the lane's total)^-1
#pragma unroll
        for (int j = K - 1; j >= 0; --j) {
            u64 inv[WX], y[WY];
            inv_mul<WX>(acc, s[j], inv);  // dx_j^-1
            inv_mul<WX>(acc, dx[j], acc);
            pt_mul_xy<WX, WY>(inv, num[j], y);
            const long long i = base + 64LL * j;
            if (i < n) pt_store<WY>(out, i, y);
        }
        if (__any(zero) && lane == 0) atomicCAS(status, 0, code);
    }
}

// ---- are_colinear ----------------------------------------------------------------------------------------------------------------
// flags[g] = 1 when the k >= 3 points of group g have pairwise different x-coordinates (an XFieldElement compared on all three
// limbs) and every point from the third on lies on the line through the first two, else 0 (the launcher answers k < 3 itself).
// The reference forms the slope a = dy / dx and tests a x + b = y with b = y0 - a x0 (:360-363).  Once the x-coordinates are
// known to differ, dx != 0, and multiplying that equation by dx gives the equivalent dy (x - x0) = (y - y0) dx: the same verdict
// in exact field arithmetic, without any inversion.
template <int WX, int WY>
__device__ __forceinline__ bool pt_on_line(const u64 (&dx)[WX], const u64 (&dy)[WY], const u64 (&x0)[WX], const u64 (&y0)[WY], const u64 (&x)[WX],
                                           const u64 (&y)[WY]) {
    u64 ex[WX], l[WY], r[WY];
    pt_sub<WX>(x, x0, ex);
    pt_mul_xy<WX, WY>(ex, dy, l);  // dy (x - x0)
    pt_sub<WY>(y, y0, r);
    pt_mul_xy<WX, WY>(dx, r, r);  // (y - y0) dx
    return pt_eq<WY>(l, r);
}

// small groups (the FRI shape k = 3 among them): one lane per group, no cross-lane operation
template <int WX, int WY>
__global__ void __launch_bounds__(kPtThreads) are_colinear_lane_kernel(const u64* xs, const u64* ys, long long n_groups, int k, int* flags) {
    const long long step = (long long)gridDim.x * kPtThreads;
    for (long long g = (long long)blockIdx.x * kPtThreads + threadIdx.x; g < n_groups; g += step) {
        const long long p = g * k;
        bool ok = true;
        for (int i = 0; i + 1 < k; ++i) {
            u64 a[WX];
            pt_load<WX>(xs, p + i, a);
            for (int j = i + 1; j < k; ++j) {
                u64 b[WX];
                pt_load<WX>(xs, p + j, b);
                ok = ok && !pt_eq<WX>(a, b);
            }
        }
        u64 xa[WX], xb[WX], ya[WY], yb[WY], dx[WX], dy[WY];
        pt_load<WX>(xs, p, xa);
        pt_load<WX>(xs, p + 1, xb);
        pt_load<WY>(ys, p, ya);
        pt_load<WY>(ys, p + 1, yb);
        pt_sub<WX>(xa, xb, dx);
        pt_sub<WY>(ya, yb, dy);
        for (int j = 2; j < k; ++j) {
            u64 x[WX], y[WY];
            pt_load<WX>(xs, p + j, x);
            pt_load<WY>(ys, p + j, y);
            ok = ok && pt_on_line<WX, WY>(dx, dy, xa, ya, x, y);
        }
        flags[g] = ok ? 1 : 0;
    }
}

// larger groups: one wave per group.  The lanes split the pairwise comparisons (row i of the triangle: lane l takes the columns
// i + 1 + l + 64 m) and the checks of the further points; neither loop holds a cross-lane operation.  The verdict is one ballot per
// group, inside the loop over the groups alone, whose bound is the same for all lanes of a wave.
template <int WX, int WY>
__global__ void __launch_bounds__(kPtThreads) are_colinear_wave_kernel(const u64* xs, const u64* ys, long long n_groups, int k, int* flags) {
    const int lane = threadIdx.x & 63;
    const long long waves = (long long)gridDim.x * (kPtThreads >> 6);
    for (long long g = (long long)blockIdx.x * (kPtThreads >> 6) + (threadIdx.x >> 6); g < n_groups; g += waves) {
        const long long p = g * k;
        bool bad = false;
        for (int i = 0; i + 1 < k; ++i) {
            u64 a[WX];
            pt_load<WX>(xs, p + i, a);
            for (int j = i + 1 + lane; j < k; j += 64) {
                u64 b[WX];
                pt_load<WX>(xs, p + j, b);
                bad = bad || pt_eq<WX>(a, b);
            }
        }
        u64 xa[WX], xb[WX], ya[WY], yb[WY], dx[WX], dy[WY];
        pt_load<WX>(xs, p, xa);
        pt_load<WX>(xs, p + 1, xb);
        pt_load<WY>(ys, p, ya);
        pt_load<WY>(ys, p + 1, yb);
        pt_sub<WX>(xa, xb, dx);
        pt_sub<WY>(ya, yb, dy);
        for (int j = 2 + lane; j < k; j += 64) {
            u64 x[WX], y[WY];
            pt_load<WX>(xs, p + j, x);
            pt_load<WY>(ys, p + j, y);
            bad = bad || !pt_on_line<WX, WY>(dx, dy, xa, ya, x, y);
        }
        const bool any_bad = __any(bad);
        if (lane == 0) flags[g] = any_bad ? 0 : 1;
    }
}

// ---- mod_pow ---------------------------------------------------------------------------------------------------------------------
// out[i] = bases[i or 0] ^ exps[i or 0]; x^0 = 1 for every x, zero included (the reference's loop starts from ONE).
// General route (a base per element): right-to-left square-and-multiply per lane; the loop runs while exponent bits are left and holds no cross-lane
// operation, so lanes with short exponents simply finish early.
template <int W>
__global__ void __launch_bounds__(kPtThreads) mod_pow_kernel(const u64* bases, const u64* exps, int exp_each, u64* out, long long n) {
    const long long step = (long long)gridDim.x * kPtThreads;
    for (long long i = (long long)blockIdx.x * kPtThreads + threadIdx.x; i < n; i += step) {
        u64 b[W], acc[W];
        pt_load<W>(bases, i, b);
        u64 e = exps[exp_each ? i : 0];
        inv_set_one<W>(acc);
        while (e) {
            if (e & 1) inv_mul<W>(acc, b, acc);
            e >>= 1;
            if (e) inv_mul<W>(b, b, b);
        }
        pt_store<W>(out, i, acc);
    }
}

// Broadcast-base route (one base for all elements: g^index, offset^j).  Every workgroup first fills a 64-entry table of
// base^(2^j) in LDS -- the 63 squarings are a chain, so one wave runs them, every lane alike, and lane j keeps entry j -- and then
// forms each element from the entries of its set bits only: a 32-bit exponent costs about 16 products instead of about 48.
template <int W>
__global__ void __launch_bounds__(kPtThreads) mod_pow_table_kernel(const u64* base, const u64* exps, int exp_each, u64* out, long long n) {
    __shared__ u64 table[64][W];
    if (threadIdx.x < 64) {
        u64 b[W];
        pt_load<W>(base, 0, b);
        for (int j = 0; j < 64; ++j) {
            if ((int)threadIdx.x == j) {
#pragma unroll
                for (int k = 0; k < W; ++k) table[j][k] = b[k];
            }
            inv_mul<W>(b, b, b);
        }
    }
    __syncthreads();
    const long long step = (long long)gridDim.x * kPtThreads;
    for (long long i = (long long)blockIdx.x * kPtThreads + threadIdx.x; i < n; i += step) {
        u64 e = exps[exp_each ? i : 0];
        u64 acc[W];
        inv_set_one<W>(acc);
        while (e) {
            const int j = __builtin_ctzll(e);
            e &= e - 1;
            u64 t[W];
#pragma unroll
            for (int k = 0; k < W; ++k) t[k] = table[j][k];
            inv_mul<W>(acc, t, acc);
        }
        pt_store<W>(out, i, acc);
    }
}

// ---- powers ----------------------------------------------------------------------------------------------------------------------
// out[i] = first * ratio^i.  S = 2^log_s threads: thread t forms first * ratio^t from the table entries ratio^(2^j) of the set bits of
// t (j < log_s) and then walks t, t + S, t + 2 S, ... with one product by ratio^S = table entry log_s per element.  Neighbouring
// lanes own neighbouring elements, so every store of a wave covers consecutive elements.
template <int W>
__global__ void __launch_bounds__(kPtThreads) powers_kernel(PtScalar first, PowersTable tab, int log_s, u64* out, long long n) {
    const long long t = (long long)blockIdx.x * kPtThreads + threadIdx.x;
    if (t >= n) return;  // (no barrier below)
    u64 pw[W], stride[W];
#pragma unroll
    for (int k = 0; k < W; ++k) pw[k] = first.v[k], stride[k] = tab.v[log_s][k];
    for (int j = 0; j < log_s; ++j) {
        if ((t >> j) & 1) {
            u64 f[W];
#pragma unroll
            for (int k = 0; k < W; ++k) f[k] = tab.v[j][k];
            inv_mul<W>(pw, f, pw);
        }
    }
    for (long long i = t; i < n; i += 1ll << log_s) {
        pt_store<W>(out, i, pw);
        inv_mul<W>(pw, stride, pw);
    }
}

// ---- gather ----------------------------------------------------------------------------------------------------------------------
// out[i] = src[indices[i]] for elements of `width` words, run over the WORDS of out so that the stores of a wave are consecutive.
// An index >= src_len is not read: it writes `code` to *status (the first non-zero code stays) and leaves its slot of out as it was.
__global__ void __launch_bounds__(kPtThreads) gather_elements_kernel(const u64* src, long long src_len, int width, const u32* indices, long long n,
                                                                       u64* out, int* status, int code) {
    const long long words = n * width;
    const long long step = (long long)gridDim.x * kPtThreads;
    for (long long t = (long long)blockIdx.x * kPtThreads + threadIdx.x; t < words; t += step) {
        const long long i = t / width;
        const int k = (int)(t - i * width);
        const long long idx = (long long)indices[i];
        if (idx < src_len)
            out[t] = src[idx * width + k];
        else if (k == 0)
            atomicCAS(status, 0, code);
    }
}

}  // namespace tfk
