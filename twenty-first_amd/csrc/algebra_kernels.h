// algebra_kernels.h -- the plain arithmetic between the library's other calls, on polynomials and codewords that stay in device
// memory (math/polynomial.rs unless noted):
//   Add :2526-2563, Sub :2565-, Neg :2700-          element-wise, the shorter operand reads as zero above its length
//   scalar_mul :498-532, Mul<S> :2650-2686          every coefficient times one scalar
//   scale :760-773                                  coefficient j times alpha^j
//   formal_derivative :275-285                      out[j] = FF::from(j + 1) * a[j + 1]
//   degree :181                                     index of the highest non-zero coefficient, -1 for the zero polynomial
//   Mul<BFieldElement> for XFieldElement            x_field_element.rs:540-548, element-wise over two vectors
//   sum_j w_j * column_j                            "scalar_mul each, then Add them all", fused: every column is read once
// A field element is W words (1 BFieldElement, 3 XFieldElement); words are canonical raw Montgomery words in and out, so every
// result is THE representative of its field element and equals the reference's however a power or a sum is formed.
//
// Addition, subtraction, negation and every product with a BFieldElement scalar act on the three words of an XFieldElement
// independently (x_field_element.rs:491-556), so those kernels run over WORDS: lane l of a wave touches word base + l, and each
// load and store instruction of a wave covers 64 consecutive words whatever the element width.  Only the XFieldElement x
// XFieldElement products need a whole element per lane; there a lane reads its three words with three loads of stride 3, which
// together cover 192 consecutive words (the layout of hadamard_xfe_kernel, poly_kernels.h).
#pragma once

#include "gl64.h"
#include "acc_cols.h"
#include "inverse_kernels.h"  // inv_mul<3>: the XFieldElement product (x_field_element.rs:512-536)

namespace tfk {

using gl::u32;
using gl::u64;

// a scalar passed to a kernel by value: W words, the rest unused
struct AlgScalar {
    u64 v[3];
};

constexpr int kAlgThreads = 256;

// word t of a packed XFieldElement array belongs to element t / 3, limb t % 3
__device__ __forceinline__ void alg_split3(long long t, long long& e, int& k) {
    e = t / 3;
    k = (int)(t - 3 * e);
}

// ---- Add / Sub ---------------------------------------------------------------------------------------------------------------
// lengths in WORDS; row r of a / b / out starts at r * na / r * nb / r * max(na, nb).  out may be a or b where the lengths agree:
// every word is read and written by the same thread.  grid = (blocks over the row, rows).
template <bool SUB>
__global__ void __launch_bounds__(kAlgThreads) poly_addsub_kernel(const u64* a, long long na, const u64* b, long long nb, u64* out, long long rows) {
    const long long nmax = na > nb ? na : nb;
    const long long step = (long long)gridDim.x * kAlgThreads;
    for (long long r = blockIdx.y; r < rows; r += gridDim.y) {
        const u64* ar = a + r * na;
        const u64* br = b + r * nb;
        u64* o = out + r * nmax;
        for (long long j = (long long)blockIdx.x * kAlgThreads + threadIdx.x; j < nmax; j += step) {
            const u64 x = j < na ? ar[j] : 0, y = j < nb ? br[j] : 0;
            o[j] = SUB ? gl::sub(x, y) : gl::add(x, y);
        }
    }
}

// ---- Neg ---------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kAlgThreads) poly_neg_kernel(const u64* a, u64* out, long long words) {
    const long long step = (long long)gridDim.x * kAlgThreads;
    for (long long t = (long long)blockIdx.x * kAlgThreads + threadIdx.x; t < words; t += step) out[t] = gl::neg(a[t]);
}

// ---- products with one scalar that run over words ---------------------------------------------------------------------------
// WS = 1: out[t] = a[t] * s (BFieldElement and XFieldElement coefficients alike, x_field_element.rs:540-548)
// WS = 3: BFieldElement coefficients times an XFieldElement scalar: out word t = a[t / 3] * s[t % 3] (Mul<XFieldElement> for
//         BFieldElement :550-556 is the lift of the coefficient, whose upper limbs are zero)
template <int WS>
__global__ void __launch_bounds__(kAlgThreads) poly_scalar_mul_words_kernel(const u64* a, AlgScalar s, u64* out, long long words) {
    const long long step = (long long)gridDim.x * kAlgThreads;
    for (long long t = (long long)blockIdx.x * kAlgThreads + threadIdx.x; t < words; t += step) {
        if constexpr (WS == 1) {
            out[t] = gl::mont_mul(a[t], s.v[0]);
        } else {
            long long e;
            int k;
            alg_split3(t, e, k);
            out[t] = gl::mont_mul(a[e], k == 0 ? s.v[0] : k == 1 ? s.v[1] : s.v[2]);
        }
    }
}

// XFieldElement coefficients times an XFieldElement scalar, one element per lane; out may be a
__global__ void __launch_bounds__(kAlgThreads) poly_scalar_mul_xx_kernel(const u64* a, AlgScalar s, u64* out, long long count) {
    const long long step = (long long)gridDim.x * kAlgThreads;
    const u64 sv[3] = {s.v[0], s.v[1], s.v[2]};
    for (long long i = (long long)blockIdx.x * kAlgThreads + threadIdx.x; i < count; i += step) {
        u64 x[3] = {a[3 * i], a[3 * i + 1], a[3 * i + 2]};
        inv_mul<3>(x, sv, x);
        out[3 * i] = x[0];
        out[3 * i + 1] = x[1];
        out[3 * i + 2] = x[2];
    }
}

// Mul<BFieldElement> for XFieldElement (x_field_element.rs:540-548) over two vectors: out word t = a[t] * b[t / 3]; out may be a
__global__ void __launch_bounds__(kAlgThreads) hadamard_xfe_bfe_kernel(const u64* a, const u64* b, u64* out, long long words) {
    const long long step = (long long)gridDim.x * kAlgThreads;
    for (long long t = (long long)blockIdx.x * kAlgThreads + threadIdx.x; t < words; t += step) out[t] = gl::mont_mul(a[t], b[t / 3]);
}

// ---- formal_derivative --------------------------------------------------------------------------------------------------------
// rows of na coefficients in, na - 1 out: out word t of a row (element j = t / W) = a word t + W times BFieldElement::new(j + 1).
// The input row is one coefficient longer than the output row, so out may NOT be a.
template <int W>
__global__ void __launch_bounds__(kAlgThreads) poly_derivative_kernel(const u64* a, long long na, u64* out, long long rows) {
    const long long nw = (na - 1) * W;
    const long long step = (long long)gridDim.x * kAlgThreads;
    for (long long r = blockIdx.y; r < rows; r += gridDim.y) {
        const u64* ar = a + r * na * W + W;
        u64* o = out + r * nw;
        for (long long t = (long long)blockIdx.x * kAlgThreads + threadIdx.x; t < nw; t += step) {
            const long long j = W == 1 ? t : t / 3;
            o[t] = gl::mont_mul(ar[t], gl::to_mont((u64)(j + 1)));
        }
    }
}

// ---- scale ------------------------------------------------------------------------------------------------------------------
// out[j] = a[j] * alpha^j.  A row is walked by S threads (S a power of two, grid = (S / 256, rows)): thread t owns the
// coefficients t, t + S, t + 2 S, ... -- a run whose neighbours in memory belong to the neighbouring lanes, so every load and
// store of a wave still covers consecutive elements.  The thread forms alpha^t ONCE by square-and-multiply on the bits of t, low
// bit first; the squarings of that chain end in alpha^S, the factor that carries the running power from one coefficient of the
// run to the next.  So a thread pays log2(S) squarings and popcount(t) products up front and one product per coefficient after
// that; the launcher picks S so that a run holds at least ScaleRun coefficients.
template <int WAL>
struct ScaleRun {
    static constexpr int value = WAL == 1 ? 16 : 64;
};

template <int WA, int WAL>
__global__ void __launch_bounds__(kAlgThreads) poly_scale_kernel(const u64* a, long long na, AlgScalar alpha, u64* out, long long rows, int log_s) {
    constexpr int WO = WA > WAL ? WA : WAL;
    const long long S = 1ll << log_s;
    const long long t = (long long)blockIdx.x * kAlgThreads + threadIdx.x;
    if (t >= na) return;  // (no barrier below)
    u64 sq[WAL], pw0[WAL];
#pragma unroll
    for (int k = 0; k < WAL; ++k) {
        sq[k] = alpha.v[k];
        pw0[k] = k ? 0 : gl::ONE;
    }
#pragma unroll 1
    for (int bit = 0; bit < log_s; ++bit) {
        if ((t >> bit) & 1) inv_mul<WAL>(pw0, sq, pw0);
        inv_mul<WAL>(sq, sq, sq);
    }
    // sq = alpha^S, pw0 = alpha^t
    for (long long r = blockIdx.y; r < rows; r += gridDim.y) {
        const u64* ar = a + r * na * WA;
        u64* o = out + r * na * WO;
        u64 pw[WAL];
#pragma unroll
        for (int k = 0; k < WAL; ++k) pw[k] = pw0[k];
        for (long long j = t; j < na; j += S) {
            u64 x[WA], y[WO];
#pragma unroll
            for (int k = 0; k < WA; ++k) x[k] = ar[j * WA + k];
            if constexpr (WA == WAL) {
                inv_mul<WA>(x, pw, y);
            } else if constexpr (WA == 3) {  // XFieldElement coefficient, BFieldElement power
#pragma unroll
                for (int k = 0; k < 3; ++k) y[k] = gl::mont_mul(x[k], pw[0]);
            } else {  // BFieldElement coefficient, XFieldElement power
#pragma unroll
                for (int k = 0; k < 3; ++k) y[k] = gl::mont_mul(x[0], pw[k]);
            }
#pragma unroll
            for (int k = 0; k < WO; ++k) o[j * WO + k] = y[k];
            if (j + S < na) inv_mul<WAL>(pw, sq, pw);
        }
    }
}

// ---- degree -----------------------------------------------------------------------------------------------------------------
// deg[r] holds -1 when the kernel starts.  A row is scanned from the top in chunks of 256 coefficients, chunk c by workgroup
// c mod gridDim.x: a workgroup stops at its first chunk with a non-zero coefficient (the lowest such lane of each wave raises
// deg[r] with a vector atomic max) and at the first chunk that lies wholly below what some workgroup has already found.  With a
// non-zero leading coefficient every workgroup reads one chunk; only a row of zeros is read to the end.
template <int W>
__global__ void __launch_bounds__(kAlgThreads) poly_degree_kernel(const u64* a, long long na, long long rows, long long* deg) {
    const long long chunks = (na + kAlgThreads - 1) / kAlgThreads;
    for (long long r = blockIdx.y; r < rows; r += gridDim.y) {
        const u64* ar = a + r * na * W;
        for (long long c = blockIdx.x; c < chunks; c += gridDim.x) {
            const long long top = na - 1 - c * kAlgThreads;  // the highest index of this chunk
            int below = 0;
            if (threadIdx.x == 0) below = *reinterpret_cast<volatile long long*>(&deg[r]) >= top;
            if (__syncthreads_or(below)) break;
            const long long i = top - threadIdx.x;
            bool nz = false;
            if (i >= 0) {
                u64 o = ar[i * W];
#pragma unroll
                for (int k = 1; k < W; ++k) o |= ar[i * W + k];
                nz = o != 0;
            }
            const unsigned long long m = __ballot(nz);
            if (m && (threadIdx.x & 63) == __ffsll((long long)m) - 1) atomicMax(&deg[r], i);
            if (__syncthreads_or(nz)) break;
        }
    }
}

// ---- linear combination --------------------------------------------------------------------------------------------------------
// out[i] = sum_{j < k} polys[j * stride + i] * weights[j],  i < n.  Lanes run along i, so a wave reads 64 consecutive elements of
// one column per load and a workgroup 2 KiB (BFieldElement columns) or 6 KiB (XFieldElement) before it moves to the next column;
// weights[j] is the same for the whole launch and comes through uniform loads.
//
// The deferred reduction and its accumulators (AccCols, acc_mul_add, acc_reduce) are in acc_cols.h, shared with deep_kernels.h.
// WP = 1 serves XFieldElement columns with BFieldElement weights too: the launcher passes 3 n words per column (the limbs are
// independent under a BFieldElement weight).  WP = 3 is XFieldElement x XFieldElement: the five coefficients of the unreduced
// degree-4 product are accumulated (sums of products only) and x^3 = x - 1 is applied once at the end, as
// x_field_element.rs:512-536 does per product:  r0 = d0 - d3,  r1 = d1 + d3 - d4,  r2 = d2 + d4.
template <int WP, int WW>
__global__ void __launch_bounds__(kAlgThreads) poly_lincomb_kernel(const u64* __restrict__ polys, long long n, long long stride, int k,
                                                                  const u64* __restrict__ w, u64* __restrict__ out) {
    static_assert(WP == 1 || WW == 3, "XFieldElement columns under BFieldElement weights run as words (WP = 1)");
    constexpr int WO = WW;  // = max(WP, WW) for the three instantiations
    const long long step = (long long)gridDim.x * kAlgThreads;
    for (long long i = (long long)blockIdx.x * kAlgThreads + threadIdx.x; i < n; i += step) {
        const u64* col = polys + i * WP;
        u64 r[WO];
        if constexpr (WP == 1) {
            AccCols acc[WO];
#pragma unroll
            for (int m = 0; m < WO; ++m) acc_zero(acc[m]);
            // four columns per step, their loads issued together (the inline assembly is a convergent operation to the compiler,
            // which therefore does not unroll a loop of unknown trip count around it)
            int j = 0;
            for (; j + 4 <= k; j += 4) {
                u64 x[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) x[u] = col[(long long)(j + u) * stride];
#pragma unroll
                for (int u = 0; u < 4; ++u)
#pragma unroll
                    for (int m = 0; m < WO; ++m) acc_mul_add(acc[m], x[u], w[(long long)(j + u) * WW + m]);
            }
            for (; j < k; ++j) {
                const u64 x = col[(long long)j * stride];
#pragma unroll
                for (int m = 0; m < WO; ++m) acc_mul_add(acc[m], x, w[(long long)j * WW + m]);
            }
#pragma unroll
            for (int m = 0; m < WO; ++m) r[m] = acc_reduce(acc[m]);
        } else {
            AccCols d[5];
#pragma unroll
            for (int m = 0; m < 5; ++m) acc_zero(d[m]);
            int j = 0;
            for (; j + 2 <= k; j += 2) {  // two columns per step, their six loads issued together
                u64 x[2][3];
#pragma unroll
                for (int u = 0; u < 2; ++u)
#pragma unroll
                    for (int p = 0; p < 3; ++p) x[u][p] = col[(long long)(j + u) * stride + p];
#pragma unroll
                for (int u = 0; u < 2; ++u)
#pragma unroll
                    for (int p = 0; p < 3; ++p)
#pragma unroll
                        for (int q = 0; q < 3; ++q) acc_mul_add(d[p + q], x[u][p], w[3ll * (j + u) + q]);
            }
            if (j < k) {
                const u64* c = col + (long long)j * stride;
                const u64 x[3] = {c[0], c[1], c[2]};
#pragma unroll
                for (int p = 0; p < 3; ++p)
#pragma unroll
                    for (int q = 0; q < 3; ++q) acc_mul_add(d[p + q], x[p], w[3ll * j + q]);
            }
            const u64 d3 = acc_reduce(d[3]), d4 = acc_reduce(d[4]);
            r[0] = gl::sub(acc_reduce(d[0]), d3);
            r[1] = gl::sub(gl::add(acc_reduce(d[1]), d3), d4);
            r[2] = gl::add(acc_reduce(d[2]), d4);
        }
#pragma unroll
        for (int m = 0; m < WO; ++m) out[i * WO + m] = r[m];
    }
}

}  // namespace tfk
