// deep_kernels.h -- the DEEP quotient: the codeword that FRI is run on, and the same value at sampled rows.
//
//     out[i] = sum_p ( sum_c w[p][c] * (T_c[i] - v[p][c]) ) / (x_i - z_p),    x_i = offset * w_n^i
//
// T_c: k1 BFieldElement columns ("main") followed by k3 XFieldElement columns ("aux"); z_p, w[p][c], v[p][c] XFieldElements, the
// weights and values point-major with the main columns first.  Words are canonical raw Montgomery words in and out.
//
// The numerator is regrouped as (sum_c w[p][c] T_c[i]) - C_p with C_p = sum_c w[p][c] v[p][c]: C_p is the same for every i and is
// formed once per call by deep_consts_kernel, the sum over the table is the weighted sum of poly_lincomb_kernel<3, 3>
// (algebra_kernels.h) with one change -- a BFieldElement column under an XFieldElement weight adds x * w[q] to coefficient q of the
// same five unreduced coefficients the XFieldElement columns use, so a point costs five AccCols whatever the mix of columns.  At
// most three terms enter a coefficient per column, so the counters stay below 2 * 3 * 65 535 < 2^19 for k1 + k3 <= 65 535: the
// bound acc_cols.h derives, now on the sum of both tables.
//
// Codeword kernel: the layout of batch_inverse_kernel (inverse_kernels.h).  A wave owns a chunk of 64 K consecutive elements, lane l
// the elements l + 64 j (j < K), so every load and store instruction of a wave touches 64 consecutive elements of one column.  Per
// element the lane walks all columns once for the NP points of the pass (four main columns, two aux columns per step, loads issued
// together), keeps the NP numerators, and then all 64 K NP denominators of the chunk are inverted with ONE inversion: running
// products per lane, inclusive prefix and suffix products over the wave (six shuffle steps each), inv_single, and back.  A zero
// denominator is replaced by ONE and flagged; the other elements of its wave keep their values.  x_i: the lane's first power of
// w_n from the table of w_n^(2^b) in the arguments, then steps of w_n^64 inside a chunk and of w_n^(64 K waves) from one chunk of
// a wave to its next.  Grid-stride over the chunks, one chunk per wave and step; the bound of that loop is the same for every lane
// of a wave, so the shuffles always run with the whole wave.
//
// Rows kernel: one wave per sampled row, lanes along the columns of the row-major row, the same accumulators on T_c - v[p][c], a
// butterfly sum over the wave and one inv_single per (row, point).
#pragma once

#include "acc_cols.h"         // AccCols, acc_mul_add, acc_reduce: the accumulators of algebra_kernels.h
#include "inverse_kernels.h"  // inv_mul, inv_single
#include "pt_elements.h"

#include <type_traits>
#include <utility>

namespace tfk {

constexpr int kDeepThreads = 256;
constexpr int kDeepWaves = kDeepThreads / 64;
constexpr int kDeepK = 4;                          // elements per lane
constexpr long long kDeepChunk = 64LL * kDeepK;    // elements per wave and step
constexpr int kDeepPassPoints = 2;                 // points per pass of the codeword kernel
constexpr int kDeepMaxPoints = 4;
constexpr int kDeepLogMax = 32;                    // n <= 2^32
constexpr long long kDeepGridCapChunks = 8192;     // chunks in flight: 2048 workgroups, eight per compute unit of 256

// one call, by value
struct DeepArgs {
    const u64* main;       // codeword form: column c at c * stride_main; rows form: row r at r * stride_main
    const u64* aux;
    long long k1, k3, stride_main, stride_aux;
    long long n;           // elements of the domain
    const u64* points;     // first point of this launch
    const u64* weights;    // its weights: (k1 + k3) XFieldElements per point
    const u64* values;     // rows form, and deep_consts_kernel
    const u64* consts;     // codeword form: C_p of this launch's points
    u64* out;
    int* status;
    const u32* indices;    // rows form
    long long n_rows;
    int n_points;          // rows form: all points
    int code_zero, code_index;
    u64 offset;
    u64 wstep;              // codeword form: w_n^(64 K waves of the launch), from one chunk of a wave to its next
    u64 wpow[kDeepLogMax];  // w_n^(2^b); ONE from b = log2 n on
};

// offset * w_n^e
__device__ __forceinline__ u64 deep_point(const DeepArgs& a, u64 e) {
    u64 x = a.offset;
#pragma unroll
    for (int b = 0; b < kDeepLogMax; ++b)
        if ((e >> b) & 1) x = gl::mont_mul(x, a.wpow[b]);
    return x;
}

// x - z for a lifted x; zero (only where `live`) is flagged and replaced by ONE, a dead slot is ONE
__device__ __forceinline__ bool deep_denominator(u64 x, const u64 (&z)[3], const u64 (&nz)[2], bool live, u64 (&d)[3]) {
    d[0] = gl::sub(x, z[0]), d[1] = nz[0], d[2] = nz[1];
    const bool zero = inv_is_zero<3>(d);
    if (zero || !live) inv_set_one<3>(d);
    return zero && live;
}

// x^3 = x - 1 on the five reduced coefficients (x_field_element.rs:512-536)
__device__ __forceinline__ void deep_reduce(const AccCols (&d)[5], u64 (&r)[3]) {
    const u64 d3 = acc_reduce(d[3]), d4 = acc_reduce(d[4]);
    r[0] = gl::sub(acc_reduce(d[0]), d3);
    r[1] = gl::sub(gl::add(acc_reduce(d[1]), d3), d4);
    r[2] = gl::add(acc_reduce(d[2]), d4);
}

// sum_c w[p][c] * T_c[i] for the NP points of the launch: every word of row i is loaded once
template <int NP>
__device__ __forceinline__ void deep_weighted_row(const DeepArgs& a, long long i, u64 (&r)[NP][3]) {
    const u64* __restrict__ w = a.weights;
    const long long k = a.k1 + a.k3;
    AccCols d[NP][5];
#pragma unroll
    for (int p = 0; p < NP; ++p)
#pragma unroll
        for (int m = 0; m < 5; ++m) acc_zero(d[p][m]);
    const u64* __restrict__ col = a.main + i;
    long long c = 0;
    for (; c + 4 <= a.k1; c += 4) {  // four columns per step, their loads issued together (poly_lincomb_kernel)
        u64 x[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) x[u] = col[(c + u) * a.stride_main];
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int p = 0; p < NP; ++p)
#pragma unroll
                for (int q = 0; q < 3; ++q) acc_mul_add(d[p][q], x[u], w[(p * k + c + u) * 3 + q]);
    }
    for (; c < a.k1; ++c) {
        const u64 x = col[c * a.stride_main];
#pragma unroll
        for (int p = 0; p < NP; ++p)
#pragma unroll
            for (int q = 0; q < 3; ++q) acc_mul_add(d[p][q], x, w[(p * k + c) * 3 + q]);
    }
    const u64* __restrict__ acol = a.aux + 3 * i;
    const u64* __restrict__ wa = w + 3 * a.k1;
    for (c = 0; c + 2 <= a.k3; c += 2) {  // two columns per step, their six loads issued together
        u64 x[2][3];
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int s = 0; s < 3; ++s) x[u][s] = acol[(c + u) * a.stride_aux + s];
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int p = 0; p < NP; ++p)
#pragma unroll
                for (int s = 0; s < 3; ++s)
#pragma unroll
                    for (int q = 0; q < 3; ++q) acc_mul_add(d[p][s + q], x[u][s], wa[(p * k + c + u) * 3 + q]);
    }
    if (c < a.k3) {
        const u64* t = acol + c * a.stride_aux;
        const u64 x[3] = {t[0], t[1], t[2]};
#pragma unroll
        for (int p = 0; p < NP; ++p)
#pragma unroll
            for (int s = 0; s < 3; ++s)
#pragma unroll
                for (int q = 0; q < 3; ++q) acc_mul_add(d[p][s + q], x[s], wa[(p * k + c) * 3 + q]);
    }
#pragma unroll
    for (int p = 0; p < NP; ++p) deep_reduce(d[p], r[p]);
}

// the inverse of this lane's total t, from ONE inversion of the product of the wave's 64 totals (batch_inverse_kernel's middle
// step); every total is non-zero.  Runs with the whole wave.
__device__ __forceinline__ void deep_wave_inverse(int lane, const u64 (&t)[3], u64 (&ti)[3]) {
    u64 pre[3], suf[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) pre[k] = suf[k] = t[k];
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        u64 up[3], dn[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            up[k] = __shfl_up(pre[k], d, 64);
            dn[k] = __shfl_down(suf[k], d, 64);
        }
        if (lane >= d) inv_mul<3>(up, pre, pre);
        if (lane + d < 64) inv_mul<3>(suf, dn, suf);
    }
    u64 w[3], wi[3], ex_pre[3], ex_suf[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        w[k] = __shfl(pre[k], 63, 64);
        ex_pre[k] = __shfl_up(pre[k], 1, 64);
        ex_suf[k] = __shfl_down(suf[k], 1, 64);
    }
    if (lane == 0) inv_set_one<3>(ex_pre);
    if (lane == 63) inv_set_one<3>(ex_suf);
    inv_single<3>(w, wi);
    inv_mul<3>(wi, ex_pre, ti);
    inv_mul<3>(ti, ex_suf, ti);
}

// consts[p] = C_p = sum_c weights[p][c] * values[p][c]: one workgroup per point
__global__ void __launch_bounds__(kDeepThreads) deep_consts_kernel(const u64* __restrict__ weights, const u64* __restrict__ values, long long k,
                                                                   u64* __restrict__ consts) {
    __shared__ u64 part[kDeepWaves][3];
    const long long p = blockIdx.x;
    u64 sum[3] = {0, 0, 0};
    for (long long c = threadIdx.x; c < k; c += kDeepThreads) {
        u64 w[3], v[3];
        pt_load<3>(weights, p * k + c, w);
        pt_load<3>(values, p * k + c, v);
        inv_mul<3>(w, v, w);
        pt_add<3>(sum, w, sum);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        u64 o[3];
#pragma unroll
        for (int m = 0; m < 3; ++m) o[m] = __shfl_xor(sum[m], d, 64);
        pt_add<3>(sum, o, sum);
    }
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int m = 0; m < 3; ++m) part[threadIdx.x >> 6][m] = sum[m];
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int wv = 1; wv < kDeepWaves; ++wv) {
            const u64 o[3] = {part[wv][0], part[wv][1], part[wv][2]};
            pt_add<3>(sum, o, sum);
        }
        pt_store<3>(consts, p, sum);
    }
}

// f(integral_constant<int, J>) for every J of the sequence, in order: the K elements of a lane are separate registers, and a loop
// over them that the compiler leaves rolled (it does, at this size, whatever the pragma says) would index them in scratch
template <int... J, class F>
__device__ __forceinline__ void deep_each(std::integer_sequence<int, J...>, F&& f) {
    (f(std::integral_constant<int, J>{}), ...);
}

// NP points of the call; ADD: a later pass, which adds its points' terms to what the passes before it stored
template <int NP, bool ADD>
__global__ void __launch_bounds__(kDeepThreads) deep_quotient_kernel(DeepArgs a) {
    constexpr int K = kDeepK;
    const int lane = threadIdx.x & 63;
    const long long waves = (long long)gridDim.x * kDeepWaves;
    const long long chunks = (a.n + kDeepChunk - 1) / kDeepChunk;
    u64 z[NP][3], nz[NP][2], cp[NP][3];
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        pt_load<3>(a.points, p, z[p]);
        pt_load<3>(a.consts, p, cp[p]);
        nz[p][0] = gl::neg(z[p][1]), nz[p][1] = gl::neg(z[p][2]);
    }
    const long long first = (long long)blockIdx.x * kDeepWaves + (threadIdx.x >> 6);
    const u64 w64 = a.wpow[6], wstep = a.wstep;
    u64 x0 = deep_point(a, (u64)(first * kDeepChunk + lane));  // (the table is read here only: it is not live in the loop)
    for (long long c = first; c < chunks; c += waves) {
        const long long base = c * kDeepChunk + lane;
        u64 xs[K], num[K][NP][3], s[K][NP][3], acc[3];
        unsigned zeros = 0;
        u64 x = x0;
        x0 = gl::mont_mul(x0, wstep);
        inv_set_one<3>(acc);
        deep_each(std::make_integer_sequence<int, K>{}, [&](auto J) {
            constexpr int j = decltype(J)::value;
            const long long i = base + 64LL * j;
            const bool live = i < a.n;
            xs[j] = x;
            x = gl::mont_mul(x, w64);
            if (live) {
                deep_weighted_row<NP>(a, i, num[j]);
#pragma unroll
                for (int p = 0; p < NP; ++p) pt_sub<3>(num[j][p], cp[p], num[j][p]);
            } else {
#pragma unroll
                for (int p = 0; p < NP; ++p) num[j][p][0] = num[j][p][1] = num[j][p][2] = 0;
            }
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                u64 d[3];
                if (deep_denominator(xs[j], z[p], nz[p], live, d)) zeros |= 1u << (j * NP + p);
#pragma unroll
                for (int m = 0; m < 3; ++m) s[j][p][m] = acc[m];
                inv_mul<3>(acc, d, acc);
            }
        });
        deep_wave_inverse(lane, acc, acc);
        deep_each(std::make_integer_sequence<int, K>{}, [&](auto J) {
            constexpr int j = K - 1 - decltype(J)::value;
            const long long i = base + 64LL * j;
            const bool live = i < a.n;
            u64 r[3] = {0, 0, 0};
#pragma unroll
            for (int p = NP - 1; p >= 0; --p) {
                u64 d[3], y[3];
                deep_denominator(xs[j], z[p], nz[p], live, d);
                inv_mul<3>(acc, s[j][p], y);
                inv_mul<3>(acc, d, acc);
                inv_mul<3>(num[j][p], y, y);
                pt_add<3>(r, y, r);
            }
            if (live) {
                if constexpr (ADD) {
                    u64 o[3];
                    pt_load<3>(a.out, i, o);
                    pt_add<3>(r, o, r);
                }
                pt_store<3>(a.out, i, r);
            }
        });
        if (__any(zeros != 0) && lane == 0) atomicCAS(a.status, 0, a.code_zero);
    }
}

// one wave per sampled row: out[r] = the quotient at index indices[r], from row r of the row-major main and aux rows
__global__ void __launch_bounds__(kDeepThreads) deep_quotient_rows_kernel(DeepArgs a) {
    const int lane = threadIdx.x & 63;
    const long long waves = (long long)gridDim.x * kDeepWaves;
    const long long k = a.k1 + a.k3;
    for (long long r = (long long)blockIdx.x * kDeepWaves + (threadIdx.x >> 6); r < a.n_rows; r += waves) {
        const u64 idx = a.indices[r];
        if (idx >= (u64)a.n) {  // (the same for every lane of the wave)
            if (lane == 0) atomicCAS(a.status, 0, a.code_index);
            continue;
        }
        const u64 x = deep_point(a, idx);
        const u64* __restrict__ mrow = a.main + r * a.stride_main;
        const u64* __restrict__ arow = a.aux + r * a.stride_aux;
        u64 res[3] = {0, 0, 0};
        bool zero = false;
        for (int p = 0; p < a.n_points; ++p) {
            const u64* __restrict__ w = a.weights + 3 * p * k;
            const u64* __restrict__ v = a.values + 3 * p * k;
            AccCols d[5];
#pragma unroll
            for (int m = 0; m < 5; ++m) acc_zero(d[m]);
            for (long long c = lane; c < a.k1; c += 64) {
                u64 wc[3], vc[3];
                pt_load<3>(w, c, wc);
                pt_load<3>(v, c, vc);
                const u64 t[3] = {gl::sub(mrow[c], vc[0]), gl::neg(vc[1]), gl::neg(vc[2])};
#pragma unroll
                for (int s = 0; s < 3; ++s)
#pragma unroll
                    for (int q = 0; q < 3; ++q) acc_mul_add(d[s + q], t[s], wc[q]);
            }
            for (long long c = lane; c < a.k3; c += 64) {
                u64 wc[3], vc[3], t[3];
                pt_load<3>(w, a.k1 + c, wc);
                pt_load<3>(v, a.k1 + c, vc);
                pt_load<3>(arow, c, t);
                pt_sub<3>(t, vc, t);
#pragma unroll
                for (int s = 0; s < 3; ++s)
#pragma unroll
                    for (int q = 0; q < 3; ++q) acc_mul_add(d[s + q], t[s], wc[q]);
            }
            u64 num[3];
            deep_reduce(d, num);
#pragma unroll
            for (int dd = 32; dd >= 1; dd >>= 1) {
                u64 o[3];
#pragma unroll
                for (int m = 0; m < 3; ++m) o[m] = __shfl_xor(num[m], dd, 64);
                pt_add<3>(num, o, num);
            }
            u64 zp[3], den[3], inv[3];
            pt_load<3>(a.points, p, zp);
            const u64 nz[2] = {gl::neg(zp[1]), gl::neg(zp[2])};
            zero |= deep_denominator(x, zp, nz, true, den);
            inv_single<3>(den, inv);
            inv_mul<3>(num, inv, num);
            pt_add<3>(res, num, res);
        }
        if (lane == 0) {
            pt_store<3>(a.out, r, res);
            if (zero) atomicCAS(a.status, 0, a.code_zero);
        }
    }
}

}  // namespace tfk
