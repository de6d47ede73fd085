// scan_kernels.h -- inclusive prefix scans along the columns of a column-major table of BFieldElements (W = 1) or XFieldElements
// (W = 3):  y_-1 = init,  y_i = a_i y_(i-1) + b_i,  out[i] = y_i.
//
// The algebra is the monoid of affine maps y -> A y + B: "first (A, B), then (A', B')" is (A' A, A' B + B'), identity (1, 0).  It is
// associative and not commutative, so every combination below keeps the order of the elements.  A sum carries B alone (A = 1), a
// product carries A alone (B = 0): the half a mode does not carry is never loaded, multiplied, shuffled or stored.
//
// A column is cut into tiles of T = 256 K elements; thread t of a 256-thread workgroup owns the K CONSECUTIVE elements
// [t K, (t + 1) K) of its tile (a scan needs the order, so the lanes cannot interleave as they do in batch_inverse_kernel), K = 16 for
// W = 1 and 8 for W = 3 (inverse_kernels.h: InvGeom).  Three launches in stream order, no workgroup ever waits for another:
//   scan_aggregate_kernel   one workgroup per (column, tile) but the column's last: each lane folds its K maps in registers, the wave
//                           folds the 64 lane totals by ordered shuffles, the four waves meet in LDS, one map per tile goes to `agg`
//   scan_spine_kernel       one workgroup per column: turns of S = 256 tile maps, scanned by shuffles and LDS, applied to the value
//                           carried in from the turn before (the column's init at first); the value at each tile's start goes to `start`
//   scan_apply_kernel       one workgroup per (column, tile): the tile is read whole into registers, the lane totals are scanned, every
//                           lane runs its K elements from the value at its own start and stores them.  All loads of a tile come
//                           before its first store, which is what makes out == b (or out == a for a product) safe.
// A column of at most T elements is one launch of scan_apply_kernel that starts from init; columns of at most 64 K elements run as
// one WAVE per column (scan_wave_kernel: no LDS, no barrier), so many short columns share workgroups.
// Every loop around a shuffle or a barrier has the same bound for all lanes of the wave / threads of the workgroup; what lies behind
// the end of a column is the identity (1, 0), never a shorter loop.  All element indices and offsets are 64-bit; the column index
// comes out of the linear block index (or a grid-stride loop), never out of gridDim.y.
#pragma once

#include "gl64.h"
#include "pt_elements.h"  // pt_add, inv_mul, inv_set_one

namespace tfk {

using gl::u64;

enum : int { kScanSum = 0, kScanProduct = 1, kScanAffine = 2 };  // TF_SCAN_SUM, TF_SCAN_PRODUCT, TF_SCAN_AFFINE

constexpr int kScanThreads = 256;
constexpr int kScanWaves = kScanThreads / 64;
constexpr int kScanSpineTurn = kScanThreads;  // S: tile maps per turn of the spine, one per thread

template <int W>
struct ScanGeom {
    static constexpr int K = InvGeom<W>::K;                       // elements per lane
    static constexpr long long WAVE = 64LL * K;                   // elements per wave
    static constexpr long long TILE = (long long)kScanThreads * K;  // T: elements per tile
};

// what a mode carries, in words per map
template <int MODE, int W>
struct ScanCarry {
    static constexpr bool A = MODE != kScanSum, B = MODE != kScanProduct;
    static constexpr int WORDS = (A ? W : 0) + (B ? W : 0);
};

// the kernels' arguments, by value.  Strides count words.  a_col / a_row: words from one column / one row of the multiplier to the
// next (a_row == 0: one multiplier for the whole column, a_col == 0: for every column); init == nullptr: the neutral start.
struct ScanArgs {
    const u64* a;
    const u64* b;
    const u64* init;
    u64* out;
    u64* agg;          // tiles x batch maps (the work space); the last tile of a column has none
    u64* start;        // tiles x batch values: y at each tile's start; nullptr: every tile starts from init (one tile per column)
    long long n, batch, tiles;
    long long a_col, a_row, stride_b, stride_out, init_col;
};

template <int W>
struct ScanMap {
    u64 a[W], b[W];
};

template <int MODE, int W>
__device__ __forceinline__ void scan_identity(ScanMap<W>& m) {
    if constexpr (ScanCarry<MODE, W>::A) inv_set_one<W>(m.a);
    if constexpr (ScanCarry<MODE, W>::B) {
#pragma unroll
        for (int k = 0; k < W; ++k) m.b[k] = 0;
    }
}

// r = "first f, then g" = (g.a f.a, g.a f.b + g.b); r may be f or g
template <int MODE, int W>
__device__ __forceinline__ void scan_then(const ScanMap<W>& f, const ScanMap<W>& g, ScanMap<W>& r) {
    if constexpr (MODE == kScanSum) {
        pt_add<W>(f.b, g.b, r.b);
    } else if constexpr (MODE == kScanProduct) {
        inv_mul<W>(g.a, f.a, r.a);
    } else {
        u64 t[W];
        inv_mul<W>(g.a, f.b, t);
        inv_mul<W>(g.a, f.a, r.a);
        pt_add<W>(t, g.b, r.b);
    }
}

// y = m(y) = m.a y + m.b
template <int MODE, int W>
__device__ __forceinline__ void scan_apply(const ScanMap<W>& m, u64 (&y)[W]) {
    if constexpr (ScanCarry<MODE, W>::A) inv_mul<W>(m.a, y, y);
    if constexpr (ScanCarry<MODE, W>::B) pt_add<W>(y, m.b, y);
}

template <int MODE, int W>
__device__ __forceinline__ void scan_shfl_up(const ScanMap<W>& m, int d, ScanMap<W>& r) {
#pragma unroll
    for (int k = 0; k < W; ++k) {
        if constexpr (ScanCarry<MODE, W>::A) r.a[k] = __shfl_up(m.a[k], d, 64);
        if constexpr (ScanCarry<MODE, W>::B) r.b[k] = __shfl_up(m.b[k], d, 64);
    }
}
template <int MODE, int W>
__device__ __forceinline__ void scan_shfl_down(const ScanMap<W>& m, int d, ScanMap<W>& r) {
#pragma unroll
    for (int k = 0; k < W; ++k) {
        if constexpr (ScanCarry<MODE, W>::A) r.a[k] = __shfl_down(m.a[k], d, 64);
        if constexpr (ScanCarry<MODE, W>::B) r.b[k] = __shfl_down(m.b[k], d, 64);
    }
}

// a map in memory: the words a mode carries, A first
template <int MODE, int W>
__device__ __forceinline__ void scan_map_store(u64* p, const ScanMap<W>& m) {
    int at = 0;
#pragma unroll
    for (int k = 0; k < W; ++k)
        if constexpr (ScanCarry<MODE, W>::A) p[at++] = m.a[k];
#pragma unroll
    for (int k = 0; k < W; ++k)
        if constexpr (ScanCarry<MODE, W>::B) p[at++] = m.b[k];
}
template <int MODE, int W>
__device__ __forceinline__ void scan_map_load(const u64* p, ScanMap<W>& m) {
    int at = 0;
#pragma unroll
    for (int k = 0; k < W; ++k)
        if constexpr (ScanCarry<MODE, W>::A) m.a[k] = p[at++];
#pragma unroll
    for (int k = 0; k < W; ++k)
        if constexpr (ScanCarry<MODE, W>::B) m.b[k] = p[at++];
}

// element i of column `col` as a map; i >= n is the identity.  WB < W: a BFieldElement column under an XFieldElement multiplier,
// read as its lift
template <int MODE, int W, int WB>
__device__ __forceinline__ void scan_load(const ScanArgs& s, long long col, long long i, ScanMap<W>& m) {
    scan_identity<MODE, W>(m);
    if (i >= s.n) return;
    if constexpr (ScanCarry<MODE, W>::A) {
        const u64* p = s.a + col * s.a_col + i * s.a_row;
#pragma unroll
        for (int k = 0; k < W; ++k) m.a[k] = p[k];
    }
    if constexpr (ScanCarry<MODE, W>::B) {
        const u64* p = s.b + col * s.stride_b + i * WB;
#pragma unroll
        for (int k = 0; k < WB; ++k) m.b[k] = p[k];
    }
}

// the column's start: init, or the neutral element (1 for a product, 0 otherwise)
template <int MODE, int W>
__device__ __forceinline__ void scan_init(const ScanArgs& s, long long col, u64 (&y)[W]) {
    if (s.init) {
#pragma unroll
        for (int k = 0; k < W; ++k) y[k] = s.init[col * s.init_col + k];
    } else {
#pragma unroll
        for (int k = 0; k < W; ++k) y[k] = 0;
        if constexpr (MODE == kScanProduct) y[0] = gl::ONE;
    }
}

// K consecutive elements from `first` on, and their fold in order
template <int MODE, int W, int WB>
__device__ __forceinline__ void scan_load_lane(const ScanArgs& s, long long col, long long first, ScanMap<W> (&e)[ScanGeom<W>::K], ScanMap<W>& total) {
    constexpr int K = ScanGeom<W>::K;
#pragma unroll
    for (int j = 0; j < K; ++j) scan_load<MODE, W, WB>(s, col, first + j, e[j]);
    total = e[0];
#pragma unroll
    for (int j = 1; j < K; ++j) scan_then<MODE, W>(total, e[j], total);
}

// inclusive scan of the lane totals over the wave, in lane order; `exc` is the map of the lanes before this one
template <int MODE, int W>
__device__ __forceinline__ void scan_wave_inclusive(int lane, ScanMap<W>& inc, ScanMap<W>& exc) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        ScanMap<W> up;
        scan_shfl_up<MODE, W>(inc, d, up);
        if (lane >= d) scan_then<MODE, W>(up, inc, inc);
    }
    scan_shfl_up<MODE, W>(inc, 1, exc);
    if (lane == 0) scan_identity<MODE, W>(exc);
}

// run the lane's K elements from y and store them
template <int MODE, int W>
__device__ __forceinline__ void scan_store_lane(const ScanArgs& s, long long col, long long first, const ScanMap<W> (&e)[ScanGeom<W>::K], u64 (&y)[W]) {
    constexpr int K = ScanGeom<W>::K;
    u64* o = s.out + col * s.stride_out;
#pragma unroll
    for (int j = 0; j < K; ++j) {
        scan_apply<MODE, W>(e[j], y);
        if (first + j < s.n) pt_store<W>(o, first + j, y);
    }
}

// one wave per column of at most 64 K elements; the waves walk the columns with a grid stride
template <int MODE, int W, int WB>
__global__ void __launch_bounds__(kScanThreads) scan_wave_kernel(ScanArgs s) {
    constexpr int K = ScanGeom<W>::K;
    const int lane = threadIdx.x & 63;
    const long long waves = (long long)gridDim.x * kScanWaves;
    for (long long col = (long long)blockIdx.x * kScanWaves + (threadIdx.x >> 6); col < s.batch; col += waves) {
        ScanMap<W> e[K], inc, exc;
        scan_load_lane<MODE, W, WB>(s, col, (long long)lane * K, e, inc);
        scan_wave_inclusive<MODE, W>(lane, inc, exc);
        u64 y[W];
        scan_init<MODE, W>(s, col, y);
        scan_apply<MODE, W>(exc, y);
        scan_store_lane<MODE, W>(s, col, (long long)lane * K, e, y);
    }
}

// the map of one tile: block = col * (tiles - 1) + tile, the last tile of a column is not needed
template <int MODE, int W, int WB>
__global__ void __launch_bounds__(kScanThreads) scan_aggregate_kernel(ScanArgs s) {
    constexpr int K = ScanGeom<W>::K;
    __shared__ ScanMap<W> totals[kScanWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long col = (long long)blockIdx.x / (s.tiles - 1), tile = (long long)blockIdx.x % (s.tiles - 1);
    ScanMap<W> e[K], total;
    scan_load_lane<MODE, W, WB>(s, col, tile * ScanGeom<W>::TILE + (long long)threadIdx.x * K, e, total);
    // ordered fold: lane l ends with the map of lanes l .. min(l + 2d - 1, 63); lane 0 with the wave's
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        ScanMap<W> dn;
        scan_shfl_down<MODE, W>(total, d, dn);
        if (lane + d < 64) scan_then<MODE, W>(total, dn, total);
    }
    if (lane == 0) totals[wave] = total;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < kScanWaves; ++w) scan_then<MODE, W>(total, totals[w], total);
        scan_map_store<MODE, W>(s.agg + (col * s.tiles + tile) * ScanCarry<MODE, W>::WORDS, total);
    }
}

// the value at every tile's start: one workgroup per column (grid stride), S tile maps per turn
template <int MODE, int W>
__global__ void __launch_bounds__(kScanThreads) scan_spine_kernel(ScanArgs s) {
    __shared__ ScanMap<W> totals[kScanWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (long long col = blockIdx.x; col < s.batch; col += gridDim.x) {
        u64 carry[W];
        scan_init<MODE, W>(s, col, carry);
        for (long long t0 = 0; t0 < s.tiles; t0 += kScanSpineTurn) {
            const long long tile = t0 + threadIdx.x;
            ScanMap<W> inc, exc;
            scan_identity<MODE, W>(inc);
            if (tile < s.tiles - 1) scan_map_load<MODE, W>(s.agg + (col * s.tiles + tile) * ScanCarry<MODE, W>::WORDS, inc);
            scan_wave_inclusive<MODE, W>(lane, inc, exc);
            if (lane == 63) totals[wave] = inc;
            __syncthreads();
            u64 y[W];
#pragma unroll
            for (int k = 0; k < W; ++k) y[k] = carry[k];
#pragma unroll
            for (int w = 0; w < kScanWaves; ++w) {
                if (w < wave) scan_apply<MODE, W>(totals[w], y);
                scan_apply<MODE, W>(totals[w], carry);
            }
            scan_apply<MODE, W>(exc, y);
            if (tile < s.tiles) pt_store<W>(s.start, col * s.tiles + tile, y);
            __syncthreads();  // totals is written again in the next turn
        }
    }
}

// one tile from the value at its start: block = col * tiles + tile
template <int MODE, int W, int WB>
__global__ void __launch_bounds__(kScanThreads) scan_apply_kernel(ScanArgs s) {
    constexpr int K = ScanGeom<W>::K;
    __shared__ ScanMap<W> totals[kScanWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long col = (long long)blockIdx.x / s.tiles, tile = (long long)blockIdx.x % s.tiles;
    const long long first = tile * ScanGeom<W>::TILE + (long long)threadIdx.x * K;
    ScanMap<W> e[K], inc, exc;
    scan_load_lane<MODE, W, WB>(s, col, first, e, inc);
    scan_wave_inclusive<MODE, W>(lane, inc, exc);
    if (lane == 63) totals[wave] = inc;
    u64 y[W];
    if (s.start) pt_load<W>(s.start, col * s.tiles + tile, y);
    else scan_init<MODE, W>(s, col, y);
    __syncthreads();
#pragma unroll
    for (int w = 0; w < kScanWaves - 1; ++w)
        if (w < wave) scan_apply<MODE, W>(totals[w], y);
    scan_apply<MODE, W>(exc, y);
    scan_store_lane<MODE, W>(s, col, first, e, y);
}

}  // namespace tfk
