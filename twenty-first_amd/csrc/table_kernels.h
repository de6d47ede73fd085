// table_kernels.h -- moving a table between the two layouts the library uses (include/tf_hip.h, "Tables"):
//   table_transpose_kernel<W>   dst line i, element o = src line o, element i, for `batch` strided matrices of W-word elements
//   table_gather_rows_kernel    out row q of table t = row indices[q] of table t, from either layout
// No field arithmetic: words are moved as they are.  All global index arithmetic is 64-bit; offsets inside a tile are 32-bit.
#pragma once
#include <hip/hip_runtime.h>

#include "gl64.h"

namespace tfk {

using gl::u32;
using gl::u64;

constexpr int kTableThreads = 256;

// The tile of the transpose: TILE x TILE elements, staged in LDS as TILE source lines of TILE * W words at a pitch of PITCH words.
//   W = 1   64 x 64 elements = 4096 words per step, lines of 512 bytes on both sides, 64 * 65 * 8 = 33 280 bytes of LDS
//   W = 3   32 x 32 elements = 3072 words per step, lines of 768 bytes on both sides, 32 * 99 * 8 = 25 344 bytes of LDS
// (a 64 x 64 tile of XFieldElements would take 99 KiB and leave one workgroup per compute unit).  Both stay below the 16 384 words a
// workgroup may move per step (tests/fence.py sizes its guards by that).
//
// PITCH = TILE * W + W.  The tile is written along source lines and read along destination lines; a u64 is two banks wide.
//   write  ds_write_b64: groups of 16 consecutive lanes, bank = (a / 4) mod 32.  TILE * W is a multiple of 16, so a group stays
//          inside one source line and writes 16 consecutive words = 32 consecutive banks: conflict-free at any pitch.
//   read   ds_read_b64: groups of 32 consecutive lanes, bank = (a / 4) mod 64, i.e. word address mod 32.  Lane l of a group reads
//          word ow = 32 g + l of destination line i, which is element o = ow / W, word k = ow % W, at word address
//          o * PITCH + i * W + k.  TILE * W is a multiple of 32, so a group stays inside one destination line and PITCH = W (mod 32):
//          the address is W * o + k + i * W = ow + i * W (mod 32) -- 32 consecutive values, conflict-free.  At PITCH = TILE * W
//          every lane of a W = 1 group would sit on one bank pair (32-way).
template <int W>
struct TableTile {
    static constexpr int TILE = W == 1 ? 64 : 32;
    static constexpr int LINE = TILE * W;   // words of a full tile line, on either side
    static constexpr int PITCH = LINE + W;
    static constexpr int WORDS = TILE * LINE;
    static_assert(LINE % 32 == 0 && PITCH % 32 == W, "the bank arithmetic above");
    static_assert(WORDS % kTableThreads == 0 && WORDS <= 16384, "whole rounds of the workgroup, within the per-step bound");
};

// src: `batch` matrices of n_outer lines of n_inner elements, line o at src + o * src_stride, matrices n_outer * src_stride apart;
// dst: n_inner lines of n_outer elements at dst_stride, matrices n_inner * dst_stride apart.  One kernel serves both directions.
// A workgroup walks the (tile, matrix) pairs with a grid stride, the tile along n_outer -- the destination's contiguous axis --
// fastest.  Full tiles index with compile-time constants; ragged edge tiles pack their to x ti elements into the same rounds with
// run-time divisions (their bank pattern is whatever the extents give; they are the edge).  Words between a line's end and its
// stride are neither read nor written.
template <int W>
__global__ void __launch_bounds__(kTableThreads) table_transpose_kernel(const u64* __restrict__ src, long long n_outer, long long n_inner,
                                                                          long long src_stride, u64* __restrict__ dst, long long dst_stride,
                                                                          long long batch) {
    using G = TableTile<W>;
    constexpr int TILE = G::TILE, LINE = G::LINE, PITCH = G::PITCH, ROUNDS = G::WORDS / kTableThreads;
    __shared__ u64 tile[TILE * PITCH];
    const long long tiles_o = (n_outer + TILE - 1) / TILE, tiles_i = (n_inner + TILE - 1) / TILE;
    const long long per_matrix = tiles_o * tiles_i, total = per_matrix * batch;
    const int tid = threadIdx.x;
    for (long long t = blockIdx.x; t < total; t += gridDim.x) {
        const long long b = t / per_matrix, r = t - b * per_matrix;
        const long long ti_idx = r / tiles_o, to_idx = r - ti_idx * tiles_o;
        const long long o0 = to_idx * TILE, i0 = ti_idx * TILE;
        const int to = (int)(n_outer - o0 < TILE ? n_outer - o0 : TILE), ti = (int)(n_inner - i0 < TILE ? n_inner - i0 : TILE);
        const u64* s = src + (b * n_outer + o0) * src_stride + i0 * W;
        u64* d = dst + (b * n_inner + i0) * dst_stride + o0 * W;
        if (to == TILE && ti == TILE) {
            u64 v[ROUNDS];
#pragma unroll
            for (int j = 0; j < ROUNDS; ++j) {
                const int idx = j * kTableThreads + tid, o = idx / LINE, iw = idx % LINE;
                v[j] = s[(long long)o * src_stride + iw];
            }
#pragma unroll
            for (int j = 0; j < ROUNDS; ++j) {
                const int idx = j * kTableThreads + tid, o = idx / LINE, iw = idx % LINE;
                tile[o * PITCH + iw] = v[j];
            }
            __syncthreads();
#pragma unroll
            for (int j = 0; j < ROUNDS; ++j) {
                const int idx = j * kTableThreads + tid, i = idx / LINE, ow = idx % LINE, o = ow / W, k = ow % W;
                d[(long long)i * dst_stride + ow] = tile[o * PITCH + i * W + k];
            }
        } else {
            const u32 in_line = (u32)ti * W, out_line = (u32)to * W, words = (u32)to * in_line;
            for (u32 idx = tid; idx < words; idx += kTableThreads) {
                const u32 o = idx / in_line, iw = idx - o * in_line;
                tile[o * PITCH + iw] = s[(long long)o * src_stride + iw];
            }
            __syncthreads();
            for (u32 idx = tid; idx < words; idx += kTableThreads) {
                const u32 i = idx / out_line, ow = idx - i * out_line, o = ow / W, k = ow - o * W;
                d[(long long)i * dst_stride + ow] = tile[o * PITCH + i * W + k];
            }
        }
        __syncthreads();  // the tile is free for the next pair
    }
}

// out row q of table t (at out + (t * k + q) * out_stride, n_cols elements of `width` words) = row indices[q] of table t, run over
// the WORDS of the rows of out so that the stores of a wave are consecutive (as gather_elements_kernel, points_kernels.h).
//   row_major   a line copy: row i of table t is n_cols * width consecutive words at table + (t * n_rows + i) * stride
//   otherwise   one scattered element per output element: element j of row i at table + (t * n_cols + j) * stride + i * width
// An index >= n_rows is not read: it leaves its row of out as it was, in every table, and writes `code` to *status (the first
// non-zero code stays), once per bad row and table.
__global__ void __launch_bounds__(kTableThreads) table_gather_rows_kernel(const u64* __restrict__ table, int row_major, long long n_rows,
                                                                            long long n_cols, int width, long long stride,
                                                                            const u32* __restrict__ indices, long long k, u64* __restrict__ out,
                                                                            long long out_stride, long long batch, int* status, int code) {
    const long long line = n_cols * width, words = batch * k * line;
    const long long step = (long long)gridDim.x * kTableThreads;
    for (long long t = (long long)blockIdx.x * kTableThreads + threadIdx.x; t < words; t += step) {
        const long long row = t / line, e = t - row * line;  // row = tbl * k + q
        const long long tbl = row / k, q = row - tbl * k;
        const long long idx = (long long)indices[q];
        if (idx < n_rows) {
            long long from;
            if (row_major) {
                from = (tbl * n_rows + idx) * stride + e;
            } else {
                const long long j = e / width;
                from = (tbl * n_cols + j) * stride + idx * width + (e - j * width);
            }
            out[row * out_stride + e] = table[from];
        } else if (e == 0) {
            atomicCAS(status, 0, code);
        }
    }
}

}  // namespace tfk
