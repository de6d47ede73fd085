// tf_table.hip -- tables between the library's two layouts: the strided transpose, the row gather from either layout and the
// low-degree extension of a row-major table (include/tf_hip.h, "Tables", has the contract; DESIGN 7.5 the tile).  Argument checks,
// the launchers over table_kernels.h and the device / host flavours behind the entry points.
#include "tf_temp.h"
#include "table_kernels.h"

namespace tfi {
namespace {

constexpr size_t kMaxLen = (size_t)1 << 30;
constexpr size_t kMaxWords = (size_t)1 << 35;             // words one call moves
constexpr size_t kMaxSpan = (size_t)1 << 40;              // words from an operand's first line to its last: 8 TiB, beyond any device
constexpr size_t kLdeBlockBytes = (size_t)256 << 20;      // table_lde_rows: a chosen bound on the two temporaries, not a measured optimum
constexpr int T = tfk::kTableThreads;

bool width_ok(int w) { return w == 1 || w == 3; }
long long block_cap() { return (long long)device_cus() * 8; }
// blocks of a grid-stride launch: eight workgroups per compute unit at the most (as blocks_for of tf_points.hip)
unsigned blocks_for(long long workgroups) { return (unsigned)std::max<long long>(1, std::min<long long>(workgroups, block_cap())); }

int need_device() {
    DeviceCtx* ctx = nullptr;
    return current_ctx(&ctx);
}

// batch * a * b * width > kMaxWords, for a, b <= kMaxLen and width <= 3 (so a * b * width cannot wrap)
bool too_many_words(size_t batch, size_t a, size_t b, int width) {
    const size_t per = a * b * (size_t)width;
    return per > kMaxWords || batch > kMaxWords / per;
}

// stride < elements * width, for any element count (the product may not be formed before the count is known to be small)
bool short_stride(size_t stride, size_t elements, int width) { return stride / (size_t)width < elements; }

// batch * lines * stride > kMaxSpan, whatever the three are: an absurd stride may not wrap span() or the kernels' 64-bit offsets
bool span_too_large(size_t batch, size_t lines, size_t stride) {
    if (!batch || !lines || !stride) return false;
    if (batch > kMaxSpan / lines) return true;
    return stride > kMaxSpan / (batch * lines);
}

// words from the first word of the first line to the last word of the last line
size_t span(size_t lines, size_t stride, size_t line_words) { return lines ? (lines - 1) * stride + line_words : 0; }

// ---------------------------------------------------------------------------------------------- launchers (device pointers, arguments checked)
template <int W>
int launch_transpose_t(const u64* src, size_t n_outer, size_t n_inner, size_t src_stride, u64* dst, size_t dst_stride, size_t batch, hipStream_t s) {
    constexpr long long TILE = tfk::TableTile<W>::TILE;
    const long long tiles = (((long long)n_outer + TILE - 1) / TILE) * (((long long)n_inner + TILE - 1) / TILE) * (long long)batch;
    hipLaunchKernelGGL(tfk::table_transpose_kernel<W>, dim3(blocks_for(tiles)), dim3(T), 0, s, src, (long long)n_outer, (long long)n_inner,
                       (long long)src_stride, dst, (long long)dst_stride, (long long)batch);
    HIPCHK(hipGetLastError());
    return TF_OK;
}

int launch_transpose(const u64* src, size_t n_outer, size_t n_inner, int w, size_t src_stride, u64* dst, size_t dst_stride, size_t batch, hipStream_t s) {
    if (!n_outer || !n_inner || !batch) return TF_OK;
    return w == 1 ? launch_transpose_t<1>(src, n_outer, n_inner, src_stride, dst, dst_stride, batch, s)
                  : launch_transpose_t<3>(src, n_outer, n_inner, src_stride, dst, dst_stride, batch, s);
}

int launch_gather_rows(const u64* table, int layout, size_t n_rows, size_t n_cols, int w, size_t stride, const uint32_t* indices, size_t k, u64* out,
                       size_t out_stride, size_t batch, int* status, hipStream_t s) {
    const long long words = (long long)(batch * k * n_cols * (size_t)w);
    hipLaunchKernelGGL(tfk::table_gather_rows_kernel, dim3(blocks_for((words + T - 1) / T)), dim3(T), 0, s, table, (int)(layout == TF_TABLE_ROW_MAJOR),
                       (long long)n_rows, (long long)n_cols, w, (long long)stride, indices, (long long)k, out, (long long)out_stride, (long long)batch, status,
                       (int)TF_ERR_INVALID_ARGUMENT);
    HIPCHK(hipGetLastError());
    return TF_OK;
}

// columns per block of table_lde_rows (0: the largest count whose two temporaries stay within kLdeBlockBytes, at least 1)
size_t lde_block_cols(size_t n, size_t m, size_t n_cols, int w, size_t cols_per_block) {
    if (cols_per_block) return std::min(cols_per_block, n_cols);
    const size_t per_col = (n + m) * (size_t)w * sizeof(u64);
    if (!per_col) return n_cols;  // (m == 0: nothing is taken)
    return std::max<size_t>(1, std::min(n_cols, kLdeBlockBytes / per_col));
}

// the argument errors of lde_dev (tf_poly.hip) in its order, then the table's own; *run = false for an empty call
int check_lde_rows(const u64* rows, size_t n, size_t n_cols, size_t rs_in, u64 offset_in, const u64* out, size_t m, size_t rs_out, int w, bool* run) {
    *run = false;
    if (n > m) return TF_ERR_ORDER_NOT_ABOVE_DEGREE;
    TRY(check_len(n));
    TRY(check_len(m));
    if (m == 0 || n_cols == 0) return TF_OK;
    if (!out || (n && !rows)) return TF_ERR_NULL_POINTER;
    if (n && offset_in == 0) return TF_ERR_INVERSE_OF_ZERO;
    if (n_cols > kMaxLen || too_many_words(1, n_cols, m, w)) return TF_ERR_LEN_TOO_LARGE;  // (m <= 2^31: the product cannot wrap)
    if ((n && rs_in < n_cols * (size_t)w) || rs_out < n_cols * (size_t)w) return TF_ERR_INVALID_ARGUMENT;
    if (span_too_large(1, n, rs_in) || span_too_large(1, m, rs_out)) return TF_ERR_LEN_TOO_LARGE;
    *run = true;
    return TF_OK;
}

}  // namespace

// Every function below returns, in this order and before any HIP call: TF_OK for an empty call, TF_ERR_NULL_POINTER,
// TF_ERR_INVALID_ARGUMENT, TF_ERR_LEN_TOO_LARGE, then TF_ERR_NO_DEVICE.  host = true: host pointers (upload, run, download, wait).

int table_transpose(const u64* src, size_t n_outer, size_t n_inner, int width, size_t src_stride, u64* dst, size_t dst_stride, size_t batch, bool host,
                    void* stream) {
    if (!n_outer || !n_inner || !batch) return TF_OK;
    if (!src || !dst) return TF_ERR_NULL_POINTER;
    if (!width_ok(width) || short_stride(src_stride, n_inner, width) || short_stride(dst_stride, n_outer, width)) return TF_ERR_INVALID_ARGUMENT;
    if (n_outer > kMaxLen || n_inner > kMaxLen || too_many_words(batch, n_outer, n_inner, width)) return TF_ERR_LEN_TOO_LARGE;
    if (span_too_large(batch, n_outer, src_stride) || span_too_large(batch, n_inner, dst_stride)) return TF_ERR_LEN_TOO_LARGE;
    TRY(need_device());
    if (!host) return launch_transpose(src, n_outer, n_inner, width, src_stride, dst, dst_stride, batch, static_cast<hipStream_t>(stream));
    // the source goes up as it lies (first line to last); the destination comes back packed and only its lines are written
    const size_t in_line = n_inner * (size_t)width, out_line = n_outer * (size_t)width, out_lines = batch * n_inner;
    std::vector<u64> packed(out_lines * out_line);
    TRY(host_roundtrip(src, span(batch * n_outer, src_stride, in_line), nullptr, 0, packed.data(), packed.size(),
                       [&](u64* d_src, u64*, u64* d_dst, hipStream_t s) { return launch_transpose(d_src, n_outer, n_inner, width, src_stride, d_dst, out_line, batch, s); }));
    for (size_t i = 0; i < out_lines; ++i) std::memcpy(dst + i * dst_stride, packed.data() + i * out_line, out_line * sizeof(u64));
    return TF_OK;
}

int table_gather_rows(const u64* table, int layout, size_t n_rows, size_t n_cols, int width, size_t stride, const uint32_t* indices, size_t k, u64* out,
                      size_t out_stride, size_t batch, bool host, void* stream, int* d_status) {
    if (!n_cols || !k || !batch) return TF_OK;
    if ((n_rows && !table) || !indices || !out || (!host && !d_status)) return TF_ERR_NULL_POINTER;
    if (!width_ok(width) || (layout != TF_TABLE_COLUMN_MAJOR && layout != TF_TABLE_ROW_MAJOR)) return TF_ERR_INVALID_ARGUMENT;
    if (short_stride(stride, layout == TF_TABLE_ROW_MAJOR ? n_cols : n_rows, width) || short_stride(out_stride, n_cols, width)) return TF_ERR_INVALID_ARGUMENT;
    if (n_rows > kMaxLen || n_cols > kMaxLen || k > kMaxLen || too_many_words(batch, k, n_cols, width)) return TF_ERR_LEN_TOO_LARGE;
    if (span_too_large(batch, layout == TF_TABLE_ROW_MAJOR ? n_rows : n_cols, stride) || span_too_large(batch, k, out_stride)) return TF_ERR_LEN_TOO_LARGE;
    const size_t line = n_cols * (size_t)width;
    TRY(need_device());
    if (!host)
        return launch_gather_rows(table, layout, n_rows, n_cols, width, stride, indices, k, out, out_stride, batch, d_status, static_cast<hipStream_t>(stream));
    hipStream_t s = host_stream();
    const bool row_major = layout == TF_TABLE_ROW_MAJOR;
    const size_t table_words = n_rows ? span(batch * (row_major ? n_rows : n_cols), stride, row_major ? line : n_rows * (size_t)width) : 0;
    DevTemp d_table(s), d_idx(s), d_out(s);  // d_out: the packed rows, then the flag word
    TRY(d_table.alloc(table_words, "table_gather_rows"));
    TRY(d_idx.alloc_bytes(k * sizeof(uint32_t), "table_gather_rows"));
    TRY(d_out.alloc(batch * k * line + 1, "table_gather_rows"));
    TRY(h2d(d_table.p, table, table_words, s));
    HIPCHK(hipMemcpyAsync(d_idx.p, indices, k * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));
    int* flag = reinterpret_cast<int*>(d_out.p + batch * k * line);
    HIPCHK(hipMemsetAsync(flag, 0, sizeof(int), s));
    TRY(launch_gather_rows(d_table.p, layout, n_rows, n_cols, width, stride, d_idx.as<uint32_t>(), k, d_out.p, line, batch, flag, s));
    std::vector<u64> packed(batch * k * line);
    int host_flag = 0;
    HIPCHK(hipMemcpyAsync(&host_flag, flag, sizeof(int), hipMemcpyDeviceToHost, s));
    TRY(d2h(packed.data(), d_out.p, packed.size(), s));
    TRY(sync(s));
    // (also after a raised status: the other rows are theirs; a bad index's row of out stays as it was)
    for (size_t r = 0; r < batch * k; ++r)
        if (indices[r % k] < n_rows) std::memcpy(out + r * out_stride, packed.data() + r * line, line * sizeof(u64));
    return host_flag ? TF_ERR_INVALID_ARGUMENT : TF_OK;
}

size_t table_lde_rows_workspace(size_t n, size_t m, size_t n_cols, int width, size_t cols_per_block) {
    if (!width_ok(width) || n > m || check_len(n) || check_len(m) || n_cols == 0 || n_cols > kMaxLen) return 0;
    if (m == 0 || too_many_words(1, n_cols, m, width)) return 0;  // an empty call takes nothing; more than 2^35 words are rejected
    return lde_block_cols(n, m, n_cols, width, cols_per_block) * (n + m) * (size_t)width * sizeof(u64);
}

// Blocks of c columns: transpose the block in (the strided transpose reads it out of the full rows), lde_dev with batch = c,
// transpose it out into the full rows of d_out.  One stream; the two column-major temporaries are taken once per call.
int table_lde_rows_dev(const u64* rows, size_t n, size_t n_cols, size_t row_stride_in, u64 offset_in, u64* out, size_t m, size_t row_stride_out,
                       u64 offset_out, size_t cols_per_block, int width, void* stream) {
    bool run = false;
    TRY(check_lde_rows(rows, n, n_cols, row_stride_in, offset_in, out, m, row_stride_out, width, &run));
    if (!run) return TF_OK;
    TRY(need_device());
    hipStream_t s = static_cast<hipStream_t>(stream);
    const size_t w = (size_t)width, c = lde_block_cols(n, m, n_cols, width, cols_per_block);
    DevTemp cols_in(s), cols_out(s);
    TRY(cols_in.alloc(c * n * w, "table_lde_rows"));
    TRY(cols_out.alloc(c * m * w, "table_lde_rows"));
    for (size_t j0 = 0; j0 < n_cols; j0 += c) {
        const size_t cb = std::min(c, n_cols - j0);
        TRY(launch_transpose(rows + j0 * w, n, cb, width, row_stride_in, cols_in.p, n * w, 1, s));
        TRY(lde_dev(cols_in.p, n, offset_in, cols_out.p, m, offset_out, cb, width, s));
        TRY(launch_transpose(cols_out.p, cb, m, width, m * w, out + j0 * w, row_stride_out, 1, s));
    }
    TRY(cols_in.release());
    return cols_out.release();
}

}  // namespace tfi
