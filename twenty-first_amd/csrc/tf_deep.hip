// tf_deep.hip -- the DEEP quotient of the extended tables at the out-of-domain points: the whole codeword FRI is run on, and the
// same value at sampled rows for the verifier.  Argument checks, the plan (chunk, points per pass, passes, launches), the work-space
// rule and the launchers over deep_kernels.h behind the entry points of include/tf_hip.h ("DEEP quotients" has the contract).
// Device pointers only: the unit takes no memory of its own -- the per-point constants live in the caller's work space, the
// descriptors travel as kernel arguments.
#include "tf_internal.h"
#include "deep_kernels.h"

namespace tfi {
namespace {

constexpr size_t kMaxLen = (size_t)1 << tfk::kDeepLogMax;
constexpr size_t kMaxColumns = 65535;            // the counter bound of the carry-deferred accumulators (algebra_kernels.h)
constexpr size_t kMaxRows = (size_t)1 << 30;
constexpr size_t kMaxSpan = (size_t)1 << 40;     // words from the first line of a table to its last: no offset wraps
constexpr int kPlanFields = 6;

int passes_of(size_t n_points) { return (int)((n_points + tfk::kDeepPassPoints - 1) / tfk::kDeepPassPoints); }
bool span_too_large(size_t lines, size_t stride) { return lines > 1 && stride > kMaxSpan / (lines - 1); }

// what (n, k1, k3, n_points) alone decide, for a call that is not empty, in the documented order
int check_shape(size_t n, size_t k1, size_t k3, size_t n_points) {
    if (n_points < 1 || n_points > (size_t)tfk::kDeepMaxPoints) return TF_ERR_INVALID_ARGUMENT;
    if (n & (n - 1)) return TF_ERR_LEN_NOT_POWER_OF_TWO;
    if (n > kMaxLen || k1 > kMaxColumns || k3 > kMaxColumns || k1 + k3 > kMaxColumns) return TF_ERR_LEN_TOO_LARGE;
    return TF_OK;
}

size_t workspace_of(size_t k1, size_t k3, size_t n_points) { return k1 + k3 ? n_points * 3 * sizeof(u64) : 0; }

void fill_domain(tfk::DeepArgs& a, size_t n, u64 offset_raw) {
    a.n = (long long)n, a.offset = offset_raw;
    a.wpow[0] = root_of_unity_mont(ilog2(n));
    for (int b = 1; b < tfk::kDeepLogMax; ++b) a.wpow[b] = gl::mont_mul(a.wpow[b - 1], a.wpow[b - 1]);
    a.code_zero = TF_ERR_INVERSE_OF_ZERO, a.code_index = TF_ERR_INVALID_ARGUMENT;
}

template <int NP>
void launch_pass(const tfk::DeepArgs& a, bool add, unsigned blocks, hipStream_t s) {
    if (add) hipLaunchKernelGGL((tfk::deep_quotient_kernel<NP, true>), dim3(blocks), dim3(tfk::kDeepThreads), 0, s, a);
    else hipLaunchKernelGGL((tfk::deep_quotient_kernel<NP, false>), dim3(blocks), dim3(tfk::kDeepThreads), 0, s, a);
}

}  // namespace

// In this order and before any HIP call: TF_OK for n == 0, TF_ERR_NULL_POINTER, TF_ERR_INVALID_ARGUMENT (n_points, a stride, a short
// work space), TF_ERR_LEN_NOT_POWER_OF_TWO, TF_ERR_LEN_TOO_LARGE, TF_ERR_INVERSE_OF_ZERO, then TF_ERR_NO_DEVICE.
int deep_quotient_dev(const u64* d_main, size_t k1, size_t stride_main, const u64* d_aux, size_t k3, size_t stride_aux, size_t n, u64 offset_raw,
                      const u64* d_points, size_t n_points, const u64* d_weights, const u64* d_values, u64* d_out, void* d_work, size_t work_bytes,
                      void* stream, int* d_status) {
    if (n == 0) return TF_OK;
    const bool any = k1 + k3 != 0;
    const size_t need = check_shape(n, k1, k3, n_points) ? 0 : workspace_of(k1, k3, n_points);
    if ((k1 && !d_main) || (k3 && !d_aux) || !d_points || (any && (!d_weights || !d_values)) || !d_out || !d_status || (need && !d_work))
        return TF_ERR_NULL_POINTER;
    if (n_points < 1 || n_points > (size_t)tfk::kDeepMaxPoints) return TF_ERR_INVALID_ARGUMENT;
    if ((k1 && stride_main < n) || (k3 && stride_aux / 3 < n)) return TF_ERR_INVALID_ARGUMENT;
    if (work_bytes < need) return TF_ERR_INVALID_ARGUMENT;
    TRY(check_shape(n, k1, k3, n_points));
    if (span_too_large(k1, stride_main) || span_too_large(k3, stride_aux)) return TF_ERR_LEN_TOO_LARGE;
    if (offset_raw == 0) return TF_ERR_INVERSE_OF_ZERO;
    DeviceCtx* ctx = nullptr;
    TRY(current_ctx(&ctx));
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (!any) {
        HIPCHK(hipMemsetAsync(d_out, 0, n * 3 * sizeof(u64), s));
        return TF_OK;
    }
    const size_t k = k1 + k3;
    u64* consts = static_cast<u64*>(d_work);
    hipLaunchKernelGGL(tfk::deep_consts_kernel, dim3((unsigned)n_points), dim3(tfk::kDeepThreads), 0, s, d_weights, d_values, (long long)k, consts);
    HIPCHK(hipGetLastError());
    tfk::DeepArgs a{};
    fill_domain(a, n, offset_raw);
    a.main = d_main, a.aux = d_aux, a.k1 = (long long)k1, a.k3 = (long long)k3;
    a.stride_main = (long long)stride_main, a.stride_aux = (long long)stride_aux;
    a.out = d_out, a.status = d_status;
    const size_t chunks = (n + (size_t)tfk::kDeepChunk - 1) / (size_t)tfk::kDeepChunk;
    const unsigned blocks = (unsigned)((std::min<size_t>(chunks, (size_t)tfk::kDeepGridCapChunks) + tfk::kDeepWaves - 1) / tfk::kDeepWaves);
    a.wstep = gl::mont_pow(a.wpow[0], ((u64)blocks * tfk::kDeepWaves * (u64)tfk::kDeepChunk) & (n - 1));
    for (size_t first = 0; first < n_points; first += tfk::kDeepPassPoints) {
        a.points = d_points + 3 * first, a.weights = d_weights + 3 * first * k, a.consts = consts + 3 * first;
        if (n_points - first >= 2) launch_pass<2>(a, first != 0, blocks, s);
        else launch_pass<1>(a, first != 0, blocks, s);
        HIPCHK(hipGetLastError());
    }
    return TF_OK;
}

size_t deep_quotient_workspace(size_t n, size_t k1, size_t k3, size_t n_points) {
    if (n == 0 || check_shape(n, k1, k3, n_points)) return 0;
    return workspace_of(k1, k3, n_points);
}

// fields: elements per wave and step, elements per lane, points per pass, passes, launches, the grid cap in chunks
int deep_quotient_plan(size_t n, size_t k1, size_t k3, size_t n_points, int* fields, int capacity) {
    if (n != 0) {
        const int rc = check_shape(n, k1, k3, n_points);
        if (rc) return -rc;
    } else if (n_points < 1 || n_points > (size_t)tfk::kDeepMaxPoints) {
        return -TF_ERR_INVALID_ARGUMENT;
    }
    const int passes = n == 0 ? 0 : k1 + k3 ? passes_of(n_points) : 1;  // (no column: one fill with zeros)
    const int launches = n == 0 ? 0 : k1 + k3 ? 1 + passes : 1;        // the constants, then the passes
    const int v[kPlanFields] = {(int)tfk::kDeepChunk, tfk::kDeepK, tfk::kDeepPassPoints, passes, launches, (int)tfk::kDeepGridCapChunks};
    for (int i = 0; i < kPlanFields && i < capacity && fields; ++i) fields[i] = v[i];
    return launches;
}

// The same order: TF_OK for n_rows == 0, TF_ERR_NULL_POINTER, TF_ERR_INVALID_ARGUMENT (n_points, a row stride), TF_ERR_LEN_NOT_POWER_OF_TWO
// (n, 0 included), TF_ERR_LEN_TOO_LARGE, TF_ERR_INVERSE_OF_ZERO, then TF_ERR_NO_DEVICE.
int deep_quotient_rows_dev(const u64* d_main_rows, size_t k1, size_t row_stride_main, const u64* d_aux_rows, size_t k3, size_t row_stride_aux, size_t n,
                           u64 offset_raw, const uint32_t* d_indices, size_t n_rows, const u64* d_points, size_t n_points, const u64* d_weights,
                           const u64* d_values, u64* d_out, void* stream, int* d_status) {
    if (n_rows == 0) return TF_OK;
    const bool any = k1 + k3 != 0;
    if ((k1 && !d_main_rows) || (k3 && !d_aux_rows) || !d_indices || !d_points || (any && (!d_weights || !d_values)) || !d_out || !d_status)
        return TF_ERR_NULL_POINTER;
    if (n_points < 1 || n_points > (size_t)tfk::kDeepMaxPoints) return TF_ERR_INVALID_ARGUMENT;
    if ((k1 && row_stride_main < k1) || (k3 && row_stride_aux / 3 < k3)) return TF_ERR_INVALID_ARGUMENT;
    if (n == 0) return TF_ERR_LEN_NOT_POWER_OF_TWO;
    TRY(check_shape(n, k1, k3, n_points));
    if (n_rows > kMaxRows || span_too_large(n_rows, row_stride_main) || span_too_large(n_rows, row_stride_aux)) return TF_ERR_LEN_TOO_LARGE;
    if (offset_raw == 0) return TF_ERR_INVERSE_OF_ZERO;
    DeviceCtx* ctx = nullptr;
    TRY(current_ctx(&ctx));
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (!any) {
        HIPCHK(hipMemsetAsync(d_out, 0, n_rows * 3 * sizeof(u64), s));
        return TF_OK;
    }
    tfk::DeepArgs a{};
    fill_domain(a, n, offset_raw);
    a.main = d_main_rows, a.aux = d_aux_rows, a.k1 = (long long)k1, a.k3 = (long long)k3;
    a.stride_main = (long long)row_stride_main, a.stride_aux = (long long)row_stride_aux;
    a.points = d_points, a.weights = d_weights, a.values = d_values, a.n_points = (int)n_points;
    a.indices = d_indices, a.n_rows = (long long)n_rows;
    a.out = d_out, a.status = d_status;
    const size_t blocks = std::min<size_t>((n_rows + tfk::kDeepWaves - 1) / tfk::kDeepWaves, (size_t)device_cus() * 8);
    hipLaunchKernelGGL(tfk::deep_quotient_rows_kernel, dim3((unsigned)blocks), dim3(tfk::kDeepThreads), 0, s, a);
    HIPCHK(hipGetLastError());
    return TF_OK;
}

}  // namespace tfi
