// tf_fri.hip -- the FRI split-and-fold of codewords over {g w_n^i} (Polynomial::get_colinear_y through (x_i, c[i]) and
// (-x_i, c[i + n/2]) at the challenge, math/polynomial.rs:386-394), one to many levels per call: argument checks, the plan of
// passes, the launcher over fri_kernels.h and the device / host flavours behind the entry points of include/tf_hip.h
// ("FRI folding" has the contract).
#include "tf_temp.h"
#include "fri_kernels.h"

namespace tfi {
namespace {

constexpr size_t kMaxLen = (size_t)1 << 30;
constexpr size_t kMaxWords = (size_t)1 << 35;
constexpr int T = tfk::kFriThreads;
constexpr int RMAX = tfk::kFriMaxLevels;

bool width_pair_ok(int wc, int wa) { return (wc == 1 && wa == 1) || (wc == 3 && wa == 3) || (wc == 1 && wa == 3); }

// the argument errors that depend on (n, levels, widths) alone, in the documented order
int check_shape(size_t n, size_t levels, int wc, int wa) {
    if (!width_pair_ok(wc, wa) || levels == 0) return TF_ERR_INVALID_ARGUMENT;
    if (n == 0 || (n & (n - 1))) return TF_ERR_LEN_NOT_POWER_OF_TWO;
    if (levels >= 64 || ((size_t)1 << levels) > n) return TF_ERR_INVALID_ARGUMENT;
    if (n > kMaxLen) return TF_ERR_LEN_TOO_LARGE;
    return TF_OK;
}

bool too_many_words(size_t n, size_t batch, int wc) { return batch > kMaxWords / (n * (size_t)wc); }

// RMAX levels per pass, the last pass takes the remainder
int passes_of(size_t levels) { return (int)((levels + RMAX - 1) / RMAX); }
int levels_of_pass(size_t levels, int pass) { return pass + 1 < passes_of(levels) ? RMAX : (int)(levels - (size_t)RMAX * pass); }
// words of the intermediate a pass leaves: batch codewords of n / 2^(levels folded so far) elements of wa words
size_t intermediate_words(size_t n, size_t batch, int wa, size_t levels, int pass) {
    int folded = 0;
    for (int p = 0; p <= pass; ++p) folded += levels_of_pass(levels, p);
    return batch * (n >> folded) * (size_t)wa;
}

template <int WC, int WA, int R>
int launch_pass_t(const u64* in, int log_m, long long total, const tfk::FriPoints& pts, const u64* alpha, long long alpha_stride, u64* out, hipStream_t s) {
    const long long cap = (long long)device_cus() * 8 * T;  // eight workgroups per compute unit at the most, as the point kernels
    int log_s = 8;
    while ((1ll << log_s) < total && (2ll << log_s) <= cap) ++log_s;
    const unsigned blocks = (unsigned)((std::min<long long>(total, 1ll << log_s) + T - 1) / T);
    hipLaunchKernelGGL((tfk::fri_fold_kernel<WC, WA, R>), dim3(blocks), dim3(T), 0, s, in, log_m, total, pts, log_s, alpha, alpha_stride, out);
    HIPCHK(hipGetLastError());
    return TF_OK;
}

template <int WC, int WA>
int launch_pass_r(int r, const u64* in, int log_m, long long total, const tfk::FriPoints& pts, const u64* alpha, long long alpha_stride, u64* out,
                  hipStream_t s) {
    if (r == 1) return launch_pass_t<WC, WA, 1>(in, log_m, total, pts, alpha, alpha_stride, out, s);
    if (r == 2) return launch_pass_t<WC, WA, 2>(in, log_m, total, pts, alpha, alpha_stride, out, s);
    if constexpr (RMAX >= 3)
        if (r == 3) return launch_pass_t<WC, WA, 3>(in, log_m, total, pts, alpha, alpha_stride, out, s);
    if constexpr (RMAX >= 4)
        if (r == 4) return launch_pass_t<WC, WA, 4>(in, log_m, total, pts, alpha, alpha_stride, out, s);
    return TF_ERR_INTERNAL;
}

// one pass: r levels of `batch` codewords of n elements of wc words over {offset w_n^i}, offset^-1 = g_inv
int launch_pass(int r, const u64* in, size_t n, size_t batch, int wc, u64 g_inv, const u64* alpha, long long alpha_stride, int wa, u64* out,
                hipStream_t s) {
    const int log_n = ilog2(n), log_m = log_n - r;
    tfk::FriPoints pts;
    pts.g_inv = g_inv;
    pts.w[0] = gl::mont_inverse(root_of_unity_mont(log_n));
    for (int j = 1; j < tfk::kFriTableLen; ++j) pts.w[j] = gl::mont_mul(pts.w[j - 1], pts.w[j - 1]);
    const long long total = (long long)batch << log_m;
    if (wa == 1) return launch_pass_r<1, 1>(r, in, log_m, total, pts, alpha, alpha_stride, out, s);
    if (wc == 1) return launch_pass_r<1, 3>(r, in, log_m, total, pts, alpha, alpha_stride, out, s);
    return launch_pass_r<3, 3>(r, in, log_m, total, pts, alpha, alpha_stride, out, s);
}

// device pointers, arguments checked: the passes of the plan, intermediates in two alternating temporaries on the caller's stream
int fold_dev(const u64* in, size_t n, size_t batch, int wc, u64 offset_raw, const u64* challenges, size_t levels, size_t n_sets, int wa, u64* out,
             hipStream_t s) {
    const int passes = passes_of(levels);
    DevTemp even(s), odd(s);  // what pass 0, 2, ... and pass 1, 3, ... leave; the last pass writes `out`
    if (passes >= 2 && even.alloc(intermediate_words(n, batch, wa, levels, 0), "fri_fold second-pass intermediate")) return TF_ERR_OUT_OF_MEMORY;
    if (passes >= 3 && odd.alloc(intermediate_words(n, batch, wa, levels, 1), "fri_fold third-pass intermediate")) return TF_ERR_OUT_OF_MEMORY;
    const long long alpha_stride = n_sets == 1 ? 0 : (long long)(levels * wa);
    u64 g_inv = gl::mont_inverse(offset_raw);
    const u64* src = in;
    int w = wc;
    size_t len = n, done = 0;
    for (int p = 0; p < passes; ++p) {
        const int r = levels_of_pass(levels, p);
        u64* dst = p + 1 == passes ? out : (p & 1) ? odd.p : even.p;
        TRY(launch_pass(r, src, len, batch, w, g_inv, challenges + done * wa, alpha_stride, wa, dst, s));
        for (int l = 0; l < r; ++l) g_inv = gl::mont_mul(g_inv, g_inv);
        src = dst, w = wa, len >>= r, done += r;
    }
    TRY(even.release());
    return odd.release();
}

}  // namespace

// In this order and before any HIP call: TF_OK for an empty call, TF_ERR_NULL_POINTER, TF_ERR_INVALID_ARGUMENT (widths, levels == 0,
// n_sets), TF_ERR_LEN_NOT_POWER_OF_TWO, TF_ERR_INVALID_ARGUMENT (2^levels > n), TF_ERR_LEN_TOO_LARGE, TF_ERR_INVERSE_OF_ZERO, then
// TF_ERR_NO_DEVICE.  host = true: host pointers (upload, run, download, wait).
int fri_fold(const u64* codewords, size_t n, size_t batch, int wc, u64 offset_raw, const u64* challenges, size_t levels, size_t n_sets, int wa, u64* out,
             bool host, void* stream) {
    if (batch == 0) return TF_OK;
    if (!codewords || !challenges || !out) return TF_ERR_NULL_POINTER;
    if (!width_pair_ok(wc, wa) || levels == 0 || (n_sets != 1 && n_sets != batch)) return TF_ERR_INVALID_ARGUMENT;
    TRY(check_shape(n, levels, wc, wa));
    if (too_many_words(n, batch, wc)) return TF_ERR_LEN_TOO_LARGE;
    if (offset_raw == 0) return TF_ERR_INVERSE_OF_ZERO;
    DeviceCtx* ctx = nullptr;
    TRY(current_ctx(&ctx));
    if (!host) return fold_dev(codewords, n, batch, wc, offset_raw, challenges, levels, n_sets, wa, out, static_cast<hipStream_t>(stream));
    return host_roundtrip(codewords, batch * n * wc, challenges, n_sets * levels * wa, out, batch * (n >> levels) * wa,
                          [&](u64* d_in, u64* d_ch, u64* d_out, hipStream_t s) {
                              return fold_dev(d_in, n, batch, wc, offset_raw, d_ch, levels, n_sets, wa, d_out, s);
                          });
}

size_t fri_fold_workspace(size_t n, size_t batch, int wc, int wa, size_t levels) {
    if (batch == 0 || check_shape(n, levels, wc, wa) || too_many_words(n, batch, wc)) return 0;
    const int passes = passes_of(levels);
    size_t words = 0;
    if (passes >= 2) words += intermediate_words(n, batch, wa, levels, 0);
    if (passes >= 3) words += intermediate_words(n, batch, wa, levels, 1);
    return words * sizeof(u64);
}

int fri_fold_plan(size_t n, size_t levels, int wc, int wa, int* levels_per_pass, int capacity) {
    const int rc = check_shape(n, levels, wc, wa);
    if (rc) return -rc;
    const int passes = passes_of(levels);
    for (int p = 0; p < passes && p < capacity && levels_per_pass; ++p) levels_per_pass[p] = levels_of_pass(levels, p);
    return passes;
}

}  // namespace tfi
