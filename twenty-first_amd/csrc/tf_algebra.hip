// tf_algebra.hip -- Add / Sub / Neg, scalar_mul, scale, formal_derivative, degree (math/polynomial.rs), the XFieldElement x
// BFieldElement pointwise product and the weighted sum of columns: argument checks, the launchers over algebra_kernels.h and the
// device / host flavours behind the entry points of include/tf_hip.h (which has the contract).
#include "tf_temp.h"
#include "algebra_kernels.h"

namespace tfi {
namespace {

constexpr size_t kMaxLen = (size_t)1 << 30;
constexpr size_t kMaxTerms = 65535;
constexpr int T = tfk::kAlgThreads;

bool width_ok(int w) { return w == 1 || w == 3; }

// blocks of a grid-stride launch over `items`: eight workgroups per compute unit at the most
unsigned blocks_for(long long items) {
    const long long cap = (long long)device_cus() * 8;
    return (unsigned)std::max<long long>(1, std::min<long long>((items + T - 1) / T, cap));
}
// the row dimension of a (blocks over the row, rows) grid; the kernels loop when there are more rows
unsigned rows_dim(size_t rows) { return (unsigned)std::min<size_t>(rows, 65535); }

tfk::AlgScalar scalar_of(const u64* s, int width) {
    tfk::AlgScalar r{{0, 0, 0}};
    for (int k = 0; k < width; ++k) r.v[k] = s[k];
    return r;
}

// ---------------------------------------------------------------------------------------------- launchers (device pointers, sizes checked)
int launch_addsub(const u64* a, size_t na, const u64* b, size_t nb, int w, u64* out, size_t batch, bool sub, hipStream_t s) {
    long long naw = (long long)(na * w), nbw = (long long)(nb * w), rows = (long long)batch;
    if (na == nb) naw *= rows, nbw *= rows, rows = 1;  // equal lengths: one flat array
    const dim3 grid(blocks_for(std::max(naw, nbw)), rows_dim((size_t)rows));
    if (sub)
        hipLaunchKernelGGL(tfk::poly_addsub_kernel<true>, grid, dim3(T), 0, s, a, naw, b, nbw, out, rows);
    else
        hipLaunchKernelGGL(tfk::poly_addsub_kernel<false>, grid, dim3(T), 0, s, a, naw, b, nbw, out, rows);
    HIPCHK(hipGetLastError());
    return TF_OK;
}

int launch_neg(const u64* a, u64* out, size_t words, hipStream_t s) {
    hipLaunchKernelGGL(tfk::poly_neg_kernel, dim3(blocks_for((long long)words)), dim3(T), 0, s, a, out, (long long)words);
    HIPCHK(hipGetLastError());
    return TF_OK;
}

int launch_scalar_mul(const u64* a, size_t count, int wa, tfk::AlgScalar sc, int ws, u64* out, hipStream_t s) {
    const long long n = (long long)count;
    if (ws == 1)
        hipLaunchKernelGGL(tfk::poly_scalar_mul_words_kernel<1>, dim3(blocks_for(n * wa)), dim3(T), 0, s, a, sc, out, n * wa);
    else if (wa == 1)
        hipLaunchKernelGGL(tfk::poly_scalar_mul_words_kernel<3>, dim3(blocks_for(n * 3)), dim3(T), 0, s, a, sc, out, n * 3);
    else
        hipLaunchKernelGGL(tfk::poly_scalar_mul_xx_kernel, dim3(blocks_for(n)), dim3(T), 0, s, a, sc, out, n);
    HIPCHK(hipGetLastError());
    return TF_OK;
}

// S = 2^log_s threads walk a row (algebra_kernels.h: poly_scale_kernel): the largest power of two, from 256 up to the launch cap,
// that still leaves every thread a run of at least ScaleRun coefficients; rows shorter than 256 runs get one workgroup
template <int WA, int WAL>
int launch_scale_t(const u64* a, size_t na, tfk::AlgScalar alpha, u64* out, size_t batch, hipStream_t s) {
    const long long cap = (long long)device_cus() * 8 * T;  // threads per row at the most
    int log_s = 8;
    while ((2ll << log_s) <= cap && (2ll << log_s) * tfk::ScaleRun<WAL>::value <= (long long)na) ++log_s;
    const dim3 grid((unsigned)((1ll << log_s) / T), rows_dim(batch));
    hipLaunchKernelGGL((tfk::poly_scale_kernel<WA, WAL>), grid, dim3(T), 0, s, a, (long long)na, alpha, out, (long long)batch, log_s);
    HIPCHK(hipGetLastError());
    return TF_OK;
}

int launch_scale(const u64* a, size_t na, int wa, tfk::AlgScalar alpha, int wal, u64* out, size_t batch, hipStream_t s) {
    if (wa == 1) return wal == 1 ? launch_scale_t<1, 1>(a, na, alpha, out, batch, s) : launch_scale_t<1, 3>(a, na, alpha, out, batch, s);
    return wal == 1 ? launch_scale_t<3, 1>(a, na, alpha, out, batch, s) : launch_scale_t<3, 3>(a, na, alpha, out, batch, s);
}

int launch_derivative(const u64* a, size_t na, int w, u64* out, size_t batch, hipStream_t s) {
    const dim3 grid(blocks_for((long long)((na - 1) * w)), rows_dim(batch));
    if (w == 1)
        hipLaunchKernelGGL(tfk::poly_derivative_kernel<1>, grid, dim3(T), 0, s, a, (long long)na, out, (long long)batch);
    else
        hipLaunchKernelGGL(tfk::poly_derivative_kernel<3>, grid, dim3(T), 0, s, a, (long long)na, out, (long long)batch);
    HIPCHK(hipGetLastError());
    return TF_OK;
}

// degrees <- -1 on the stream, then (na > 0) the scan from the top: 64 workgroups per row at the most
int launch_degree(const u64* a, size_t na, int w, size_t batch, long long* deg, hipStream_t s) {
    HIPCHK(hipMemsetAsync(deg, 0xFF, batch * sizeof(long long), s));
    if (na == 0) return TF_OK;
    const dim3 grid((unsigned)std::min<size_t>((na + T - 1) / T, 64), rows_dim(batch));
    if (w == 1)
        hipLaunchKernelGGL(tfk::poly_degree_kernel<1>, grid, dim3(T), 0, s, a, (long long)na, (long long)batch, deg);
    else
        hipLaunchKernelGGL(tfk::poly_degree_kernel<3>, grid, dim3(T), 0, s, a, (long long)na, (long long)batch, deg);
    HIPCHK(hipGetLastError());
    return TF_OK;
}

int launch_lincomb_t(const u64* polys, size_t n, int wp, size_t stride, size_t k, const u64* w, int ww, u64* out, hipStream_t s) {
    long long items = (long long)n;
    if (wp == 3 && ww == 1) items *= 3, wp = 1;  // BFieldElement weights: the limbs of a column are independent words
    const dim3 grid(blocks_for(items));
    if (wp == 1 && ww == 1)
        hipLaunchKernelGGL((tfk::poly_lincomb_kernel<1, 1>), grid, dim3(T), 0, s, polys, items, (long long)stride, (int)k, w, out);
    else if (wp == 1)
        hipLaunchKernelGGL((tfk::poly_lincomb_kernel<1, 3>), grid, dim3(T), 0, s, polys, items, (long long)stride, (int)k, w, out);
    else
        hipLaunchKernelGGL((tfk::poly_lincomb_kernel<3, 3>), grid, dim3(T), 0, s, polys, items, (long long)stride, (int)k, w, out);
    HIPCHK(hipGetLastError());
    return TF_OK;
}

int launch_lincomb(const u64* polys, size_t n, int wp, size_t stride, size_t k, const u64* w, int ww, u64* out, hipStream_t s) {
    if (k == 0) {  // the empty Sum (b_field_element.rs:214, x_field_element.rs:294)
        HIPCHK(hipMemsetAsync(out, 0, n * (size_t)std::max(wp, ww) * sizeof(u64), s));
        return TF_OK;
    }
    return launch_lincomb_t(polys, n, wp, stride, k, w, ww, out, s);
}

int need_device() {
    DeviceCtx* ctx = nullptr;
    return current_ctx(&ctx);
}

}  // namespace

// Every function below returns, in this order and before any HIP call: TF_OK for an empty call, TF_ERR_NULL_POINTER,
// TF_ERR_INVALID_ARGUMENT, TF_ERR_LEN_TOO_LARGE, then TF_ERR_NO_DEVICE.  host = true: host pointers (upload, run, download, wait).

int poly_addsub(const u64* a, size_t na, const u64* b, size_t nb, int width, u64* out, size_t batch, bool sub, bool host, void* stream) {
    const size_t nmax = std::max(na, nb);
    if (nmax == 0 || batch == 0) return TF_OK;
    if ((na && !a) || (nb && !b) || !out) return TF_ERR_NULL_POINTER;
    if (!width_ok(width)) return TF_ERR_INVALID_ARGUMENT;
    if (nmax > kMaxLen) return TF_ERR_LEN_TOO_LARGE;
    TRY(need_device());
    if (!host) return launch_addsub(a, na, b, nb, width, out, batch, sub, static_cast<hipStream_t>(stream));
    // (an empty operand is a null pointer on the device too, as the _dev form takes it: the kernel reads no word of it)
    return host_roundtrip(a, na * width * batch, b, nb * width * batch, out, nmax * width * batch,
                          [&](u64* da, u64* db, u64* dout, hipStream_t s) { return launch_addsub(da, na, db, nb, width, dout, batch, sub, s); });
}

int poly_neg(const u64* a, size_t na, int width, u64* out, size_t batch, bool host, void* stream) {
    if (na == 0 || batch == 0) return TF_OK;
    if (!a || !out) return TF_ERR_NULL_POINTER;
    if (!width_ok(width)) return TF_ERR_INVALID_ARGUMENT;
    if (na > kMaxLen) return TF_ERR_LEN_TOO_LARGE;
    TRY(need_device());
    const size_t words = na * width * batch;
    if (!host) return launch_neg(a, out, words, static_cast<hipStream_t>(stream));
    return host_roundtrip(a, words, nullptr, 0, out, words, [&](u64* da, u64*, u64* dout, hipStream_t s) { return launch_neg(da, dout, words, s); });
}

// scale = false: scalar_mul (every coefficient times `scalar`); scale = true: coefficient j times scalar^j
int poly_scalar_mul(const u64* a, size_t na, int width_a, const u64* scalar, int width_s, u64* out, size_t batch, bool scale, bool host, void* stream) {
    if (na == 0 || batch == 0) return TF_OK;
    if (!a || !scalar || !out) return TF_ERR_NULL_POINTER;
    if (!width_ok(width_a) || !width_ok(width_s)) return TF_ERR_INVALID_ARGUMENT;
    if (na > kMaxLen) return TF_ERR_LEN_TOO_LARGE;
    TRY(need_device());
    const tfk::AlgScalar sc = scalar_of(scalar, width_s);
    const int wo = std::max(width_a, width_s);
    auto run = [&](const u64* da, u64* dout, hipStream_t s) {
        return scale ? launch_scale(da, na, width_a, sc, width_s, dout, batch, s) : launch_scalar_mul(da, na * batch, width_a, sc, width_s, dout, s);
    };
    if (!host) return run(a, out, static_cast<hipStream_t>(stream));
    return host_roundtrip(a, na * width_a * batch, nullptr, 0, out, na * wo * batch, [&](u64* da, u64*, u64* dout, hipStream_t s) { return run(da, dout, s); });
}

int poly_derivative(const u64* a, size_t na, int width, u64* out, size_t batch, bool host, void* stream) {
    if (na <= 1 || batch == 0) return TF_OK;
    if (!a || !out) return TF_ERR_NULL_POINTER;
    if (!width_ok(width)) return TF_ERR_INVALID_ARGUMENT;
    if (na > kMaxLen) return TF_ERR_LEN_TOO_LARGE;
    TRY(need_device());
    if (!host) return launch_derivative(a, na, width, out, batch, static_cast<hipStream_t>(stream));
    return host_roundtrip(a, na * width * batch, nullptr, 0, out, (na - 1) * width * batch,
                          [&](u64* da, u64*, u64* dout, hipStream_t s) { return launch_derivative(da, na, width, dout, batch, s); });
}

int poly_degree(const u64* a, size_t na, int width, size_t batch, long long* degrees, bool host, void* stream) {
    if (batch == 0) return TF_OK;
    if ((na && !a) || !degrees) return TF_ERR_NULL_POINTER;
    if (!width_ok(width)) return TF_ERR_INVALID_ARGUMENT;
    if (na > kMaxLen) return TF_ERR_LEN_TOO_LARGE;
    if (host && na == 0) {  // the zero polynomial, by length alone
        std::fill(degrees, degrees + batch, -1ll);
        return TF_OK;
    }
    TRY(need_device());
    if (!host) return launch_degree(a, na, width, batch, degrees, static_cast<hipStream_t>(stream));
    return host_roundtrip(a, na * width * batch, nullptr, 0, reinterpret_cast<u64*>(degrees), batch, [&](u64* da, u64*, u64* ddeg, hipStream_t s) {
        return launch_degree(da, na, width, batch, reinterpret_cast<long long*>(ddeg), s);
    });
}

int hadamard_xfe_bfe_dev(const u64* a, const u64* b, u64* out, size_t count, void* stream) {
    if (count == 0) return TF_OK;
    if (!a || !b || !out) return TF_ERR_NULL_POINTER;
    TRY(need_device());
    const long long words = 3ll * (long long)count;
    hipLaunchKernelGGL(tfk::hadamard_xfe_bfe_kernel, dim3(blocks_for(words)), dim3(T), 0, static_cast<hipStream_t>(stream), a, b, out, words);
    HIPCHK(hipGetLastError());
    return TF_OK;
}

int poly_lincomb(const u64* polys, size_t n, int width_p, size_t stride, size_t k, const u64* weights, int width_w, u64* out, bool host, void* stream) {
    if (n == 0) return TF_OK;
    if ((k && (!polys || !weights)) || !out) return TF_ERR_NULL_POINTER;
    if (!width_ok(width_p) || !width_ok(width_w)) return TF_ERR_INVALID_ARGUMENT;
    if (stride / (size_t)width_p < n) return TF_ERR_INVALID_ARGUMENT;  // stride < n * width_p
    if (n > kMaxLen || k > kMaxTerms) return TF_ERR_LEN_TOO_LARGE;
    TRY(need_device());
    if (!host) return launch_lincomb(polys, n, width_p, stride, k, weights, width_w, out, static_cast<hipStream_t>(stream));
    hipStream_t s = host_stream();
    // the columns are packed on the way up (the words between n * width_p and stride are never read, on the host either)
    const size_t col = n * width_p, wp = k * col, ww = k * width_w, wo = n * std::max(width_p, width_w);
    DevTemp dp(s), dw(s), dout(s);  // (k = 0: no columns and no weights, two null pointers that launch_lincomb never passes on)
    TRY(dp.alloc(wp, "poly algebra"));
    TRY(dw.alloc(ww, "poly algebra"));
    TRY(dout.alloc(wo, "poly algebra"));
    if (k) {
        HIPCHK(hipMemcpy2DAsync(dp.p, col * sizeof(u64), polys, stride * sizeof(u64), col * sizeof(u64), k, hipMemcpyHostToDevice, s));
        TRY(sync(s));  // pageable host memory: the caller may reuse it when the call returns
    }
    TRY(h2d(dw.p, weights, ww, s));
    TRY(launch_lincomb(dp.p, n, width_p, col, k, dw.p, width_w, dout.p, s));
    TRY(d2h(out, dout.p, wo, s));
    return sync(s);
}

}  // namespace tfi
