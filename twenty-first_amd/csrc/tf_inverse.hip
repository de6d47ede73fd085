// tf_inverse.hip -- FiniteField::batch_inversion (math/traits.rs:93-121) and Inverse::inverse_or_zero (:39-45) over a vector of
// BFieldElements / XFieldElements: the launcher over inverse_kernels.h and the device / host flavours behind the entry points of
// include/tf_hip.h.
#include "tf_temp.h"
#include "inverse_kernels.h"

namespace tfi {
namespace {

// one wave per chunk of 64 K elements, four waves per block, grid-stride beyond eight blocks per compute unit
template <int L, bool OR_ZERO>
int launch_inverse(const u64* in, size_t n, u64* out, int* status, hipStream_t s) {
    const long long cap = (long long)device_cus() * 8;
    const long long chunks = ((long long)n + tfk::InvGeom<L>::CHUNK - 1) / tfk::InvGeom<L>::CHUNK;
    const long long blocks = std::min<long long>((chunks + 3) / 4, cap);
    hipLaunchKernelGGL((tfk::batch_inverse_kernel<L, OR_ZERO>), dim3((unsigned)blocks), dim3(256), 0, s, in, (long long)n, out, status,
                       (int)TF_ERR_INVERSE_OF_ZERO);
    HIPCHK(hipGetLastError());
    return TF_OK;
}

int launch(const u64* in, size_t n, u64* out, int L, bool or_zero, int* status, hipStream_t s) {
    if (L == 1) return or_zero ? launch_inverse<1, true>(in, n, out, status, s) : launch_inverse<1, false>(in, n, out, status, s);
    return or_zero ? launch_inverse<3, true>(in, n, out, status, s) : launch_inverse<3, false>(in, n, out, status, s);
}

// zero the flag word, run, copy the flag back and wait: TF_ERR_INVERSE_OF_ZERO when some element is zero (traits.rs:106)
int run_checked(const u64* in, size_t n, u64* out, int L, int* flag, hipStream_t s) {
    HIPCHK(hipMemsetAsync(flag, 0, sizeof(int), s));
    TRY(launch(in, n, out, L, false, flag, s));
    int host_flag = 0;
    HIPCHK(hipMemcpyAsync(&host_flag, flag, sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    return host_flag ? TF_ERR_INVERSE_OF_ZERO : TF_OK;
}

}  // namespace

// device pointers.  or_zero: inverse_or_zero, enqueue only.  batch_inversion with d_status (the _dev_async contract): enqueue only,
// a zero element writes TF_ERR_INVERSE_OF_ZERO to *d_status if it still holds 0; without d_status: a flag word of the pool is
// copied back, so the call blocks once.
int batch_inverse_dev(const u64* in, size_t n, u64* out, int L, bool or_zero, void* stream, int* d_status) {
    if (n == 0) return TF_OK;
    if (!in || !out) return TF_ERR_NULL_POINTER;
    DeviceCtx* ctx = nullptr;
    TRY(current_ctx(&ctx));
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (or_zero || d_status) return launch(in, n, out, L, or_zero, d_status, s);
    DevTemp flag(s);
    TRY(flag.alloc(1, "batch_inversion flag"));
    return run_checked(in, n, out, L, flag.as<int>(), s);
}

// host pointers: one upload, the inversion in place on the device, one download (in == out is fine)
int batch_inverse_host(const u64* in, size_t n, u64* out, int L, bool or_zero) {
    if (n == 0) return TF_OK;
    if (!in || !out) return TF_ERR_NULL_POINTER;
    DeviceCtx* ctx = nullptr;
    TRY(current_ctx(&ctx));
    hipStream_t s = host_stream();
    const size_t words = n * L;
    DevTemp d(s);  // the elements, then the flag word
    TRY(d.alloc(words + 1, "batch_inversion host buffer"));
    TRY(h2d(d.p, in, words, s));
    int rc = TF_OK;
    if (or_zero) {
        TRY(launch(d.p, n, d.p, L, true, nullptr, s));
    } else {
        rc = run_checked(d.p, n, d.p, L, reinterpret_cast<int*>(d.p + words), s);
        if (rc) return rc;  // (the output of a failed call is unspecified: nothing is copied)
    }
    TRY(d2h(out, d.p, words, s));
    TRY(sync(s));
    return rc;
}

}  // namespace tfi
