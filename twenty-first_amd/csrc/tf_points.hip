// tf_points.hip -- Polynomial::get_colinear_y / are_colinear (math/polynomial.rs:348-394), element-wise mod_pow, geometric
// sequences and index gathers over vectors that stay in device memory: argument checks, the launchers over points_kernels.h and
// the device / host flavours behind the entry points of include/tf_hip.h ("Points, powers and gathers" has the contract).
#include "tf_temp.h"
#include "points_kernels.h"

namespace tfi {
namespace {

constexpr size_t kMaxLen = (size_t)1 << 30;
constexpr size_t kMaxGroup = 1024;  // are_colinear: the uniqueness test is pairwise
constexpr int T = tfk::kPtThreads;
// are_colinear: groups of up to kLaneGroup points take one lane each, larger ones one wave each
constexpr size_t kLaneGroup = 16;
// mod_pow, broadcast base: elements per thread a workgroup should find before it pays for its table of squares
constexpr long long kTableItems = 4;

bool width_ok(int w) { return w == 1 || w == 3; }
bool width_pair_ok(int wx, int wy) { return (wx == 1 && wy == 1) || (wx == 3 && wy == 3) || (wx == 1 && wy == 3); }

long long block_cap() { return (long long)device_cus() * 8; }
// blocks of a grid-stride launch over `items` threads' worth of work: eight workgroups per compute unit at the most
unsigned blocks_for(long long items) { return (unsigned)std::max<long long>(1, std::min<long long>((items + T - 1) / T, block_cap())); }
// ... over `items` waves' worth of work (four waves per workgroup)
unsigned wave_blocks_for(long long items) { return (unsigned)std::max<long long>(1, std::min<long long>((items + 3) / 4, block_cap())); }

int need_device() {
    DeviceCtx* ctx = nullptr;
    return current_ctx(&ctx);
}

// ---------------------------------------------------------------------------------------------- launchers (device pointers, arguments checked)
template <int WX, int WY>
int launch_colinear_y_t(const u64* x0, const u64* y0, const u64* x1, const u64* y1, size_t n, const u64* p2x, bool each, u64* out, int* status,
                        hipStream_t s) {
    const long long chunks = ((long long)n + tfk::ColinearGeom<WX, WY>::CHUNK - 1) / tfk::ColinearGeom<WX, WY>::CHUNK;
    hipLaunchKernelGGL((tfk::get_colinear_y_kernel<WX, WY>), dim3(wave_blocks_for(chunks)), dim3(T), 0, s, x0, y0, x1, y1, (long long)n, p2x,
                       (int)each, out, status, (int)TF_ERR_INVERSE_OF_ZERO);
    HIPCHK(hipGetLastError());
    return TF_OK;
}

int launch_colinear_y(const u64* x0, const u64* y0, const u64* x1, const u64* y1, size_t n, const u64* p2x, bool each, int wx, int wy, u64* out,
                      int* status, hipStream_t s) {
    if (wy == 1) return launch_colinear_y_t<1, 1>(x0, y0, x1, y1, n, p2x, each, out, status, s);
    if (wx == 1) return launch_colinear_y_t<1, 3>(x0, y0, x1, y1, n, p2x, each, out, status, s);
    return launch_colinear_y_t<3, 3>(x0, y0, x1, y1, n, p2x, each, out, status, s);
}

template <int WX, int WY>
int launch_are_colinear_t(const u64* xs, const u64* ys, size_t n_groups, size_t k, int* flags, hipStream_t s) {
    const long long g = (long long)n_groups;
    if (k <= kLaneGroup)
        hipLaunchKernelGGL((tfk::are_colinear_lane_kernel<WX, WY>), dim3(blocks_for(g)), dim3(T), 0, s, xs, ys, g, (int)k, flags);
    else
        hipLaunchKernelGGL((tfk::are_colinear_wave_kernel<WX, WY>), dim3(wave_blocks_for(g)), dim3(T), 0, s, xs, ys, g, (int)k, flags);
    HIPCHK(hipGetLastError());
    return TF_OK;
}

int launch_are_colinear(const u64* xs, const u64* ys, size_t n_groups, size_t k, int wx, int wy, int* flags, hipStream_t s) {
    if (k < 3) {  // :349-351
        HIPCHK(hipMemsetAsync(flags, 0, n_groups * sizeof(int), s));
        return TF_OK;
    }
    if (wy == 1) return launch_are_colinear_t<1, 1>(xs, ys, n_groups, k, flags, s);
    if (wx == 1) return launch_are_colinear_t<1, 3>(xs, ys, n_groups, k, flags, s);
    return launch_are_colinear_t<3, 3>(xs, ys, n_groups, k, flags, s);
}

template <int W>
int launch_mod_pow_t(const u64* bases, bool base_each, const u64* exps, bool exp_each, u64* out, size_t n, hipStream_t s) {
    const long long count = (long long)n;
    if (base_each) {
        hipLaunchKernelGGL(tfk::mod_pow_kernel<W>, dim3(blocks_for(count)), dim3(T), 0, s, bases, exps, (int)exp_each, out, count);
    } else {
        const unsigned blocks = blocks_for((count + kTableItems - 1) / kTableItems);
        hipLaunchKernelGGL(tfk::mod_pow_table_kernel<W>, dim3(blocks), dim3(T), 0, s, bases, exps, (int)exp_each, out, count);
    }
    HIPCHK(hipGetLastError());
    return TF_OK;
}

int launch_mod_pow(const u64* bases, bool base_each, const u64* exps, bool exp_each, int w, u64* out, size_t n, hipStream_t s) {
    return w == 1 ? launch_mod_pow_t<1>(bases, base_each, exps, exp_each, out, n, s) : launch_mod_pow_t<3>(bases, base_each, exps, exp_each, out, n, s);
}

// r = a * b on the host, elements of w words (x_field_element.rs:512-536 with self = [c, b, a], other = [f, e, d]); r may be a or b
void host_mul(const u64* x, const u64* y, u64* r, int w) {
    if (w == 1) {
        r[0] = gl::mont_mul(x[0], y[0]);
        return;
    }
    const u64 c = x[0], b = x[1], a = x[2], f = y[0], e = y[1], d = y[2];
    const u64 ae = gl::mont_mul(a, e), bd = gl::mont_mul(b, d), ad = gl::mont_mul(a, d);
    const u64 r0 = gl::sub(gl::sub(gl::mont_mul(c, f), ae), bd);
    const u64 r1 = gl::add(gl::add(gl::sub(gl::add(gl::mont_mul(b, f), gl::mont_mul(c, e)), ad), ae), bd);
    const u64 r2 = gl::add(gl::add(gl::add(gl::mont_mul(a, f), gl::mont_mul(b, e)), gl::mont_mul(c, d)), ad);
    r[0] = r0, r[1] = r1, r[2] = r2;
}

// S = 2^log_s threads (points_kernels.h: powers_kernel): the power of two that covers n, from one workgroup up to the launch cap
int launch_powers(const u64* first, const u64* ratio, int w, u64* out, size_t n, hipStream_t s) {
    const long long cap = block_cap() * T;
    int log_s = 8;
    while ((1ll << log_s) < (long long)n && (2ll << log_s) <= cap) ++log_s;
    tfk::PtScalar f{{0, 0, 0}};
    tfk::PowersTable tab{};
    for (int k = 0; k < w; ++k) f.v[k] = first[k], tab.v[0][k] = ratio[k];
    for (int j = 1; j < tfk::kPowersTableLen; ++j) host_mul(tab.v[j - 1], tab.v[j - 1], tab.v[j], w);
    const dim3 grid((unsigned)((1ll << log_s) / T));
    if (w == 1)
        hipLaunchKernelGGL(tfk::powers_kernel<1>, grid, dim3(T), 0, s, f, tab, log_s, out, (long long)n);
    else
        hipLaunchKernelGGL(tfk::powers_kernel<3>, grid, dim3(T), 0, s, f, tab, log_s, out, (long long)n);
    HIPCHK(hipGetLastError());
    return TF_OK;
}

// host arrays -> one DevTemp each (waiting for each upload, see h2d)
struct Uploads {
    explicit Uploads(hipStream_t s) : s_(s) {}
    int put(const u64* host, size_t words, const u64** dev, const char* what) {
        bufs_.emplace_back(new DevTemp(s_));
        TRY(bufs_.back()->alloc(words, what));
        TRY(h2d(bufs_.back()->p, host, words, s_));
        *dev = bufs_.back()->p;
        return TF_OK;
    }
    hipStream_t s_;
    std::vector<std::unique_ptr<DevTemp>> bufs_;
};

}  // namespace

// Every function below returns, in this order and before any HIP call: TF_OK for an empty call, TF_ERR_NULL_POINTER,
// TF_ERR_INVALID_ARGUMENT, TF_ERR_LEN_TOO_LARGE, then TF_ERR_NO_DEVICE.  host = true: host pointers (upload, run, download, wait).

int get_colinear_y(const u64* x0, const u64* y0, const u64* x1, const u64* y1, size_t n, const u64* p2x, size_t n_p2x, int wx, int wy, u64* out,
                   bool host, void* stream, int* d_status) {
    if (n == 0) return TF_OK;
    if (!x0 || !y0 || !x1 || !y1 || !p2x || !out || (!host && !d_status)) return TF_ERR_NULL_POINTER;
    if (!width_pair_ok(wx, wy) || (n_p2x != 1 && n_p2x != n)) return TF_ERR_INVALID_ARGUMENT;
    if (n > kMaxLen) return TF_ERR_LEN_TOO_LARGE;
    TRY(need_device());
    const bool each = n_p2x == n && n != 1;
    if (!host) return launch_colinear_y(x0, y0, x1, y1, n, p2x, each, wx, wy, out, d_status, static_cast<hipStream_t>(stream));
    hipStream_t s = host_stream();
    Uploads up(s);
    const u64 *dx0, *dy0, *dx1, *dy1, *dp;
    TRY(up.put(x0, n * wx, &dx0, "get_colinear_y host buffers"));
    TRY(up.put(y0, n * wy, &dy0, "get_colinear_y host buffers"));
    TRY(up.put(x1, n * wx, &dx1, "get_colinear_y host buffers"));
    TRY(up.put(y1, n * wy, &dy1, "get_colinear_y host buffers"));
    TRY(up.put(p2x, n_p2x * wy, &dp, "get_colinear_y host buffers"));
    DevTemp dout(s);  // the quotients, then the flag word
    TRY(dout.alloc(n * wy + 1, "get_colinear_y host buffers"));
    int* flag = reinterpret_cast<int*>(dout.p + n * wy);
    HIPCHK(hipMemsetAsync(flag, 0, sizeof(int), s));
    TRY(launch_colinear_y(dx0, dy0, dx1, dy1, n, dp, each, wx, wy, dout.p, flag, s));
    int host_flag = 0;
    HIPCHK(hipMemcpyAsync(&host_flag, flag, sizeof(int), hipMemcpyDeviceToHost, s));
    TRY(d2h(out, dout.p, n * wy, s));  // (also after a raised status: the other triples' outputs are theirs)
    TRY(sync(s));
    return host_flag ? TF_ERR_INVERSE_OF_ZERO : TF_OK;
}

int are_colinear(const u64* xs, const u64* ys, size_t n_groups, size_t k, int wx, int wy, int* flags, bool host, void* stream) {
    if (n_groups == 0) return TF_OK;
    if (!flags || (k && (!xs || !ys))) return TF_ERR_NULL_POINTER;
    if (!width_pair_ok(wx, wy)) return TF_ERR_INVALID_ARGUMENT;
    if (k > kMaxGroup || n_groups > kMaxLen || n_groups * std::max<size_t>(k, 1) > kMaxLen) return TF_ERR_LEN_TOO_LARGE;
    if (host && k < 3) {  // :349-351, by the group size alone
        std::fill(flags, flags + n_groups, 0);
        return TF_OK;
    }
    TRY(need_device());
    if (!host) return launch_are_colinear(xs, ys, n_groups, k, wx, wy, flags, static_cast<hipStream_t>(stream));
    hipStream_t s = host_stream();
    Uploads up(s);
    const u64 *dxs, *dys;
    TRY(up.put(xs, n_groups * k * wx, &dxs, "are_colinear host buffers"));
    TRY(up.put(ys, n_groups * k * wy, &dys, "are_colinear host buffers"));
    DevTemp df(s);
    TRY(df.alloc_bytes(n_groups * sizeof(int), "are_colinear host buffers"));
    TRY(launch_are_colinear(dxs, dys, n_groups, k, wx, wy, df.as<int>(), s));
    HIPCHK(hipMemcpyAsync(flags, df.p, n_groups * sizeof(int), hipMemcpyDeviceToHost, s));
    return sync(s);
}

int mod_pow(const u64* bases, size_t n_bases, const uint64_t* exps, size_t n_exps, int width, u64* out, size_t n, bool host, void* stream) {
    if (n == 0) return TF_OK;
    if (!bases || !exps || !out) return TF_ERR_NULL_POINTER;
    if (!width_ok(width) || (n_bases != 1 && n_bases != n) || (n_exps != 1 && n_exps != n)) return TF_ERR_INVALID_ARGUMENT;
    if (n > kMaxLen) return TF_ERR_LEN_TOO_LARGE;
    TRY(need_device());
    const bool base_each = n_bases == n && n != 1, exp_each = n_exps == n && n != 1;
    if (!host) return launch_mod_pow(bases, base_each, exps, exp_each, width, out, n, static_cast<hipStream_t>(stream));
    hipStream_t s = host_stream();
    Uploads up(s);
    const u64 *db, *de;
    TRY(up.put(bases, n_bases * width, &db, "mod_pow host buffers"));
    TRY(up.put(exps, n_exps, &de, "mod_pow host buffers"));
    DevTemp dout(s);
    TRY(dout.alloc(n * width, "mod_pow host buffers"));
    TRY(launch_mod_pow(db, base_each, de, exp_each, width, dout.p, n, s));
    TRY(d2h(out, dout.p, n * width, s));
    return sync(s);
}

int powers(const u64* first, const u64* ratio, int width, u64* out, size_t n, bool host, void* stream) {
    if (n == 0) return TF_OK;
    if (!first || !ratio || !out) return TF_ERR_NULL_POINTER;
    if (!width_ok(width)) return TF_ERR_INVALID_ARGUMENT;
    if (n > kMaxLen) return TF_ERR_LEN_TOO_LARGE;
    TRY(need_device());
    if (!host) return launch_powers(first, ratio, width, out, n, static_cast<hipStream_t>(stream));
    hipStream_t s = host_stream();
    DevTemp dout(s);
    TRY(dout.alloc(n * width, "powers host buffer"));
    TRY(launch_powers(first, ratio, width, dout.p, n, s));
    TRY(d2h(out, dout.p, n * width, s));
    return sync(s);
}

int gather_elements_dev(const u64* src, size_t src_len, int width, const uint32_t* indices, size_t n, u64* out, void* stream, int* d_status) {
    if (n == 0) return TF_OK;
    if ((src_len && !src) || !indices || !out || !d_status) return TF_ERR_NULL_POINTER;
    if (width < 1 || width > 16) return TF_ERR_INVALID_ARGUMENT;
    if (n > kMaxLen || src_len > kMaxLen) return TF_ERR_LEN_TOO_LARGE;
    TRY(need_device());
    const long long words = (long long)n * width;
    hipLaunchKernelGGL(tfk::gather_elements_kernel, dim3(blocks_for(words)), dim3(T), 0, static_cast<hipStream_t>(stream), src, (long long)src_len, width,
                       indices, (long long)n, out, d_status, (int)TF_ERR_INVALID_ARGUMENT);
    HIPCHK(hipGetLastError());
    return TF_OK;
}

}  // namespace tfi
