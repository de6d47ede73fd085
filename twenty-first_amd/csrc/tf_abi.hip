// tf_abi.hip -- the C ABI of libtf_hip.so (include/tf_hip.h): host-pointer wrappers and the extern "C" entry points.
#include "tf_temp.h"
#include "aux_kernels.h"

#include <functional>
#include <utility>

namespace tfi {

// ------------------------------------------------------------------------------------ host-pointer wrappers
// Host buffers are pageable: the runtime stages such copies, and a staged H2D chunk was observed to land
// AFTER a kernel enqueued behind it on the same stream had already rewritten the destination in place.
// The host-pointer entry points therefore wait for the upload before enqueueing compute.
int h2d(u64* d, const u64* h, size_t words, hipStream_t s) {
    if (!words) return TF_OK;
    HIPCHK(hipMemcpyAsync(d, h, words * sizeof(u64), hipMemcpyHostToDevice, s));
    HIPCHK(hipStreamSynchronize(s));
    return TF_OK;
}

// One private non-blocking stream per (host thread, device) for the host-pointer entry points; destroyed with the thread
// (the workers of tf_*_multi are short-lived threads).
struct HostStreams {
    hipStream_t s[kMaxDevices] = {};
    ~HostStreams() {
        for (int d = 0; d < kMaxDevices; ++d)
            if (s[d]) (void)hipStreamDestroy(s[d]);
    }
};
hipStream_t host_stream() {
    thread_local HostStreams streams;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) return nullptr;
    if (!streams.s[dev]) {
        if (hipStreamCreateWithFlags(&streams.s[dev], hipStreamNonBlocking) != hipSuccess) {
            (void)hipGetLastError();
            streams.s[dev] = nullptr;
        }
    }
    return streams.s[dev];
}
int d2h(u64* h, const u64* d, size_t words, hipStream_t s) {
    if (!words) return TF_OK;
    HIPCHK(hipMemcpyAsync(h, d, words * sizeof(u64), hipMemcpyDeviceToHost, s));
    return TF_OK;
}
int sync(hipStream_t s) {
    HIPCHK(hipStreamSynchronize(s));
    return TF_OK;
}


int ntt_host(u64* x, size_t n, size_t batch, int L, int inverse) {
    TRY(check_len(n));
    if (n <= 1 || batch == 0) return TF_OK;
    if (!x) return TF_ERR_NULL_POINTER;
    return host_in_place(x, n * batch * L, nullptr, 0, [&](u64* d, u64*, hipStream_t s) { return ntt_dev(d, n, batch, L, inverse, s); });
}

int coset_eval_host(const u64* coeffs, size_t n_coeffs, u64 offset_raw, u64* out, size_t order, size_t batch, int L) {
    if (n_coeffs > order) return TF_ERR_ORDER_NOT_ABOVE_DEGREE;
    TRY(check_len(order));
    if (order == 0 || batch == 0) return TF_OK;
    if (!out || (n_coeffs && !coeffs)) return TF_ERR_NULL_POINTER;
    return host_roundtrip(coeffs, n_coeffs * batch * L, nullptr, 0, out, order * batch * L, [&](u64* c, u64*, u64* o, hipStream_t s) {
        return coset_eval_dev(c, n_coeffs, offset_raw, o, order, batch, L, s);
    });
}

// Host flavour of the inclusion-proof calls (tf_proof.hip): uploads the ranges the offsets use, runs the batch, copies the verdicts
// (and the paths) back.
int merkle_proofs_host(const uint32_t* heights, size_t n, const uint64_t* loff, const uint64_t* idx, const uint64_t* dig, const uint64_t* aoff,
                       const uint64_t* auth, const uint64_t* roots, int* statuses, uint64_t* paths_out, bool paths) {
    if (n == 0) return TF_OK;
    if (!heights || !loff || !aoff || !statuses) return TF_ERR_NULL_POINTER;
    size_t path_words = 0;
    for (size_t p = 0; p < n; ++p) {
        if (loff[p + 1] < loff[p] || aoff[p + 1] < aoff[p]) return TF_ERR_INVALID_ARGUMENT;
        if (heights[p] < 64) path_words += (loff[p + 1] - loff[p]) * heights[p];
    }
    const size_t nk = loff[n] - loff[0], na = aoff[n] - aoff[0];
    if ((nk && (!idx || !dig)) || (na && !auth) || (!paths && !roots) || (paths && path_words && !paths_out)) return TF_ERR_NULL_POINTER;
    DeviceCtx* ctx = nullptr;
    TRY(current_ctx(&ctx));
    hipStream_t s = host_stream();
    DevTemp di(s), dd(s), da(s), dr(s), dst(s), dp(s);
    TRY(di.alloc(nk, "merkle proofs host buffers"));
    TRY(dd.alloc(5 * nk, "merkle proofs host buffers"));
    TRY(da.alloc(5 * na, "merkle proofs host buffers"));
    TRY(dr.alloc(paths ? 0 : 5 * n, "merkle proofs host roots"));
    TRY(dst.alloc_bytes(n * sizeof(int), "merkle proofs host buffers"));
    TRY(dp.alloc(paths ? 5 * path_words : 0, "merkle proofs host paths"));
    if (nk) {
        TRY(h2d(di.p, idx + loff[0], nk, s));
        TRY(h2d(dd.p, dig + 5 * loff[0], 5 * nk, s));
    }
    if (na) TRY(h2d(da.p, auth + 5 * aoff[0], 5 * na, s));
    if (!paths) TRY(h2d(dr.p, roots, 5 * n, s));
    TRY(merkle_proofs_dev(heights, n, loff, di.p, dd.p, aoff, da.p, dr.p, reinterpret_cast<int*>(dst.p), dp.p, paths, loff[0], aoff[0], s));
    HIPCHK(hipMemcpyAsync(statuses, dst.p, n * sizeof(int), hipMemcpyDeviceToHost, s));
    if (paths) TRY(d2h(paths_out, dp.p, 5 * path_words, s));
    return sync(s);
}

// tf_debug_mul_pow2_dev: one kernel instantiation per exponent, picked from a table
template <int E>
void mul_pow2_launch(u64* d_x, size_t count, hipStream_t s) {
    const unsigned blocks = (unsigned)((count + 6 * 256 - 1) / (6 * 256));
    hipLaunchKernelGGL(tfk::mul_pow2_kernel<E>, dim3(blocks), dim3(256), 0, s, d_x, (unsigned long long)count);
}
template <int... E>
void mul_pow2_dispatch(int e, u64* d_x, size_t count, hipStream_t s, std::integer_sequence<int, E...>) {
    using Fn = void (*)(u64*, size_t, hipStream_t);
    static const Fn table[] = {&mul_pow2_launch<E>...};
    table[e](d_x, count, s);
}
}  // namespace tfi

using namespace tfi;


// ==================================================================================== C ABI
extern "C" {

const char* tf_status_string(int status) {
    switch (status) {
        case TF_OK: return "TF_OK";
        case TF_ERR_TOO_FEW_LEAFS: return "TF_ERR_TOO_FEW_LEAFS";
        case TF_ERR_INCORRECT_NUMBER_OF_LEAFS: return "TF_ERR_INCORRECT_NUMBER_OF_LEAFS";
        case TF_ERR_TREE_TOO_HIGH: return "TF_ERR_TREE_TOO_HIGH";
        case TF_ERR_LEN_NOT_POWER_OF_TWO: return "TF_ERR_LEN_NOT_POWER_OF_TWO";
        case TF_ERR_LEN_TOO_LARGE: return "TF_ERR_LEN_TOO_LARGE";
        case TF_ERR_ORDER_NOT_ABOVE_DEGREE: return "TF_ERR_ORDER_NOT_ABOVE_DEGREE";
        case TF_ERR_NULL_POINTER: return "TF_ERR_NULL_POINTER";
        case TF_ERR_NO_DEVICE: return "TF_ERR_NO_DEVICE";
        case TF_ERR_HIP: return "TF_ERR_HIP";
        case TF_ERR_OUT_OF_MEMORY: return "TF_ERR_OUT_OF_MEMORY";
        case TF_ERR_LEAF_INDEX_INVALID: return "TF_ERR_LEAF_INDEX_INVALID";
        case TF_ERR_INVERSE_OF_ZERO: return "TF_ERR_INVERSE_OF_ZERO";
        case TF_ERR_BUFFER_TOO_SMALL: return "TF_ERR_BUFFER_TOO_SMALL";
        case TF_ERR_EMPTY_DOMAIN: return "TF_ERR_EMPTY_DOMAIN";
        case TF_ERR_DIVISION_BY_ZERO: return "TF_ERR_DIVISION_BY_ZERO";
        case TF_ERR_DIVISION_NOT_CLEAN: return "TF_ERR_DIVISION_NOT_CLEAN";
        case TF_ERR_INVALID_ARGUMENT: return "TF_ERR_INVALID_ARGUMENT";
        case TF_ERR_INTERNAL: return "TF_ERR_INTERNAL";
        case TF_ERR_AUTH_STRUCTURE_LENGTH_MISMATCH: return "TF_ERR_AUTH_STRUCTURE_LENGTH_MISMATCH";
        case TF_ERR_REPEATED_LEAF_DIGEST_MISMATCH: return "TF_ERR_REPEATED_LEAF_DIGEST_MISMATCH";
        case TF_ERR_ROOT_MISMATCH: return "TF_ERR_ROOT_MISMATCH";
        case TF_ERR_MMR_LEAF_INDEX_OUT_OF_RANGE: return "TF_ERR_MMR_LEAF_INDEX_OUT_OF_RANGE";
        case TF_ERR_MMR_PEAK_COUNT_MISMATCH: return "TF_ERR_MMR_PEAK_COUNT_MISMATCH";
        case TF_ERR_MMR_AUTH_PATH_LENGTH_MISMATCH: return "TF_ERR_MMR_AUTH_PATH_LENGTH_MISMATCH";
        case TF_ERR_MMR_PEAK_MISMATCH: return "TF_ERR_MMR_PEAK_MISMATCH";
        case TF_ERR_UPPER_BOUND_NOT_POWER_OF_TWO: return "TF_ERR_UPPER_BOUND_NOT_POWER_OF_TWO";
        case TF_ERR_MMR_INCONSISTENT_OLD: return "TF_ERR_MMR_INCONSISTENT_OLD";
        case TF_ERR_MMR_INCONSISTENT_NEW: return "TF_ERR_MMR_INCONSISTENT_NEW";
        case TF_ERR_MMR_OLD_HAS_MORE_LEAFS: return "TF_ERR_MMR_OLD_HAS_MORE_LEAFS";
        case TF_ERR_MMR_SUCCESSOR_PATH_TOO_SHORT: return "TF_ERR_MMR_SUCCESSOR_PATH_TOO_SHORT";
        case TF_ERR_MMR_SUCCESSOR_PATH_TOO_LONG: return "TF_ERR_MMR_SUCCESSOR_PATH_TOO_LONG";
        case TF_ERR_MMR_DIFFERENT_SHARED_PEAK: return "TF_ERR_MMR_DIFFERENT_SHARED_PEAK";
        case TF_ERR_MMR_DIFFERENT_UNSHARED_PEAK: return "TF_ERR_MMR_DIFFERENT_UNSHARED_PEAK";
        default: return "TF_ERR_UNKNOWN";
    }
}

const char* tf_last_error(void) { return t_last_error.c_str(); }
int tf_version(void) { return 1002; }
#ifndef TF_SOURCE_HASH
#define TF_SOURCE_HASH "unknown"
#endif
const char* tf_source_hash(void) { return TF_SOURCE_HASH; }

int tf_release_caches(void) try {
    DeviceCtx* ctx = nullptr;
    const int rc = current_ctx(&ctx);
    if (rc) return rc;
    return release_caches(ctx);
} TF_ABI_CATCH

int tf_device_count(void) {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return count;
}

void tf_set_ntt_tile_bytes(size_t bytes) {
    read_env();
    g_tile_bytes = bytes ? bytes : (size_t(2048) << 20);
}
size_t tf_get_ntt_tile_bytes(void) {
    read_env();
    return g_tile_bytes;
}
void tf_set_batch_eval_route(int route) { g_batch_eval_route.store(route == 1 || route == 2 ? route : 0, std::memory_order_relaxed); }
void tf_set_ntt_pipe(int streams) {
    read_env();
    g_pipe.store(std::min(std::max(streams, 0), kMaxPipe), std::memory_order_relaxed);  // 0 = automatic
}
int tf_get_ntt_pipe(void) {
    read_env();
    return g_pipe.load(std::memory_order_relaxed);
}

// measurement helper (not part of the drop-in boundary): the shader clock the GPU is running at right now, from the ratio of
// the shader-cycle counter to the constant-rate wall clock over a ~0.5 ms spin of one wave.  bench.py records it next to its
// timings so that a run taken while the GPU sits in a low power state can be told from a slow kernel.
double tf_debug_sclk_mhz(void) {
    int dev = 0, wall_khz = 0;
    if (hipGetDevice(&dev) != hipSuccess) return -1.0;
    if (hipDeviceGetAttribute(&wall_khz, hipDeviceAttributeWallClockRate, dev) != hipSuccess || wall_khz <= 0) wall_khz = 100000;
    unsigned long long* d = nullptr;
    if (hipMalloc(reinterpret_cast<void**>(&d), 2 * sizeof(unsigned long long)) != hipSuccess) return -1.0;
    hipLaunchKernelGGL(tfk::sclk_probe_kernel, dim3(1), dim3(64), 0, hipStream_t(0), d);
    unsigned long long h[2] = {0, 0};
    const hipError_t e = hipMemcpy(h, d, sizeof(h), hipMemcpyDeviceToHost);
    (void)hipFree(d);
    if (e != hipSuccess || h[1] == 0) return -1.0;
    return (double)h[0] / (double)h[1] * (double)wall_khz / 1000.0;
}

// synthetic-input helper (not part of the drop-in boundary): d_out[i] = new(splitmix64(seed ^ (first_index + i)) mod p)
int tf_debug_fill_random_dev(uint64_t* d_out, size_t count, uint64_t seed, uint64_t first_index, void* stream) try {
    if (count == 0) return TF_OK;
    if (!d_out) return TF_ERR_NULL_POINTER;
    DeviceCtx* ctx = nullptr;
    int rc = current_ctx(&ctx);
    if (rc) return rc;
    const unsigned blocks = (unsigned)std::min<size_t>((count + 255) / 256, size_t(1) << 20);
    hipLaunchKernelGGL(tfk::fill_random_kernel, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream), d_out,
                       (unsigned long long)count, (u64)seed, (unsigned long long)first_index);
    HIPCHK(hipGetLastError());
    return TF_OK;
} TF_ABI_CATCH

// test helper (not part of the drop-in boundary): d_x[i] <- d_x[i] * 2^e mod p, one kernel instantiation per exponent
int tf_debug_mul_pow2_dev(uint64_t* d_x, size_t count, int e, void* stream) try {
    if (e < 0 || e >= 192 || count > (size_t(1) << 40)) return TF_ERR_INVALID_ARGUMENT;
    if (count == 0) return TF_OK;
    if (!d_x) return TF_ERR_NULL_POINTER;
    DeviceCtx* ctx = nullptr;
    int rc = current_ctx(&ctx);
    if (rc) return rc;
    mul_pow2_dispatch(e, reinterpret_cast<u64*>(d_x), count, static_cast<hipStream_t>(stream), std::make_integer_sequence<int, 192>{});
    HIPCHK(hipGetLastError());
    return TF_OK;
} TF_ABI_CATCH

// test helper (not part of the drop-in boundary): one hand-scheduled field primitive over count operand pairs
int tf_debug_field_op_dev(int op, const uint64_t* d_a, const uint64_t* d_b, uint64_t* d_out0, uint64_t* d_out1, size_t count, void* stream) try {
    if (op < 0 || op >= TF_FIELD_OP_COUNT || count > (size_t(1) << 32)) return TF_ERR_INVALID_ARGUMENT;
    if (count == 0) return TF_OK;
    if (!d_a || !d_out0 || (!d_b && op != TF_FIELD_OP_CANONICAL) || (!d_out1 && field_op_two_outputs(op))) return TF_ERR_NULL_POINTER;
    DeviceCtx* ctx = nullptr;
    int rc = current_ctx(&ctx);
    if (rc) return rc;
    debug_field_op_dev(op, d_a, d_b, d_out0, d_out1, count, static_cast<hipStream_t>(stream));
    HIPCHK(hipGetLastError());
    return TF_OK;
} TF_ABI_CATCH

// test helper (not part of the drop-in boundary): one composition of the NTT register networks over blocks of 32 (or 64) words
int tf_debug_ntt_network_dev(int form, uint64_t* d_x, size_t count, void* stream) try {
    if (form < 0 || form >= TF_NTT_NETWORK_FORM_COUNT || count > (size_t(1) << 32)) return TF_ERR_INVALID_ARGUMENT;
    if (count % (size_t)debug_ntt_network_words(form)) return TF_ERR_INVALID_ARGUMENT;
    if (count == 0) return TF_OK;
    if (!d_x) return TF_ERR_NULL_POINTER;
    DeviceCtx* ctx = nullptr;
    int rc = current_ctx(&ctx);
    if (rc) return rc;
    debug_ntt_network_dev(form, reinterpret_cast<u64*>(d_x), count, static_cast<hipStream_t>(stream));
    HIPCHK(hipGetLastError());
    return TF_OK;
} TF_ABI_CATCH

void tf_debug_ntt_network_config(int* lazy, int* asm_bfly, int* asm_pow2, int* pow2_wide) { debug_ntt_network_config(lazy, asm_bfly, asm_pow2, pow2_wide); }

// the guard mode for library-owned device memory (tf_temp_guard.hip)
int tf_debug_temp_guard(int mode) try {
    return temp_guard_set_mode(mode);
} TF_ABI_CATCH
int tf_debug_temp_guard_report(uint64_t* ledger, uint64_t* label_blocks, uint64_t* label_bytes, size_t capacity, size_t* n_labels) try {
    return temp_guard_report(ledger, label_blocks, label_bytes, capacity, n_labels);
} TF_ABI_CATCH
int tf_debug_temp_guard_reset(void) try {
    return temp_guard_reset();
} TF_ABI_CATCH
const char* tf_debug_temp_guard_label(size_t id) { return temp_guard_label(id); }
size_t tf_debug_temp_guard_words(void) { return TF_TEMP_GUARD_WORDS; }
int tf_debug_temp_guard_selftest(int defect, size_t n_words, uint64_t* out_word) try {
    return temp_guard_selftest(defect, n_words, out_word);
} TF_ABI_CATCH
int tf_debug_force_temp_tables(int on) try {
    return force_temp_tables(on);
} TF_ABI_CATCH

void tf_set_ntt_min_passes(int passes) { g_min_passes.store(passes, std::memory_order_relaxed); }
void tf_set_ntt_latency_kernel(int mode) { g_lat_mode.store(mode < 0 ? -1 : (mode ? 1 : 0), std::memory_order_relaxed); }
void tf_set_ntt_two_pass(int mode) { g_pre2_mode.store(mode < 0 ? -1 : (mode > 3 ? 1 : mode), std::memory_order_relaxed); }
void tf_set_ntt_small_launch(int mode) { g_small_launch_mode.store(mode < 0 ? -1 : (mode ? 1 : 0), std::memory_order_relaxed); }
// The plan of one transform: number of global passes and log2 of each pass's radix (planner introspection for the CPU tests).
// The route tf_poly_batch_evaluate_* takes for this shape: 1 Horner, 2 zerofier tree; 0 for a width that is not 1 / 3.  Host logic
// only (no device is touched), so the CPU tests pin the router.
int tf_batch_eval_plan(size_t n_coeffs, size_t n_points, size_t batch, int width) {
    if (width != 1 && width != 3) return 0;
    return tree_route(n_coeffs, n_points, batch, width) ? 2 : 1;
}
int tf_ntt_plan(size_t n, int width, int* log2_radix_out) {
    if (check_len(n) || n <= 1 || (width != 1 && width != 3) || !log2_radix_out) return 0;
    for (int i = 0; i < 4; ++i) log2_radix_out[i] = 0;
    // a plain transform in a call with enough work for the wide tiles (a real call with little work may take a latency-shaped route instead)
    const NttPlan plan = plan_ntt_large(n, width);
    if (plan.route != NttRoute::Passes) {  // one pass, or the whole transform per workgroup
        log2_radix_out[0] = ilog2(n);
        return 1;
    }
    for (int i = 0; i < plan.P; ++i) log2_radix_out[i] = plan.a[i];
    return plan.P;
}

int tf_ntt_launch_count(size_t n, size_t batch, int width) {
    if (check_len(n) || n <= 1 || batch == 0 || (width != 1 && width != 3)) return 0;
    NttShape s;  // a plain in-place call
    s.n = n, s.batch = batch, s.L = width;
    return plan_ntt(s).launches;
}

int tf_ntt_bfe(uint64_t* x, size_t n, size_t batch, int inverse) try { return ntt_host(x, n, batch, 1, inverse); } TF_ABI_CATCH
int tf_ntt_xfe(uint64_t* x, size_t n, size_t batch, int inverse) try { return ntt_host(x, n, batch, 3, inverse); } TF_ABI_CATCH
int tf_ntt_bfe_dev(uint64_t* d_x, size_t n, size_t batch, int inverse, void* stream) try {
    return ntt_dev(d_x, n, batch, 1, inverse, stream);
} TF_ABI_CATCH
int tf_ntt_xfe_dev(uint64_t* d_x, size_t n, size_t batch, int inverse, void* stream) try {
    return ntt_dev(d_x, n, batch, 3, inverse, stream);
} TF_ABI_CATCH

int tf_coset_eval_bfe(const uint64_t* c, size_t nc, uint64_t off, uint64_t* out, size_t order, size_t batch) try {
    return coset_eval_host(c, nc, off, out, order, batch, 1);
} TF_ABI_CATCH
int tf_coset_eval_xfe(const uint64_t* c, size_t nc, uint64_t off, uint64_t* out, size_t order, size_t batch) try {
    return coset_eval_host(c, nc, off, out, order, batch, 3);
} TF_ABI_CATCH
int tf_coset_eval_bfe_dev(const uint64_t* c, size_t nc, uint64_t off, uint64_t* out, size_t order, size_t batch,
                          void* stream) try {
    return coset_eval_dev(c, nc, off, out, order, batch, 1, stream);
} TF_ABI_CATCH
int tf_coset_eval_xfe_dev(const uint64_t* c, size_t nc, uint64_t off, uint64_t* out, size_t order, size_t batch,
                          void* stream) try {
    return coset_eval_dev(c, nc, off, out, order, batch, 3, stream);
} TF_ABI_CATCH

int tf_tip5_permute_dev(uint64_t* d_states, size_t count, void* stream) try { return tip5_permute_dev(d_states, count, stream); } TF_ABI_CATCH
int tf_tip5_hash_pairs_dev(const uint64_t* d_in, uint64_t* d_out, size_t count, void* stream) try {
    return tip5_hash_pairs_dev(d_in, d_out, count, stream);
} TF_ABI_CATCH
int tf_tip5_hash_varlen_rows_dev(const uint64_t* d_rows, size_t row_len, size_t n_rows, uint64_t* d_out, void* stream) try {
    return tip5_hash_varlen_rows_dev(d_rows, row_len, n_rows, d_out, stream);
} TF_ABI_CATCH
int tf_merkle_build_dev(const uint64_t* d_leaves, size_t n, uint64_t* d_nodes, size_t batch, void* stream) try {
    return merkle_build_dev(d_leaves, n, d_nodes, batch, stream);
} TF_ABI_CATCH
int tf_merkle_root_dev(const uint64_t* d_leaves, size_t n, uint64_t* d_root, size_t batch, void* stream) try {
    return merkle_root_dev(d_leaves, n, d_root, batch, stream);
} TF_ABI_CATCH

int tf_tip5_trace_dev(uint64_t* d_states, uint64_t* d_trace, size_t count, void* stream) try { return tip5_trace_dev(d_states, d_trace, count, stream); } TF_ABI_CATCH
int tf_tip5_trace(uint64_t* states, uint64_t* trace, size_t count) try {
    if (count == 0) return TF_OK;
    if (!states || !trace) return TF_ERR_NULL_POINTER;
    DeviceCtx* ctx = nullptr;
    TRY(current_ctx(&ctx));
    hipStream_t s = host_stream();
    DevTemp d(s), t(s);
    TRY(d.alloc(count * 16, "tip5_trace host buffers"));
    TRY(t.alloc(count * 96, "tip5_trace host buffers"));
    TRY(h2d(d.p, states, count * 16, s));
    TRY(tip5_trace_dev(d.p, t.p, count, s));
    TRY(d2h(states, d.p, count * 16, s));
    TRY(d2h(trace, t.p, count * 96, s));
    return sync(s);
} TF_ABI_CATCH
int tf_tip5_permute(uint64_t* states, size_t count) try {
    if (count == 0) return TF_OK;
    if (!states) return TF_ERR_NULL_POINTER;
    return host_in_place(states, count * 16, nullptr, 0, [&](u64* d, u64*, hipStream_t s) { return tip5_permute_dev(d, count, s); });
} TF_ABI_CATCH

int tf_tip5_hash_pairs(const uint64_t* in, uint64_t* out, size_t count) try {
    if (count == 0) return TF_OK;
    if (!in || !out) return TF_ERR_NULL_POINTER;
    return host_roundtrip(in, count * 10, nullptr, 0, out, count * 5, [&](u64* i, u64*, u64* o, hipStream_t s) { return tip5_hash_pairs_dev(i, o, count, s); });
} TF_ABI_CATCH

int tf_tip5_hash_varlen_rows(const uint64_t* rows, size_t row_len, size_t n_rows, uint64_t* out) try {
    if (n_rows == 0) return TF_OK;
    if (!out || (row_len && !rows)) return TF_ERR_NULL_POINTER;
    DeviceCtx* ctx = nullptr;
    TRY(current_ctx(&ctx));
    hipStream_t s = host_stream();
    DevTemp din(s), dout(s);
    TRY(din.alloc(std::max<size_t>(1, n_rows * row_len), "hash_varlen_rows host buffers"));
    TRY(dout.alloc(n_rows * 5, "hash_varlen_rows host buffers"));
    TRY(h2d(din.p, rows, n_rows * row_len, s));
    TRY(tip5_hash_varlen_rows_dev(din.p, row_len, n_rows, dout.p, s));
    TRY(d2h(out, dout.p, n_rows * 5, s));
    return sync(s);
} TF_ABI_CATCH

// ---- warm-up: one blocking call per shape, so that the *_dev calls of that shape never leave the stream ---------------------------
// The first call of a shape on a device builds its twiddle / power tables (hipMalloc + a build kernel the host waits for), opens the
// dynamic LDS of the kernels it launches (hipFuncSetAttribute), uploads the Tip5 constants, creates the library's memory pool, side
// streams and scratch blocks.  Some of those synchronise the whole DEVICE.  A caller that drives several GPUs from one host thread
// ("eight GPUs from one thread") calls tf_prepare_* once per device and shape at start-up; every later *_dev call of that
// shape only enqueues (tests/test_gpu_parity.py::test_one_host_thread_round_robin_never_blocks).  Implementation: the shape itself, once,
// on zeroed scratch of the same size (the plan -- passes, tile sizes, tables -- depends on n, batch and width, so nothing smaller is exact).
static int prepare_run(size_t in_words, size_t out_words, const std::function<int(u64*, u64*, hipStream_t)>& body) {
    DeviceCtx* ctx = nullptr;
    TRY(current_ctx(&ctx));
    hipStream_t s = host_stream();
    DevTemp a(s), b(s);
    if (a.alloc(in_words, "prepare buffers") || b.alloc(out_words, "prepare buffers")) return TF_ERR_OUT_OF_MEMORY;
    if (in_words) HIPCHK(hipMemsetAsync(a.p, 0, in_words * sizeof(u64), s));
    TRY(body(a.p, b.p, s));
    return sync(s);
}
int tf_prepare_ntt(size_t n, size_t batch, int width, int inverse) try {
    if (width != 1 && width != 3) return TF_ERR_INVALID_ARGUMENT;
    TRY(check_len(n));
    if (n <= 1 || batch == 0) return TF_OK;
    return prepare_run(n * batch * (size_t)width, 0, [=](u64* x, u64*, hipStream_t s) { return ntt_dev(x, n, batch, width, inverse, s); });
} TF_ABI_CATCH
int tf_prepare_coset_eval(size_t n_coeffs, uint64_t offset_raw, size_t order, size_t batch, int width) try {
    if (width != 1 && width != 3) return TF_ERR_INVALID_ARGUMENT;
    if (n_coeffs > order) return TF_ERR_ORDER_NOT_ABOVE_DEGREE;
    TRY(check_len(order));
    if (order == 0 || batch == 0) return TF_OK;
    return prepare_run(n_coeffs * batch * (size_t)width, order * batch * (size_t)width,
                       [=](u64* c, u64* o, hipStream_t s) { return coset_eval_dev(c, n_coeffs, offset_raw, o, order, batch, width, s); });
} TF_ABI_CATCH
int tf_prepare_merkle(size_t n_leaves, size_t batch) try {
    TRY(check_leaves(n_leaves));
    if (batch == 0) return TF_OK;
    return prepare_run(n_leaves * batch * 5, n_leaves * batch * 10, [=](u64* l, u64* nd, hipStream_t s) {
        TRY(merkle_build_dev(l, n_leaves, nd, batch, s));
        return merkle_root_dev(l, n_leaves, nd, batch, s);  // (the root-only route has kernels and scratch of its own)
    });
} TF_ABI_CATCH

int tf_merkle_build(const uint64_t* leaves, size_t n, uint64_t* nodes_out, size_t batch) try {
    TRY(check_leaves(n));
    if (batch == 0) return TF_OK;
    if (!leaves || !nodes_out) return TF_ERR_NULL_POINTER;
    return host_roundtrip(
        leaves, n * batch * 5, nullptr, 0, nodes_out, n * batch * 10, [&](u64* l, u64*, u64* o, hipStream_t s) { return merkle_build_dev(l, n, o, batch, s); },
        TF_ERR_TREE_TOO_HIGH, TF_ERR_TREE_TOO_HIGH);  // merkle_tree.rs:405-410
} TF_ABI_CATCH

}  // extern "C"  (closed for one internal helper of tf_multi.hip that needs this unit's host-pointer plumbing)
namespace tfi {
// ONE subtree of a host-resident tree on the calling thread's current device (tf_merkle_{build,root}_multi when there are more
// devices than trees): subtree `sub` of `n_sub` of a tree whose node array starts at nodes_tree (heap order, 2 n words-of-5; or null for
// a root-only build).  `leaves_sub` = its m = n / n_sub leaves.  Layer l of the subtree is the run [(n_sub + sub) 2^l, (n_sub + sub + 1) 2^l)
// of the whole tree's array -- the reference's own slicing, util_types/merkle_tree.rs:247-275 (subtrees_mut) -- so the D2H copies put every
// node where par_new would have written it; the subtree's root also goes to root_out (5 words).
int merkle_subtree_host(const u64* leaves_sub, size_t m, u64* nodes_tree, size_t n_sub, size_t sub, u64* root_out) {
    TRY(check_leaves(m));
    if (!leaves_sub || !root_out) return TF_ERR_NULL_POINTER;
    DeviceCtx* ctx = nullptr;
    TRY(current_ctx(&ctx));
    hipStream_t s = host_stream();
    DevTemp din(s), dout(s);
    if (din.alloc(m * 5, "merkle subtree host leafs")) return TF_ERR_TREE_TOO_HIGH;
    TRY(h2d(din.p, leaves_sub, m * 5, s));
    if (!nodes_tree) {
        TRY(dout.alloc(5, "merkle subtree host root"));
        TRY(merkle_root_dev(din.p, m, dout.p, 1, s));
        TRY(d2h(root_out, dout.p, 5, s));
        return sync(s);
    }
    if (dout.alloc(m * 10, "merkle subtree host nodes")) return TF_ERR_TREE_TOO_HIGH;
    TRY(merkle_build_dev(din.p, m, dout.p, 1, s));
    for (size_t l = 0; (size_t(1) << l) <= m; ++l) {
        const size_t w = size_t(1) << l;  // nodes of layer l: local heap indices [w, 2 w)
        TRY(d2h(nodes_tree + ((n_sub + sub) << l) * 5, dout.p + w * 5, w * 5, s));
    }
    TRY(d2h(root_out, dout.p + 5, 5, s));
    return sync(s);
}
}  // namespace tfi
extern "C" {

int tf_merkle_root(const uint64_t* leaves, size_t n, uint64_t* root_out, size_t batch) try {
    TRY(check_leaves(n));
    if (batch == 0) return TF_OK;
    if (!leaves || !root_out) return TF_ERR_NULL_POINTER;
    return host_roundtrip(
        leaves, n * batch * 5, nullptr, 0, root_out, batch * 5, [&](u64* l, u64*, u64* o, hipStream_t s) { return merkle_root_dev(l, n, o, batch, s); },
        TF_ERR_TREE_TOO_HIGH);
} TF_ABI_CATCH

// ---- SURVEY 8(f1)-(f3) ---------------------------------------------------------------------------
int tf_coset_interpolate_bfe_dev(const uint64_t* v, size_t n, uint64_t off, uint64_t* out, size_t batch, void* stream) try {
    return coset_interp_dev(v, n, off, out, batch, 1, stream);
} TF_ABI_CATCH
int tf_coset_interpolate_xfe_dev(const uint64_t* v, size_t n, uint64_t off, uint64_t* out, size_t batch, void* stream) try {
    return coset_interp_dev(v, n, off, out, batch, 3, stream);
} TF_ABI_CATCH
int tf_hadamard_bfe_dev(const uint64_t* a, const uint64_t* b, uint64_t* out, size_t count, void* stream) try {
    return hadamard_dev(a, b, out, count, 1, stream);
} TF_ABI_CATCH
int tf_hadamard_xfe_dev(const uint64_t* a, const uint64_t* b, uint64_t* out, size_t count, void* stream) try {
    return hadamard_dev(a, b, out, count, 3, stream);
} TF_ABI_CATCH
int tf_poly_mul_bfe_dev(const uint64_t* a, size_t na, const uint64_t* b, size_t nb, uint64_t* out, size_t batch, void* stream) try {
    return poly_mul_dev(a, na, b, nb, out, batch, 1, stream);
} TF_ABI_CATCH
int tf_poly_mul_xfe_dev(const uint64_t* a, size_t na, const uint64_t* b, size_t nb, uint64_t* out, size_t batch, void* stream) try {
    return poly_mul_dev(a, na, b, nb, out, batch, 3, stream);
} TF_ABI_CATCH
int tf_poly_square_bfe_dev(const uint64_t* a, size_t na, uint64_t* out, size_t batch, void* stream) try {
    return poly_square_dev(a, na, out, batch, 1, stream);
} TF_ABI_CATCH
int tf_poly_square_xfe_dev(const uint64_t* a, size_t na, uint64_t* out, size_t batch, void* stream) try {
    return poly_square_dev(a, na, out, batch, 3, stream);
} TF_ABI_CATCH
int tf_lde_bfe_dev(const uint64_t* v, size_t n, uint64_t off_in, uint64_t* out, size_t m, uint64_t off_out, size_t batch, void* stream) try {
    return lde_dev(v, n, off_in, out, m, off_out, batch, 1, stream);
} TF_ABI_CATCH
int tf_lde_xfe_dev(const uint64_t* v, size_t n, uint64_t off_in, uint64_t* out, size_t m, uint64_t off_out, size_t batch, void* stream) try {
    return lde_dev(v, n, off_in, out, m, off_out, batch, 3, stream);
} TF_ABI_CATCH
int tf_poly_batch_evaluate_bfe_dev(const uint64_t* c, size_t nc, const uint64_t* pts, size_t np, uint64_t* out, void* stream) try {
    return batch_evaluate_dev(c, nc, nc, 1, pts, np, out, 1, stream);
} TF_ABI_CATCH
int tf_poly_batch_evaluate_xfe_dev(const uint64_t* c, size_t nc, const uint64_t* pts, size_t np, uint64_t* out, void* stream) try {
    return batch_evaluate_dev(c, nc, 3 * nc, 1, pts, np, out, 3, stream);
} TF_ABI_CATCH
int tf_coset_extrapolate_bfe_dev(uint64_t offset, const uint64_t* cw, size_t n, size_t batch, const uint64_t* pts, size_t np,
                                 uint64_t* out, void* stream) try {
    return coset_extrapolate_dev(offset, cw, n, batch, pts, np, out, 1, stream);
} TF_ABI_CATCH
int tf_coset_extrapolate_xfe_dev(uint64_t offset, const uint64_t* cw, size_t n, size_t batch, const uint64_t* pts, size_t np,
                                 uint64_t* out, void* stream) try {
    return coset_extrapolate_dev(offset, cw, n, batch, pts, np, out, 3, stream);
} TF_ABI_CATCH
int tf_tip5_hash_table_rows_dev(const uint64_t* d_table, size_t n_rows, size_t n_cols, int width, size_t col_stride, uint64_t* d_digests,
                                size_t batch, void* stream) try {
    return hash_table_rows_dev(d_table, n_rows, n_cols, width, col_stride, d_digests, batch, stream);
} TF_ABI_CATCH
int tf_merkle_from_columns_dev(const uint64_t* d_table, size_t n_rows, size_t n_cols, int width, size_t col_stride, uint64_t* d_nodes,
                               size_t batch, void* stream) try {
    return merkle_from_columns_dev(d_table, n_rows, n_cols, width, col_stride, d_nodes, batch, stream);
} TF_ABI_CATCH
int tf_merkle_from_rows_dev(const uint64_t* d_rows, size_t row_len, size_t n_rows, uint64_t* d_nodes, size_t batch, void* stream) try {
    return merkle_from_rows_dev(d_rows, row_len, n_rows, d_nodes, batch, stream);
} TF_ABI_CATCH

int tf_coset_interpolate_bfe(const uint64_t* v, size_t n, uint64_t off, uint64_t* out, size_t batch) try {
    TRY(check_len(n));
    if (n == 0 || batch == 0) return TF_OK;
    if (!v || !out) return TF_ERR_NULL_POINTER;
    if (off == 0) return TF_ERR_INVERSE_OF_ZERO;
    return host_roundtrip(v, n * batch, nullptr, 0, out, n * batch,
                          [&](u64* a, u64*, u64* o, hipStream_t s) { return coset_interp_dev(a, n, off, o, batch, 1, s); });
} TF_ABI_CATCH
int tf_coset_interpolate_xfe(const uint64_t* v, size_t n, uint64_t off, uint64_t* out, size_t batch) try {
    TRY(check_len(n));
    if (n == 0 || batch == 0) return TF_OK;
    if (!v || !out) return TF_ERR_NULL_POINTER;
    if (off == 0) return TF_ERR_INVERSE_OF_ZERO;
    return host_roundtrip(v, 3 * n * batch, nullptr, 0, out, 3 * n * batch,
                          [&](u64* a, u64*, u64* o, hipStream_t s) { return coset_interp_dev(a, n, off, o, batch, 3, s); });
} TF_ABI_CATCH
int tf_poly_mul_bfe(const uint64_t* a, size_t na, const uint64_t* b, size_t nb, uint64_t* out, size_t batch) try {
    if (batch == 0 || na == 0 || nb == 0) return TF_OK;
    if (!a || !b || !out) return TF_ERR_NULL_POINTER;
    return host_roundtrip(a, na * batch, b, nb * batch, out, (na + nb - 1) * batch,
                          [&](u64* x, u64* y, u64* o, hipStream_t s) { return poly_mul_dev(x, na, y, nb, o, batch, 1, s); });
} TF_ABI_CATCH
int tf_poly_mul_xfe(const uint64_t* a, size_t na, const uint64_t* b, size_t nb, uint64_t* out, size_t batch) try {
    if (batch == 0 || na == 0 || nb == 0) return TF_OK;
    if (!a || !b || !out) return TF_ERR_NULL_POINTER;
    return host_roundtrip(a, 3 * na * batch, b, 3 * nb * batch, out, 3 * (na + nb - 1) * batch,
                          [&](u64* x, u64* y, u64* o, hipStream_t s) { return poly_mul_dev(x, na, y, nb, o, batch, 3, s); });
} TF_ABI_CATCH
int tf_poly_square_bfe(const uint64_t* a, size_t na, uint64_t* out, size_t batch) try {
    if (batch == 0 || na == 0) return TF_OK;
    if (!a || !out) return TF_ERR_NULL_POINTER;
    return host_roundtrip(a, na * batch, nullptr, 0, out, (2 * na - 1) * batch,
                          [&](u64* x, u64*, u64* o, hipStream_t s) { return poly_square_dev(x, na, o, batch, 1, s); });
} TF_ABI_CATCH
int tf_poly_square_xfe(const uint64_t* a, size_t na, uint64_t* out, size_t batch) try {
    if (batch == 0 || na == 0) return TF_OK;
    if (!a || !out) return TF_ERR_NULL_POINTER;
    return host_roundtrip(a, 3 * na * batch, nullptr, 0, out, 3 * (2 * na - 1) * batch,
                          [&](u64* x, u64*, u64* o, hipStream_t s) { return poly_square_dev(x, na, o, batch, 3, s); });
} TF_ABI_CATCH
int tf_poly_batch_evaluate_bfe(const uint64_t* c, size_t nc, const uint64_t* pts, size_t np, uint64_t* out) try {
    if (np == 0) return TF_OK;
    if (!pts || !out || (nc && !c)) return TF_ERR_NULL_POINTER;
    return host_roundtrip(c, nc, pts, np, out, np,
                          [&](u64* dc, u64* dp, u64* o, hipStream_t s) { return batch_evaluate_dev(dc, nc, nc, 1, dp, np, o, 1, s); });
} TF_ABI_CATCH
int tf_poly_batch_evaluate_xfe(const uint64_t* c, size_t nc, const uint64_t* pts, size_t np, uint64_t* out) try {
    if (np == 0) return TF_OK;
    if (!pts || !out || (nc && !c)) return TF_ERR_NULL_POINTER;
    return host_roundtrip(c, 3 * nc, pts, 3 * np, out, 3 * np,
                          [&](u64* dc, u64* dp, u64* o, hipStream_t s) { return batch_evaluate_dev(dc, nc, 3 * nc, 1, dp, np, o, 3, s); });
} TF_ABI_CATCH
int tf_poly_zerofier_bfe_dev(const uint64_t* r, size_t n, uint64_t* out, void* stream) try { return zerofier_dev(r, n, out, 1, stream); } TF_ABI_CATCH
int tf_poly_zerofier_xfe_dev(const uint64_t* r, size_t n, uint64_t* out, void* stream) try { return zerofier_dev(r, n, out, 3, stream); } TF_ABI_CATCH
static int zerofier_host(const uint64_t* r, size_t n, uint64_t* out, int L) {
    if (!out || (n && !r)) return TF_ERR_NULL_POINTER;
    return host_roundtrip(r, n * L, nullptr, 0, out, (n + 1) * L, [&](u64* dr, u64*, u64* o, hipStream_t s) { return zerofier_dev(dr, n, o, L, s); });
}
int tf_poly_zerofier_bfe(const uint64_t* r, size_t n, uint64_t* out) try { return zerofier_host(r, n, out, 1); } TF_ABI_CATCH
int tf_poly_zerofier_xfe(const uint64_t* r, size_t n, uint64_t* out) try { return zerofier_host(r, n, out, 3); } TF_ABI_CATCH
int tf_poly_interpolate_bfe_dev(const uint64_t* d, const uint64_t* v, size_t n, size_t rows, uint64_t* out, void* stream) try {
    return interpolate_dev(d, v, n, rows, out, 1, stream);
} TF_ABI_CATCH
int tf_poly_interpolate_xfe_dev(const uint64_t* d, const uint64_t* v, size_t n, size_t rows, uint64_t* out, void* stream) try {
    return interpolate_dev(d, v, n, rows, out, 3, stream);
} TF_ABI_CATCH
static int interpolate_host(const uint64_t* d, const uint64_t* v, size_t n, size_t rows, uint64_t* out, int L) {
    if (n == 0) return TF_ERR_EMPTY_DOMAIN;
    if (rows == 0) return TF_OK;
    if (!d || !v || !out) return TF_ERR_NULL_POINTER;
    return host_roundtrip(d, n * L, v, rows * n * L, out, rows * n * L,
                          [&](u64* dd, u64* dv, u64* o, hipStream_t s) { return interpolate_dev(dd, dv, n, rows, o, L, s); });
}
int tf_poly_interpolate_bfe(const uint64_t* d, const uint64_t* v, size_t n, size_t rows, uint64_t* out) try { return interpolate_host(d, v, n, rows, out, 1); } TF_ABI_CATCH
int tf_poly_interpolate_xfe(const uint64_t* d, const uint64_t* v, size_t n, size_t rows, uint64_t* out) try { return interpolate_host(d, v, n, rows, out, 3); } TF_ABI_CATCH
static int tree_new_any(const uint64_t* domain, size_t n, int L, bool on_device, void* stream, tf_zerofier_tree** tree) {
    if (!tree) return TF_ERR_NULL_POINTER;
    *tree = nullptr;
    TreeHandle* H = nullptr;
    int rc;
    if (on_device) {
        rc = tree_handle_new(domain, n, L, stream, &H);
    } else {
        if (n && !domain) return TF_ERR_NULL_POINTER;
        rc = host_roundtrip(domain, n * L, nullptr, 0, nullptr, 0, [&](u64* d, u64*, u64*, hipStream_t s) { return tree_handle_new(d, n, L, s, &H); });
    }
    if (rc) return rc;
    *tree = reinterpret_cast<tf_zerofier_tree*>(H);
    return TF_OK;
}
static int tree_new_async(const uint64_t* d_domain, size_t n, int L, void* stream, tf_zerofier_tree** tree) {
    if (!tree) return TF_ERR_NULL_POINTER;
    *tree = nullptr;
    TreeHandle* H = nullptr;
    const int rc = tree_handle_new(d_domain, n, L, stream, &H, true);
    if (rc) return rc;
    *tree = reinterpret_cast<tf_zerofier_tree*>(H);
    return TF_OK;
}
static TreeHandle* tree_of(const tf_zerofier_tree* t) { return const_cast<TreeHandle*>(reinterpret_cast<const TreeHandle*>(t)); }
int tf_zerofier_tree_new_bfe(const uint64_t* domain, size_t n, tf_zerofier_tree** tree) try { return tree_new_any(domain, n, 1, false, nullptr, tree); } TF_ABI_CATCH
int tf_zerofier_tree_new_xfe(const uint64_t* domain, size_t n, tf_zerofier_tree** tree) try { return tree_new_any(domain, n, 3, false, nullptr, tree); } TF_ABI_CATCH
int tf_zerofier_tree_new_bfe_dev(const uint64_t* d_domain, size_t n, void* stream, tf_zerofier_tree** tree) try {
    return tree_new_any(d_domain, n, 1, true, stream, tree);
} TF_ABI_CATCH
int tf_zerofier_tree_new_xfe_dev(const uint64_t* d_domain, size_t n, void* stream, tf_zerofier_tree** tree) try {
    return tree_new_any(d_domain, n, 3, true, stream, tree);
} TF_ABI_CATCH
void tf_zerofier_tree_free(tf_zerofier_tree* tree) { tree_handle_free(tree_of(tree)); }
size_t tf_zerofier_tree_num_points(const tf_zerofier_tree* tree) { return tree ? tree_handle_num_points(tree_of(tree)) : 0; }
int tf_zerofier_tree_width(const tf_zerofier_tree* tree) { return tree ? tree_handle_width(tree_of(tree)) : 0; }
int tf_zerofier_tree_zerofier_dev(const tf_zerofier_tree* tree, uint64_t* d_out, void* stream) try { return tree_handle_zerofier(tree_of(tree), d_out, stream); } TF_ABI_CATCH
int tf_zerofier_tree_batch_evaluate_dev(const tf_zerofier_tree* tree, const uint64_t* d_coeffs, size_t n_coeffs, size_t batch, uint64_t* d_out,
                                        void* stream) try {
    return tree_handle_batch_evaluate(tree_of(tree), d_coeffs, n_coeffs, batch, d_out, stream);
} TF_ABI_CATCH
int tf_zerofier_tree_interpolate_dev(tf_zerofier_tree* tree, const uint64_t* d_values, size_t rows, uint64_t* d_out, void* stream) try {
    return tree_handle_interpolate(tree_of(tree), d_values, rows, d_out, stream);
} TF_ABI_CATCH
// ---- enqueue-and-return variants (tf_hip.h): panic cases go to *d_status on the device, nothing synchronises
int tf_poly_interpolate_bfe_dev_async(const uint64_t* d, const uint64_t* v, size_t n, size_t rows, uint64_t* out, void* stream, int* d_status) try {
    if (!d_status) return TF_ERR_NULL_POINTER;
    return interpolate_dev(d, v, n, rows, out, 1, stream, d_status);
} TF_ABI_CATCH
int tf_poly_interpolate_xfe_dev_async(const uint64_t* d, const uint64_t* v, size_t n, size_t rows, uint64_t* out, void* stream, int* d_status) try {
    if (!d_status) return TF_ERR_NULL_POINTER;
    return interpolate_dev(d, v, n, rows, out, 3, stream, d_status);
} TF_ABI_CATCH
int tf_poly_clean_divide_bfe_dev_async(const uint64_t* a, size_t na, const uint64_t* b, size_t nb, uint64_t* out, void* stream, int* d_status) try {
    if (!d_status) return TF_ERR_NULL_POINTER;
    return clean_divide_dev(a, na, b, nb, out, stream, 1, d_status);
} TF_ABI_CATCH
int tf_poly_clean_divide_many_bfe_dev_async(const uint64_t* a, size_t na, size_t batch, const uint64_t* b, size_t nb, uint64_t* out, void* stream,
                                            int* d_status) try {
    if (!d_status) return TF_ERR_NULL_POINTER;
    return clean_divide_dev(a, na, b, nb, out, stream, batch, d_status);
} TF_ABI_CATCH
int tf_zerofier_tree_new_bfe_dev_async(const uint64_t* d_domain, size_t n, void* stream, tf_zerofier_tree** tree) try {
    return tree_new_async(d_domain, n, 1, stream, tree);
} TF_ABI_CATCH
int tf_zerofier_tree_new_xfe_dev_async(const uint64_t* d_domain, size_t n, void* stream, tf_zerofier_tree** tree) try {
    return tree_new_async(d_domain, n, 3, stream, tree);
} TF_ABI_CATCH
int tf_zerofier_tree_interpolate_dev_async(tf_zerofier_tree* tree, const uint64_t* d_values, size_t rows, uint64_t* d_out, void* stream, int* d_status) try {
    if (!d_status) return TF_ERR_NULL_POINTER;
    return tree_handle_interpolate(tree_of(tree), d_values, rows, d_out, stream, d_status);
} TF_ABI_CATCH
int tf_zerofier_tree_zerofier(const tf_zerofier_tree* tree, uint64_t* out) try {
    if (!tree || !out) return TF_ERR_NULL_POINTER;
    TreeHandle* H = tree_of(tree);
    const size_t hn = tree_handle_num_points(H), hl = (size_t)tree_handle_width(H);
    return host_roundtrip(nullptr, 0, nullptr, 0, out, (hn + 1) * hl, [&](u64*, u64*, u64* o, hipStream_t s) { return tree_handle_zerofier(H, o, s); });
} TF_ABI_CATCH
int tf_zerofier_tree_batch_evaluate(const tf_zerofier_tree* tree, const uint64_t* coeffs, size_t n_coeffs, size_t batch, uint64_t* out) try {
    if (!tree) return TF_ERR_NULL_POINTER;
    TreeHandle* H = tree_of(tree);
    const size_t hn = tree_handle_num_points(H), hl = (size_t)tree_handle_width(H);
    if (hn == 0 || batch == 0) return TF_OK;
    if (!out || (n_coeffs && !coeffs)) return TF_ERR_NULL_POINTER;
    return host_roundtrip(coeffs, batch * n_coeffs * hl, nullptr, 0, out, batch * hn * hl,
                          [&](u64* dc, u64*, u64* o, hipStream_t s) { return tree_handle_batch_evaluate(H, dc, n_coeffs, batch, o, s); });
} TF_ABI_CATCH
int tf_zerofier_tree_interpolate(tf_zerofier_tree* tree, const uint64_t* values, size_t rows, uint64_t* out) try {
    if (!tree) return TF_ERR_NULL_POINTER;
    TreeHandle* H = tree_of(tree);
    const size_t hn = tree_handle_num_points(H), hl = (size_t)tree_handle_width(H);
    if (hn == 0) return TF_ERR_EMPTY_DOMAIN;
    if (rows == 0) return TF_OK;
    if (!values || !out) return TF_ERR_NULL_POINTER;
    return host_roundtrip(values, rows * hn * hl, nullptr, 0, out, rows * hn * hl,
                          [&](u64* dv, u64*, u64* o, hipStream_t s) { return tree_handle_interpolate(H, dv, rows, o, s); });
} TF_ABI_CATCH
int tf_coset_eval_xfe_xoffset_dev(const uint64_t* c, size_t nc, const uint64_t offset[3], uint64_t* out, size_t order, size_t batch, void* stream) try {
    return coset_eval_xoffset_dev(c, nc, offset, out, order, batch, stream);
} TF_ABI_CATCH
int tf_coset_interpolate_xfe_xoffset_dev(const uint64_t* v, size_t n, const uint64_t offset[3], uint64_t* out, size_t batch, void* stream) try {
    return coset_interp_xoffset_dev(v, n, offset, out, batch, stream);
} TF_ABI_CATCH
int tf_coset_eval_xfe_xoffset(const uint64_t* c, size_t nc, const uint64_t offset[3], uint64_t* out, size_t order, size_t batch) try {
    if (nc > order) return TF_ERR_ORDER_NOT_ABOVE_DEGREE;
    int rc = check_len(order);
    if (rc) return rc;
    if (order == 0 || batch == 0) return TF_OK;
    if (!out || !offset || (nc && !c)) return TF_ERR_NULL_POINTER;
    return host_roundtrip(c, 3 * nc * batch, nullptr, 0, out, 3 * order * batch,
                          [&](u64* dc, u64*, u64* o, hipStream_t s) { return coset_eval_xoffset_dev(dc, nc, offset, o, order, batch, s); });
} TF_ABI_CATCH
int tf_coset_interpolate_xfe_xoffset(const uint64_t* v, size_t n, const uint64_t offset[3], uint64_t* out, size_t batch) try {
    int rc = check_len(n);
    if (rc) return rc;
    if (n == 0 || batch == 0) return TF_OK;
    if (!v || !out || !offset) return TF_ERR_NULL_POINTER;
    return host_roundtrip(v, 3 * n * batch, nullptr, 0, out, 3 * n * batch,
                          [&](u64* dv, u64*, u64* o, hipStream_t s) { return coset_interp_xoffset_dev(dv, n, offset, o, batch, s); });
} TF_ABI_CATCH
int tf_barycentric_evaluate_bfe_dev(const uint64_t* cw, size_t n, size_t batch, const uint64_t x[3], uint64_t* out, void* stream) try {
    return barycentric_dev(cw, n, batch, 1, x, out, stream);
} TF_ABI_CATCH
int tf_barycentric_evaluate_xfe_dev(const uint64_t* cw, size_t n, size_t batch, const uint64_t x[3], uint64_t* out, void* stream) try {
    return barycentric_dev(cw, n, batch, 3, x, out, stream);
} TF_ABI_CATCH
static int barycentric_host(const uint64_t* cw, size_t n, size_t batch, int width, const uint64_t x[3], uint64_t* out) {
    int rc = check_len(n);
    if (rc) return rc;
    if (!x) return TF_ERR_NULL_POINTER;
    if (n == 0) return TF_ERR_INVERSE_OF_ZERO;
    if (batch == 0) return barycentric_dev(nullptr, n, 0, width, x, nullptr, nullptr);  // the argument checks alone
    if (!cw || !out) return TF_ERR_NULL_POINTER;
    return host_roundtrip(cw, batch * n * width, nullptr, 0, out, 3 * batch,
                          [&](u64* dc, u64*, u64* o, hipStream_t s) { return barycentric_dev(dc, n, batch, width, x, o, s); });
}
int tf_barycentric_evaluate_bfe(const uint64_t* cw, size_t n, size_t batch, const uint64_t x[3], uint64_t* out) try { return barycentric_host(cw, n, batch, 1, x, out); } TF_ABI_CATCH
int tf_barycentric_evaluate_xfe(const uint64_t* cw, size_t n, size_t batch, const uint64_t x[3], uint64_t* out) try { return barycentric_host(cw, n, batch, 3, x, out); } TF_ABI_CATCH
// Polynomial<BFieldElement>::evaluate::<XFieldElement, XFieldElement> (polynomial.rs:309-320) for `batch` polynomials at n_points
// extension-field points: out[(b * n_points + i) * 3] = f_b(points[i]).  Horner (the shape of the use: every column polynomial
// of a table at a few out-of-domain points).
int tf_poly_evaluate_bfe_at_xfe_dev(const uint64_t* c, size_t nc, size_t batch, const uint64_t* pts, size_t np, uint64_t* out, void* stream) try {
    if (np == 0 || batch == 0) return TF_OK;
    if (!pts || !out || (nc && !c)) return TF_ERR_NULL_POINTER;
    DeviceCtx* ctx = nullptr;
    int rc = current_ctx(&ctx);
    if (rc) return rc;
    return batch_evaluate_horner(c, nc, nc, batch, pts, np, out, 3, stream, 1);
} TF_ABI_CATCH
int tf_poly_evaluate_bfe_at_xfe(const uint64_t* c, size_t nc, size_t batch, const uint64_t* pts, size_t np, uint64_t* out) try {
    if (np == 0 || batch == 0) return TF_OK;
    if (!pts || !out || (nc && !c)) return TF_ERR_NULL_POINTER;
    return host_roundtrip(c, batch * nc, pts, 3 * np, out, 3 * batch * np,
                          [&](u64* dc, u64* dp, u64* o, hipStream_t s) { return batch_evaluate_horner(dc, nc, nc, batch, dp, np, o, 3, s, 1); });
} TF_ABI_CATCH
int tf_poly_clean_divide_bfe_dev(const uint64_t* a, size_t na, const uint64_t* b, size_t nb, uint64_t* out, void* stream) try {
    return clean_divide_dev(a, na, b, nb, out, stream);
} TF_ABI_CATCH
int tf_poly_mul_shared_bfe_dev(const uint64_t* a, size_t na, size_t batch, const uint64_t* b, size_t nb, uint64_t* out, void* stream) try {
    return poly_mul_shared_dev(a, na, batch, b, nb, out, 1, stream);
} TF_ABI_CATCH
int tf_poly_mul_shared_xfe_dev(const uint64_t* a, size_t na, size_t batch, const uint64_t* b, size_t nb, uint64_t* out, void* stream) try {
    return poly_mul_shared_dev(a, na, batch, b, nb, out, 3, stream);
} TF_ABI_CATCH
int tf_poly_clean_divide_many_bfe_dev(const uint64_t* a, size_t na, size_t batch, const uint64_t* b, size_t nb, uint64_t* out, void* stream) try {
    return clean_divide_dev(a, na, b, nb, out, stream, batch);
} TF_ABI_CATCH
int tf_poly_clean_divide_many_bfe(const uint64_t* a, size_t na, size_t batch, const uint64_t* b, size_t nb, uint64_t* out) try {
    if (nb == 0) return TF_ERR_DIVISION_BY_ZERO;
    if (na < nb) return na ? TF_ERR_DIVISION_NOT_CLEAN : TF_OK;
    if (batch == 0) return TF_OK;
    if (!a || !b || !out) return TF_ERR_NULL_POINTER;
    return host_roundtrip(a, batch * na, b, nb, out, batch * (na - nb + 1),
                          [&](u64* da, u64* db, u64* o, hipStream_t s) { return clean_divide_dev(da, na, db, nb, o, s, batch); });
} TF_ABI_CATCH
int tf_poly_clean_divide_bfe(const uint64_t* a, size_t na, const uint64_t* b, size_t nb, uint64_t* out) try {
    if (nb == 0) return TF_ERR_DIVISION_BY_ZERO;
    if (na < nb) return na ? TF_ERR_DIVISION_NOT_CLEAN : TF_OK;
    if (!a || !b || !out) return TF_ERR_NULL_POINTER;
    return host_roundtrip(a, na, b, nb, out, na - nb + 1, [&](u64* da, u64* db, u64* o, hipStream_t s) { return clean_divide_dev(da, na, db, nb, o, s); });
} TF_ABI_CATCH
// Polynomial::divide / reduce / Div / Rem and formal_power_series_inverse_newton (tf_divide.hip)
int tf_poly_divide_bfe(const uint64_t* a, size_t na, size_t batch, const uint64_t* b, size_t nb, uint64_t* q, uint64_t* r) try {
    return divide_host(a, na, batch, b, nb, q, r, 1);
} TF_ABI_CATCH
int tf_poly_divide_xfe(const uint64_t* a, size_t na, size_t batch, const uint64_t* b, size_t nb, uint64_t* q, uint64_t* r) try {
    return divide_host(a, na, batch, b, nb, q, r, 3);
} TF_ABI_CATCH
int tf_poly_divide_bfe_dev(const uint64_t* d_a, size_t na, size_t batch, const uint64_t* d_b, size_t nb, uint64_t* d_q, uint64_t* d_r, void* stream,
                           int* d_status) try {
    if (!d_status) return TF_ERR_NULL_POINTER;
    return divide_dev(d_a, na, batch, d_b, nb, d_q, d_r, stream, d_status, 1);
} TF_ABI_CATCH
int tf_poly_divide_xfe_dev(const uint64_t* d_a, size_t na, size_t batch, const uint64_t* d_b, size_t nb, uint64_t* d_q, uint64_t* d_r, void* stream,
                           int* d_status) try {
    if (!d_status) return TF_ERR_NULL_POINTER;
    return divide_dev(d_a, na, batch, d_b, nb, d_q, d_r, stream, d_status, 3);
} TF_ABI_CATCH
size_t tf_poly_fps_inverse_newton_len(size_t nf, size_t precision) { return fps_len(nf, precision); }
int tf_poly_fps_inverse_newton_bfe(const uint64_t* f, size_t nf, size_t precision, uint64_t* out) try {
    return fps_host(f, nf, precision, out, 1);
} TF_ABI_CATCH
int tf_poly_fps_inverse_newton_xfe(const uint64_t* f, size_t nf, size_t precision, uint64_t* out) try {
    return fps_host(f, nf, precision, out, 3);
} TF_ABI_CATCH
int tf_poly_fps_inverse_newton_bfe_dev(const uint64_t* d_f, size_t nf, size_t precision, uint64_t* d_out, void* stream, int* d_status) try {
    if (!d_status) return TF_ERR_NULL_POINTER;
    return fps_dev(d_f, nf, precision, d_out, stream, d_status, 1);
} TF_ABI_CATCH
int tf_poly_fps_inverse_newton_xfe_dev(const uint64_t* d_f, size_t nf, size_t precision, uint64_t* d_out, void* stream, int* d_status) try {
    if (!d_status) return TF_ERR_NULL_POINTER;
    return fps_dev(d_f, nf, precision, d_out, stream, d_status, 3);
} TF_ABI_CATCH
// FiniteField::batch_inversion / Inverse::inverse_or_zero over a vector (tf_inverse.hip)
int tf_batch_inversion_bfe(const uint64_t* in, size_t n, uint64_t* out) try { return batch_inverse_host(in, n, out, 1, false); } TF_ABI_CATCH
int tf_batch_inversion_xfe(const uint64_t* in, size_t n, uint64_t* out) try { return batch_inverse_host(in, n, out, 3, false); } TF_ABI_CATCH
int tf_batch_inversion_bfe_dev(const uint64_t* d_in, size_t n, uint64_t* d_out, void* stream) try {
    return batch_inverse_dev(d_in, n, d_out, 1, false, stream, nullptr);
} TF_ABI_CATCH
int tf_batch_inversion_xfe_dev(const uint64_t* d_in, size_t n, uint64_t* d_out, void* stream) try {
    return batch_inverse_dev(d_in, n, d_out, 3, false, stream, nullptr);
} TF_ABI_CATCH
int tf_batch_inversion_bfe_dev_async(const uint64_t* d_in, size_t n, uint64_t* d_out, void* stream, int* d_status) try {
    if (n && !d_status) return TF_ERR_NULL_POINTER;
    return batch_inverse_dev(d_in, n, d_out, 1, false, stream, d_status);
} TF_ABI_CATCH
int tf_batch_inversion_xfe_dev_async(const uint64_t* d_in, size_t n, uint64_t* d_out, void* stream, int* d_status) try {
    if (n && !d_status) return TF_ERR_NULL_POINTER;
    return batch_inverse_dev(d_in, n, d_out, 3, false, stream, d_status);
} TF_ABI_CATCH
int tf_inverse_or_zero_bfe(const uint64_t* in, size_t n, uint64_t* out) try { return batch_inverse_host(in, n, out, 1, true); } TF_ABI_CATCH
int tf_inverse_or_zero_xfe(const uint64_t* in, size_t n, uint64_t* out) try { return batch_inverse_host(in, n, out, 3, true); } TF_ABI_CATCH
int tf_inverse_or_zero_bfe_dev(const uint64_t* d_in, size_t n, uint64_t* d_out, void* stream) try {
    return batch_inverse_dev(d_in, n, d_out, 1, true, stream, nullptr);
} TF_ABI_CATCH
int tf_inverse_or_zero_xfe_dev(const uint64_t* d_in, size_t n, uint64_t* d_out, void* stream) try {
    return batch_inverse_dev(d_in, n, d_out, 3, true, stream, nullptr);
} TF_ABI_CATCH

// Add / Sub / Neg, scalar_mul, scale, formal_derivative, degree, XFieldElement x BFieldElement products and weighted sums (tf_algebra.hip)
int tf_poly_add(const uint64_t* a, size_t na, const uint64_t* b, size_t nb, int width, uint64_t* out, size_t batch) try {
    return poly_addsub(a, na, b, nb, width, out, batch, false, true, nullptr);
} TF_ABI_CATCH
int tf_poly_add_dev(const uint64_t* a, size_t na, const uint64_t* b, size_t nb, int width, uint64_t* out, size_t batch, void* stream) try {
    return poly_addsub(a, na, b, nb, width, out, batch, false, false, stream);
} TF_ABI_CATCH
int tf_poly_sub(const uint64_t* a, size_t na, const uint64_t* b, size_t nb, int width, uint64_t* out, size_t batch) try {
    return poly_addsub(a, na, b, nb, width, out, batch, true, true, nullptr);
} TF_ABI_CATCH
int tf_poly_sub_dev(const uint64_t* a, size_t na, const uint64_t* b, size_t nb, int width, uint64_t* out, size_t batch, void* stream) try {
    return poly_addsub(a, na, b, nb, width, out, batch, true, false, stream);
} TF_ABI_CATCH
int tf_poly_neg(const uint64_t* a, size_t na, int width, uint64_t* out, size_t batch) try {
    return poly_neg(a, na, width, out, batch, true, nullptr);
} TF_ABI_CATCH
int tf_poly_neg_dev(const uint64_t* a, size_t na, int width, uint64_t* out, size_t batch, void* stream) try {
    return poly_neg(a, na, width, out, batch, false, stream);
} TF_ABI_CATCH
int tf_poly_scalar_mul(const uint64_t* a, size_t na, int width_a, const uint64_t* scalar, int width_s, uint64_t* out, size_t batch) try {
    return poly_scalar_mul(a, na, width_a, scalar, width_s, out, batch, false, true, nullptr);
} TF_ABI_CATCH
int tf_poly_scalar_mul_dev(const uint64_t* a, size_t na, int width_a, const uint64_t* scalar, int width_s, uint64_t* out, size_t batch,
                           void* stream) try {
    return poly_scalar_mul(a, na, width_a, scalar, width_s, out, batch, false, false, stream);
} TF_ABI_CATCH
int tf_poly_scale(const uint64_t* a, size_t na, int width_a, const uint64_t* alpha, int width_alpha, uint64_t* out, size_t batch) try {
    return poly_scalar_mul(a, na, width_a, alpha, width_alpha, out, batch, true, true, nullptr);
} TF_ABI_CATCH
int tf_poly_scale_dev(const uint64_t* a, size_t na, int width_a, const uint64_t* alpha, int width_alpha, uint64_t* out, size_t batch,
                      void* stream) try {
    return poly_scalar_mul(a, na, width_a, alpha, width_alpha, out, batch, true, false, stream);
} TF_ABI_CATCH
int tf_poly_formal_derivative(const uint64_t* a, size_t na, int width, uint64_t* out, size_t batch) try {
    return poly_derivative(a, na, width, out, batch, true, nullptr);
} TF_ABI_CATCH
int tf_poly_formal_derivative_dev(const uint64_t* a, size_t na, int width, uint64_t* out, size_t batch, void* stream) try {
    return poly_derivative(a, na, width, out, batch, false, stream);
} TF_ABI_CATCH
int tf_poly_degree(const uint64_t* a, size_t na, int width, size_t batch, int64_t* degrees) try {
    return poly_degree(a, na, width, batch, reinterpret_cast<long long*>(degrees), true, nullptr);
} TF_ABI_CATCH
int tf_poly_degree_dev(const uint64_t* a, size_t na, int width, size_t batch, int64_t* degrees, void* stream) try {
    return poly_degree(a, na, width, batch, reinterpret_cast<long long*>(degrees), false, stream);
} TF_ABI_CATCH
int tf_hadamard_xfe_bfe_dev(const uint64_t* a, const uint64_t* b, uint64_t* out, size_t count, void* stream) try {
    return hadamard_xfe_bfe_dev(a, b, out, count, stream);
} TF_ABI_CATCH
int tf_poly_linear_combination(const uint64_t* polys, size_t n, int width_p, size_t stride, size_t k, const uint64_t* weights, int width_w,
                               uint64_t* out) try {
    return poly_lincomb(polys, n, width_p, stride, k, weights, width_w, out, true, nullptr);
} TF_ABI_CATCH
int tf_poly_linear_combination_dev(const uint64_t* polys, size_t n, int width_p, size_t stride, size_t k, const uint64_t* weights, int width_w,
                                   uint64_t* out, void* stream) try {
    return poly_lincomb(polys, n, width_p, stride, k, weights, width_w, out, false, stream);
} TF_ABI_CATCH
// get_colinear_y / are_colinear, element-wise mod_pow, geometric sequences and index gathers (tf_points.hip)
int tf_get_colinear_y(const uint64_t* x0, const uint64_t* y0, const uint64_t* x1, const uint64_t* y1, size_t n, const uint64_t* p2x, size_t n_p2x,
                      int width_x, int width_y, uint64_t* out) try {
    return get_colinear_y(x0, y0, x1, y1, n, p2x, n_p2x, width_x, width_y, out, true, nullptr, nullptr);
} TF_ABI_CATCH
int tf_get_colinear_y_dev(const uint64_t* x0, const uint64_t* y0, const uint64_t* x1, const uint64_t* y1, size_t n, const uint64_t* p2x, size_t n_p2x,
                          int width_x, int width_y, uint64_t* out, void* stream, int* d_status) try {
    return get_colinear_y(x0, y0, x1, y1, n, p2x, n_p2x, width_x, width_y, out, false, stream, d_status);
} TF_ABI_CATCH
int tf_are_colinear(const uint64_t* xs, const uint64_t* ys, size_t n_groups, size_t k, int width_x, int width_y, int* flags) try {
    return are_colinear(xs, ys, n_groups, k, width_x, width_y, flags, true, nullptr);
} TF_ABI_CATCH
int tf_are_colinear_dev(const uint64_t* xs, const uint64_t* ys, size_t n_groups, size_t k, int width_x, int width_y, int* flags, void* stream) try {
    return are_colinear(xs, ys, n_groups, k, width_x, width_y, flags, false, stream);
} TF_ABI_CATCH
int tf_mod_pow(const uint64_t* bases, size_t n_bases, const uint64_t* exps, size_t n_exps, int width, uint64_t* out, size_t n) try {
    return mod_pow(bases, n_bases, exps, n_exps, width, out, n, true, nullptr);
} TF_ABI_CATCH
int tf_mod_pow_dev(const uint64_t* bases, size_t n_bases, const uint64_t* exps, size_t n_exps, int width, uint64_t* out, size_t n, void* stream) try {
    return mod_pow(bases, n_bases, exps, n_exps, width, out, n, false, stream);
} TF_ABI_CATCH
int tf_powers(const uint64_t* first, const uint64_t* ratio, int width, uint64_t* out, size_t n) try {
    return powers(first, ratio, width, out, n, true, nullptr);
} TF_ABI_CATCH
int tf_powers_dev(const uint64_t* first, const uint64_t* ratio, int width, uint64_t* out, size_t n, void* stream) try {
    return powers(first, ratio, width, out, n, false, stream);
} TF_ABI_CATCH
int tf_gather_elements_dev(const uint64_t* src, size_t src_len, int width, const uint32_t* indices, size_t n, uint64_t* out, void* stream,
                           int* d_status) try {
    return gather_elements_dev(src, src_len, width, indices, n, out, stream, d_status);
} TF_ABI_CATCH
// the FRI split-and-fold, one to many levels per call (tf_fri.hip)
int tf_fri_fold(const uint64_t* codewords, size_t n, size_t batch, int width_c, uint64_t offset_raw, const uint64_t* challenges, size_t levels,
                size_t n_sets, int width_a, uint64_t* out) try {
    return fri_fold(codewords, n, batch, width_c, offset_raw, challenges, levels, n_sets, width_a, out, true, nullptr);
} TF_ABI_CATCH
int tf_fri_fold_dev(const uint64_t* codewords, size_t n, size_t batch, int width_c, uint64_t offset_raw, const uint64_t* challenges, size_t levels,
                    size_t n_sets, int width_a, uint64_t* out, void* stream) try {
    return fri_fold(codewords, n, batch, width_c, offset_raw, challenges, levels, n_sets, width_a, out, false, stream);
} TF_ABI_CATCH
size_t tf_fri_fold_workspace(size_t n, size_t batch, int width_c, int width_a, size_t levels) try {
    return fri_fold_workspace(n, batch, width_c, width_a, levels);
} catch (...) {
    ::tfi::abi_caught("C++ exception in tf_fri_fold_workspace", TF_ERR_INTERNAL);
    return 0;
}
int tf_fri_fold_plan(size_t n, size_t levels, int width_c, int width_a, int* levels_per_pass, int capacity) try {
    return fri_fold_plan(n, levels, width_c, width_a, levels_per_pass, capacity);
} TF_ABI_CATCH
// prefix scans along columns: sums, products, the affine recurrence (tf_scan.hip)
int tf_scan_sum_dev(const uint64_t* in, size_t n, size_t batch, int width, size_t stride_in, const uint64_t* init, size_t n_init, uint64_t* out,
                    size_t stride_out, void* d_work, size_t work_bytes, void* stream) try {
    return scan_dev(TF_SCAN_SUM, nullptr, 0, 0, width, 0, in, width, stride_in, n, batch, init, n_init, out, stride_out, d_work, work_bytes, stream);
} TF_ABI_CATCH
int tf_scan_product_dev(const uint64_t* in, size_t n, size_t batch, int width, size_t stride_in, const uint64_t* init, size_t n_init, uint64_t* out,
                        size_t stride_out, void* d_work, size_t work_bytes, void* stream) try {
    return scan_dev(TF_SCAN_PRODUCT, in, n, 1, width, stride_in, nullptr, width, 0, n, batch, init, n_init, out, stride_out, d_work, work_bytes, stream);
} TF_ABI_CATCH
int tf_scan_affine_dev(const uint64_t* a, size_t a_len, size_t a_sets, int width_a, size_t stride_a, const uint64_t* b, int width_b, size_t stride_b,
                       size_t n, size_t batch, const uint64_t* init, size_t n_init, uint64_t* out, size_t stride_out, void* d_work, size_t work_bytes,
                       void* stream) try {
    return scan_dev(TF_SCAN_AFFINE, a, a_len, a_sets, width_a, stride_a, b, width_b, stride_b, n, batch, init, n_init, out, stride_out, d_work, work_bytes,
                    stream);
} TF_ABI_CATCH
size_t tf_scan_workspace(int mode, size_t n, size_t batch, int width_out) try {
    return scan_workspace(mode, n, batch, width_out);
} catch (...) {
    ::tfi::abi_caught("C++ exception in tf_scan_workspace", TF_ERR_INTERNAL);
    return 0;
}
int tf_scan_plan(int mode, size_t n, size_t batch, int width_out, int* info, int capacity) try {
    return scan_plan(mode, n, batch, width_out, info, capacity);
} TF_ABI_CATCH
// the DEEP quotient: whole codewords and sampled rows (tf_deep.hip)
int tf_deep_quotient_dev(const uint64_t* d_main, size_t k1, size_t stride_main, const uint64_t* d_aux, size_t k3, size_t stride_aux, size_t n,
                         uint64_t offset_raw, const uint64_t* d_points, size_t n_points, const uint64_t* d_weights, const uint64_t* d_values,
                         uint64_t* d_out, void* d_work, size_t work_bytes, void* stream, int* d_status) try {
    return deep_quotient_dev(d_main, k1, stride_main, d_aux, k3, stride_aux, n, offset_raw, d_points, n_points, d_weights, d_values, d_out, d_work,
                             work_bytes, stream, d_status);
} TF_ABI_CATCH
size_t tf_deep_quotient_workspace(size_t n, size_t k1, size_t k3, size_t n_points) try {
    return deep_quotient_workspace(n, k1, k3, n_points);
} catch (...) {
    ::tfi::abi_caught("C++ exception in tf_deep_quotient_workspace", TF_ERR_INTERNAL);
    return 0;
}
int tf_deep_quotient_plan(size_t n, size_t k1, size_t k3, size_t n_points, int* fields, int capacity) try {
    return deep_quotient_plan(n, k1, k3, n_points, fields, capacity);
} TF_ABI_CATCH
int tf_deep_quotient_rows_dev(const uint64_t* d_main_rows, size_t k1, size_t row_stride_main, const uint64_t* d_aux_rows, size_t k3,
                              size_t row_stride_aux, size_t n, uint64_t offset_raw, const uint32_t* d_indices, size_t n_rows,
                              const uint64_t* d_points, size_t n_points, const uint64_t* d_weights, const uint64_t* d_values, uint64_t* d_out,
                              void* stream, int* d_status) try {
    return deep_quotient_rows_dev(d_main_rows, k1, row_stride_main, d_aux_rows, k3, row_stride_aux, n, offset_raw, d_indices, n_rows, d_points, n_points,
                                  d_weights, d_values, d_out, stream, d_status);
} TF_ABI_CATCH
// tables between the column-major and the row-major layout: transpose, row gather, row-major LDE (tf_table.hip)
int tf_table_transpose(const uint64_t* src, size_t n_outer, size_t n_inner, int width, size_t src_stride, uint64_t* dst, size_t dst_stride,
                       size_t batch) try {
    return table_transpose(src, n_outer, n_inner, width, src_stride, dst, dst_stride, batch, true, nullptr);
} TF_ABI_CATCH
int tf_table_transpose_dev(const uint64_t* src, size_t n_outer, size_t n_inner, int width, size_t src_stride, uint64_t* dst, size_t dst_stride,
                           size_t batch, void* stream) try {
    return table_transpose(src, n_outer, n_inner, width, src_stride, dst, dst_stride, batch, false, stream);
} TF_ABI_CATCH
int tf_table_gather_rows(const uint64_t* table, int layout, size_t n_rows, size_t n_cols, int width, size_t stride, const uint32_t* indices, size_t k,
                         uint64_t* out, size_t out_stride, size_t batch) try {
    return table_gather_rows(table, layout, n_rows, n_cols, width, stride, indices, k, out, out_stride, batch, true, nullptr, nullptr);
} TF_ABI_CATCH
int tf_table_gather_rows_dev(const uint64_t* table, int layout, size_t n_rows, size_t n_cols, int width, size_t stride, const uint32_t* indices,
                             size_t k, uint64_t* out, size_t out_stride, size_t batch, void* stream, int* d_status) try {
    return table_gather_rows(table, layout, n_rows, n_cols, width, stride, indices, k, out, out_stride, batch, false, stream, d_status);
} TF_ABI_CATCH
int tf_table_lde_rows_bfe_dev(const uint64_t* rows, size_t n, size_t n_cols, size_t row_stride_in, uint64_t off_in, uint64_t* out, size_t m,
                              size_t row_stride_out, uint64_t off_out, size_t cols_per_block, void* stream) try {
    return table_lde_rows_dev(rows, n, n_cols, row_stride_in, off_in, out, m, row_stride_out, off_out, cols_per_block, 1, stream);
} TF_ABI_CATCH
int tf_table_lde_rows_xfe_dev(const uint64_t* rows, size_t n, size_t n_cols, size_t row_stride_in, uint64_t off_in, uint64_t* out, size_t m,
                              size_t row_stride_out, uint64_t off_out, size_t cols_per_block, void* stream) try {
    return table_lde_rows_dev(rows, n, n_cols, row_stride_in, off_in, out, m, row_stride_out, off_out, cols_per_block, 3, stream);
} TF_ABI_CATCH
size_t tf_table_lde_rows_workspace(size_t n, size_t m, size_t n_cols, int width, size_t cols_per_block) try {
    return table_lde_rows_workspace(n, m, n_cols, width, cols_per_block);
} catch (...) {
    ::tfi::abi_caught("C++ exception in tf_table_lde_rows_workspace", TF_ERR_INTERNAL);
    return 0;
}
static int coset_extrapolate_host(uint64_t offset, const uint64_t* cw, size_t n, size_t batch, const uint64_t* pts, size_t np,
                                  uint64_t* out, int L) {
    if (n == 0) return TF_ERR_LEN_NOT_POWER_OF_TWO;
    int rc = check_len(n);
    if (rc) return rc;
    if (batch == 0 || np == 0) return TF_OK;
    if (!cw || !pts || !out) return TF_ERR_NULL_POINTER;
    if (offset == 0) return TF_ERR_INVERSE_OF_ZERO;
    return host_roundtrip(cw, batch * n * L, pts, np * L, out, batch * np * L, [&](u64* dc, u64* dp, u64* o, hipStream_t s) {
        return coset_extrapolate_dev(offset, dc, n, batch, dp, np, o, L, s);
    });
}
int tf_coset_extrapolate_bfe(uint64_t offset, const uint64_t* cw, size_t n, size_t batch, const uint64_t* pts, size_t np, uint64_t* out) try {
    return coset_extrapolate_host(offset, cw, n, batch, pts, np, out, 1);
} TF_ABI_CATCH
int tf_coset_extrapolate_xfe(uint64_t offset, const uint64_t* cw, size_t n, size_t batch, const uint64_t* pts, size_t np, uint64_t* out) try {
    return coset_extrapolate_host(offset, cw, n, batch, pts, np, out, 3);
} TF_ABI_CATCH
int tf_tip5_hash_table_rows(const uint64_t* table, size_t n_rows, size_t n_cols, int width, size_t col_stride, uint64_t* digests,
                            size_t batch) try {
    if (width != 1 && width != 3) return TF_ERR_NULL_POINTER;
    if (n_rows == 0 || batch == 0) return TF_OK;
    if (!digests || (n_cols && !table)) return TF_ERR_NULL_POINTER;
    return host_roundtrip(table, batch * n_cols * col_stride, nullptr, 0, digests, batch * n_rows * 5,
                          [&](u64* dt, u64*, u64* o, hipStream_t s) { return hash_table_rows_dev(dt, n_rows, n_cols, width, col_stride, o, batch, s); });
} TF_ABI_CATCH
int tf_merkle_from_columns(const uint64_t* table, size_t n_rows, size_t n_cols, int width, size_t col_stride, uint64_t* nodes_out,
                           size_t batch) try {
    if (width != 1 && width != 3) return TF_ERR_NULL_POINTER;
    int rc = check_leaves(n_rows);
    if (rc) return rc;
    if (batch == 0) return TF_OK;
    if (!nodes_out || (n_cols && !table)) return TF_ERR_NULL_POINTER;
    return host_roundtrip(table, batch * n_cols * col_stride, nullptr, 0, nodes_out, batch * n_rows * 10,
                          [&](u64* dt, u64*, u64* o, hipStream_t s) { return merkle_from_columns_dev(dt, n_rows, n_cols, width, col_stride, o, batch, s); });
} TF_ABI_CATCH
int tf_merkle_from_rows(const uint64_t* rows, size_t row_len, size_t n_rows, uint64_t* nodes_out, size_t batch) try {
    TRY(check_leaves(n_rows));
    if (batch == 0) return TF_OK;
    if (!nodes_out || (row_len && !rows)) return TF_ERR_NULL_POINTER;
    return host_roundtrip(rows, n_rows * row_len * batch, nullptr, 0, nodes_out, n_rows * batch * 10,
                          [&](u64* r, u64*, u64* o, hipStream_t s) { return merkle_from_rows_dev(r, row_len, n_rows, o, batch, s); });
} TF_ABI_CATCH

int tf_merkle_auth_structure_indices(size_t num_leafs, const uint64_t* leaf_indices, size_t k, uint64_t* out_indices,
                                     size_t capacity, size_t* out_count) try {
    if ((k && !leaf_indices) || !out_count) return TF_ERR_NULL_POINTER;
    std::vector<unsigned long long> idx;
    TRY(auth_structure_indices(num_leafs, leaf_indices, k, &idx));
    *out_count = idx.size();
    if (!out_indices || capacity == 0) return TF_OK;  // sizing call: only the count
    if (capacity < idx.size()) return TF_ERR_BUFFER_TOO_SMALL;  // nothing is written; *out_count says what is needed
    for (size_t i = 0; i < idx.size(); ++i) out_indices[i] = idx[i];
    return TF_OK;
} TF_ABI_CATCH

int tf_merkle_authentication_structure_dev(const uint64_t* d_nodes, size_t num_leafs, const uint64_t* leaf_indices, size_t k,
                                           uint64_t* out_digests, size_t capacity_digests, size_t* out_count, void* stream) try {
    if (!d_nodes || (k && !leaf_indices) || !out_count) return TF_ERR_NULL_POINTER;
    std::vector<unsigned long long> idx;
    TRY(auth_structure_indices(num_leafs, leaf_indices, k, &idx));
    *out_count = idx.size();
    if (idx.empty() || !out_digests) return TF_OK;
    if (capacity_digests < idx.size()) return TF_ERR_BUFFER_TOO_SMALL;
    DeviceCtx* ctx = nullptr;
    TRY(current_ctx(&ctx));
    hipStream_t s = static_cast<hipStream_t>(stream);
    DevTemp didx(s), dout(s);
    TRY(didx.alloc(idx.size(), "authentication structure gather"));
    TRY(dout.alloc(idx.size() * 5, "authentication structure gather"));
    TRY(h2d(didx.p, reinterpret_cast<const u64*>(idx.data()), idx.size(), s));
    TRY(gather_digests_dev(d_nodes, reinterpret_cast<const unsigned long long*>(didx.p), idx.size(), dout.p, s));
    TRY(d2h(out_digests, dout.p, idx.size() * 5, s));
    return sync(s);
} TF_ABI_CATCH

int tf_merkle_auth_structure_from_leafs(const uint64_t* leafs, size_t num_leafs, size_t batch, const uint64_t* leaf_indices, size_t k,
                                        uint64_t* out_digests, size_t capacity_digests, size_t* out_count, uint64_t* roots) try {
    return merkle_open_host(leafs, num_leafs, batch, leaf_indices, k, out_digests, capacity_digests, out_count, roots);
} TF_ABI_CATCH
int tf_merkle_auth_structure_from_leafs_dev(const uint64_t* d_leafs, size_t num_leafs, size_t batch, const uint64_t* leaf_indices, size_t k,
                                            uint64_t* d_out_digests, size_t capacity_digests, size_t* out_count, uint64_t* d_roots,
                                            void* stream) try {
    return merkle_open_dev(d_leafs, num_leafs, batch, leaf_indices, k, d_out_digests, capacity_digests, out_count, d_roots,
                           static_cast<hipStream_t>(stream));
} TF_ABI_CATCH
size_t tf_merkle_auth_structure_from_leafs_workspace(size_t num_leafs, size_t batch, size_t k_nodes) try {
    return merkle_open_workspace(num_leafs, batch, k_nodes);
} catch (...) {  // (a size, not a status: the guard's message is kept, the size is 0)
    ::tfi::abi_caught("C++ exception in tf_merkle_auth_structure_from_leafs_workspace", TF_ERR_INTERNAL);
    return 0;
}

// the same openings with the leaf indices in device memory (tf_merkle_open.hip, second half)
size_t tf_merkle_auth_structure_max_nodes(size_t num_leafs, size_t k) try {
    return merkle_plan_max_nodes(num_leafs, k);
} catch (...) {
    ::tfi::abi_caught("C++ exception in tf_merkle_auth_structure_max_nodes", TF_ERR_INTERNAL);
    return 0;
}
int tf_merkle_auth_structure_indices_dev(size_t num_leafs, const uint32_t* d_leaf_indices, size_t k, size_t n_lists, uint32_t* d_node_indices,
                                         size_t capacity, uint32_t* d_counts, uint32_t* d_level_ends, void* stream, int* d_status) try {
    return merkle_plan_dev(num_leafs, d_leaf_indices, k, n_lists, d_node_indices, capacity, d_counts, d_level_ends, static_cast<hipStream_t>(stream),
                           d_status);
} TF_ABI_CATCH
int tf_merkle_authentication_structure_sampled_dev(const uint64_t* d_nodes, size_t num_leafs, const uint32_t* d_leaf_indices, size_t k,
                                                   size_t n_lists, size_t trees_per_list, uint64_t* d_out_digests, size_t capacity,
                                                   uint32_t* d_counts, void* stream, int* d_status) try {
    return merkle_nodes_sampled_dev(d_nodes, num_leafs, d_leaf_indices, k, n_lists, trees_per_list, d_out_digests, capacity, d_counts,
                                    static_cast<hipStream_t>(stream), d_status);
} TF_ABI_CATCH
int tf_merkle_auth_structure_from_leafs_sampled_dev(const uint64_t* d_leafs, size_t num_leafs, const uint32_t* d_leaf_indices, size_t k,
                                                    size_t n_lists, size_t trees_per_list, uint64_t* d_out_digests, size_t capacity,
                                                    uint32_t* d_counts, uint64_t* d_roots, void* stream, int* d_status) try {
    return merkle_open_sampled_dev(d_leafs, num_leafs, d_leaf_indices, k, n_lists, trees_per_list, d_out_digests, capacity, d_counts, d_roots,
                                   static_cast<hipStream_t>(stream), d_status);
} TF_ABI_CATCH
size_t tf_merkle_auth_structure_from_leafs_sampled_workspace(size_t num_leafs, size_t trees, size_t k, size_t n_lists) try {
    return merkle_open_sampled_workspace(num_leafs, trees, k, n_lists);
} catch (...) {
    ::tfi::abi_caught("C++ exception in tf_merkle_auth_structure_from_leafs_sampled_workspace", TF_ERR_INTERNAL);
    return 0;
}

int tf_merkle_verify_proofs(const uint32_t* tree_heights, size_t n_proofs, const uint64_t* leaf_offsets, const uint64_t* leaf_indices,
                            const uint64_t* leaf_digests, const uint64_t* auth_offsets, const uint64_t* auth_digests,
                            const uint64_t* expected_roots, int* statuses) try {
    return merkle_proofs_host(tree_heights, n_proofs, leaf_offsets, leaf_indices, leaf_digests, auth_offsets, auth_digests, expected_roots,
                              statuses, nullptr, false);
} TF_ABI_CATCH
int tf_merkle_verify_proofs_dev(const uint32_t* tree_heights, size_t n_proofs, const uint64_t* leaf_offsets, const uint64_t* d_leaf_indices,
                                const uint64_t* d_leaf_digests, const uint64_t* auth_offsets, const uint64_t* d_auth_digests,
                                const uint64_t* d_expected_roots, int* d_statuses, void* stream) try {
    return merkle_proofs_dev(tree_heights, n_proofs, leaf_offsets, d_leaf_indices, d_leaf_digests, auth_offsets, d_auth_digests, d_expected_roots,
                             d_statuses, nullptr, false, 0, 0, static_cast<hipStream_t>(stream));
} TF_ABI_CATCH
int tf_merkle_authentication_paths(const uint32_t* tree_heights, size_t n_proofs, const uint64_t* leaf_offsets, const uint64_t* leaf_indices,
                                   const uint64_t* leaf_digests, const uint64_t* auth_offsets, const uint64_t* auth_digests,
                                   uint64_t* paths_out, int* statuses) try {
    return merkle_proofs_host(tree_heights, n_proofs, leaf_offsets, leaf_indices, leaf_digests, auth_offsets, auth_digests, nullptr, statuses,
                              paths_out, true);
} TF_ABI_CATCH
int tf_merkle_authentication_paths_dev(const uint32_t* tree_heights, size_t n_proofs, const uint64_t* leaf_offsets,
                                       const uint64_t* d_leaf_indices, const uint64_t* d_leaf_digests, const uint64_t* auth_offsets,
                                       const uint64_t* d_auth_digests, uint64_t* d_paths_out, int* d_statuses, void* stream) try {
    return merkle_proofs_dev(tree_heights, n_proofs, leaf_offsets, d_leaf_indices, d_leaf_digests, auth_offsets, d_auth_digests, nullptr,
                             d_statuses, d_paths_out, true, 0, 0, static_cast<hipStream_t>(stream));
} TF_ABI_CATCH


int tf_mmr_append(uint64_t leaf_count, const uint64_t* old_peaks, const uint64_t* new_leafs, size_t k, uint64_t* new_peaks, uint64_t* proofs) try {
    return mmr_append_host(leaf_count, old_peaks, new_leafs, k, new_peaks, proofs);
} TF_ABI_CATCH
int tf_mmr_append_dev(uint64_t leaf_count, const uint64_t* d_old_peaks, const uint64_t* d_new_leafs, size_t k, uint64_t* d_new_peaks,
                      uint64_t* d_proofs, void* stream) try {
    return mmr_append_dev(leaf_count, d_old_peaks, d_new_leafs, k, d_new_peaks, d_proofs, static_cast<hipStream_t>(stream));
} TF_ABI_CATCH
int tf_mmr_bag_peaks(const uint64_t* leaf_counts, size_t n_acc, const uint64_t* peaks, uint64_t* out) try {
    return mmr_bag_peaks_host(leaf_counts, n_acc, peaks, out);
} TF_ABI_CATCH
int tf_mmr_bag_peaks_dev(const uint64_t* leaf_counts, size_t n_acc, const uint64_t* d_peaks, uint64_t* d_out, void* stream) try {
    return mmr_bag_peaks_dev(leaf_counts, n_acc, d_peaks, d_out, static_cast<hipStream_t>(stream));
} TF_ABI_CATCH
int tf_mmr_verify_membership_proofs(uint64_t leaf_count, const uint64_t* peaks, size_t n_peaks, size_t n_proofs, const uint64_t* leaf_indices,
                                    const uint64_t* leaf_digests, const uint64_t* path_offsets, const uint64_t* paths, int* statuses) try {
    return mmr_verify_host(leaf_count, peaks, n_peaks, n_proofs, leaf_indices, leaf_digests, path_offsets, paths, statuses);
} TF_ABI_CATCH
int tf_mmr_verify_membership_proofs_dev(uint64_t leaf_count, const uint64_t* d_peaks, size_t n_peaks, size_t n_proofs,
                                        const uint64_t* d_leaf_indices, const uint64_t* d_leaf_digests, const uint64_t* path_offsets,
                                        const uint64_t* d_paths, int* d_statuses, void* stream) try {
    return mmr_verify_dev(leaf_count, d_peaks, n_peaks, n_proofs, d_leaf_indices, d_leaf_digests, path_offsets, d_paths, d_statuses, 0,
                          static_cast<hipStream_t>(stream));
} TF_ABI_CATCH
int tf_mmr_batch_mutate_leafs(uint64_t leaf_count, uint64_t* peaks, size_t n_mut, const uint64_t* mut_indices, const uint64_t* new_leafs,
                              const uint64_t* mut_offsets, const uint64_t* mut_paths, size_t n_own, const uint64_t* own_indices,
                              const uint64_t* own_offsets, uint64_t* own_paths, int* modified) try {
    return mmr_mutate_host(leaf_count, peaks, n_mut, mut_indices, new_leafs, mut_offsets, mut_paths, n_own, own_indices, own_offsets, own_paths,
                           modified);
} TF_ABI_CATCH
int tf_mmr_batch_mutate_leafs_dev(uint64_t leaf_count, uint64_t* d_peaks, size_t n_mut, const uint64_t* mut_indices, const uint64_t* d_new_leafs,
                                  const uint64_t* mut_offsets, const uint64_t* d_mut_paths, size_t n_own, const uint64_t* own_indices,
                                  const uint64_t* own_offsets, uint64_t* d_own_paths, int* d_modified, void* stream) try {
    return mmr_mutate_dev(leaf_count, d_peaks, n_mut, mut_indices, d_new_leafs, mut_offsets, d_mut_paths, n_own, own_indices, own_offsets,
                          d_own_paths, d_modified, 0, 0, static_cast<hipStream_t>(stream));
} TF_ABI_CATCH
size_t tf_mmr_successor_proof_len(uint64_t leaf_count, uint64_t k) { return mmr_successor_proof_len(leaf_count, k); }  // bit arithmetic only
int tf_mmr_successor_proof_new(uint64_t leaf_count, const uint64_t* old_peaks, const uint64_t* new_leafs, size_t k, uint64_t* paths_out,
                               uint64_t* new_peaks) try {
    return mmr_successor_new_host(leaf_count, old_peaks, new_leafs, k, paths_out, new_peaks);
} TF_ABI_CATCH
int tf_mmr_successor_proof_new_dev(uint64_t leaf_count, const uint64_t* d_old_peaks, const uint64_t* d_new_leafs, size_t k, uint64_t* d_paths_out,
                                   uint64_t* d_new_peaks, void* stream) try {
    return mmr_successor_new_dev(leaf_count, d_old_peaks, d_new_leafs, k, d_paths_out, d_new_peaks, static_cast<hipStream_t>(stream));
} TF_ABI_CATCH
int tf_mmr_verify_successor_proofs(size_t n_proofs, const uint64_t* old_leaf_counts, const uint64_t* new_leaf_counts, const uint64_t* old_peak_offsets,
                                   const uint64_t* old_peaks, const uint64_t* new_peak_offsets, const uint64_t* new_peaks, const uint64_t* path_offsets,
                                   const uint64_t* paths, int* statuses) try {
    return mmr_successor_verify_host(n_proofs, old_leaf_counts, new_leaf_counts, old_peak_offsets, old_peaks, new_peak_offsets, new_peaks, path_offsets,
                                     paths, statuses);
} TF_ABI_CATCH
int tf_mmr_verify_successor_proofs_dev(size_t n_proofs, const uint64_t* old_leaf_counts, const uint64_t* new_leaf_counts,
                                       const uint64_t* old_peak_offsets, const uint64_t* d_old_peaks, const uint64_t* new_peak_offsets,
                                       const uint64_t* d_new_peaks, const uint64_t* path_offsets, const uint64_t* d_paths, int* d_statuses,
                                       void* stream) try {
    return mmr_successor_verify_dev(n_proofs, old_leaf_counts, new_leaf_counts, old_peak_offsets, d_old_peaks, new_peak_offsets, d_new_peaks,
                                    path_offsets, d_paths, d_statuses, 0, 0, 0, static_cast<hipStream_t>(stream));
} TF_ABI_CATCH
int tf_mmr_update_proofs_from_append(uint64_t leaf_count, const uint64_t* old_peaks, const uint64_t* new_leafs, size_t k, size_t n_own,
                                     const uint64_t* own_indices, const uint64_t* own_offsets, const uint64_t* own_paths, uint64_t* out_offsets,
                                     uint64_t* out_paths, size_t capacity_digests, int* modified, uint64_t* new_peaks) try {
    return mmr_update_proofs_host(leaf_count, old_peaks, new_leafs, k, n_own, own_indices, own_offsets, own_paths, out_offsets, out_paths,
                                  capacity_digests, modified, new_peaks);
} TF_ABI_CATCH
int tf_mmr_update_proofs_from_append_dev(uint64_t leaf_count, const uint64_t* d_old_peaks, const uint64_t* d_new_leafs, size_t k, size_t n_own,
                                         const uint64_t* own_indices, const uint64_t* own_offsets, const uint64_t* d_own_paths,
                                         uint64_t* out_offsets, uint64_t* d_out_paths, size_t capacity_digests, int* modified, uint64_t* d_new_peaks,
                                         void* stream) try {
    return mmr_update_proofs_dev(leaf_count, d_old_peaks, d_new_leafs, k, n_own, own_indices, own_offsets, d_own_paths, out_offsets, d_out_paths,
                                 capacity_digests, modified, d_new_peaks, 0, static_cast<hipStream_t>(stream));
} TF_ABI_CATCH

// ---- device-resident Tip5 sponges (tf_sponge.hip)
int tf_tip5_sponge_init(uint64_t* states, size_t count, int fixed_length) try {
    return sponge_init_host(states, count, fixed_length);
} TF_ABI_CATCH
int tf_tip5_sponge_init_dev(uint64_t* d_states, size_t count, int fixed_length, void* stream) try {
    return sponge_init_dev(d_states, count, fixed_length, static_cast<hipStream_t>(stream));
} TF_ABI_CATCH
int tf_tip5_sponge_absorb(uint64_t* states, size_t count, const uint64_t* input, size_t n_chunks) try {
    if (n_chunks > (size_t(1) << 56)) return TF_ERR_INVALID_ARGUMENT;
    return sponge_absorb_host(states, count, input, 10 * n_chunks, nullptr, false);
} TF_ABI_CATCH
int tf_tip5_sponge_absorb_dev(uint64_t* d_states, size_t count, const uint64_t* d_input, size_t n_chunks, void* stream) try {
    if (n_chunks > (size_t(1) << 56)) return TF_ERR_INVALID_ARGUMENT;
    return sponge_absorb_dev(d_states, count, d_input, 10 * n_chunks, nullptr, false, 0, static_cast<hipStream_t>(stream));
} TF_ABI_CATCH
int tf_tip5_sponge_pad_and_absorb_all(uint64_t* states, size_t count, const uint64_t* input, size_t len, const uint64_t* offsets) try {
    return sponge_absorb_host(states, count, input, len, offsets, true);
} TF_ABI_CATCH
int tf_tip5_sponge_pad_and_absorb_all_dev(uint64_t* d_states, size_t count, const uint64_t* d_input, size_t len, const uint64_t* offsets,
                                          void* stream) try {
    return sponge_absorb_dev(d_states, count, d_input, len, offsets, true, 0, static_cast<hipStream_t>(stream));
} TF_ABI_CATCH
int tf_tip5_sponge_squeeze(uint64_t* states, size_t count, size_t n_squeezes, uint64_t* out) try {
    return sponge_squeeze_host(states, count, n_squeezes, 10, out);
} TF_ABI_CATCH
int tf_tip5_sponge_squeeze_dev(uint64_t* d_states, size_t count, size_t n_squeezes, uint64_t* d_out, void* stream) try {
    return sponge_squeeze_dev(d_states, count, n_squeezes, 10, d_out, static_cast<hipStream_t>(stream));
} TF_ABI_CATCH
int tf_tip5_sponge_sample_scalars(uint64_t* states, size_t count, size_t num_elements, uint64_t* out) try {
    return sponge_squeeze_host(states, count, num_elements, 3, out);
} TF_ABI_CATCH
int tf_tip5_sponge_sample_scalars_dev(uint64_t* d_states, size_t count, size_t num_elements, uint64_t* d_out, void* stream) try {
    return sponge_squeeze_dev(d_states, count, num_elements, 3, d_out, static_cast<hipStream_t>(stream));
} TF_ABI_CATCH
int tf_tip5_sponge_sample_indices(uint64_t* states, size_t count, uint32_t upper_bound, size_t num_indices, uint32_t* out_u32) try {
    return sponge_indices_host(states, count, upper_bound, num_indices, out_u32);
} TF_ABI_CATCH
int tf_tip5_sponge_sample_indices_dev(uint64_t* d_states, size_t count, uint32_t upper_bound, size_t num_indices, uint32_t* d_out_u32,
                                      void* stream) try {
    return sponge_indices_dev(d_states, count, upper_bound, num_indices, d_out_u32, static_cast<hipStream_t>(stream));
} TF_ABI_CATCH

}  // extern "C"


