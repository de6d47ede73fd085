// tf_ntt.hip -- device context, table caches and run_ntt of libtf_hip.so: every launcher of ntt_kernels.h.  What a call runs is
// decided in tf_plan.hip (plan_ntt); run_ntt executes the plan.
//
// One process drives one or more MI355X devices; all state is per HIP device and guarded by a mutex,
// kernels are enqueued on the caller's stream, and nothing here synchronises the device except the
// one-off construction of a twiddle table.  There is no CPU fallback anywhere in this library.
#include "tf_temp.h"
#include "ntt_kernels.h"

namespace tfi {


// ------------------------------------------------------------------------------------ errors
thread_local std::string t_last_error;

int hip_fail(hipError_t e, const char* what, const char* file, int line) {
    char buf[512];
    snprintf(buf, sizeof(buf), "%s failed: %s (%s:%d)", what, hipGetErrorString(e), file, line);
    t_last_error = buf;
    (void)hipGetLastError();
    if (e == hipErrorNoDevice || e == hipErrorInvalidDevice || e == hipErrorInsufficientDriver || e == hipErrorNotInitialized)
        return TF_ERR_NO_DEVICE;
    if (e == hipErrorOutOfMemory || e == hipErrorMemoryAllocation) return TF_ERR_OUT_OF_MEMORY;
    return TF_ERR_HIP;
}

// what TF_ABI_CATCH (tf_guard.h) calls for an exception that reached an entry point
int abi_caught(const char* what, int status) noexcept {
    try {
        t_last_error = std::string("C++ exception at the C ABI: ") + (what ? what : "?");
    } catch (...) {  // (not even the message could be allocated: the status alone reports)
    }
    return status;
}

// ------------------------------------------------------------------------------------ field helpers (host)
// w_n = 7^((p-1)/n): equals every entry of PRIMITIVE_ROOTS (b_field_element.rs:43-78).
u64 root_of_unity_mont(int log_n) { return gl::mont_pow(gl::to_mont(7), (gl::P - 1) >> log_n); }

// ------------------------------------------------------------------------------------ per-device context
// (struct DeviceCtx: tf_internal.h)
// What the caches may pin for the life of the process; a table that does not fit becomes a stream-ordered temporary
// that is rebuilt per call and released after the pass that reads it.
constexpr size_t kPostCacheBudget = size_t(4) << 30;   // inter-pass twiddles (2^20: 8 MiB, 2^28: 2 GiB)
constexpr size_t kPowCacheBudget = size_t(1) << 30;    // offset^j tables (n_coeffs words each)

DeviceCtx g_ctx[kMaxDevices];

// Grids that are sized from the CU count (launch_rows32, mx_blocks) take the CURRENT device's: round 5 cached the count of whichever
// device made the first call, which on a heterogeneous or partitioned node sized every other device's grids wrong (only
// speed was at stake -- those kernels walk their work with a grid stride).
int device_cus() {
    static std::atomic<int> cus[kMaxDevices];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) {
        (void)hipGetLastError();
        return 256;
    }
    int n = cus[dev].load(std::memory_order_relaxed);
    if (n > 0) return n;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) {
        (void)hipGetLastError();
        n = 256;
    }
    cus[dev].store(n, std::memory_order_relaxed);
    return n;
}

int current_ctx(DeviceCtx** out) {
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0) {
        t_last_error = std::string("no usable HIP device: ") + hipGetErrorString(e);
        (void)hipGetLastError();
        return TF_ERR_NO_DEVICE;
    }
    int dev = 0;
    HIPCHK(hipGetDevice(&dev));
    if (dev < 0 || dev >= kMaxDevices) return TF_ERR_NO_DEVICE;
    *out = &g_ctx[dev];
    if (!g_ctx[dev].pool_ready.load(std::memory_order_acquire)) {
        // The library's stream-ordered temporaries come from a pool of its own:
        //  - freed blocks stay cached (release threshold: the default 0 hands memory back to the OS at every synchronisation,
        //    which makes per-call work space expensive);
        //  - hipMemPoolReuseFollowEventDependencies OFF.  The scratch cache below makes callers' streams wait on each other's
        //    events; with that reuse policy on, the runtime then hands a block freed on stream A to stream B while A's kernels
        //    still use it (ROCm 7.0: several host threads walking one zerofier tree on their own streams got wrong words about
        //    once in 10^4 calls, tools/stress_threads.py; every other policy combination ran clean, profiles/r03_pool_reuse.txt).
        // The application's default pool is left alone.
        std::lock_guard<std::mutex> lk(g_ctx[dev].mu);
        if (!g_ctx[dev].pool_ready.load(std::memory_order_relaxed)) {
            hipMemPoolProps props{};
            props.allocType = hipMemAllocationTypePinned;
            props.handleTypes = hipMemHandleTypeNone;
            props.location.type = hipMemLocationTypeDevice;
            props.location.id = dev;
            hipMemPool_t pool = nullptr;
            bool own = true;
            if (hipMemPoolCreate(&pool, &props) != hipSuccess) {
                // no pool of our own: the device's default one.  It belongs to the application, so only the ONE attribute correctness
                // needs is changed on it (the reuse policy below); its release threshold stays what the application set (tf_hip.h)
                pool = nullptr;
                own = false;
                (void)hipGetLastError();
                (void)hipDeviceGetDefaultMemPool(&pool, dev);
            }
            if (pool) {
                uint64_t thr = UINT64_MAX;
                if (own) (void)hipMemPoolSetAttribute(pool, hipMemPoolAttrReleaseThreshold, &thr);
                int follow = 0;
                (void)hipMemPoolSetAttribute(pool, hipMemPoolReuseFollowEventDependencies, &follow);
            }
            (void)hipGetLastError();
            g_ctx[dev].pool = pool;
            g_ctx[dev].pool_ready.store(true, std::memory_order_release);
        }
    }
    return TF_OK;
}

// Every stream-ordered temporary of the library: from the context's pool (pool_free_async gives it back, whatever the pool).
hipError_t pool_malloc_async(void** p, size_t bytes, hipStream_t stream, const char* what) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    hipMemPool_t pool = (dev >= 0 && dev < kMaxDevices && g_ctx[dev].pool_ready.load(std::memory_order_acquire)) ? g_ctx[dev].pool : nullptr;
    if (!pool) {  // (an entry point that allocates before it looked its context up)
        DeviceCtx* ctx = nullptr;
        if (current_ctx(&ctx) == TF_OK) pool = ctx->pool;
    }
    if (const int mode = (int)(g_temp_guard_state.load(std::memory_order_relaxed) & 0xFF)) return temp_guard_malloc(p, bytes, stream, what, pool, dev, mode);
    return pool ? hipMallocFromPoolAsync(p, bytes, pool, stream) : hipMallocAsync(p, bytes, stream);
}
hipError_t pool_free_async(void* p, hipStream_t stream) {
    if (g_temp_guard_state.load(std::memory_order_relaxed)) return temp_guard_free(p, stream);  // (the mode is on, or a guarded block is alive)
    return hipFreeAsync(p, stream);
}

// Work space between the passes of a multi-pass transform.  Round 1 took it from the stream-ordered pool on every call; a
// call of another size in between (bench.py's parity sample, a coset evaluation) splits the pooled block and the next full-size
// call then pays a fresh 2 GiB device allocation inside its timed path (observed: +120 ms on one step).  Blocks are therefore
// kept whole in a small per-device cache and handed from call to call with an event fence: release records an event on the
// releasing stream, the next taker's stream waits for it -- no host synchronisation, any mix of streams and host threads.
constexpr size_t kScratchCacheBytes = size_t(12) << 30;  // blocks beyond this are freed when they come back
int scratch_acquire(DeviceCtx* ctx, size_t bytes, hipStream_t stream, DeviceCtx::ScratchBlock* out, const char* what) {
    if (g_temp_guard_state.load(std::memory_order_relaxed) & 0xFF) {  // guard mode: a guarded pool block, no cache, no event
        *out = DeviceCtx::ScratchBlock{};
        out->bytes = bytes;
        const hipError_t e = pool_malloc_async(reinterpret_cast<void**>(&out->p), bytes, stream, what);
        if (e == hipSuccess) return TF_OK;
        out->p = nullptr;
        return hip_fail(e, (std::string("pool_malloc_async(") + what + ")").c_str(), __FILE__, __LINE__);
    }
    {
        std::lock_guard<std::mutex> lk(ctx->mu);
        int best = -1;
        for (int i = 0; i < (int)ctx->scratch_free.size(); ++i) {
            const auto& b = ctx->scratch_free[i];
            if (b.bytes >= bytes && (best < 0 || b.bytes < ctx->scratch_free[best].bytes)) best = i;
        }
        if (best >= 0 && ctx->scratch_free[best].bytes <= 4 * bytes + (size_t(64) << 20)) {  // do not pin a huge block under a small call
            *out = ctx->scratch_free[best];
            ctx->scratch_free.erase(ctx->scratch_free.begin() + best);
            ctx->scratch_bytes -= out->bytes;
        } else {
            out->p = nullptr;
        }
    }
    if (out->p) {
        hipError_t e = hipStreamWaitEvent(stream, out->ready, 0);
        if (e != hipSuccess) return hip_fail(e, "hipStreamWaitEvent(scratch)", __FILE__, __LINE__);
        return TF_OK;
    }
    out->bytes = bytes;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&out->p), bytes);
    if (e != hipSuccess) {
        // make room: drop every cached block (after their last users) and retry once
        std::vector<DeviceCtx::ScratchBlock> drop;
        {
            std::lock_guard<std::mutex> lk(ctx->mu);
            drop.swap(ctx->scratch_free);
            ctx->scratch_bytes = 0;
        }
        (void)hipGetLastError();
        for (auto& b : drop) {
            (void)hipEventSynchronize(b.ready);
            (void)hipEventDestroy(b.ready);
            (void)hipFree(b.p);
        }
        e = hipMalloc(reinterpret_cast<void**>(&out->p), bytes);
        if (e != hipSuccess) return hip_fail(e, "hipMalloc(ntt scratch)", __FILE__, __LINE__);
    }
    e = hipEventCreateWithFlags(&out->ready, hipEventDisableTiming);
    if (e != hipSuccess) {
        (void)hipFree(out->p);
        return hip_fail(e, "hipEventCreate(scratch)", __FILE__, __LINE__);
    }
    return TF_OK;
}
void scratch_release(DeviceCtx* ctx, DeviceCtx::ScratchBlock blk, hipStream_t stream) {
    if (!blk.p) return;
    if (!blk.ready) {  // taken in guard mode: checked and freed behind the launches on `stream`
        (void)pool_free_async(blk.p, stream);
        return;
    }
    if (hipEventRecord(blk.ready, stream) != hipSuccess) {  // cannot fence it: wait, then free
        (void)hipGetLastError();
        (void)hipStreamSynchronize(stream);
        (void)hipEventDestroy(blk.ready);
        (void)hipFree(blk.p);
        return;
    }
    // The block that comes back is the one most likely to be wanted again: it is always kept (unless it alone exceeds the budget) and the
    // OLDEST cached blocks make room for it.  Round 5 dropped the NEW block when the cache was full -- after sixteen blocks of other sizes
    // had accumulated (a long-lived process, the test suite) every release then waited for its stream and every acquire allocated from
    // the device, for ever (0.9 ms of host time per call in test_one_host_thread_round_robin_never_blocks).  The evicted blocks were
    // released long ago, so waiting for their events does not wait for anything.
    std::vector<DeviceCtx::ScratchBlock> evict;
    bool keep;
    {
        std::lock_guard<std::mutex> lk(ctx->mu);
        keep = blk.bytes <= kScratchCacheBytes;
        if (keep) {
            while (!ctx->scratch_free.empty() && (ctx->scratch_bytes + blk.bytes > kScratchCacheBytes || ctx->scratch_free.size() >= 16)) {
                evict.push_back(ctx->scratch_free.front());  // (release order = vector order: the front is the least recently used)
                ctx->scratch_bytes -= ctx->scratch_free.front().bytes;
                ctx->scratch_free.erase(ctx->scratch_free.begin());
            }
            ctx->scratch_free.push_back(blk);
            ctx->scratch_bytes += blk.bytes;
        }
    }
    for (auto& b : evict) {
        (void)hipEventSynchronize(b.ready);
        (void)hipEventDestroy(b.ready);
        (void)hipFree(b.p);
    }
    if (!keep) {
        (void)hipEventSynchronize(blk.ready);
        (void)hipEventDestroy(blk.ready);
        (void)hipFree(blk.p);
    }
}

// tf_release_caches: give back what the current device's context pins for speed -- the scratch blocks between transform passes
// (up to 12 GiB), the inter-pass twiddle tables (up to 4 GiB) and the coset power tables (up to 1 GiB).  Waits for the device
// first (tables may be read by kernels in flight); the next call rebuilds what it needs.  The small tables (inner twiddles,
// Tip5 constants) stay.
int release_caches(DeviceCtx* ctx) {
    HIPCHK(hipDeviceSynchronize());
    std::vector<DeviceCtx::ScratchBlock> drop;
    std::vector<u64*> tabs;
    {
        std::lock_guard<std::mutex> lk(ctx->mu);
        drop.swap(ctx->scratch_free);
        ctx->scratch_bytes = 0;
        for (auto it = ctx->tables.begin(); it != ctx->tables.end();) {
            if ((it->first >> 56) == 2 /* TAG_POST */) {
                tabs.push_back(it->second);
                it = ctx->tables.erase(it);
            } else {
                ++it;
            }
        }
        ctx->cached_post_bytes = 0;
        for (auto& kv : ctx->pow_tables) tabs.push_back(kv.second);
        ctx->pow_tables.clear();
        ctx->cached_pow_bytes = 0;
        for (auto& kv : ctx->scaled_post) tabs.push_back(kv.second);
        ctx->scaled_post.clear();
        ctx->cached_scaled_post_bytes = 0;
    }
    for (auto& b : drop) {
        (void)hipEventDestroy(b.ready);
        (void)hipFree(b.p);
    }
    for (u64* t : tabs) (void)hipFree(t);
    if (ctx->pool) (void)hipMemPoolTrimTo(ctx->pool, 0);  // the cached stream-ordered temporaries too
    (void)hipGetLastError();
    return TF_OK;
}

int upload_table(const std::vector<u64>& host, u64** dev) {
    u64* d = nullptr;
    HIPCHK(hipMalloc(&d, host.size() * sizeof(u64)));
    hipError_t e = hipMemcpy(d, host.data(), host.size() * sizeof(u64), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(d);
        return hip_fail(e, "hipMemcpy(table)", __FILE__, __LINE__);
    }
    *dev = d;
    return TF_OK;
}

// split powers: hi[i] = base^(i << h), lo[i] = base^i  (both Montgomery)
void split_powers(u64 base, int log_total, int* h_out, std::vector<u64>* hi, std::vector<u64>* lo) {
    int h = (log_total + 1) / 2;
    size_t nlo = size_t(1) << h, nhi = size_t(1) << (log_total - h);
    lo->resize(nlo);
    hi->resize(nhi);
    u64 acc = gl::ONE;
    for (size_t i = 0; i < nlo; ++i) {
        (*lo)[i] = acc;
        acc = gl::mont_mul(acc, base);
    }
    u64 step = acc;  // base^(2^h)
    acc = gl::ONE;
    for (size_t i = 0; i < nhi; ++i) {
        (*hi)[i] = acc;
        acc = gl::mont_mul(acc, step);
    }
    *h_out = h;
}

// (table keys: tf_internal.h)

// inner[g*32 + k1] = w_R^(+-g*k1) * (scale_log_n ? n^-1 : 1),  R = 32 << p2
// pre = 2 (a = 10 only): the pass is a 2048-point DFT run as two 1024-point workgroups per tile (ntt_kernels.h, PRE2); two tables
// back to back, table q: inner[q * 1024 + g*32 + k1] = w_1024^(+-g k1) * w_2048^(+-q g) * scale -- the part of the radix-2 stage's
// twiddle that depends on g rides on the inner twiddle.
int get_inner_table(DeviceCtx* ctx, int a, bool inverse, int scale_log_n, const u64** out, int pre = 1) {
    const int p2 = a - 5;
    if (p2 == 0 && scale_log_n == 0) {
        *out = nullptr;
        return TF_OK;
    }
    const u64 key = make_key(TAG_INNER, a, inverse, scale_log_n, pre > 1 ? pre - 1 : 0);  // (pre = 2 keeps its round-3 key)
    std::lock_guard<std::mutex> lk(ctx->mu);
    const int P2 = 1 << p2;
    auto it = ctx->tables.find(key);
    if (it != ctx->tables.end()) {
        *out = it->second;
        return TF_OK;
    }
    u64 w = root_of_unity_mont(a);
    if (inverse) w = gl::mont_inverse(w);
    u64 scale = gl::ONE;
    if (scale_log_n) scale = gl::mont_inverse(gl::to_mont(u64(1) << scale_log_n));
    std::vector<u64> t(size_t(P2) * 32);
    u64 wg = gl::ONE;  // w^g
    for (int g = 0; g < P2; ++g) {
        u64 acc = scale;
        for (int k = 0; k < 32; ++k) {
            t[size_t(g) * 32 + k] = acc;
            acc = gl::mont_mul(acc, wg);
        }
        wg = gl::mont_mul(wg, w);
    }
    if (pre > 1) {
        u64 wp = root_of_unity_mont(a + 1);  // w_{R pre}
        if (inverse) wp = gl::mont_inverse(wp);
        t.resize(size_t(P2) * 32 * pre);
        u64 wq = wp;  // w_{R pre}^q
        for (int q = 1; q < pre; ++q) {
            u64 wqg = gl::ONE;  // w_{R pre}^(q g)
            for (int g = 0; g < P2; ++g) {
                for (int k = 0; k < 32; ++k) t[size_t(q) * P2 * 32 + size_t(g) * 32 + k] = gl::mont_mul(t[size_t(g) * 32 + k], wqg);
                wqg = gl::mont_mul(wqg, wq);
            }
            wq = gl::mont_mul(wq, wp);
        }
    }
    u64* d = nullptr;
    int rc = upload_table(t, &d);
    if (rc) return rc;
    ctx->tables[key] = d;
    *out = d;
    return TF_OK;
}

// T[k*B + b] = w_M^(+-k*b), k < R = 2^a, b < B = M / R
// Inter-pass twiddles T[k * B + b] = w_M^(k * b), M = 2^log_m = R * B.  Tables up to 2^28 entries (2 GiB) are built once
// and cached; larger ones (single transforms of 2^29 .. 2^31 points) are stream-ordered temporaries:
// *own takes them and gives them back after the passes that read them.
constexpr int kMaxCachedPostLog = 28;
// Tables of up to 2^22 words (32 MiB) are cached whatever the budget says: round 6 found that a process which had once transformed
// 2^27 / 2^28 points (two tables of 1-2 GiB) ran every LATER shape on temporaries -- each call then built its table, and the builder of
// that time uploaded host-computed split tables and waited for the stream (0.85 ms of host time per call of a 2^16-point coset
// evaluation in tests/test_gpu_parity.py::test_one_host_thread_round_robin_never_blocks).  Temporaries are now built entirely on the
// caller's stream (their split tables by square-and-multiply on the device) and nothing waits.
constexpr int kAlwaysCachedPostLog = 22;
int get_post_table(DeviceCtx* ctx, int log_m, int a, bool inverse, hipStream_t stream, const u64** out, DevTemp* own) {
    bool temp = log_m > kMaxCachedPostLog || g_force_temp_tables.load(std::memory_order_relaxed);  // (tf_debug_force_temp_tables)
    const u64 key = make_key(TAG_POST, log_m, a, inverse, 0);
    std::unique_lock<std::mutex> lk(ctx->mu);
    if (!temp) {
        auto it = ctx->tables.find(key);
        if (it != ctx->tables.end()) {
            *out = it->second;
            return TF_OK;
        }
        if (log_m > kAlwaysCachedPostLog && ctx->cached_post_bytes + (sizeof(u64) << log_m) > kPostCacheBudget) temp = true;  // over budget: temporary
    }
    u64 w = root_of_unity_mont(log_m);
    if (inverse) w = gl::mont_inverse(w);
    const long long M = 1ll << log_m, R = 1ll << a, B = M / R;
    const int threads = 256;
    const long long blocks = (M + threads - 1) / threads;
    u64* d = nullptr;
    if (temp) {
        lk.unlock();
        // hi[i] = w^(i << h), lo[i] = w^i (split_powers), computed ON the device and freed behind the build, all on the caller's stream
        const int h = (log_m + 1) / 2;
        const long long nlo = 1ll << h, nhi = 1ll << (log_m - h);
        u64* d_split = nullptr;
        // (the split powers and the table: always taken together, one label)
        hipError_t e = pool_malloc_async(reinterpret_cast<void**>(&d_split), size_t(nlo + nhi) * sizeof(u64), stream, "temporary twiddle table");
        if (e == hipSuccess) e = pool_malloc_async(reinterpret_cast<void**>(&d), size_t(M) * sizeof(u64), stream, "temporary twiddle table");
        if (e != hipSuccess) {
            if (d_split) (void)pool_free_async(d_split, stream);
            return hip_fail(e, "pool_malloc_async(temporary twiddle table)", __FILE__, __LINE__);
        }
        hipLaunchKernelGGL(tfk::build_split_powers_kernel, dim3((unsigned)((nhi + 255) / 256)), dim3(256), 0, stream, d_split, w, h, nhi);
        hipLaunchKernelGGL(tfk::build_split_powers_kernel, dim3((unsigned)((nlo + 255) / 256)), dim3(256), 0, stream, d_split + nhi, w, 0, nlo);
        hipLaunchKernelGGL(tfk::build_post_tw_kernel, dim3((unsigned)blocks), dim3(threads), 0, stream, d, d_split, d_split + nhi, h, R, B);
        e = hipGetLastError();
        (void)pool_free_async(d_split, stream);
        if (e != hipSuccess) {
            (void)pool_free_async(d, stream);
            return hip_fail(e, "build_post_tw_kernel (temporary)", __FILE__, __LINE__);
        }
        own->adopt(d);
        *out = d;
        return TF_OK;
    }
    int h = 0;
    std::vector<u64> hi, lo;
    split_powers(w, log_m, &h, &hi, &lo);
    u64 *d_hi = nullptr, *d_lo = nullptr;
    int rc = upload_table(hi, &d_hi);
    if (rc) return rc;
    rc = upload_table(lo, &d_lo);
    if (rc) {
        (void)hipFree(d_hi);
        return rc;
    }
    hipError_t e = hipMalloc(&d, size_t(M) * sizeof(u64));
    if (e != hipSuccess) {
        (void)hipFree(d_hi);
        (void)hipFree(d_lo);
        return hip_fail(e, "hipMalloc(twiddle table)", __FILE__, __LINE__);
    }
    hipLaunchKernelGGL(tfk::build_post_tw_kernel, dim3((unsigned)blocks), dim3(threads), 0, hipStream_t(0), d, d_hi, d_lo, h, R, B);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(hipStream_t(0));
    (void)hipFree(d_hi);
    (void)hipFree(d_lo);
    if (e != hipSuccess) {
        (void)hipFree(d);
        return hip_fail(e, "build_post_tw_kernel", __FILE__, __LINE__);
    }
    ctx->tables[key] = d;
    ctx->cached_post_bytes += size_t(M) * sizeof(u64);
    *out = d;
    return TF_OK;
}

// tables of ntt_block_kernel (2^11 <= n <= 2^14): tw1[q * REST + rest] = w_n^(+-q * rest), tw2[k2 * P3 + j3] =
// w_{32 P3}^(+-k2 * j3) (* n^-1 for the inverse)
int get_block_tables(DeviceCtx* ctx, int log_n, bool inverse, const u64** tw1, const u64** tw2) {
    const u64 key1 = make_key(TAG_BLOCK1, log_n, inverse, 0, 0), key2 = make_key(TAG_BLOCK2, log_n, inverse, 0, 0);
    std::lock_guard<std::mutex> lk(ctx->mu);
    auto i1 = ctx->tables.find(key1), i2 = ctx->tables.find(key2);
    if (i1 != ctx->tables.end() && i2 != ctx->tables.end()) {
        *tw1 = i1->second;
        *tw2 = i2->second;
        return TF_OK;
    }
    const int n = 1 << log_n, rest_n = n / 32, p3 = n / 1024;
    u64 w = root_of_unity_mont(log_n);
    if (inverse) w = gl::mont_inverse(w);
    std::vector<u64> t1((size_t)n), t2((size_t)32 * p3);
    u64 wq = gl::ONE;  // w^q
    for (int q = 0; q < 32; ++q) {
        u64 acc = gl::ONE;
        for (int r = 0; r < rest_n; ++r) {
            t1[size_t(q) * rest_n + r] = acc;
            acc = gl::mont_mul(acc, wq);
        }
        wq = gl::mont_mul(wq, w);
    }
    const u64 w32 = gl::mont_pow(w, 32);  // w_{n / 32} = w_{32 P3}
    const u64 scale = inverse ? gl::mont_inverse(gl::to_mont(u64(n))) : gl::ONE;
    u64 wk = gl::ONE;  // w32^k2
    for (int k2 = 0; k2 < 32; ++k2) {
        u64 acc = scale;
        for (int j3 = 0; j3 < p3; ++j3) {
            t2[size_t(k2) * p3 + j3] = acc;
            acc = gl::mont_mul(acc, wk);
        }
        wk = gl::mont_mul(wk, w32);
    }
    u64 *d1 = nullptr, *d2 = nullptr;
    int rc = upload_table(t1, &d1);
    if (rc) return rc;
    rc = upload_table(t2, &d2);
    if (rc) {
        (void)hipFree(d1);
        return rc;
    }
    ctx->tables[key1] = d1;
    ctx->tables[key2] = d2;
    *tw1 = d1;
    *tw2 = d2;
    return TF_OK;
}

// stage tables of the reference (ntt.rs:309-324) for n <= 16
int get_tiny_table(DeviceCtx* ctx, int log_n, bool inverse, const u64** out) {
    const u64 key = make_key(TAG_TINY, log_n, inverse, 0, 0);
    std::lock_guard<std::mutex> lk(ctx->mu);
    auto it = ctx->tables.find(key);
    if (it != ctx->tables.end()) {
        *out = it->second;
        return TF_OK;
    }
    const int n = 1 << log_n;
    std::vector<u64> t(std::max(1, n - 1), gl::ONE);
    u64 w = root_of_unity_mont(log_n);
    if (inverse) w = gl::mont_inverse(w);
    for (int i = 0; i < log_n; ++i) {
        const int m = 1 << i;
        u64 wm = gl::mont_pow(w, u64(n / (2 * m)));
        u64 acc = gl::ONE;
        for (int j = 0; j < m; ++j) {
            t[m - 1 + j] = acc;
            acc = gl::mont_mul(acc, wm);
        }
    }
    u64* d = nullptr;
    int rc = upload_table(t, &d);
    if (rc) return rc;
    ctx->tables[key] = d;
    *out = d;
    return TF_OK;
}

// offset^j, j < n  (the power chain of Polynomial::scale, polynomial.rs:766-771): the builder of the CACHED tables (PowTable::acquire)
int build_pow_tables(u64 offset_raw, u64 w, size_t cosets, size_t n, u64* d, hipStream_t s) {
    // table c (c < cosets) = powers of base_c = offset * w^c: out[c * n + j] = base_c^j = HI_c[j >> h] * LO_c[j & (2^h - 1)].
    // The split tables of ALL cosets go up in one allocation and ONE kernel fills every table (grid.y = coset).
    const int log_total = std::max(1, ilog2(n));
    int h = 0;
    std::vector<u64> hi, lo, all;
    size_t nhi = 0, nlo = 0;
    u64 base = offset_raw;
    for (size_t c = 0; c < cosets; ++c) {
        split_powers(base, log_total, &h, &hi, &lo);
        nhi = hi.size(), nlo = lo.size();
        if (c == 0) all.reserve(cosets * (nhi + nlo));
        all.insert(all.end(), hi.begin(), hi.end());
        all.insert(all.end(), lo.begin(), lo.end());
        base = gl::mont_mul(base, w);
    }
    u64* d_all = nullptr;
    int rc = upload_table(all, &d_all);
    if (rc) return rc;
    const int threads = 256;
    const long long blocks = ((long long)n + threads - 1) / threads;
    if (n) {
        hipLaunchKernelGGL(tfk::build_pow_tables_kernel, dim3((unsigned)blocks, (unsigned)cosets), dim3(threads), 0, s, d, d_all, h,
                           (long long)n, (long long)nhi, (long long)nlo);
    }
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(s);  // the split tables are freed below; the build kernel is microseconds
    (void)hipFree(d_all);
    if (e != hipSuccess) return hip_fail(e, "build_pow_tables_kernel", __FILE__, __LINE__);
    return TF_OK;
}

// (class PowTable: tf_internal.h)  A cached table is never freed while another thread may use it; a temporary is private to its owner.
int PowTable::acquire(u64 offset_raw, size_t n, size_t cosets, int log_order) {
    release();
    std::unique_lock<std::mutex> lk(ctx_->mu);
    auto key = std::make_pair(offset_raw, u64(n) | (u64(cosets) << 40) | (u64(log_order) << 56));
    auto it = ctx_->pow_tables.find(key);
    if (it != ctx_->pow_tables.end()) {
        table_ = it->second;
        return TF_OK;
    }
    const size_t words = std::max<size_t>(n * cosets, 1);
    const bool cacheable = ctx_->pow_tables.size() < 16 && ctx_->cached_pow_bytes + words * sizeof(u64) <= kPowCacheBudget;
    const u64 w = cosets > 1 ? root_of_unity_mont(log_order) : gl::ONE;
    if (cacheable) {
        u64* d = nullptr;
        HIPCHK(hipMalloc(&d, words * sizeof(u64)));
        int rc = build_pow_tables(offset_raw, w, cosets, n, d, 0);
        if (rc) {
            (void)hipFree(d);
            return rc;
        }
        ctx_->pow_tables[key] = d;
        ctx_->cached_pow_bytes += words * sizeof(u64);
        table_ = d;
        return TF_OK;
    }
    lk.unlock();  // a temporary is private to this call: build it without holding the device context
    // ... and without leaving the caller's stream.  Round 6 (tests/test_gpu_parity.py::test_one_host_thread_round_robin_never_blocks, a
    // process whose cache is full): (1) the split-table builder uploads host-built tables and WAITS for the stream -- the temporary is
    // built by one kernel instead, every word by square-and-multiply; (2) hipFreeAsync of a pool block behind the launches blocked the
    // host for the depth of the queue (0.8-1.0 ms per call, measured around that one call) when several streams share the pool -- the
    // temporary therefore lives in a block of the scratch cache (hipMalloc'ed blocks handed on with event fences, no stream-ordered free).
    int rc = scratch_acquire(ctx_, words * sizeof(u64), s_, &blk_, "temporary power table");
    if (rc) {
        blk_ = DeviceCtx::ScratchBlock{};  // (nothing of ours to give back)
        return rc;
    }
    tfk::PowBases pb{};
    u64 base = offset_raw;
    for (size_t c = 0; c < cosets && c < 64; ++c) {
        pb.base[c] = base;
        base = gl::mont_mul(base, w);
    }
    if (n) hipLaunchKernelGGL(tfk::build_pow_tables_direct_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)cosets), dim3(256), 0, s_, blk_.p, pb, (long long)n);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        release();
        return hip_fail(e, "build_pow_tables_direct_kernel", __FILE__, __LINE__);
    }
    table_ = blk_.p;
    return TF_OK;
}

// The inter-pass table of a forward first pass with the COLUMN part of a coset evaluation's scaling folded in: T'[k B + b] =
// w_M^(k b) * offset^b (ntt_col2048_kernel: the factor is constant along a column, so it commutes with the column pass).  One table per
// (offset, M, R); at most four / kScaledPostBudget bytes stay cached (a prover evaluates on one coset), anything beyond is a
// stream-ordered temporary that *own gives back after the pass.  Built on `stream`; the first build of a cached table synchronises it once.
constexpr size_t kScaledPostBudget = size_t(512) << 20;
int get_scaled_post_table(DeviceCtx* ctx, int log_m, int a, u64 offset_raw, hipStream_t stream, const u64** out, DevTemp* own) {
    const auto key = std::make_pair(offset_raw, (u64(log_m) << 8) | u64(a));
    const bool forced = g_force_temp_tables.load(std::memory_order_relaxed);  // (tf_debug_force_temp_tables: the uncached route)
    if (!forced) {
        std::lock_guard<std::mutex> lk(ctx->mu);
        auto it = ctx->scaled_post.find(key);
        if (it != ctx->scaled_post.end()) {
            *out = it->second;
            return TF_OK;
        }
    }
    const long long M = 1ll << log_m, B = M >> a;
    const u64* T = nullptr;
    DevTemp t_own(stream);  // (given back behind the build below)
    TRY(get_post_table(ctx, log_m, a, false, stream, &T, &t_own));
    PowTable S(ctx, stream);  // (given back behind the build below)
    TRY(S.acquire(offset_raw, (size_t)B));
    bool cache;
    {
        std::lock_guard<std::mutex> lk(ctx->mu);
        cache = !forced && ctx->scaled_post.size() < 4 && ctx->cached_scaled_post_bytes + size_t(M) * sizeof(u64) <= kScaledPostBudget;
    }
    u64* d = nullptr;
    hipError_t e = cache ? hipMalloc(&d, size_t(M) * sizeof(u64))
                         : pool_malloc_async(reinterpret_cast<void**>(&d), size_t(M) * sizeof(u64), stream, "temporary scaled twiddle table");
    if (e == hipSuccess) {
        hipLaunchKernelGGL(tfk::scale_post_tw_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, stream, d, T, S.get(), B, M);
        e = hipGetLastError();
        if (e == hipSuccess && cache) e = hipStreamSynchronize(stream);  // other streams may use the cached table from now on
    }
    S.release();
    if (e != hipSuccess) {
        if (d) { if (cache) (void)hipFree(d); else (void)pool_free_async(d, stream); }
        return hip_fail(e, "scale_post_tw_kernel", __FILE__, __LINE__);
    }
    if (cache) {
        std::lock_guard<std::mutex> lk(ctx->mu);
        auto it = ctx->scaled_post.find(key);
        if (it != ctx->scaled_post.end()) {  // another host thread built it meanwhile
            (void)hipFree(d);
            d = it->second;
        } else {
            ctx->scaled_post[key] = d;
            ctx->cached_scaled_post_bytes += size_t(M) * sizeof(u64);
        }
    } else {
        own->adopt(d);
    }
    *out = d;
    return TF_OK;
}

// ------------------------------------------------------------------------------------ NTT pass launches
// (which passes a call runs: plan_ntt, tf_plan.hip; here a planned pass becomes kernel arguments and a launch)
struct Launch {
    tfk::NttPassArgs a;
    unsigned tiles;
    unsigned threads;
    size_t lds_bytes;
    bool bad_geometry = false;  // planner self-check failed: launch_pass refuses the launch
    bool narrow = false;        // planned with the narrow tiles of a small call (NttPlan::narrow): the generic last pass
};

int pad_to_residue(int base, int residue) {  // smallest s >= base with s == residue (mod 32)
    int r = ((residue - base) % 32 + 32) % 32;
    return base + r;
}

// Words per exchange round of a workgroup of g.wg threads (NttPlan::wg: 512, or 256 for the narrow tiles; tf_plan.hip has the
// geometry and its measurements)
int round_elems(const NttPlan& g) { return g.wg * 16; }

// thread / LDS geometry shared by all pass types: nc columns, exchanged in rounds of cpr columns
void finish_geometry(Launch* l, int nc, int p2, const NttPlan& g) {
    tfk::NttPassArgs& A = l->a;
    const int P2 = 1 << p2, R = 32 << p2;
    A.p2 = p2;
    A.nc = nc;
    A.cpr = std::max(1, std::min(nc, round_elems(g) / R));
    A.nrounds = (nc + A.cpr - 1) / A.cpr;
    A.s2 = A.cpr;
    A.s3 = 1;
    A.s1 = pad_to_residue(P2 * A.cpr, A.cpr % 32);  // consecutive k1 rows land cpr banks apart: conflict-free reads
    l->threads = (unsigned)(nc * P2);
    l->narrow = g.narrow;
    l->lds_bytes = size_t(32) * A.s1 * sizeof(u64);
    A.nc_magic = nc > 1 ? (u32)((u64(1) << 32) / (u64)nc + 1) : 0;  // umulhi(t, magic) == t / nc (nc == 1: kernel uses t)
    for (u32 t = 0; t < l->threads; ++t) {
        const u32 q = (u32)(((u64)t * A.nc_magic) >> 32);
        if (nc != 1 && q != t / (u32)nc) l->bad_geometry = true;  // never observed: the magic is exact for t < 1024, nc <= 1024
    }
}

// Column pass: view [batch][outer][R][B*L words]; DFT along R for each of the B*L word-columns; same position in and out.
// pre2: a = 11, run as pairs of 1024-point halves (ntt_kernels.h, PRE2): the kernel radix is 1024, the rows of a column 2048.
Launch plan_column_pass(const NttPlan& g, const u64* in, u64* out, long long in_bs, long long out_bs, size_t batch, long long outer, int a,
                        long long B, int L, bool pre2 = false) {
    Launch l{};
    tfk::NttPassArgs& A = l.a;
    const int p2 = (pre2 ? a - 1 : a) - 5, P2 = 1 << p2;
    const long long R = 1ll << a, Bw = B * L;
    int nc = (int)std::min<long long>(std::max(1, g.wg / P2), Bw);
    A.in = in;
    A.out = out;
    A.L = L;
    A.d1 = (u32)outer;
    A.d2 = (u32)((Bw + nc - 1) / nc);
    A.d01 = (u32)(batch * outer);
    A.ib0 = in_bs;
    A.ib1 = R * Bw;
    A.ib2 = nc;
    A.ob0 = out_bs;
    A.ob1 = R * Bw;
    A.ob2 = nc;
    A.in_cs_hi = L;
    A.out_cs_hi = L;
    A.in_rs = Bw;
    A.out_rs = Bw;
    A.tw_rs = B;
    A.ps_rs = B;
    A.ps_col = 1;
    A.col_limit = (int)Bw;
    A.n_coeffs = -1;
    A.n_out = -1;
    {
        const int G = (nc * (int)sizeof(u64) < 128) ? 2 : 1;  // pair tiles narrower than a 128-byte line
        A.xcd_order = (A.d2 % (8 * G) == 0) ? G : ((A.d2 % 8 == 0) ? 1 : 0);
        // table slice of one column tile = R rows x nc words; an XCD owns d2 / 8 column tiles and has a 4 MiB L2
        if (A.xcd_order) A.xcd_colfast = (size_t(A.d2 / 8) * size_t(R) * nc * sizeof(u64) <= (size_t(2) << 20)) ? 1 : 0;
    }
    finish_geometry(&l, nc, p2, g);
    l.tiles = (unsigned)(batch * outer * A.d2);
    if (pre2) {
        A.out_rs = 2 * Bw;  // kernel row k' of half h is row 2 k' + h of the 2048
        A.tw_rs = 2 * B;
        A.pre2_in_off = 1024 * Bw;
        A.pre2_out_off = Bw;
        A.pre2_tw_off = B;
        A.pre2_map = (l.tiles % 8 == 0) ? 1 : 2;
        l.tiles *= 2;
    }
    return l;
}

// The R = 1024 instantiations address memory through buffer resources: resource base + 32-bit per-thread offset + 32-bit
// per-slot offset (ntt_kernels.h, buf_load).  A thread's row offset is at most 31 rows, a slot's at most 992 rows: with
// row strides of rs words everything stays below 2^32 bytes when 1024 * rs * 8 (+ the tile's column span) does.
bool fits_buffer_offsets(const Launch& l) {
    const unsigned long long lim = 1ull << 32;
    const unsigned long long col_span = (unsigned long long)std::max(l.a.nc, 16) * 8ull * 3ull;  // columns of a tile, any limb
    const auto ok = [&](long long rs_words, long long cs_hi_words, unsigned long long rows = 1024ull) {
        const unsigned long long cols = (unsigned long long)(cs_hi_words < 0 ? 0 : cs_hi_words) * 8ull * 16ull;  // ch < 16 columns of a tile
        return rows * (unsigned long long)rs_words * 8ull + cols + col_span < lim;
    };
    // (a PRE2 launch also reads the partner rows, 1024 rows further; the one-workgroup 2048-point column pass, p2 = 6, spans 2048 rows
    //  on every side)
    const unsigned long long rows = l.a.p2 == 6 ? 2048ull : 1024ull;
    return ok(l.a.in_rs, l.a.in_cs_hi, l.a.pre2_map ? 2048ull : rows) && ok(l.a.out_rs, l.a.out_cs_hi, rows) && ok(l.a.tw_rs, 0, rows);
}

// rows (independent DFTs) per tile for the passes whose columns are whole rows of elements
int rows_per_tile(const NttPlan& g, int P2, int L, long long limit) {
    int nc_max = std::max(1, g.wg / P2);
    int T = std::max(1, nc_max / L);
    return (int)std::min<long long>(T, limit);
}

// Last pass of a multi-pass transform: rows (k1, rho) of R contiguous elements; DFT along the row;
// output element k of row (k1, rho) goes to  k1 + N1 * (rho + Q * k)  (digit reversal = natural order).
// A tile is T consecutive k1: its T*L word-columns are contiguous on the OUTPUT side.
// split = N2 > 0 (four-pass transforms, one polynomial per launch): rho = k2 * (Q / N2) + k3 on the input side but
// k2 + N2 * k3 on the output side; the kernel's batch index carries k2 and its rho index carries k3.
// words > 0: word-granular tiles of `words` adjacent output WORDS (whole 128-byte lines) instead of T whole elements; for
// XFieldElement rows (24-byte elements) a tile then starts and ends inside an element (NttPassArgs::wtiles).
Launch plan_transpose_pass(const NttPlan& g, const u64* in, u64* out, long long in_bs, long long out_bs, size_t batch, int a, long long N1,
                           long long Q, int L, long long split = 0, int words = 0, int pre = 1) {
    Launch l{};
    tfk::NttPassArgs& A = l.a;
    const int p2 = a - (pre == 2 ? 1 : 0) - 5, P2 = 1 << p2;
    const long long R = 1ll << a;  // elements per row (pre = 2: 2048, transformed as two interleaved 1024-point classes)
    int T = rows_per_tile(g, P2, L, N1);
    {
        // the kernel addresses its loads as uniform 64-bit base + 32-bit per-thread byte offset; the offset spans the
        // tile's T rows, Q * R * L words apart: keep it below 2^32 (only binds for n = 2^31)
        const long long row_words = Q * R * L;
        const long long t_max = ((1ll << 29) - (1ll << 16)) / row_words;
        if (t_max < T) T = (int)std::max<long long>(1, t_max);
        if (t_max < words / L + 2) words = 0;  // rows a word-granular tile can span
    }
    const int nc = words ? words : T * L;
    A.in = in;
    A.out = out;
    A.L = L;
    A.d1 = (u32)Q;
    A.d2 = words ? (u32)((N1 * L + words - 1) / words) : (u32)((N1 + T - 1) / T);
    A.wtiles = words ? 1 : 0;
    A.d01 = (u32)(batch * Q);
    A.ib0 = in_bs;
    A.ib1 = R * L;
    A.ib2 = (long long)T * Q * R * L;  // (ib2 / ob2 / js_i2 are not used by word-granular tiles)
    A.in_cs_hi = Q * R * L;
    A.in_rs = L;
    A.ob0 = out_bs;
    A.ob1 = N1 * L;
    A.ob2 = (long long)T * L;
    A.out_cs_hi = L;
    A.out_rs = N1 * Q * L;
    A.col_limit = (int)(N1 * L);
    A.n_coeffs = -1;
    A.n_out = -1;
    A.js_i1 = N1;
    A.js_i2 = T;
    A.js_c = 1;
    A.js_k = N1 * Q;
    A.xcd_order = (nc * (int)sizeof(u64) < 128 && A.d2 % 16 == 0) ? 2 : 0;  // output segments narrower than a line: pair them
    if (split) {
        const long long N3 = Q / split;
        A.d1 = (u32)N3;
        A.ib0 = N3 * R * L;
        A.ob0 = N1 * L;
        A.ob1 = N1 * split * L;
        A.js_i0 = N1;
        A.js_i1 = N1 * split;
        batch = 1;
    }
    finish_geometry(&l, nc, p2, g);
    l.tiles = (unsigned)(batch * Q * A.d2);
    if (pre > 1) {
        A.pre2_in_off = 1024 * L;
        A.pre2_out_off = A.out_rs;  // output k = pre k' + q
        A.pre2_js_off = A.js_k;
        A.out_rs *= pre;
        A.js_k *= pre;
        A.pre2_map = (l.tiles % 8 == 0) ? 1 : 2;
        l.tiles *= (unsigned)pre;
    }
    return l;
}

// Single pass (32 <= n <= 1024): a tile is T whole transforms, output in natural order at the same place.
Launch plan_row_pass(const NttPlan& g, const u64* in, u64* out, long long in_bs, long long out_bs, size_t batch, int a, int L) {
    Launch l{};
    tfk::NttPassArgs& A = l.a;
    const int p2 = a - 5, P2 = 1 << p2;
    const int T = rows_per_tile(g, P2, L, (long long)batch);
    const int nc = T * L;
    A.in = in;
    A.out = out;
    A.L = L;
    A.d1 = 1;
    A.d2 = (u32)((batch + T - 1) / T);
    A.d01 = 1;
    A.ib2 = (long long)T * in_bs;
    A.ob2 = (long long)T * out_bs;
    A.in_cs_hi = in_bs;
    A.out_cs_hi = out_bs;
    A.in_rs = L;
    A.out_rs = L;
    A.col_limit = (int)std::min<size_t>(batch * L, 0x7fffffff);
    A.ps_rs = 1;
    A.ps_col = 0;
    A.n_coeffs = -1;
    A.n_out = -1;
    A.js_k = 1;  // single pass: output element index = k
    A.xcd_order = 0;
    finish_geometry(&l, nc, p2, g);
    if (p2 >= 1) {
        // rows are contiguous: put the lanes along the row (8 * P2-byte pieces become P2 times longer).  Exchange layout
        // idx = k1 * s1 + cc * P2 + g with s1 = 1 (mod 32): a half-wave writes 32 consecutive words and reads
        // g' * s1 + cc * P2 = g' + cc * P2 (mod 32), all different.
        A.gfast = 1;
        A.s2 = 1;
        A.s3 = P2;
        A.s1 = pad_to_residue(P2 * A.cpr, 1);
        l.lds_bytes = size_t(32) * A.s1 * sizeof(u64);
    }
    l.tiles = A.d2;
    return l;
}

// One hipFuncSetAttribute per (kernel instantiation, device) to open the dynamic LDS above 48 KiB.  First use is serialised
// under a lock: a launch of the same function from another host thread while the attribute is being set is not safe (seen as a
// rare failure of the four-threads-one-tree test when a kernel's first use fell inside the threaded section).
std::mutex g_func_attr_mutex;
int ensure_dynamic_lds(const void* fn, int bytes, std::atomic<unsigned long long>& done_mask) {
    int dev = 0;
    HIPCHK(hipGetDevice(&dev));
    const unsigned long long bit = 1ull << (dev & 63);
    if (done_mask.load(std::memory_order_acquire) & bit) return TF_OK;
    std::lock_guard<std::mutex> guard(g_func_attr_mutex);
    if (done_mask.load(std::memory_order_acquire) & bit) return TF_OK;
    HIPCHK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    done_mask.fetch_or(bit, std::memory_order_release);
    return TF_OK;
}

template <bool INV, int SCALE, bool LAST1024 = false, bool R1024 = false, bool COL = false, bool PRE2 = false>
int launch_pass_t(const Launch& l, hipStream_t stream) {
    // one attribute call per (instantiation, device): the kernels use up to the full 160 KiB of dynamic LDS
    static std::atomic<unsigned long long> done_mask{0};
    if (int rc_attr = ensure_dynamic_lds(reinterpret_cast<const void*>(&tfk::ntt_pass_kernel<INV, SCALE, LAST1024, R1024, COL, PRE2>), (int)(160 * 1024), done_mask)) return rc_attr;
    // the R = 1024 column-pass instantiation stages its inner twiddle table behind the exchange buffer (LAST1024: part of
    // kLast1024LdsBytes already)
    const size_t lds_bytes = l.lds_bytes + ((TF_LDS_TW && !LAST1024 && l.a.inner_tw) ? (size_t(1) << l.a.p2) * tfk::kLdsTwStride * sizeof(u64) : 0);
    hipLaunchKernelGGL((tfk::ntt_pass_kernel<INV, SCALE, LAST1024, R1024, COL, PRE2>), dim3(l.tiles), dim3(l.threads), lds_bytes, stream,
                       l.a);
    HIPCHK(hipGetLastError());
    return TF_OK;
}

// the 2048-point column pass in one workgroup (2048 rows x 8 word-columns, ntt_col2048_kernel)
template <bool INV, int SCALE>
int launch_col2048_t(const Launch& l, hipStream_t stream) {
    static std::atomic<unsigned long long> done_mask{0};
    if (int rc_attr = ensure_dynamic_lds(reinterpret_cast<const void*>(&tfk::ntt_col2048_kernel<INV, SCALE>), (int)(160 * 1024), done_mask)) return rc_attr;
    const size_t lds_bytes = size_t(32) * tfk::kC8S1 * sizeof(u64);  // (the inner table is staged inside the exchange buffer)
    hipLaunchKernelGGL((tfk::ntt_col2048_kernel<INV, SCALE>), dim3(l.tiles), dim3(512), lds_bytes, stream, l.a);
    HIPCHK(hipGetLastError());
    return TF_OK;
}

constexpr size_t kLast1024LdsBytes = (size_t(tfk::kL1024ExchangeWords) + (TF_LDS_TW ? 32 * tfk::kLdsTwStride : 0)) * sizeof(u64);

int launch_pass(const Launch& l, bool inverse, hipStream_t stream) {
    if (l.tiles == 0) return TF_OK;
    if (l.bad_geometry) {
        t_last_error = "NTT planner self-check failed (thread-to-column division is not exact for this geometry)";
        return TF_ERR_HIP;
    }
    if (l.a.p2 == 5 && !l.a.inner_tw) {  // the R = 1024 instantiations run lazy networks and rely on the product that follows
        t_last_error = "internal: R = 1024 pass without its inner twiddle table";
        return TF_ERR_HIP;
    }
    // the plain R = 1024 last-pass kernel: the only one that truncates its output and shifts its tiles
    const bool fits = fits_buffer_offsets(l);
    // the constant-geometry column pass (R1024) only with exactly the geometry its immediates assume; anything else is COL's
    const bool std_geo = l.threads == 512 && l.a.nc == tfk::kR1024Nc && l.a.cpr == tfk::kR1024Cpr && l.a.nrounds == tfk::kR1024Rounds &&
                         l.a.s1 == tfk::kR1024S1 && l.a.s2 == tfk::kR1024Cpr && l.a.s3 == 1 && !l.a.gfast;
    const bool plain_last1024 = l.a.p2 == 5 && !l.a.post_tw && !l.a.gfast && !l.a.pre_scale && l.a.n_coeffs < 0 && !l.a.in2 &&
                                (!l.a.post_scale || inverse) && !l.narrow && fits;
    if (l.a.p2 == 6) {
        // a 2048-point column pass in ONE workgroup of 2048 rows x 8 word-columns (ntt_kernels.h, ntt_col2048_kernel): planned by
        // run_ntt only, with exactly the geometry the kernel's immediates assume
        const bool geo = l.threads == 512 && l.a.nc == tfk::kC8Nc && l.a.cpr == tfk::kC8Cpr && l.a.nrounds == tfk::kC8Rounds && l.a.s1 == tfk::kC8S1 &&
                         l.a.s2 == tfk::kC8Cpr && l.a.s3 == 1 && !l.a.gfast && !l.a.wtiles;
        const bool load_work = l.a.pre_scale || l.a.n_coeffs >= 0;
        if (!geo || !fits || !l.a.post_tw || !l.a.inner_tw || l.a.in2 || l.a.n_out >= 0 || l.a.post_scale || l.a.pre2_map ||
            (load_work && inverse) || (l.a.pre_scale && l.a.ps_col)) {
            t_last_error = "internal: one-workgroup 2048-point column pass outside the shapes it supports";
            return TF_ERR_HIP;
        }
        if (load_work) return launch_col2048_t<false, 1>(l, stream);
        return inverse ? launch_col2048_t<true, 0>(l, stream) : launch_col2048_t<false, 0>(l, stream);
    }
    if (l.a.pre2_map) {
        // a 2048-point pass as two 1024-point halves per tile (ntt_kernels.h, PRE2): only planned by run_ntt when all of this holds
        const bool column = l.a.post_tw != nullptr;
        if (l.a.p2 != 5 || !fits || l.a.in2 || l.a.n_out >= 0 || l.a.gfast || (column && !std_geo) ||
            (!column && (l.a.pre_scale || l.a.n_coeffs >= 0)) || (l.a.post_scale && (column || !inverse)) ||
            ((l.a.pre_scale || l.a.n_coeffs >= 0) && inverse)) {
            t_last_error = "internal: two-pass (PRE2) launch outside the shapes it supports";
            return TF_ERR_HIP;
        }
        if (column) {
            if (l.a.pre_scale || l.a.n_coeffs >= 0) return launch_pass_t<false, 1, false, true, false, true>(l, stream);
            return inverse ? launch_pass_t<true, 0, false, true, false, true>(l, stream) : launch_pass_t<false, 0, false, true, false, true>(l, stream);
        }
        Launch l2 = l;
        l2.lds_bytes = std::max(l.lds_bytes, kLast1024LdsBytes);
        l2.threads = 512;
        if (l.a.post_scale) return launch_pass_t<true, 2, true, false, false, true>(l2, stream);
        return inverse ? launch_pass_t<true, 0, true, false, false, true>(l2, stream) : launch_pass_t<false, 0, true, false, false, true>(l2, stream);
    }
    if ((l.a.n_out >= 0 || l.a.col_shift0 || l.a.col_shift_i0) && !plain_last1024) {  // anything else would overrun the caller's buffer
        t_last_error = "internal: truncated output or shifted tiles requested from a pass that does not support them";
        return TF_ERR_HIP;
    }
    if (l.a.pre_scale || l.a.n_coeffs >= 0 || l.a.in2) {
        // work on load: coset scaling, zero padding, or the pointwise product with a second operand (forward or inverse;
        // constant-P2 variant for a forward first pass with R = 1024)
        if (inverse) return launch_pass_t<true, 1>(l, stream);
        if (l.a.p2 == 5 && l.a.post_tw && fits && std_geo) return launch_pass_t<false, 1, false, true>(l, stream);
        if (l.a.post_tw && fits && !l.a.gfast) return launch_pass_t<false, 1, false, false, true>(l, stream);
        return launch_pass_t<false, 1>(l, stream);
    }
    if (l.a.post_scale) {  // coset interpolation: inverse, scale on store
        if (plain_last1024) {  // R = 1024 last pass: the specialised kernel with the multiplication in its fused tail
            Launch l2 = l;
            l2.lds_bytes = std::max(l.lds_bytes, kLast1024LdsBytes);
            l2.threads = 512;
            return launch_pass_t<true, 2, true>(l2, stream);
        }
        return launch_pass_t<true, 2>(l, stream);
    }
    // last pass of a plain transform with R = 1024: specialised kernel (constant P2, stores fused with level 5)
    // (not for single-pass transforms: their stores run along the row as well, which only the gfast roles give -- 1.05 vs 1.20 ms)
    const bool last1024 = l.a.p2 == 5 && !l.a.post_tw && !l.narrow && !l.a.gfast && fits;
    const bool r1024 = l.a.p2 == 5 && l.a.post_tw && fits && std_geo;  // column pass with R = 1024
    if (last1024) {  // this instantiation lays its exchange buffer out itself (32 x 289 words, ntt_kernels.h)
        Launch l2 = l;
        l2.lds_bytes = std::max(l.lds_bytes, kLast1024LdsBytes);
        l2.threads = 512;  // 16 column slots x 32, also for tiles of 15 word-columns (XFE)
        return inverse ? launch_pass_t<true, 0, true>(l2, stream) : launch_pass_t<false, 0, true>(l2, stream);
    }
    // any other column pass whose offsets fit: the same treatment with a run-time P2 (COL)
    const bool col = l.a.post_tw && !r1024 && fits && !l.a.gfast;
    if (inverse) return r1024 ? launch_pass_t<true, 0, false, true>(l, stream)
                              : (col ? launch_pass_t<true, 0, false, false, true>(l, stream) : launch_pass_t<true, 0>(l, stream));
    if (r1024) return launch_pass_t<false, 0, false, true>(l, stream);
    if (col) return launch_pass_t<false, 0, false, false, true>(l, stream);
    return launch_pass_t<false, 0>(l, stream);
}

int check_len(size_t n) {
    if (n != 0 && (n & (n - 1))) return TF_ERR_LEN_NOT_POWER_OF_TWO;  // ntt.rs:137
    if (n > (size_t(1) << 31)) return TF_ERR_LEN_TOO_LARGE;           // ntt.rs:134-139: lengths beyond u32::MAX panic
    return TF_OK;
}

// n <= 32: wave-private tiles (ntt_rows32w_kernel), a grid-stride walk of two workgroups per CU
template <bool INV, int L, int LOGN>
int launch_rows32w_t(const tfk::NttRows32Args& a, unsigned grid, hipStream_t stream) {
    static std::atomic<unsigned long long> done_mask{0};
    if (int rc_attr = ensure_dynamic_lds(reinterpret_cast<const void*>(&tfk::ntt_rows32w_kernel<INV, L, LOGN>), (int)(160 * 1024), done_mask)) return rc_attr;
    hipLaunchKernelGGL((tfk::ntt_rows32w_kernel<INV, L, LOGN>), dim3(grid), dim3(256), size_t(4) * 64 * 33 * sizeof(u64), stream, a);
    HIPCHK(hipGetLastError());
    return TF_OK;
}
template <bool INV, int L>
int launch_rows32w_n(const tfk::NttRows32Args& a, unsigned grid, int log_n, hipStream_t stream) {
    switch (log_n) {
        case 1: return launch_rows32w_t<INV, L, 1>(a, grid, stream);
        case 2: return launch_rows32w_t<INV, L, 2>(a, grid, stream);
        case 3: return launch_rows32w_t<INV, L, 3>(a, grid, stream);
        case 4: return launch_rows32w_t<INV, L, 4>(a, grid, stream);
        case 6:
            if constexpr (L == 1) return launch_rows32w_t<INV, 1, 6>(a, grid, stream);
            return TF_ERR_NULL_POINTER;  // (not reached: run_ntt sends XFieldElement transforms of 64 points to the row pass)
        default: return launch_rows32w_t<INV, L, 5>(a, grid, stream);
    }
}

// batch contiguous transforms of n = 2^log_n <= 32 points (BFieldElement: <= 64)
int launch_rows32(const NttCall& c, hipStream_t stream) {
    const int cus = device_cus(), log_n = ilog2(c.n), L = c.L;
    tfk::NttRows32Args a{};
    a.in = c.in;
    a.out = c.out;
    a.total_transforms = (long long)c.batch;
    a.scale = c.inverse ? gl::mont_inverse(gl::to_mont(u64(1) << log_n)) : 0;
    a.L = L;
    const size_t words = c.batch * c.n * size_t(L), per_tile = L == 1 ? 2048 : 2016;  // words per wave and tile
    const size_t tiles = (words + per_tile - 1) / per_tile, wgs = (tiles + 3) / 4;
    const unsigned grid = (unsigned)std::min(wgs, size_t(cus) * 2);  // two workgroups are resident per CU (LDS); they walk the tiles
    if (L == 1) return c.inverse ? launch_rows32w_n<true, 1>(a, grid, log_n, stream) : launch_rows32w_n<false, 1>(a, grid, log_n, stream);
    return c.inverse ? launch_rows32w_n<true, 3>(a, grid, log_n, stream) : launch_rows32w_n<false, 3>(a, grid, log_n, stream);
}

// 2^11 <= n <= 2^14, contiguous BFieldElement transforms: whole transform per workgroup (ntt_block_kernel)
template <int LOGP3, bool INV, int SCALE>
int launch_block_t(const tfk::NttBlockArgs& a, unsigned grid, hipStream_t stream) {
    static std::atomic<unsigned long long> done_mask{0};
    if (int rc_attr = ensure_dynamic_lds(reinterpret_cast<const void*>(&tfk::ntt_block_kernel<LOGP3, INV, SCALE>), (int)(160 * 1024), done_mask)) return rc_attr;
    constexpr int P3 = 1 << LOGP3;
    const size_t lds_bytes = size_t(8) * (1056 + 32 / P3) * sizeof(u64);  // exchange 1 is the larger of the two layouts
    hipLaunchKernelGGL((tfk::ntt_block_kernel<LOGP3, INV, SCALE>), dim3(grid), dim3(512), lds_bytes, stream, a);
    HIPCHK(hipGetLastError());
    return TF_OK;
}

int launch_block(DeviceCtx* ctx, const NttCall& c, hipStream_t stream) {
    const int log_n = ilog2(c.n);
    tfk::NttBlockArgs a{};
    int rc = get_block_tables(ctx, log_n, c.inverse, &a.tw1, &a.tw2);
    if (rc) return rc;
    a.in = c.in;
    a.out = c.out;
    a.pre_scale = c.pre_scale;
    a.post_scale = c.post_scale;
    a.n_coeffs = c.n_coeffs;
    a.in_bs = c.in_bs;
    a.out_bs = c.out_bs;
    a.total_transforms = (long long)c.batch * c.L;  // limb transforms (ntt_kernels.h)
    a.in2 = c.in2;
    a.n_out = c.n_out;
    a.L = c.L;
    const int lp3 = log_n - 10, T = 16 >> lp3;
    const unsigned grid = (unsigned)((c.batch * (size_t)c.L + T - 1) / T);
    const bool scaled_load = c.pre_scale || c.n_coeffs >= 0, scaled_store = c.post_scale != nullptr;
    if (c.in2) {  // the inverse transform of a product: second operand on load, truncated store
        switch (lp3) {
            case 1: return launch_block_t<1, true, 3>(a, grid, stream);
            case 2: return launch_block_t<2, true, 3>(a, grid, stream);
            case 3: return launch_block_t<3, true, 3>(a, grid, stream);
            default: return launch_block_t<4, true, 3>(a, grid, stream);
        }
    }
    switch (lp3 * 2 + (c.inverse ? 1 : 0)) {
        case 2: return scaled_load ? launch_block_t<1, false, 1>(a, grid, stream) : launch_block_t<1, false, 0>(a, grid, stream);
        case 3: return scaled_store ? launch_block_t<1, true, 2>(a, grid, stream) : launch_block_t<1, true, 0>(a, grid, stream);
        case 4: return scaled_load ? launch_block_t<2, false, 1>(a, grid, stream) : launch_block_t<2, false, 0>(a, grid, stream);
        case 5: return scaled_store ? launch_block_t<2, true, 2>(a, grid, stream) : launch_block_t<2, true, 0>(a, grid, stream);
        case 6: return scaled_load ? launch_block_t<3, false, 1>(a, grid, stream) : launch_block_t<3, false, 0>(a, grid, stream);
        case 7: return scaled_store ? launch_block_t<3, true, 2>(a, grid, stream) : launch_block_t<3, true, 0>(a, grid, stream);
        case 8: return scaled_load ? launch_block_t<4, false, 1>(a, grid, stream) : launch_block_t<4, false, 0>(a, grid, stream);
        default: return scaled_store ? launch_block_t<4, true, 2>(a, grid, stream) : launch_block_t<4, true, 0>(a, grid, stream);
    }
}

// (launchers of the latency-shaped kernels: tf_lat.hip)

// ------------------------------------------------------------------------------------ run_ntt: plan, then execute
// (NttCall, the one description of a transform call: tf_internal.h.  The executors of this unit take a call that went through with_strides.)
NttShape shape_of(const NttCall& call) {
    const NttCall c = with_strides(call);
    NttShape s;
    s.n = c.n, s.batch = c.batch, s.L = c.L, s.inverse = c.inverse, s.cosets = c.cosets, s.n_coeffs = c.n_coeffs, s.n_out = c.n_out;
    s.pre_scale = c.pre_scale != nullptr, s.post_scale = c.post_scale != nullptr, s.in2 = c.in2 != nullptr, s.coset_offset = c.coset_offset != nullptr;
    s.packed = c.in_bs == (long long)c.n * c.L && c.out_bs == (long long)c.n * c.L;
    return s;
}

// n <= 16: one thread per transform
int run_tiny(DeviceCtx* ctx, const NttCall& c, hipStream_t stream) {
    const int log_n = ilog2(c.n);
    const u64* tw = nullptr;
    TRY(get_tiny_table(ctx, log_n, c.inverse, &tw));
    tfk::NttTinyArgs A{};
    A.in = c.in;
    A.out = c.out;
    A.tw = tw;
    A.pre_scale = c.pre_scale;
    A.post_scale = c.post_scale;
    A.n_coeffs = c.n_coeffs;
    A.in_bs = c.in_bs;
    A.out_bs = c.out_bs;
    A.count = (long long)c.batch * c.L;
    A.scale = (c.inverse && log_n > 0) ? gl::mont_inverse(gl::to_mont(u64(c.n))) : 0;
    A.log_n = log_n;
    A.L = c.L;
    const long long blocks = (A.count + 255) / 256;
    hipLaunchKernelGGL(tfk::ntt_tiny_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, A);
    HIPCHK(hipGetLastError());
    return TF_OK;
}

// n <= 1024 in one pass: a tile is whole transforms
int run_row(DeviceCtx* ctx, const NttCall& c, const NttPlan& plan, hipStream_t stream) {
    const int log_n = ilog2(c.n);
    const u64* inner = nullptr;
    TRY(get_inner_table(ctx, log_n, c.inverse, c.inverse ? log_n : 0, &inner));
    // 2^31 columns limit per launch: split huge batches
    const size_t max_batch = size_t(1) << 24;
    for (size_t b0 = 0; b0 < c.batch; b0 += max_batch) {
        const size_t nb = std::min(max_batch, c.batch - b0);
        Launch l = plan_row_pass(plan, c.in + b0 * c.in_bs, c.out + b0 * c.out_bs, c.in_bs, c.out_bs, nb, log_n, c.L);
        l.a.inner_tw = inner;
        l.a.pre_scale = c.pre_scale;
        l.a.post_scale = c.post_scale;
        l.a.n_coeffs = c.n_coeffs;
        l.a.in2 = c.in2 ? c.in2 + b0 * c.in_bs : nullptr;
        TRY(launch_pass(l, c.inverse, stream));
    }
    return TF_OK;
}

// The work space between the passes of one call and, with K > 1 tile streams, the fork of the caller's stream into them and the join
// back (event edges only, no host synchronisation).  One owner, in the style of DevTemp (tf_temp.h): finish() -- or the destructor, on
// any early return -- joins whatever was enqueued on the side streams, destroys the events and hands the scratch block back behind
// the join.
class TileScope {
public:
    TileScope(DeviceCtx* ctx, hipStream_t stream) : ctx_(ctx), stream_(stream) {}
    TileScope(const TileScope&) = delete;
    TileScope& operator=(const TileScope&) = delete;
    ~TileScope() { (void)finish(); }

    u64* scratch() const { return blk_.p; }
    int acquire(size_t bytes) {
        const int rc = scratch_acquire(ctx_, bytes, stream_, &blk_, "ntt inter-pass scratch");
        if (rc) blk_ = DeviceCtx::ScratchBlock{};  // (nothing of ours to give back)
        return rc;
    }
    // the K side streams wait for everything the caller's stream holds so far
    int fork(int K, const hipStream_t* side) {
        K_ = K;
        side_ = side;
        hipError_t e = hipEventCreateWithFlags(&ev_fork_, hipEventDisableTiming);
        for (int i = 0; i < K && e == hipSuccess; ++i) e = hipEventCreateWithFlags(&ev_join_[i], hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventRecord(ev_fork_, stream_);
        for (int i = 0; i < K && e == hipSuccess; ++i) e = hipStreamWaitEvent(side[i], ev_fork_, 0);
        if (e != hipSuccess) {
            // nothing has been enqueued on the side streams that touches the scratch: release and report
            (void)finish();
            return hip_fail(e, "fork into the tile streams", __FILE__, __LINE__);
        }
        forked_ = true;
        return TF_OK;
    }
    int finish() {
        hipError_t je = hipSuccess;
        if (forked_) {  // join: whatever was enqueued (also after a failed launch) finishes before the caller's stream goes on
            for (int i = 0; i < K_; ++i) {
                hipError_t e1 = hipEventRecord(ev_join_[i], side_[i]);
                if (e1 == hipSuccess) e1 = hipStreamWaitEvent(stream_, ev_join_[i], 0);
                if (e1 != hipSuccess) je = e1;
            }
            forked_ = false;
        }
        if (ev_fork_) (void)hipEventDestroy(ev_fork_);
        ev_fork_ = nullptr;
        for (int i = 0; i < kMaxPipe; ++i) {
            if (ev_join_[i]) (void)hipEventDestroy(ev_join_[i]);
            ev_join_[i] = nullptr;
        }
        if (je != hipSuccess) (void)hipDeviceSynchronize();  // cannot order the release after the side streams any other way
        scratch_release(ctx_, blk_, stream_);
        blk_ = DeviceCtx::ScratchBlock{};
        if (je != hipSuccess) return hip_fail(je, "join of the tile streams", __FILE__, __LINE__);
        return TF_OK;
    }

private:
    DeviceCtx* ctx_;
    hipStream_t stream_;
    DeviceCtx::ScratchBlock blk_;
    int K_ = 0;
    const hipStream_t* side_ = nullptr;
    bool forked_ = false;
    hipEvent_t ev_fork_ = nullptr, ev_join_[kMaxPipe] = {nullptr, nullptr, nullptr, nullptr};
};

// multi-pass: n = N_1 * ... * N_P, every N_i = 2^(a_i) <= 1024.  Passes 1 .. P-1 are column passes (DFT over digit i,
// inter-pass twiddle, same position in and out); the last pass transforms the contiguous rows of N_P elements and
// scatters output digit k_P to  k_1 + N_1 k_2 + ... + N_1..N_{P-1} k_P  (natural order).  Everything that was decided -- passes,
// radices, pairs, tiles, streams -- is read from the plan.
int run_passes(DeviceCtx* ctx, const NttCall& c, const NttPlan& plan, hipStream_t stream) {
    const int P = plan.P, L = c.L, log_n = ilog2(c.n);
    const int (&a)[4] = plan.a;
    const bool (&pre2)[4] = plan.pre2;
    const bool inverse = c.inverse, scaled_c8 = plan.c8 && c.pre_scale;  // the first pass's table has offset^b folded in (ntt_col2048_kernel)
    const size_t n = c.n, cosets = c.cosets;
    const u64* inner[4] = {nullptr, nullptr, nullptr, nullptr};
    for (int i = 0; i < P; ++i)
        TRY(get_inner_table(ctx, pre2[i] ? 10 : a[i], inverse, (i == P - 1 && inverse) ? log_n : 0, &inner[i], pre2[i] ? 2 : 1));  // n^-1 rides on the last pass
    const u64* post[3] = {nullptr, nullptr, nullptr};
    // tables too large to cache: given back on the caller's stream when the call returns, behind the join of the tile streams
    DevTemp post_own[3] = {DevTemp(stream), DevTemp(stream), DevTemp(stream)};
    {
        int rest = log_n;
        for (int i = 0; i + 1 < P; ++i) {
            if (i == 0 && scaled_c8) {
                TRY(get_scaled_post_table(ctx, rest, a[i], *c.coset_offset, stream, &post[i], &post_own[i]));
            } else {
                TRY(get_post_table(ctx, rest, a[i], inverse, stream, &post[i], &post_own[i]));
            }
            rest -= a[i];
        }
    }
    const size_t poly_bytes = n * cosets * size_t(L) * sizeof(u64), tb = plan.tb;
    // pipelined tiles: tile t runs on side stream t % K with scratch tile t % K; the caller's stream forks into the side streams
    // before the first tile and joins them after the last
    int K = plan.K;
    hipStream_t side[kMaxPipe] = {nullptr, nullptr, nullptr, nullptr};
    if (K > 1) {
        std::lock_guard<std::mutex> lk(ctx->mu);
        for (int i = 0; i < K; ++i) {
            if (!ctx->side[i] && hipStreamCreateWithFlags(&ctx->side[i], hipStreamNonBlocking) != hipSuccess) {
                (void)hipGetLastError();
                ctx->side[i] = nullptr;
                K = 1;  // no side streams: the plain one-stream plan
                break;
            }
            side[i] = ctx->side[i];
        }
    }
    TileScope tiles(ctx, stream);  // (declared after the tables: it joins and releases before they are given back)
    TRY(tiles.acquire(size_t(K) * tb * poly_bytes));
    if (K > 1) TRY(tiles.fork(K, side));
    const long long sbs = (long long)(n * cosets) * L;  // scratch batch stride
    long long N[4];
    for (int i = 0; i < 4; ++i) N[i] = 1ll << a[i];
    int rc = TF_OK;
    size_t tile_no = 0;
    for (size_t b0 = 0; b0 < c.batch && rc == TF_OK; b0 += tb, ++tile_no) {
        const size_t nb = std::min(tb, c.batch - b0);
        hipStream_t const ts = K > 1 ? side[tile_no % K] : stream;
        u64* const scratch = K > 1 ? tiles.scratch() + (tile_no % K) * tb * (size_t)sbs : tiles.scratch();
        const u64* tin = c.in + (long long)b0 * c.in_bs;
        u64* tout = c.out + (long long)b0 * c.out_bs;
        // column passes: the first reads the caller's input, the last writes the scratch tile, the ones between work
        // in place on the output
        const u64* src = tin;
        long long src_bs = c.in_bs;
        long long outer = 1, B = (long long)n;
        for (int i = 0; i + 1 < P && rc == TF_OK; ++i) {
            B >>= a[i];
            const bool to_scratch = i == P - 2;
            // a truncated output (n_out >= 0) is smaller than the transform: the middle passes then work in place on the
            // INPUT, which the caller gives up (fast_multiply's temporary)
            u64* dst = to_scratch ? scratch : (c.n_out >= 0 ? const_cast<u64*>(tin) : tout);
            const long long dst_bs = to_scratch ? sbs : (c.n_out >= 0 ? c.in_bs : c.out_bs);
            Launch p = plan_column_pass(plan, src, dst, src_bs, dst_bs, nb, (i == 0) ? (long long)cosets : outer, a[i], B, L, pre2[i]);
            p.a.inner_tw = inner[i];
            p.a.post_tw = post[i];
            if (pre2[i]) {
                // partner coefficients are n / 2 apart: offset^(n/2) is word n / 2 of the scale table when the polynomial is that long
                p.a.pre2_cp = c.pre_scale ? c.pre_scale + ((long long)(n / 2) < c.n_coeffs ? (long long)(n / 2) : 0) : nullptr;
            }
            if (i == 0) {
                p.a.pre_scale = c.pre_scale;
                if (scaled_c8) p.a.ps_col = 0;  // the column part offset^b of the scaling comes with the inter-pass table
                p.a.n_coeffs = c.n_coeffs;
                p.a.in2 = c.in2 ? c.in2 + (long long)b0 * c.in_bs : nullptr;
                if (cosets > 1) {  // "outer" index = coset c: same input for every c, output row (k_1, c), scale table c
                    p.a.ib1 = 0;
                    p.a.ob1 = B * L;
                    p.a.out_rs = (long long)cosets * B * L;
                    p.a.ps_i1 = c.n_coeffs;
                }
                outer = (long long)cosets;
            }
            rc = launch_pass(p, inverse, ts);
            src = dst;
            src_bs = dst_bs;
            outer <<= a[i];
        }
        if (rc) break;
        if (P < 4) {
            // (plan.words: XFieldElement rows in word-granular tiles, whole 128-byte lines on the output side)
            Launch pl = plan_transpose_pass(plan, scratch, tout, sbs, c.out_bs, nb, a[P - 1], N[0] * (long long)cosets, P == 3 ? N[1] : 1, L, 0,
                                            plan.words, pre2[P - 1] ? 2 : 1);
            pl.a.inner_tw = inner[P - 1];
            pl.a.post_scale = c.post_scale;
            pl.a.n_out = c.n_out;
            if (plan.plain1024 && pl.a.nc == 16 && (unsigned long long)n * L * sizeof(u64) < (1ull << 32)) {
                // The R = 1024 last pass stores 128-byte segments of 16 adjacent output words.  When the output of batch entry
                // b does not start on a cache line (a truncated product: stride n_out = na + nb - 1 words, or a caller's
                // unaligned pointer) every segment would straddle two lines written by workgroups on different XCDs: shift
                // the tile boundaries of entry b by s = (word address of its first output) mod 16 columns so that they fall
                // on lines again; the first tile of a row wraps around to the row's last s columns.  (n * L * 8 < 2^32: the
                // wrapped lanes' 32-bit byte offset spans the whole transform.)  Measured, tools/trunc_align.py: 256 products
                // of 2^19 x 2^19 7.29 -> 7.05 ms, 1024 of 2^17 x 2^17 7.19 -> 6.66, 64 of 2^21 x 2^21 10.25 -> 9.65.
                pl.a.col_shift0 = (int)((reinterpret_cast<uintptr_t>(tout) / sizeof(u64)) & 15);
                pl.a.col_shift_i0 = (int)(c.out_bs & 15);
                pl.a.col_wrap = pl.a.col_limit;
            }
            rc = launch_pass(pl, inverse, ts);
        } else {
            for (size_t b = 0; b < nb && rc == TF_OK; ++b) {
                Launch pl = plan_transpose_pass(plan, scratch + (long long)b * sbs, tout + (long long)b * c.out_bs, sbs, c.out_bs, 1, a[3], N[0],
                                                N[1] * N[2], L, N[1]);
                pl.a.inner_tw = inner[3];
                pl.a.post_scale = c.post_scale;
                rc = launch_pass(pl, inverse, ts);
            }
        }
    }
    const int jrc = tiles.finish();
    return jrc ? jrc : rc;
}

// The transform proper: the call (NttCall, tf_internal.h, has the contract of every operand) is planned once and handed to the
// executor of its route.
int run_ntt(DeviceCtx* ctx, const NttCall& call, hipStream_t stream) {
    if (call.n == 0 || call.batch == 0) return TF_OK;
    const NttCall c = with_strides(call);
    const NttPlan plan = plan_ntt(shape_of(c));
    switch (plan.route) {
        case NttRoute::Rows32: return launch_rows32(c, stream);
        case NttRoute::Tiny: return run_tiny(ctx, c, stream);
        case NttRoute::Lat: return launch_lat(ctx, c, stream);
        case NttRoute::Lat2: return launch_lat2(ctx, c, stream);
        case NttRoute::Row: return run_row(ctx, c, plan, stream);
        // (a product's inverse carries in2 and n_out and nothing else; every other shape on this route carries neither)
        case NttRoute::Block: return launch_block(ctx, c, stream);
        case NttRoute::Passes: return run_passes(ctx, c, plan, stream);
    }
    return TF_ERR_HIP;
}

int ntt_dev(u64* d_x, size_t n, size_t batch, int L, int inverse, void* stream) {
    int rc = check_len(n);
    if (rc) return rc;
    if (n <= 1 || batch == 0) return TF_OK;  // ntt.rs:170-173 ; length 1 is the identity (n^-1 = 1)
    if (!d_x) return TF_ERR_NULL_POINTER;
    DeviceCtx* ctx = nullptr;
    rc = current_ctx(&ctx);
    if (rc) return rc;
    return run_ntt(ctx, NttCall(d_x, d_x, n, batch, L, inverse != 0), static_cast<hipStream_t>(stream));
}

int coset_eval_dev(const u64* d_coeffs, size_t n_coeffs, u64 offset_raw, u64* d_out, size_t order, size_t batch, int L,
                   void* stream) {
    if (n_coeffs > order) return TF_ERR_ORDER_NOT_ABOVE_DEGREE;  // polynomial.rs:1388-1392
    int rc = check_len(order);
    if (rc) return rc;
    if (order == 0 || batch == 0) return TF_OK;
    if (!d_out || (n_coeffs && !d_coeffs)) return TF_ERR_NULL_POINTER;
    DeviceCtx* ctx = nullptr;
    rc = current_ctx(&ctx);
    if (rc) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (n_coeffs == 0) {  // the zero polynomial evaluates to zero everywhere
        HIPCHK(hipMemsetAsync(d_out, 0, order * batch * size_t(L) * sizeof(u64), s));
        return TF_OK;
    }
    // the blown-up evaluation on order / len cosets of the padded coefficient length where it saves a global pass (coset_split, tf_plan.hip)
    const size_t cosets = coset_split(n_coeffs, order, batch, L);
    PowTable pw(ctx, s);  // (given back behind the transform's launches when the call returns)
    NttCall c = ntt_of_coeffs(d_coeffs, n_coeffs, d_out, order / cosets, batch, L);
    c.out_bs = (long long)order * L;
    if (cosets > 1) {
        TRY(pw.acquire(offset_raw, n_coeffs, cosets, ilog2(order)));
        c.cosets = cosets;
    } else {
        TRY(pw.acquire(offset_raw, n_coeffs));
        c.coset_offset = &offset_raw;
    }
    c.pre_scale = pw.get();
    return run_ntt(ctx, c, s);
}


// ------------------------------------------------------------------------------------ tf_debug_ntt_network_dev
// ONE composition of the register networks of ntt_network.h (and of the glue of ntt_kernels.h that hands words to level 1), with the
// template arguments of its call sites, over blocks of 32 consecutive words: thread t loads x[q] = d_x[B t + q], runs the form and
// stores x[0 .. 31] back in place.  B = 32, or 64 for the PRE2 / C8 forms, whose second 32 words are the partner block w (read, never
// written).  The forms and their input contracts (what the call sites guarantee; the caller of this entry point keeps to them):
//   NET32   dit_half<INV,0>, dit_half<INV,16>, dit_level<INV,5>; variant 0: lazy, WIDE = TF_POW2_WIDE (ntt_pass_kernel step 1, the
//           R = 32 / 1024 passes), 1: lazy, WIDE = 2 (ntt_block_kernel stages A and B, LOGP3 = 4), 2: canonical (ntt_rows32_kernel forward)
//   LEVELS  dit_level<INV,1> .. dit_level<INV,p2>, lazy or canonical (the column pass's run-time p2 step, step 2 of the two-pass and
//           eight-column kernels, rows32_network, the canonical LOGP3 tail of ntt_block_kernel)
//   TAIL5   canonical dit_half<INV,0>, dit_half<INV,16>, then DitRange<INV,5,Q0,Q0+4,false> for Q0 = 0, 4, 8, 12 (tail_p5)
//   LAT     DitRange<INV,l,0,4,false> for l = 1 .. LOGR on slots 0 .. 7 (lat_dft); slots 8 .. 31 pass through
//   PRE2    pre2_combine8<INV,0/8/16/24>(x, w, half), pre2_shift where ntt_pass_kernel applies it, then the lazy NET32
//   C8      c8_combine8<INV,0/8/16/24>(x, w, half), pre2_shift<INV> when half, then lazy levels 1 .. 5 (the eight-column kernel)
// lazy forms: even slots any 64-bit word, odd slots (second operands of level 1) < p; canonical forms: every word < p; PRE2 / C8: both
// blocks canonical (loaded words or Montgomery products).
constexpr int kNetLevels = 6, kNetTail5 = 26, kNetLat = 28, kNetPre2 = 34, kNetC8 = 38;
static_assert(kNetC8 + 4 == TF_NTT_NETWORK_FORM_COUNT, "include/tf_hip.h lists the forms");
constexpr int net_form_words(int form) { return form >= kNetPre2 ? 64 : 32; }

template <bool INV, bool LAZY, int WIDE>
__device__ __forceinline__ void net32_form(u64 (&x)[32]) {
    tfk::dit_half<INV, 0, LAZY, WIDE>(x);
    tfk::dit_half<INV, 16, LAZY, WIDE>(x);
    tfk::dit_level<INV, 5, LAZY, WIDE>(x);
}
template <bool INV, bool LAZY, int P2, int LVL = 1>
__device__ __forceinline__ void levels_form(u64 (&x)[32]) {
    if constexpr (LVL <= P2) {
        tfk::dit_level<INV, LVL, LAZY>(x);
        levels_form<INV, LAZY, P2, LVL + 1>(x);
    }
}

template <int FORM>
__global__ void __launch_bounds__(256) ntt_network_form_kernel(u64* d, unsigned long long blocks, int half) {
    constexpr int B = net_form_words(FORM);
    const unsigned long long t = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= blocks) return;
    u64* const p = d + t * B;
    u64 x[32];
#pragma unroll
    for (int q = 0; q < 32; ++q) x[q] = p[q];
    if constexpr (FORM < kNetLevels) {
        constexpr bool INV = (FORM & 1) != 0;
        constexpr int V = FORM >> 1;
        if constexpr (V == 0) net32_form<INV, true, TF_POW2_WIDE>(x);
        else if constexpr (V == 1) net32_form<INV, true, 2>(x);
        else net32_form<INV, false, TF_POW2_WIDE>(x);
    } else if constexpr (FORM < kNetTail5) {
        constexpr int K = FORM - kNetLevels;
        levels_form<(K & 1) != 0, ((K >> 1) & 1) != 0, (K >> 2) + 1>(x);
    } else if constexpr (FORM < kNetLat) {
        constexpr bool INV = ((FORM - kNetTail5) & 1) != 0;
        tfk::dit_half<INV, 0>(x);
        tfk::dit_half<INV, 16>(x);
        tfk::DitRange<INV, 5, 0, 4, false>::run(x);
        tfk::DitRange<INV, 5, 4, 8, false>::run(x);
        tfk::DitRange<INV, 5, 8, 12, false>::run(x);
        tfk::DitRange<INV, 5, 12, 16, false>::run(x);
    } else if constexpr (FORM < kNetPre2) {
        constexpr int K = FORM - kNetLat;
        constexpr bool INV = (K & 1) != 0;
        constexpr int LOGR = (K >> 1) + 1;
        tfk::DitRange<INV, 1, 0, 4, false>::run(x);
        if constexpr (LOGR >= 2) tfk::DitRange<INV, 2, 0, 4, false>::run(x);
        if constexpr (LOGR >= 3) tfk::DitRange<INV, 3, 0, 4, false>::run(x);
    } else {
        constexpr bool INV = (FORM & 1) != 0;  // (kNetPre2 and kNetC8 are even)
        u64 wa[8], wb[8];
        if constexpr (FORM < kNetC8) {
            // the order of ntt_pass_kernel's overlapped load: the first sixteen slots go through levels 1-4 before the last sixteen are combined
#pragma unroll
            for (int i = 0; i < 8; ++i) wa[i] = p[32 + i], wb[i] = p[40 + i];
            tfk::pre2_combine8<INV, 0>(x, wa, half != 0);
            tfk::pre2_combine8<INV, 8>(x, wb, half != 0);
            if (half) tfk::pre2_shift<INV, 1, 16>(x);
            tfk::dit_half<INV, 0, true>(x);
#pragma unroll
            for (int i = 0; i < 8; ++i) wa[i] = p[48 + i], wb[i] = p[56 + i];
            tfk::pre2_combine8<INV, 16>(x, wa, half != 0);
            tfk::pre2_combine8<INV, 24>(x, wb, half != 0);
            if (half) tfk::pre2_shift<INV, 16, 32>(x);
            tfk::dit_half<INV, 16, true>(x);
            tfk::dit_level<INV, 5, true>(x);
        } else {
#pragma unroll
            for (int i = 0; i < 8; ++i) wa[i] = p[32 + i], wb[i] = p[40 + i];
            tfk::c8_combine8<INV, 0>(x, wa, half != 0);
            tfk::c8_combine8<INV, 8>(x, wb, half != 0);
#pragma unroll
            for (int i = 0; i < 8; ++i) wa[i] = p[48 + i], wb[i] = p[56 + i];
            tfk::c8_combine8<INV, 16>(x, wa, half != 0);
            tfk::c8_combine8<INV, 24>(x, wb, half != 0);
            if (half) tfk::pre2_shift<INV>(x);
            levels_form<INV, true, 5>(x);
        }
    }
#pragma unroll
    for (int q = 0; q < 32; ++q) p[q] = x[q];
}

template <int FORM>
void network_form_launch(u64* d_x, size_t blocks, hipStream_t s) {
    const int half = FORM >= kNetPre2 ? ((FORM - kNetPre2) >> 1) & 1 : 0;
    hipLaunchKernelGGL(ntt_network_form_kernel<FORM>, dim3((unsigned)((blocks + 255) / 256)), dim3(256), 0, s, d_x, (unsigned long long)blocks, half);
}
template <int... FORM>
void network_form_dispatch(int form, u64* d_x, size_t blocks, hipStream_t s, std::integer_sequence<int, FORM...>) {
    using Fn = void (*)(u64*, size_t, hipStream_t);
    static const Fn table[] = {&network_form_launch<FORM>...};
    table[form](d_x, blocks, s);
}
int debug_ntt_network_words(int form) { return net_form_words(form); }
void debug_ntt_network_dev(int form, u64* d_x, size_t count, hipStream_t s) {
    network_form_dispatch(form, d_x, count / (size_t)net_form_words(form), s, std::make_integer_sequence<int, TF_NTT_NETWORK_FORM_COUNT>{});
}
void debug_ntt_network_config(int* lazy, int* asm_bfly, int* asm_pow2, int* pow2_wide) {
    if (lazy) *lazy = TF_LAZY;
    if (asm_bfly) *asm_bfly = TF_ASM_BFLY;
    if (asm_pow2) *asm_pow2 = TF_ASM_POW2;
    if (pow2_wide) *pow2_wide = TF_POW2_WIDE;
}


}  // namespace tfi
