// tf_temp.h -- the host plumbing every translation unit of libtf_hip.so repeats around its launches (host code only, no kernel):
//   DevTemp         the one owner of a stream-ordered device temporary (taken from the pool and given back on the same stream)
//   StagedUpload    host-built words -> page-locked staging -> a DevTemp, without waiting for the stream (stage_acquire, tf_proof.hip)
//   Tip5ConstsOnce  a unit's own copy of the Tip5 constants, uploaded once per device
//   host_roundtrip  the host-pointer flavour of a call: upload <= 2 inputs, run the _dev form, download one output, wait
#pragma once
#include "tf_internal.h"

namespace tfi {

// A block from the library's pool, given back with pool_free_async on the stream it was taken on.  The destructor covers every early exit
// of the function that owns it: the free is enqueued behind whatever that function has launched so far.  A function that reports a
// failed free ends in release().  alloc(0) leaves p null and is TF_OK.
class DevTemp {
   public:
    u64* p = nullptr;
    explicit DevTemp(hipStream_t stream) : s_(stream) {}
    DevTemp(const DevTemp&) = delete;
    DevTemp& operator=(const DevTemp&) = delete;
    ~DevTemp() {
        if (p) (void)pool_free_async(p, s_);
    }
    // `what`: the site's label, a literal (tests/test_temp_guard_cpu.py): the error message names it, and the guard mode counts the
    // request and reports a trodden guard under it
    int alloc(size_t words, const char* what) { return alloc_bytes(words * sizeof(u64), what); }
    int alloc_bytes(size_t bytes, const char* what) {
        if (p) return TF_ERR_INTERNAL;  // one block per owner
        if (!bytes) return TF_OK;
        const hipError_t e = pool_malloc_async(reinterpret_cast<void**>(&p), bytes, s_, what);
        if (e == hipSuccess) return TF_OK;
        p = nullptr;
        return hip_fail(e, (std::string("pool_malloc_async(") + what + ")").c_str(), __FILE__, __LINE__);
    }
    // a block that another function took from the pool on this stream (get_post_table's temporary tables)
    void adopt(u64* block) { p = block; }
    template <class T>
    T* as() const {
        return reinterpret_cast<T*>(p);
    }
    hipStream_t stream() const { return s_; }
    // frees now, behind the launches enqueued so far, and says whether that worked
    int release() {
        if (!p) return TF_OK;
        const hipError_t e = pool_free_async(p, s_);
        p = nullptr;
        return e == hipSuccess ? TF_OK : hip_fail(e, "pool_free_async", __FILE__, __LINE__);
    }

   private:
    hipStream_t s_;
};

// Host-built words (descriptors, move lists, plans) reach the device through the pinned staging blocks of stage_acquire: the _dev
// forms never wait for their stream, which a copy from pageable memory may.  put() copies into a block of its own, freed on the
// stream when the upload goes out of scope (after the launches that read it are enqueued); copy_to() into a block the caller owns.
class StagedUpload {
   public:
    explicit StagedUpload(hipStream_t stream) : d_(stream) {}
    int put(int dev, const void* host, size_t bytes, const char* what) {
        if (!bytes) return TF_OK;
        TRY(d_.alloc_bytes(bytes, what));
        return copy_to(dev, d_.p, host, bytes, d_.stream(), what);
    }
    template <class T>
    const T* as() const {
        return d_.as<const T>();
    }
    static int copy_to(int dev, void* d_dst, const void* host, size_t bytes, hipStream_t s, const char* what) {
        if (!bytes) return TF_OK;
        Staging stg;
        TRY(stage_acquire(dev, bytes, &stg));
        std::memcpy(stg.p, host, bytes);
        const hipError_t e = hipMemcpyAsync(d_dst, stg.p, bytes, hipMemcpyHostToDevice, s);
        stage_release(dev, stg, s);
        return e == hipSuccess ? TF_OK : hip_fail(e, (std::string("hipMemcpyAsync(") + what + ")").c_str(), __FILE__, __LINE__);
    }

   private:
    DevTemp d_;
};

// Every translation unit that includes tip5_kernels.h in a namespace of its own is a code object with its own __constant__ copy of
// the Tip5 constants.  ensure() returns the current device and uploads the unit's copy on the first call for that device: the round
// constants into `g_tip5`, and for a unit that runs the matrix-pipe kernels their tables into `g_tip5_mx` (fill_tip5_mx of the unit's
// namespace, found through the type).
class Tip5ConstsOnce {
   public:
    template <class Consts, class... MxConsts>
    int ensure(int* dev, const Consts& g_tip5, const MxConsts&... g_tip5_mx) {
        static_assert(sizeof...(MxConsts) <= 1, "one table of the matrix-pipe form, or none");
        DeviceCtx* ctx = nullptr;
        TRY(current_ctx(&ctx));
        *dev = (int)(ctx - g_ctx);
        std::lock_guard<std::mutex> lk(mu_);
        if (ready_[*dev]) return TF_OK;
        Consts c;
        for (int i = 0; i < 80; ++i) c.rc[i] = gl::to_mont(kRoundConstants[i]);
        HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(g_tip5), &c, sizeof(c)));
        if constexpr (sizeof...(MxConsts) == 1) TRY(upload_mx(c.rc, g_tip5_mx...));
        HIPCHK(hipDeviceSynchronize());
        ready_[*dev] = true;
        return TF_OK;
    }

   private:
    template <class MxConsts>
    static int upload_mx(const u64* rc_mont, const MxConsts& g_tip5_mx) {
        MxConsts mx;
        fill_tip5_mx(mx, rc_mont);
        HIPCHK(hipMemcpyToSymbol(HIP_SYMBOL(g_tip5_mx), &mx, sizeof(mx)));
        return TF_OK;
    }
    std::mutex mu_;
    bool ready_[kMaxDevices] = {};
};

// The host-pointer flavour of a call on the thread's own stream: allocate, upload in1 and in2 (waiting for each upload, see h2d),
// run body(d_in1, d_in2, d_out, stream), download `out`, wait.  A buffer of zero words is a null pointer.  A failed allocation maps
// through hip_fail unless the caller names the status its contract gives it (oom_in for the inputs, oom_out for the output).
// host_in_place is the same for a call that rewrites its first operand: one block is uploaded from x and downloaded to x, and body
// is body(d_x, d_in2, stream).
template <class F>
int host_roundtrip(const u64* in1, size_t w1, const u64* in2, size_t w2, u64* out, size_t wo, F&& body, int oom_in = 0, int oom_out = 0,
                   bool in_place = false) {
    DeviceCtx* ctx = nullptr;
    TRY(current_ctx(&ctx));
    hipStream_t s = host_stream();
    DevTemp d1(s), d2(s), dout(s);
    auto take = [](DevTemp& d, size_t words, int oom) {
        const int rc = d.alloc(words, "host round trip");
        return rc && oom ? oom : rc;
    };
    TRY(take(d1, w1, oom_in));
    TRY(take(d2, w2, oom_in));
    if (!in_place) TRY(take(dout, wo, oom_out));
    u64* const d_out = in_place ? d1.p : dout.p;
    TRY(h2d(d1.p, in1, w1, s));
    TRY(h2d(d2.p, in2, w2, s));
    TRY(body(d1.p, d2.p, d_out, s));
    TRY(d2h(out, d_out, wo, s));
    return sync(s);
}
template <class F>
int host_in_place(u64* x, size_t words, const u64* in2, size_t w2, F&& body) {
    return host_roundtrip(x, words, in2, w2, x, words, [&](u64* d_x, u64* d_in2, u64*, hipStream_t s) { return body(d_x, d_in2, s); }, 0, 0, true);
}

}  // namespace tfi
