// tf_sponge.hip -- batches of device-resident Tip5 sponges (sponge_kernels.h): Tip5::new, Sponge::absorb / squeeze /
// pad_and_absorb_all, Tip5::sample_scalars / sample_indices (tip5/mod.rs:511-526, :636-698; util_types/sponge.rs:41-55), one launch per call.
#include "tf_temp.h"

// As tf_proof.hip and tf_mmr.hip: this unit has its own copy of the Tip5 constants, in a namespace of its own, uploaded once per device.
namespace tfs {
#include "sponge_kernels.h"
}

namespace tfi {

namespace {
using tfs::tfk::SpongeArgs;
using tfs::tfk::kSpongeAbsorb;
using tfs::tfk::kSpongeIndices;
using tfs::tfk::kSpongeSqueeze;

Tip5ConstsOnce g_consts;
int ctx_dev(int* dev) { return g_consts.ensure(dev, tfs::tfk::g_tip5, tfs::tfk::g_tip5_mx); }

// The offsets of a ragged absorb reach the device through the pinned staging of tf_proof.hip / tf_mmr.hip, and the _dev form never
// waits for its stream.  The kernel reads them where they are: page-locked host memory is mapped into the device's address space
// (hipHostGetDevicePointer), every offset is read once, and a copy into device memory in front of the launch cost more than the
// reads over the link (T3 of DESIGN 4.7: 27 us against the 91 us of the kernel).  The block goes back to the pool when the MappedWords
// go out of scope, after the launch that reads it is enqueued; it is handed out again once that launch has completed.
struct MappedWords {
    const void* d = nullptr;  // what the kernel reads
    int dev = 0;
    Staging stg;
    hipStream_t s = nullptr;
    ~MappedWords() {
        if (stg.p) stage_release(dev, stg, s);
    }
    // (named map, not put: tests/test_temp_guard_cpu.py takes every `.put(` in csrc/ for a pool allocation that must carry a label,
    //  and this one takes a pinned staging block, no pool memory)
    int map(int device, const void* host, size_t bytes, hipStream_t st) {
        dev = device;
        s = st;
        TRY(stage_acquire(dev, bytes, &stg));
        std::memcpy(stg.p, host, bytes);
        void* mapped = nullptr;
        HIPCHK(hipHostGetDevicePointer(&mapped, stg.p, 0));
        d = mapped;
        return TF_OK;
    }
};

// One launch of the sponge program: the latency form (a row pair per sponge under the coop_two_rows rule, else a row) for at most
// kCoopMaxCount sponges, the matrix-pipe form above.
template <int OP>
int launch_program(const SpongeArgs& g, hipStream_t s) {
    if (g.count <= kCoopMaxCount) {
        if (coop_two_rows(g.count))
            hipLaunchKernelGGL((tfs::tfk::tip5_sponge_coop_kernel<2, OP>), dim3((unsigned)((g.count + 7) / 8)), dim3(256), 0, s, g);
        else
            hipLaunchKernelGGL((tfs::tfk::tip5_sponge_coop_kernel<1, OP>), dim3((unsigned)((g.count + 15) / 16)), dim3(256), 0, s, g);
    } else {
        hipLaunchKernelGGL((tfs::tfk::tip5_sponge_mx_kernel<OP>), dim3(mx_blocks(g.count)), dim3(256), 0, s, g);
    }
    HIPCHK(hipGetLastError());
    return TF_OK;
}

// Argument checks shared by the host-pointer and the _dev forms; all of them come before a device is touched.  *noop: nothing to do.
constexpr size_t kMaxWords = size_t(1) << 60;  // keeps every product of two arguments below 2^63 words
inline bool too_many(size_t a, size_t b) { return b && a > kMaxWords / b; }

int check_absorb(const u64* states, size_t count, const u64* in, size_t len, const uint64_t* offsets, bool pad, bool* noop, size_t* in_words) {
    *noop = count == 0;
    *in_words = 0;
    if (*noop) return TF_OK;
    if (!states) return TF_ERR_NULL_POINTER;
    if (offsets) {
        uint64_t decreasing = 0;  // (no early exit: the loop vectorises, and a call of 2^16 sponges pays it on every call)
        for (size_t i = 0; i < count; ++i) decreasing |= (uint64_t)(offsets[i + 1] < offsets[i]);
        if (decreasing) return TF_ERR_INVALID_ARGUMENT;
        if (offsets[count] > kMaxWords) return TF_ERR_INVALID_ARGUMENT;
        *in_words = offsets[count] - offsets[0];
    } else {
        if (too_many(count, len)) return TF_ERR_INVALID_ARGUMENT;
        *in_words = count * len;
    }
    if (*in_words && !in) return TF_ERR_NULL_POINTER;
    if (!pad && len == 0) *noop = true;  // zero absorbs
    return TF_OK;
}
int check_squeeze(const u64* states, size_t count, size_t per_sponge, size_t words_each, const void* out, bool* noop) {
    *noop = count == 0;
    if (*noop) return TF_OK;
    if (!states) return TF_ERR_NULL_POINTER;
    if (too_many(per_sponge, words_each) || too_many(count, per_sponge * words_each)) return TF_ERR_INVALID_ARGUMENT;
    *noop = per_sponge == 0;
    if (!*noop && !out) return TF_ERR_NULL_POINTER;
    return TF_OK;
}
int check_indices(const u64* states, size_t count, uint32_t upper_bound, size_t num, const uint32_t* out, bool* noop) {
    if (upper_bound == 0 || (upper_bound & (upper_bound - 1))) return TF_ERR_UPPER_BOUND_NOT_POWER_OF_TWO;  // mod.rs:637, also for an empty batch
    return check_squeeze(states, count, num, 1, out, noop);
}
}  // namespace

// ------------------------------------------------------------------------------------ _dev forms
int sponge_init_dev(u64* states, size_t count, int fixed_length, hipStream_t s) {
    if (count == 0) return TF_OK;
    if (!states) return TF_ERR_NULL_POINTER;
    if (too_many(count, 16)) return TF_ERR_INVALID_ARGUMENT;
    int dev = 0;
    TRY(ctx_dev(&dev));
    const long long words = 16ll * (long long)count;
    hipLaunchKernelGGL(tfs::tfk::tip5_sponge_init_kernel, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, s, states, words, fixed_length ? 1 : 0);
    HIPCHK(hipGetLastError());
    return TF_OK;
}

// `in` is indexed from in_base (the host form uploads only [offsets[0], offsets[count]))
int sponge_absorb_dev(u64* states, size_t count, const u64* in, size_t len, const uint64_t* offsets, bool pad, uint64_t in_base, hipStream_t s) {
    bool noop;
    size_t in_words;
    TRY(check_absorb(states, count, in, len, offsets, pad, &noop, &in_words));
    if (noop) return TF_OK;
    if (offsets && offsets[0] < in_base) return TF_ERR_INVALID_ARGUMENT;
    int dev = 0;
    TRY(ctx_dev(&dev));
    SpongeArgs g{};
    g.states = states;
    g.count = (long long)count;
    g.in = in ? in - in_base : nullptr;
    g.len = (long long)len;
    g.pad = pad ? 1 : 0;
    MappedWords up;
    if (offsets) {
        TRY(up.map(dev, offsets, (count + 1) * sizeof(uint64_t), s));
        g.offsets = static_cast<const unsigned long long*>(up.d);
    }
    return launch_program<kSpongeAbsorb>(g, s);
}

// per_sponge elements of words_each words: squeeze (n_squeezes x 10) and sample_scalars (num_elements x 3)
int sponge_squeeze_dev(u64* states, size_t count, size_t per_sponge, size_t words_each, u64* out, hipStream_t s) {
    bool noop;
    TRY(check_squeeze(states, count, per_sponge, words_each, out, &noop));
    if (noop) return TF_OK;
    int dev = 0;
    TRY(ctx_dev(&dev));
    SpongeArgs g{};
    g.states = states;
    g.count = (long long)count;
    g.out = out;
    g.out_words = (long long)(per_sponge * words_each);
    return launch_program<kSpongeSqueeze>(g, s);
}

int sponge_indices_dev(u64* states, size_t count, uint32_t upper_bound, size_t num, uint32_t* out, hipStream_t s) {
    bool noop;
    TRY(check_indices(states, count, upper_bound, num, out, &noop));
    if (noop) return TF_OK;
    int dev = 0;
    TRY(ctx_dev(&dev));
    SpongeArgs g{};
    g.states = states;
    g.count = (long long)count;
    g.out_idx = out;
    g.num_indices = (long long)num;
    g.mask = upper_bound - 1;
    return launch_program<kSpongeIndices>(g, s);
}

// ------------------------------------------------------------------------------------ host flavours
// Upload the states (and the input), run the _dev form on the thread's stream, copy back, synchronise.
int sponge_init_host(u64* states, size_t count, int fixed_length) {
    if (count == 0) return TF_OK;
    if (!states) return TF_ERR_NULL_POINTER;
    if (too_many(count, 16)) return TF_ERR_INVALID_ARGUMENT;
    return host_roundtrip(nullptr, 0, nullptr, 0, states, 16 * count,
                          [&](u64*, u64*, u64* st, hipStream_t s) { return sponge_init_dev(st, count, fixed_length, s); });
}

int sponge_absorb_host(u64* states, size_t count, const u64* in, size_t len, const uint64_t* offsets, bool pad) {
    bool noop;
    size_t in_words;
    TRY(check_absorb(states, count, in, len, offsets, pad, &noop, &in_words));
    if (noop) return TF_OK;
    const uint64_t base = offsets ? offsets[0] : 0;
    return host_in_place(states, 16 * count, in_words ? in + base : nullptr, in_words,
                         [&](u64* st, u64* din, hipStream_t s) { return sponge_absorb_dev(st, count, din, len, offsets, pad, base, s); });
}

int sponge_squeeze_host(u64* states, size_t count, size_t per_sponge, size_t words_each, u64* out) {
    bool noop;
    TRY(check_squeeze(states, count, per_sponge, words_each, out, &noop));
    if (noop) return TF_OK;
    DeviceCtx* ctx = nullptr;
    TRY(current_ctx(&ctx));
    hipStream_t s = host_stream();
    const size_t out_words = count * per_sponge * words_each;
    DevTemp st(s), dout(s);
    TRY(st.alloc(16 * count, "sponge_squeeze host buffers"));
    TRY(h2d(st.p, states, 16 * count, s));
    TRY(dout.alloc(out_words, "sponge_squeeze host buffers"));
    TRY(sponge_squeeze_dev(st.p, count, per_sponge, words_each, dout.p, s));
    TRY(d2h(out, dout.p, out_words, s));
    TRY(d2h(states, st.p, 16 * count, s));
    return sync(s);
}

int sponge_indices_host(u64* states, size_t count, uint32_t upper_bound, size_t num, uint32_t* out) {
    bool noop;
    TRY(check_indices(states, count, upper_bound, num, out, &noop));
    if (noop) return TF_OK;
    DeviceCtx* ctx = nullptr;
    TRY(current_ctx(&ctx));
    hipStream_t s = host_stream();
    DevTemp st(s), dout(s);
    TRY(st.alloc(16 * count, "sponge_indices host buffers"));
    TRY(h2d(st.p, states, 16 * count, s));
    TRY(dout.alloc_bytes(count * num * sizeof(uint32_t), "sponge_indices host buffers"));
    TRY(sponge_indices_dev(st.p, count, upper_bound, num, dout.as<uint32_t>(), s));
    HIPCHK(hipMemcpyAsync(out, dout.p, count * num * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    TRY(d2h(states, st.p, 16 * count, s));
    return sync(s);
}

}  // namespace tfi
