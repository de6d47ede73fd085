// tf_temp_guard.hip -- the guard mode for library-owned device memory (tf_debug_temp_guard, include/tf_hip.h): host code and three
// tiny debug kernels (fill, check, the self-test's planted defect).  When the mode is on, every block pool_malloc_async hands out --
// the DevTemp / StagedUpload temporaries of every unit, the buffers of the host-pointer forms, and the inter-pass scratch that
// scratch_acquire then takes from the pool as well -- is
//
//     [ kTempGuardWords poison | payload, poisoned too | kTempGuardWords poison ]
//
// and pool_free_async checks both guards on the freeing stream before the block goes back.  A kernel that runs a tile past its work
// area shows in the ledger; a kernel that reads a work word before writing it computes with the poison, and its output changes with
// the mode.  With the mode off, pool_malloc_async and pool_free_async load one relaxed atomic and branch.
#include "tf_temp.h"
#include "tf_temp_guard.h"

#include <deque>
#include <unordered_map>

namespace tfi {

static_assert(kTempGuardWords == TF_TEMP_GUARD_WORDS && kTempGuardLedgerWords == TF_TEMP_GUARD_LEDGER_WORDS, "include/tf_hip.h states both");

// low 8 bits: the mode; the rest: guarded blocks alive.  Zero <=> nothing to do on any path.
std::atomic<unsigned long long> g_temp_guard_state{0};
std::atomic<int> g_force_temp_tables{0};

namespace {

constexpr unsigned long long kLive = 1ull << 8;

struct Block {
    void* base;
    size_t bytes;  // the caller's request
    int label, dev, mode;
};
struct LabelCount {
    std::string text;
    unsigned long long blocks = 0, bytes = 0;
};

std::mutex g_mu;
std::unordered_map<void*, Block> g_blocks;         // payload pointer -> block
std::deque<LabelCount> g_labels;                   // label id -> text and what was requested under it since the last reset (a deque: the texts never move)
std::map<std::string, int> g_label_ids;
unsigned long long* g_ledger[kMaxDevices] = {};  // device memory, kTempGuardLedgerWords words

int label_id_locked(const char* what) {
    const std::string text = what ? what : "";
    auto it = g_label_ids.find(text);
    if (it != g_label_ids.end()) return it->second;
    const int id = (int)g_labels.size();
    g_labels.push_back(LabelCount{text});
    g_label_ids[text] = id;
    return id;
}

__global__ void temp_guard_fill_kernel(unsigned long long* base, long long words, int mode) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < words; i += (long long)gridDim.x * blockDim.x)
        base[i] = temp_guard_poison(mode, (unsigned long long)i);
}

// One workgroup walks the front guard, then the back guard.  `entries` 32-bit entries per guard; the back guard starts at entry
// back_first of the block; payload_first is the payload's first entry (offsets are reported relative to it).
__global__ void temp_guard_check_kernel(const unsigned* base, long long entries, long long payload_first, long long back_first, int mode, int label,
                                        unsigned long long* ledger) {
    __shared__ unsigned long long s_count, s_first;
    bool block_counted = false;  // (thread 0's)
    for (int side = 0; side < 2; ++side) {
        if (threadIdx.x == 0) s_count = 0, s_first = ~0ull;
        __syncthreads();
        const long long first = side ? back_first : 0;
        unsigned long long count = 0, lowest = ~0ull;
        for (long long e = first + threadIdx.x; e < first + entries; e += blockDim.x) {
            if (base[e] != temp_guard_poison32(mode, (unsigned long long)e)) {
                ++count;
                if ((unsigned long long)e < lowest) lowest = (unsigned long long)e;
            }
        }
        if (count) {
            atomicAdd(&s_count, count);
            atomicMin(&s_first, lowest);
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            if (side == 0) atomicAdd(&ledger[kTgBlocksChecked], 1ull);
            if (s_count) {
                atomicAdd(&ledger[kTgEntriesOffending], s_count);
                if (!block_counted) atomicAdd(&ledger[kTgBlocksOffending], 1ull);
                block_counted = true;
                const unsigned long long slot = atomicAdd(&ledger[kTgRecords], 1ull);
                if (slot >= (unsigned long long)kTempGuardRecords) {
                    atomicAdd(&ledger[kTgRecords], ~0ull);  // (back to kTempGuardRecords: the count is the number of records kept)
                } else {
                    unsigned long long* r = ledger + kTgRecordBase + kTgRecordWords * slot;
                    r[0] = (unsigned long long)label;
                    r[1] = (unsigned long long)side;
                    r[2] = (unsigned long long)((long long)s_first - payload_first);
                    r[3] = s_count;
                }
            }
        }
        __syncthreads();
    }
}

// The self-test's one store (or none).  Every target lies inside the block's OWN guard words -- memory the block owns --, so nothing
// here faults and no neighbouring allocation is touched; defect 5 stores nothing and reads payload[0], which nobody wrote.
__global__ void temp_guard_selftest_kernel(unsigned long long* payload, long long n_words, int defect, unsigned long long* out) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const unsigned long long mark = 0x5A5AC3C3A5A53C3Cull;  // (neither half is a half of any poison word it can replace)
    if (defect == 1) payload[-1] = mark;
    if (defect == 2) payload[n_words] = mark;
    if (defect == 3) payload[n_words + (long long)kTempGuardWords - 1] = mark;
    if (defect == 4) reinterpret_cast<unsigned*>(payload)[2 * n_words + 1] = 0xA5A53C3Cu;  // (the payload is 2 n_words + 1 entries)
    out[0] = defect == 5 ? payload[0] : 0;
}

hipError_t ledger_for(int dev, unsigned long long** out) {
    std::lock_guard<std::mutex> lk(g_mu);
    if (!g_ledger[dev]) {
        unsigned long long* d = nullptr;
        hipError_t e = hipMalloc(reinterpret_cast<void**>(&d), kTempGuardLedgerWords * sizeof(unsigned long long));
        if (e == hipSuccess) e = hipMemset(d, 0, kTempGuardLedgerWords * sizeof(unsigned long long));
        if (e != hipSuccess) {
            if (d) (void)hipFree(d);
            return e;
        }
        g_ledger[dev] = d;
    }
    *out = g_ledger[dev];
    return hipSuccess;
}

size_t round_up(size_t x, size_t m) { return (x + m - 1) / m * m; }

}  // namespace

// pool_malloc_async with the mode on: the request plus a guard on each side, all of it poisoned on the caller's stream
hipError_t temp_guard_malloc(void** p, size_t bytes, hipStream_t stream, const char* what, hipMemPool_t pool, int dev, int mode) {
    unsigned long long* ledger = nullptr;
    hipError_t e = ledger_for(dev, &ledger);
    if (e != hipSuccess) return e;
    const size_t guard = kTempGuardWords * sizeof(u64);
    const size_t total = round_up(guard + round_up(bytes, 4) + guard, 8);
    void* base = nullptr;
    e = pool ? hipMallocFromPoolAsync(&base, total, pool, stream) : hipMallocAsync(&base, total, stream);
    if (e != hipSuccess) return e;
    const long long words = (long long)(total / 8);
    const unsigned blocks = (unsigned)std::min<long long>((words + 255) / 256, 4096);
    hipLaunchKernelGGL(temp_guard_fill_kernel, dim3(blocks), dim3(256), 0, stream, static_cast<unsigned long long*>(base), words, mode);
    e = hipGetLastError();
    if (e != hipSuccess) {
        (void)hipFreeAsync(base, stream);
        return e;
    }
    void* payload = static_cast<char*>(base) + guard;
    {
        std::lock_guard<std::mutex> lk(g_mu);
        const int id = label_id_locked(what);
        g_labels[id].blocks += 1;
        g_labels[id].bytes += bytes;
        g_blocks[payload] = Block{base, bytes, id, dev, mode};
    }
    g_temp_guard_state.fetch_add(kLive, std::memory_order_relaxed);
    *p = payload;
    return hipSuccess;
}

// pool_free_async with a non-zero state: a registered block is checked on `stream` and its base freed; anything else is freed as it is
hipError_t temp_guard_free(void* p, hipStream_t stream) {
    Block b{};
    {
        std::lock_guard<std::mutex> lk(g_mu);
        auto it = g_blocks.find(p);
        if (it == g_blocks.end()) return hipFreeAsync(p, stream);
        b = it->second;
        g_blocks.erase(it);
    }
    g_temp_guard_state.fetch_sub(kLive, std::memory_order_relaxed);
    unsigned long long* ledger = g_ledger[b.dev];  // (set before the block was registered)
    const long long entries = 2 * (long long)kTempGuardWords;
    const long long payload_first = entries, back_first = entries + (long long)(round_up(b.bytes, 4) / 4);
    hipLaunchKernelGGL(temp_guard_check_kernel, dim3(1), dim3(1024), 0, stream, static_cast<const unsigned*>(b.base), entries, payload_first, back_first, b.mode,
                       b.label, ledger);
    const hipError_t e = hipGetLastError();
    const hipError_t ef = hipFreeAsync(b.base, stream);
    return e != hipSuccess ? e : ef;
}

// ------------------------------------------------------------------------------------ what the tf_debug_temp_guard* entry points do
// (the extern "C" functions themselves are in tf_abi.hip, with every other entry point; include/tf_hip.h has the contract)

int temp_guard_set_mode(int mode) {
    if (mode < 0 || mode > kTempGuardModes) return TF_ERR_INVALID_ARGUMENT;
    unsigned long long old = g_temp_guard_state.load(std::memory_order_relaxed);
    while (!g_temp_guard_state.compare_exchange_weak(old, (old & ~0xFFull) | (unsigned long long)mode, std::memory_order_relaxed)) {
    }
    return TF_OK;
}

int force_temp_tables(int on) {
    g_force_temp_tables.store(on ? 1 : 0, std::memory_order_relaxed);
    return TF_OK;
}

int temp_guard_reset() {
    DeviceCtx* ctx = nullptr;
    TRY(current_ctx(&ctx));
    const int dev = (int)(ctx - g_ctx);
    HIPCHK(hipDeviceSynchronize());
    std::lock_guard<std::mutex> lk(g_mu);
    for (auto& l : g_labels) l.blocks = l.bytes = 0;
    if (g_ledger[dev]) HIPCHK(hipMemset(g_ledger[dev], 0, kTempGuardLedgerWords * sizeof(unsigned long long)));
    return TF_OK;
}

int temp_guard_report(uint64_t* ledger, uint64_t* label_blocks, uint64_t* label_bytes, size_t capacity, size_t* n_labels) {
    if (!ledger || !n_labels || (capacity && (!label_blocks || !label_bytes))) return TF_ERR_NULL_POINTER;
    DeviceCtx* ctx = nullptr;
    TRY(current_ctx(&ctx));
    const int dev = (int)(ctx - g_ctx);
    HIPCHK(hipDeviceSynchronize());
    std::lock_guard<std::mutex> lk(g_mu);
    std::fill(ledger, ledger + kTempGuardLedgerWords, uint64_t(0));
    if (g_ledger[dev]) HIPCHK(hipMemcpy(ledger, g_ledger[dev], kTempGuardLedgerWords * sizeof(uint64_t), hipMemcpyDeviceToHost));
    *n_labels = g_labels.size();
    for (size_t i = 0; i < g_labels.size() && i < capacity; ++i) {
        label_blocks[i] = g_labels[i].blocks;
        label_bytes[i] = g_labels[i].bytes;
    }
    return TF_OK;
}

const char* temp_guard_label(size_t id) {
    std::lock_guard<std::mutex> lk(g_mu);
    return id < g_labels.size() ? g_labels[id].text.c_str() : nullptr;  // (entries of the deque are never removed or rewritten)
}

int temp_guard_selftest(int defect, size_t n_words, uint64_t* out_word) {
    if (!out_word) return TF_ERR_NULL_POINTER;
    if (defect < 0 || defect > 5 || n_words == 0 || n_words > (size_t(1) << 24)) return TF_ERR_INVALID_ARGUMENT;
    if ((g_temp_guard_state.load(std::memory_order_relaxed) & 0xFF) == 0) return TF_ERR_INVALID_ARGUMENT;  // planted stores need their guards
    DeviceCtx* ctx = nullptr;
    TRY(current_ctx(&ctx));
    hipStream_t s = host_stream();
    DevTemp block(s), out(s);
    // the two blocks of the self-test, always taken together: the payload under test and the word the kernel hands back
    TRY(block.alloc_bytes(defect == 4 ? n_words * 8 + 4 : n_words * 8, "selftest"));
    TRY(out.alloc(1, "selftest"));
    {
        std::lock_guard<std::mutex> lk(g_mu);  // a block that was taken while another thread switched the mode off has no guards
        if (!g_blocks.count(block.p) || !g_blocks.count(out.p)) return TF_ERR_INVALID_ARGUMENT;
    }
    hipLaunchKernelGGL(temp_guard_selftest_kernel, dim3(1), dim3(64), 0, s, reinterpret_cast<unsigned long long*>(block.p), (long long)n_words, defect,
                       reinterpret_cast<unsigned long long*>(out.p));
    HIPCHK(hipGetLastError());
    TRY(d2h(reinterpret_cast<u64*>(out_word), out.p, 1, s));
    TRY(block.release());
    TRY(out.release());
    return sync(s);
}

}  // namespace tfi
