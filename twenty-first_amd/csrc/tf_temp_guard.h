// tf_temp_guard.h -- the constants and the poison sequence of the guard mode for library-owned device memory (tf_debug_temp_guard,
// include/tf_hip.h; the mechanism is tf_temp_guard.hip).  Plain C++ when a host compiler reads it: tests/test_temp_guard_cpu.py
// compiles it alone and compares the constant and the first words of the sequence with tests/fence.py.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define TF_TG_HD __host__ __device__
#else
#define TF_TG_HD
#endif

namespace tfi {

// Guard words on each side of a guarded block: tests/fence.py's G (the largest per-workgroup tile of any kernel, 16 384 words, plus
// 4096).  kTempGuardWords * 8 is a multiple of 256, so the payload keeps the alignment the pool gives the block.
constexpr size_t kTempGuardWords = 16384 + 4096;
static_assert((kTempGuardWords * 8) % 256 == 0, "the payload must keep the pool's alignment");

constexpr int kTempGuardModes = 3;  // 1 zeros, 2 all ones, 3 the canonical pseudo-random words: fence.POISONS, in this order

// word i of fence._poison_sequence(kind, ., "int64", salt = 0); i counts 64-bit words from the BASE of the guarded block (the front
// guard starts at word 0), so the check kernel recomputes any word from its index
TF_TG_HD inline uint64_t temp_guard_poison(int mode, uint64_t i) {
    if (mode == 1) return 0;
    if (mode == 2) return ~uint64_t(0);
    uint64_t z = (i + 0xFE4CEull) * 0x9E3779B97F4A7C15ull + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z % 0xFFFFFFFF00000000ull + 1;  // canonical (below p = 2^64 - 2^32 + 1) and never 0
}
// the 32-bit entry e of the block (the check compares entries: a payload may end on a 4-byte boundary)
TF_TG_HD inline uint32_t temp_guard_poison32(int mode, uint64_t e) { return uint32_t(temp_guard_poison(mode, e >> 1) >> (32 * (e & 1))); }

// the ledger as tf_debug_temp_guard_report returns it (64-bit words)
enum : int {
    kTgBlocksChecked = 0,    // guarded blocks freed (and so checked) since the last reset
    kTgBlocksOffending = 1,  // of these, blocks with an offending entry in either guard
    kTgEntriesOffending = 2, // offending 32-bit entries in total
    kTgRecords = 3,          // records that follow (at most kTempGuardRecords; later offending guards are only counted)
    kTgRecordBase = 4,       // per record: label id, side (0 front, 1 back), payload-relative offset of the first offending entry
    kTgRecordWords = 4,      //             (32-bit entries; negative in the front guard), offending entries of that guard
    kTempGuardRecords = 16,
    kTempGuardLedgerWords = kTgRecordBase + kTgRecordWords * kTempGuardRecords,
};

}  // namespace tfi
