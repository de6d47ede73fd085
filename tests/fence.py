"""Guard-word harness for the device entry points: where a call touches memory, not what it computes.

Every tensor argument of a fenced call lives inside its own, larger allocation

    [ front guard | shift | payload | back guard ]

and only `payload` (a contiguous view) is handed to the wrapper.  The guards of every argument, the whole payload of every pure
output and the padding words of padded operands are filled with a poison before the call; the call runs once per poison and per
shift.  After ONE synchronisation four things are checked, in this order:

    guard   every word of the allocation outside the payload still holds its fill            (a store past either end)
    input   every const input payload is bit-identical to what was uploaded                  (a const operand modified)
    output  every output word equals the reference                                            (a word never stored; a stray load that
                                                                                               reaches the result shows under one of the
                                                                                               three poisons: zero hides an extra term of
                                                                                               a sum, ones and the random words do not)
    kept    a slot the documentation leaves "as it was", and every padding word, holds its poison

The arena is plain torch and works on CPU tensors as well: tests/test_fence_cpu.py feeds it fake operations with each defect and
checks that each is reported with the right check and offset.

The arena sees the tensor arguments only.  The library's own device memory -- the pool temporaries of every call and the buffers of
the host-pointer / numpy API -- is fenced by the library itself: tf_debug_temp_guard (include/tf_hip.h) puts G poisoned words on each
side of every block it takes, poisons the block, and checks the guards when the block is given back.  temp_guarded() below switches
that mode on around a call and asserts a clean ledger; tests/test_gpu_temp_guard.py runs every fenced call and every host form under
it.  What remains unseen after both: memory the library keeps for the life of the process (cached twiddle and power tables, the
Tip5 constants, the arena of a persistent zerofier tree), its page-locked staging blocks, and a stray LOAD from a neighbouring
allocation that happens to hold the same words under all three poisons.
"""
import contextlib
import ctypes

import numpy as np

# Guard words (entries, for the 32-bit tensors) on each side of a payload.  A condition, not a measurement: G must exceed what ONE
# workgroup of any kernel reached at the fenced shapes moves per step of its launch, so that a workgroup that starts one tile early,
# or runs one tile past the end of its operand, lands inside a guard and not in a neighbouring allocation.  Per workgroup, from the
# kernel headers (csrc/*.h):
#   ntt_pass_kernel, ntt_col1024_chain_kernel, ntt_col2048_kernel   512 threads x 32 rows (2048 rows x 8 columns)   16 384 words
#   ntt_block_kernel (2^11 <= n <= 2^14, BFE)                       a whole transform: "one 512-thread tile"        16 384 words
#   ntt_rows32_kernel                                               512 transforms of 32 (170 x 32 x 3 for XFE)      16 384 words
#   ntt_lat_kernel                                                  a whole transform of <= 4096 points, x 3 for XFE 12 288 words
#   batch_inverse_kernel                                            4 waves x 64 lanes x 16 (x 8 x 3 for XFE)        4096 / 6144 words
#   get_colinear_y_kernel                                           4 waves x 64 lanes x 8 / 8 / 4 triples x 1 / 3 / 3 words <= 6144 words
#   tip5_permute_mx_kernel with a trace                             64 permutations (4 lanes each) x 96 words        6144 words
#   leaf kernels of the zerofier tree                               1024 points x 3 words                            3072 words
# Everything else stays far below these: a few words per thread of a 256-thread workgroup, 128 pairs of digests for a workgroup of the
# Merkle subtree kernel.  The largest is 16 384 words; G is that plus 4096.
G = 16384 + 4096

P = (1 << 64) - (1 << 32) + 1
POISONS = ("zeros", "ones", "random")
SHIFTS = (0, 1)
CHECKS = ("guard", "input", "output", "kept")

_NP = {"int64": np.uint64, "int32": np.uint32}


class FenceError(AssertionError):
    """One tripped fence: which entry point, shape, shift and poison, which check, on which operand, the offset of the first
    offending word relative to the payload (negative: before its start; >= the payload's length: behind its end) and how many words
    offend."""

    def __init__(self, entry, shape, shift, poison, check, operand, offset, count):
        self.entry, self.shape, self.shift, self.poison = entry, shape, shift, poison
        self.check, self.operand, self.offset, self.count = check, operand, int(offset), int(count)
        super().__init__(f"{entry} {shape}: shift {shift}, poison {poison}: check '{check}' failed on '{operand}': first offending word at "
                         f"payload offset {self.offset}, {self.count} offending word(s)")


def _splitmix(idx):
    z = idx * np.uint64(0x9E3779B97F4A7C15) + np.uint64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


_poison_cache = {}


def _poison_sequence(kind, count, dtype, salt):
    npt = _NP[dtype]
    if kind == "zeros":
        return np.zeros(count, dtype=npt)
    if kind == "ones":
        return np.full(count, np.iinfo(npt).max, dtype=npt)
    assert kind == "random"
    with np.errstate(over="ignore"):
        z = _splitmix(np.arange(count, dtype=np.uint64) + np.uint64(0xFE4CE + 0x10001 * salt))
    if dtype == "int32":
        return (z >> np.uint64(33)).astype(np.uint32) | np.uint32(0x40000000)  # positive, far beyond any count or index in use
    return z % np.uint64(P - 1) + np.uint64(1)


def poison_words(kind, count, dtype="int64", salt=0):
    """`count` poison words of one kind: all zero; all ones (as a 64-bit word not canonical: >= p); a fixed pseudo-random sequence
    (64-bit: canonical words below p, none of them 0) -- for the 32-bit tensors 0, -1 and a fixed pattern.  Word i depends on
    (kind, dtype, salt, i) only, so the sequences are generated once and handed out as copies of their prefixes."""
    key = (kind, dtype, salt)
    if key not in _poison_cache or _poison_cache[key].size < count:
        _poison_cache[key] = _poison_sequence(kind, max(count, 2 * G + (1 << 17) + 64), dtype, salt)
    return _poison_cache[key][:count].copy()


class Operand:
    """One tensor argument.  `data`: the payload before the call (None: a pure output, all poison); `poisoned`: bool mask of payload
    words that are filled with poison instead (padding of a strided operand, a status nobody pre-sets); `expect`: the payload after
    the call (None: a const input, which must come back as uploaded); `kept`: bool mask of payload words that must still hold what
    they held before the call, whatever `expect` says there."""

    def __init__(self, name, n, dtype="int64", data=None, poisoned=None, expect=None, kept=None, const=False):
        npt = _NP[dtype]
        self.name, self.n, self.dtype, self.const = name, int(n), dtype, const
        self.data = None if data is None else np.ascontiguousarray(data).reshape(-1).view(npt).copy()
        assert self.data is None or self.data.size == self.n, (name, self.n)
        self.poisoned = np.ones(self.n, dtype=bool) if data is None else (np.zeros(self.n, dtype=bool) if poisoned is None else np.asarray(poisoned, dtype=bool))
        self.expect = None if expect is None else np.ascontiguousarray(expect).reshape(-1).view(npt).copy()
        assert self.expect is None or self.expect.size == self.n, (name, self.n, self.expect.size)
        self.kept = np.zeros(self.n, dtype=bool) if kept is None else np.asarray(kept, dtype=bool)
        assert self.poisoned.size == self.n and self.kept.size == self.n, name


def inp(name, data, dtype="int64", padding=None):
    """a const input; `padding`: mask of words the call may not look at (poisoned, and they too come back unchanged)"""
    data = np.ascontiguousarray(data).reshape(-1)
    return Operand(name, data.size, dtype, data=data, poisoned=padding, const=True)


def out(name, expect, dtype="int64", kept=None):
    """a pure output of expect.size words, poisoned before the call; `kept`: mask of words that must still be poison afterwards"""
    expect = np.ascontiguousarray(expect).reshape(-1)
    return Operand(name, expect.size, dtype, expect=expect, kept=kept)


def inout(name, data, expect, dtype="int64", kept=None):
    """an operand updated in place"""
    data = np.ascontiguousarray(data).reshape(-1)
    return Operand(name, data.size, dtype, data=data, expect=expect, kept=kept)


def _torch_dtype(dtype):
    import torch

    return torch.int64 if dtype == "int64" else torch.int32


def _first(bad):
    idx = np.flatnonzero(bad)
    return (int(idx[0]), int(idx.size)) if idx.size else None


class _Slot:
    """one operand inside its arena"""

    def __init__(self, op, shift, poison, salt, device):
        import torch

        self.op = op
        item = 8 if op.dtype == "int64" else 4
        total = G + 16 + op.n + G
        self.buf = torch.empty(total, dtype=_torch_dtype(op.dtype), device=device)
        # the first entry at or behind the front guard that sits on a 16-byte boundary, then `shift` entries on
        start = G
        while (self.buf.data_ptr() + start * item) % 16:
            start += 1
        self.start = start + shift
        assert self.start + op.n + G <= total
        before = poison_words(poison, total, op.dtype, salt)
        if op.data is not None:
            pay = before[self.start:self.start + op.n]
            pay[~op.poisoned] = op.data[~op.poisoned]
        self.before = before
        self.buf.copy_(torch.from_numpy(before.view(np.int64 if op.dtype == "int64" else np.int32)))
        self.payload = self.buf[self.start:self.start + op.n]
        assert self.payload.is_contiguous() and (op.n == 0 or (self.payload.data_ptr() % 16 == 0) == (shift == 0))

    def check(self, report):
        op, s, n = self.op, self.start, self.op.n
        after = self.buf.cpu().numpy().view(_NP[op.dtype])
        bad = after != self.before
        inside = np.zeros(bad.size, dtype=bool)
        inside[s:s + n] = True
        hit = _first(bad & ~inside)
        if hit:
            report("guard", op.name, hit[0] - s, hit[1])
        pay, pre = after[s:s + n], self.before[s:s + n]
        if op.expect is None:
            hit = _first(pay != pre)
            if hit:
                report("input", op.name, *hit)
            return
        hit = _first((pay != op.expect) & ~op.kept)
        if hit:
            report("output", op.name, *hit)
        hit = _first((pay != pre) & op.kept)
        if hit:
            report("kept", op.name, *hit)


def run_once(entry, shape, operands, call, shift, poison, device="cuda"):
    """One fenced call: build the arenas, hand `call` the payload views by name, synchronise once, check.  Raises FenceError on the
    first failing check (guards of all operands first, then inputs, then outputs, then kept slots)."""
    import torch

    slots = [_Slot(op, shift, poison, k, device) for k, op in enumerate(operands)]
    call(**{s.op.name: s.payload for s in slots})
    if str(device).startswith("cuda"):
        torch.cuda.synchronize()
    found = []
    for s in slots:
        s.check(lambda check, operand, offset, count: found.append((CHECKS.index(check), check, operand, offset, count)))
    if found:
        _, check, operand, offset, count = min(found, key=lambda f: f[0])
        raise FenceError(entry, shape, shift, poison, check, operand, offset, count)


def run(entry, shape, operands, call, device="cuda", shifts=SHIFTS, poisons=POISONS):
    """The fenced call under every shift and every poison.  `call` must be repeatable: it is made once per combination, each time
    on fresh arenas."""
    for shift in shifts:
        for poison in poisons:
            run_once(entry, shape, operands, call, shift, poison, device)


# ------------------------------------------------------------------ the library's own device memory (tf_debug_temp_guard)
TEMP_POISONS = (1, 2, 3)          # the modes of tf_debug_temp_guard: POISONS, in this order
LEDGER_WORDS = 4 + 4 * 16         # TF_TEMP_GUARD_LEDGER_WORDS
SIDES = ("front", "back")


class TempGuardReport:
    """tf_debug_temp_guard_report, decoded: blocks checked, blocks with an offending entry, offending 32-bit entries, the records
    (label, side, payload-relative offset of the first offending entry, offending entries) of the first 16 offending guards, and
    {label: (blocks, bytes)} requested since the last reset (labels with no request left out)."""

    def __init__(self, lib):
        ledger = (ctypes.c_uint64 * LEDGER_WORDS)()
        n = ctypes.c_size_t(0)
        cap = 1024
        blocks, nbytes = (ctypes.c_uint64 * cap)(), (ctypes.c_uint64 * cap)()
        rc = lib.tf_debug_temp_guard_report(ledger, blocks, nbytes, cap, ctypes.byref(n))
        assert rc == 0 and n.value <= cap, (rc, n.value)
        text = lambda i: lib.tf_debug_temp_guard_label(i).decode()  # noqa: E731
        self.blocks_checked, self.blocks_offending, self.entries_offending = int(ledger[0]), int(ledger[1]), int(ledger[2])
        self.records = [(text(int(ledger[4 + 4 * r])), SIDES[int(ledger[5 + 4 * r])], int(np.uint64(ledger[6 + 4 * r]).astype(np.int64)), int(ledger[7 + 4 * r]))
                        for r in range(int(ledger[3]))]
        self.labels = {text(i): (int(blocks[i]), int(nbytes[i])) for i in range(n.value) if blocks[i]}

    def __repr__(self):
        return (f"checked {self.blocks_checked} blocks, {self.blocks_offending} offending, {self.entries_offending} offending entries, "
                f"records {self.records}, labels {self.labels}")


@contextlib.contextmanager
def temp_guarded(lib, mode, must_see=(), clean=True):
    """The body runs with the library's own device memory guarded and poisoned with `mode` (one of TEMP_POISONS): counters and ledger
    are reset before, the mode is switched off in any case, and after a body that did not raise the report is taken (it waits for
    the device) and must show no offending entry (clean) and at least one block under every label of `must_see`.  Yields a list that
    holds the report afterwards."""
    assert mode in TEMP_POISONS
    assert lib.tf_debug_temp_guard_reset() == 0
    assert lib.tf_debug_temp_guard(mode) == 0
    box = []
    try:
        yield box
        box.append(TempGuardReport(lib))
    finally:
        assert lib.tf_debug_temp_guard(0) == 0
    report = box[0]
    if clean:
        assert report.entries_offending == 0 and report.blocks_offending == 0, f"temporary poison {POISONS[mode - 1]}: a guard of the library's own memory was written: {report}"
    missing = [label for label in must_see if label not in report.labels]
    assert not missing, f"no block was requested under {missing}: {report}"
