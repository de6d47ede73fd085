"""The fence harness (tests/fence.py) on CPU tensors: fake operations written with torch carry one defect each, and every one must be
reported with the right check, operand, offset and count; a correct operation passes under every poison and shift.  These fakes are
the mutation evidence for tests/test_gpu_fences.py -- nothing in the product is mutated.  The last test keeps the table of
test_gpu_fences.py complete: a public callable of twenty-first_amd/device.py without a row and without a commented exclusion fails."""
import inspect

import numpy as np
import pytest

from tests import fence

G = fence.G
N = 37


def _at(t, off):
    """the one word `off` words from the start of the view t, inside or outside of it (same storage)"""
    import torch

    return torch.as_strided(t, (1,), (1,), t.storage_offset() + off)


def _operands(n=N):
    rng = np.random.default_rng(7)
    a = rng.integers(1, 1 << 62, n, dtype=np.int64)
    b = rng.integers(1, 1 << 62, n, dtype=np.int64)
    return a, b, [fence.inp("a", a), fence.inp("b", b), fence.out("out", a + b)]


def good(a, b, out):
    out.copy_(a + b)


def store_before(a, b, out):
    good(a, b, out)
    _at(out, -1).fill_(0x1234567)


def store_behind(a, b, out):
    good(a, b, out)
    _at(out, out.numel()).fill_(0x1234567)


def store_far_behind(a, b, out):
    good(a, b, out)
    _at(out, out.numel() + G - 1).fill_(0x1234567)


def skip_word(a, b, out):
    keep = out[5].clone()
    good(a, b, out)
    out[5] = keep


def flip_input(a, b, out):
    good(a, b, out)
    a[3] ^= 1


def add_guard_word(a, b, out):
    good(a, b, out)
    out[-1] += _at(a, a.numel())[0]


def multiply_by_guard_word(a, b, out):
    good(a, b, out)
    out[-1] *= _at(a, a.numel())[0]


def _trip(op, shift, poison, operands=None):
    with pytest.raises(fence.FenceError) as e:
        fence.run_once("fake", f"n={N}", operands or _operands()[2], op, shift, poison, device="cpu")
    return e.value


@pytest.mark.parametrize("shift", fence.SHIFTS)
@pytest.mark.parametrize("poison", fence.POISONS)
def test_every_fake_defect_is_reported(shift, poison):
    for op, check, operand, offset in ((store_before, "guard", "out", -1), (store_behind, "guard", "out", N),
                                       (store_far_behind, "guard", "out", N + G - 1), (skip_word, "output", "out", 5),
                                       (flip_input, "input", "a", 3)):
        e = _trip(op, shift, poison)
        assert (e.check, e.operand, e.offset, e.count) == (check, operand, offset, 1), (op.__name__, str(e))
        assert (e.entry, e.shape, e.shift, e.poison) == ("fake", f"n={N}", shift, poison)
        for word in ("fake", f"n={N}", f"shift {shift}", f"poison {poison}", f"'{check}'", f"offset {offset}", "1 offending"):
            assert word in str(e), (word, str(e))


@pytest.mark.parametrize("shift", fence.SHIFTS)
def test_a_stray_load_shows_under_the_poisons_that_are_not_its_identity(shift):
    ops = _operands()[2]
    # an extra term of a sum: zero hides it, the other two fills do not
    fence.run_once("fake", f"n={N}", ops, add_guard_word, shift, "zeros", device="cpu")
    for poison in ("ones", "random"):
        e = _trip(add_guard_word, shift, poison)
        assert (e.check, e.operand, e.offset, e.count) == ("output", "out", N - 1, 1)
    # an extra factor of a product: zero wipes the result, all ones negates it
    for poison in fence.POISONS:
        e = _trip(multiply_by_guard_word, shift, poison)
        assert (e.check, e.operand, e.offset, e.count) == ("output", "out", N - 1, 1)
    # run() walks every poison, so the sum is caught as well, and by the first fill that can see it
    with pytest.raises(fence.FenceError) as e:
        fence.run("fake", f"n={N}", ops, add_guard_word, device="cpu", shifts=(shift,))
    assert e.value.poison == "ones"


def test_a_correct_operation_passes_every_poison_and_shift():
    fence.run("fake", f"n={N}", _operands()[2], good, device="cpu")
    fence.run("fake", "n=0", _operands(0)[2], good, device="cpu")


def test_payloads_sit_on_and_off_a_16_byte_boundary():
    seen = []

    def look(a, b, out):
        seen.append((a.data_ptr() % 16, out.data_ptr() % 16, a.is_contiguous(), a.numel()))
        good(a, b, out)

    fence.run("fake", f"n={N}", _operands()[2], look, device="cpu", poisons=("zeros",))
    assert seen == [(0, 0, True, N), (8, 8, True, N)]


def test_poisons_are_what_they_claim():
    z, o, r = (fence.poison_words(k, 1000) for k in fence.POISONS)
    assert not z.any() and (o == np.uint64(2 ** 64 - 1)).all() and int(o[0]) >= fence.P
    assert (r < np.uint64(fence.P)).all() and (r != 0).all() and np.unique(r).size == 1000
    assert np.array_equal(r, fence.poison_words("random", 1000)) and not np.array_equal(r, fence.poison_words("random", 1000, salt=1))
    z, o, r = (fence.poison_words(k, 1000, "int32") for k in fence.POISONS)
    assert not z.any() and (o.view(np.int32) == -1).all() and (r.view(np.int32) > 1 << 30).all()


def test_padding_kept_slots_and_32_bit_operands():
    """a strided input whose padding may not be looked at, an output with a slot that stays as it was, an int32 status"""
    n = 8
    cols = np.arange(1, 2 * n + 1, dtype=np.int64)
    padding = np.zeros(2 * n, dtype=bool)
    padding[n - 2:n] = True        # two padding words behind the first column of 6
    kept = np.zeros(n - 2, dtype=bool)
    kept[4] = True

    def ops():
        want = cols[:n - 2] + cols[n:2 * n - 2]
        return [fence.inp("cols", cols, padding=padding), fence.out("out", want, kept=kept),
                fence.inout("status", np.array([5], dtype=np.int32), np.array([5], dtype=np.int32), dtype="int32"),
                fence.out("flags", np.array([1, 0, 1], dtype=np.int32), dtype="int32")]

    def fine(cols, out, status, flags):
        s = cols[:n - 2] + cols[n:2 * n - 2]
        out[:4] = s[:4]
        out[5:] = s[5:]
        flags.copy_(flags.new_tensor([1, 0, 1]))

    fence.run("fake", "padded", ops(), fine, device="cpu")

    def reads_padding(cols, out, status, flags):
        fine(cols, out, status, flags)
        out[0] += cols[n - 1]

    def writes_kept(cols, out, status, flags):
        fine(cols, out, status, flags)
        out[4] = 99

    def writes_padding(cols, out, status, flags):
        fine(cols, out, status, flags)
        cols[n - 2] = 99

    def sets_status(cols, out, status, flags):
        fine(cols, out, status, flags)
        status[0] = 12

    def flag_behind(cols, out, status, flags):
        fine(cols, out, status, flags)
        _at(flags, 3).fill_(7)

    for op, poison, want in ((reads_padding, "ones", ("output", "out", 0, 1)), (writes_kept, "zeros", ("kept", "out", 4, 1)),
                             (writes_padding, "zeros", ("input", "cols", n - 2, 1)), (sets_status, "random", ("output", "status", 0, 1)),
                             (flag_behind, "random", ("guard", "flags", 3, 1))):
        with pytest.raises(fence.FenceError) as e:
            fence.run_once("fake", "padded", ops(), op, 1, poison, device="cpu")
        assert (e.value.check, e.value.operand, e.value.offset, e.value.count) == want, op.__name__


def test_several_offending_words_are_counted_from_the_first():
    def tail(a, b, out):
        good(a, b, out)
        for k in (2, 3, 9):
            _at(out, out.numel() + k).fill_(0x55)

    e = _trip(tail, 0, "random")
    assert (e.check, e.offset, e.count) == ("guard", N + 2, 3)


# ------------------------------------------------------------------ the table of test_gpu_fences.py is complete
# public callables of device.py that need no row, each with its reason
NOT_FENCED = {
    "debug_mul_pow2_": "debug helper: tests/test_gpu_pow2_products.py carries its own canaries",
    "debug_field_op": "debug helper: tests/test_gpu_field_primitives.py puts canary words behind each output",
    "debug_ntt_network_": "debug helper: tests/test_gpu_ntt_networks.py puts canary words behind each output",
    "debug_ntt_network_config": "reads compile-time switches: no tensor",
    "authentication_path_words": "host arithmetic: no tensor",
    "authentication_structure_from_leafs_workspace": "host arithmetic: no tensor",
    "mmr_successor_proof_len": "host arithmetic: no tensor",
    "ZerofierTree.close": "releases the handle: no tensor",
}


def _public_callables(device):
    names = []
    for name, obj in vars(device).items():
        if name.startswith("_") or getattr(obj, "__module__", None) != device.__name__:
            continue
        if inspect.isfunction(obj):
            names.append(name)
        elif inspect.isclass(obj):
            names.append(name)  # the constructor
            names += [f"{name}.{m}" for m, f in vars(obj).items() if inspect.isfunction(f) and not m.startswith("_")]
    return names


def test_every_public_entry_point_of_device_py_has_a_fence_row(tf):
    from tests import test_gpu_fences

    names = _public_callables(tf.device)
    assert len(names) > 60 and "ZerofierTree.interpolate" in names and "ntt_" in names
    rows = set(test_gpu_fences.ROWS)
    missing = [n for n in names if n not in rows and n not in NOT_FENCED]
    assert not missing, f"device.py entry points without a row in tests/test_gpu_fences.py (or a reasoned exclusion here): {missing}"
    assert not rows & set(NOT_FENCED), "an entry point is both fenced and excluded"
    stale = [n for n in list(rows) + list(NOT_FENCED) if n not in names]
    assert not stale, f"rows or exclusions that name nothing in device.py: {stale}"
