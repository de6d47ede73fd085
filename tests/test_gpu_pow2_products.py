"""The power-of-two products of the NTT networks (gl::Pow2Mul and its sign, csrc/gl64.h) against Python integers.

tf_debug_mul_pow2_dev runs x <- x * 2^e mod p through exactly the hand-scheduled forms the networks use -- one block of four
and one block of two products per thread -- for ANY 64-bit input word: the lazy networks feed these products words >= p.
All 192 exponents (2 has order 192 mod p), every edge word of the carry paths, and 2^16 random words.
"""
import numpy as np
import pytest

P = 0xFFFFFFFF00000001
ALL = 2 ** 64 - 1
N_RANDOM = 1 << 16
GUARD = 64  # words behind the operands that the kernel must leave alone (the count is no multiple of a thread's six words)


def _edge_words():
    words = [0, 1, P - 1, P, P + 1, ALL, 2 ** 32 - 1, 2 ** 32, 2 ** 64 - 2 ** 32 - 1, 2 ** 64 - 2 ** 32 + 1]
    words += [(ALL << s) & ALL for s in range(64)]  # all-ones shifted left by every amount
    words += [ALL >> s for s in range(64)]          # ... and right
    return words


@pytest.fixture(scope="module")
def operands():
    """edge words + 2^16 random words: half uniform over 2^64, a quarter in [p, 2^64) (non-canonical, as lazy operands are),
    a quarter with an all-ones or all-zeros half (the words on which a carry or borrow ripples through)."""
    rng = np.random.default_rng(0x706F7732)
    q = N_RANDOM // 4
    uniform = rng.integers(0, 2 ** 64, size=2 * q, dtype=np.uint64)
    above_p = np.uint64(P) + rng.integers(0, 2 ** 32 - 1, size=q, dtype=np.uint64)
    half = rng.integers(0, 2 ** 32, size=q, dtype=np.uint64)
    kind = rng.integers(0, 4, size=q)
    rippling = np.where(kind == 0, half, np.where(kind == 1, half << np.uint64(32), np.where(
        kind == 2, half | np.uint64(0xFFFFFFFF00000000), (half << np.uint64(32)) | np.uint64(0xFFFFFFFF))))
    x = np.concatenate([np.array(_edge_words(), dtype=np.uint64), uniform, above_p, rippling.astype(np.uint64)])
    assert int((x >= np.uint64(P)).sum()) >= q and len(x) % 6 != 0
    x.setflags(write=False)
    return x, [int(v) for v in x]


@pytest.mark.gpu
@pytest.mark.parametrize("first", range(0, 192, 24))
def test_every_exponent_against_python_integers(tf, operands, first):
    """x * 2^e mod p, canonical, for e = first .. first + 23 (all 192 over the eight cases), on edge and random words"""
    import torch

    assert tf.lib().tf_device_count() > 0, "no HIP device visible: the product has no CPU fallback"
    x, ints = operands
    n = len(x)
    canary = np.full(GUARD, 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    src = torch.from_numpy(np.concatenate([x, canary]).view(np.int64)).cuda()
    for e in range(first, first + 24):
        d = src.clone()
        tf.device.debug_mul_pow2_(d[:n], e)
        torch.cuda.synchronize()
        got = d.cpu().numpy().view(np.uint64)
        want = np.array([(v << e) % P for v in ints], dtype=np.uint64)
        bad = np.nonzero(got[:n] != want)[0]
        assert bad.size == 0, f"e = {e}: {bad.size} words differ, first x = {ints[bad[0]]:#x}: got {int(got[bad[0]]):#x}, want {int(want[bad[0]]):#x}"
        assert np.array_equal(got[n:], canary), f"e = {e}: words behind the operands were written"


@pytest.mark.gpu
@pytest.mark.parametrize("count", [1, 3, 4, 5, 6, 7, 1535, 1536, 1537])
def test_ragged_counts(tf, count):
    """counts around a thread's six words (a partial block of four, a partial block of two) and around one workgroup's 1536"""
    import torch

    rng = np.random.default_rng(count)
    x = rng.integers(0, 2 ** 64, size=count + GUARD, dtype=np.uint64)
    d = torch.from_numpy(x.view(np.int64)).cuda()
    for e in (7, 42, 78, 96, 191):  # one exponent per form, the pass-through and the largest
        tf.device.debug_mul_pow2_(d[:count], e)
    torch.cuda.synchronize()
    got = d.cpu().numpy().view(np.uint64)
    k = 7 + 42 + 78 + 96 + 191
    assert [int(v) for v in got[:count]] == [(int(v) << k) % P for v in x[:count]]
    assert np.array_equal(got[count:], x[count:])


def test_exponent_out_of_range_is_an_error(tf):
    """no device needed: the exponent is checked before anything is launched"""
    lib = tf.lib()
    assert lib.tf_debug_mul_pow2_dev(None, 0, 192, None) == 17  # TF_ERR_INVALID_ARGUMENT
    assert lib.tf_debug_mul_pow2_dev(None, 0, -1, None) == 17
    assert lib.tf_debug_mul_pow2_dev(None, 0, 0, None) == 0  # nothing to do
