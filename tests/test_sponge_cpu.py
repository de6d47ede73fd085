"""Tip5 sponges without a GPU: the restatement of the reference's sponge functions (tests/sponge_ref.py) against facts that do not
depend on it, and every argument error the six sponge calls return before they touch a device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import sponge_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "twenty-first_amd", "host")
NULL_POINTER, INVALID_ARGUMENT, NOT_POWER_OF_TWO = 7, 17, 26


# ------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("length", [0, 1, 9, 10, 11, 20, 33])
def test_ref_pad_and_absorb_all_is_hash_varlen(oracle, length):
    x = oracle.fill_random(length, 0x5B0 + length)
    assert np.array_equal(ref.pad_and_absorb_all(ref.init(), x)[:5], oracle.hash_varlen(x))


def test_ref_init_domains():
    assert not ref.init().any()
    f = ref.init(True)
    assert not f[:10].any() and (f[10:] == 0xFFFFFFFF).all()


@pytest.mark.parametrize("n", [0, 1, 3, 4, 10, 100])
def test_ref_sample_scalars_is_a_prefix_of_the_squeezes(oracle, n):
    s0 = oracle.fill_random(16, 0x5C0 + n)
    k = (3 * n + 9) // 10
    s_sq, words = ref.squeeze_many(s0, k)
    s, sc = ref.sample_scalars(s0, n)
    assert sc.shape == (n, 3) and np.array_equal(sc.reshape(-1), words.reshape(-1)[:3 * n])
    assert np.array_equal(s, s_sq)
    if n == 0:
        assert np.array_equal(s, s0)


def test_ref_squeeze_is_rate_then_permutation(oracle):
    s0 = oracle.fill_random(16, 0x5D0)
    s, out = ref.squeeze(s0)
    assert np.array_equal(out, s0[:10]) and np.array_equal(s, oracle.tip5_permutation(s0))


@pytest.mark.parametrize("upper_bound,num", [(2, 0), (4, 1), (8, 9), (16, 10), (32, 11), (64, 19), (128, 20), (256, 21), (512, 65),
                                              (1 << 31, 40), (1, 5)])
def test_ref_sample_indices_are_below_the_bound(oracle, upper_bound, num):
    s0 = oracle.fill_random(16, 0x5E0 + num)
    s, idx = ref.sample_indices(s0, upper_bound, num)
    assert idx.size == num and (idx < upper_bound).all()
    # no element of a hash output is MAX: the indices are the low bits of the first `num` squeezed values
    s_sq, words = ref.squeeze_many(s0, (num + 9) // 10)
    assert np.array_equal(s, s_sq)
    want = [(ref.value(w) & 0xFFFFFFFF) % upper_bound for w in words.reshape(-1)[:num]]
    assert idx.tolist() == want


def test_ref_sample_indices_skips_max(oracle):
    """the caller's state is what the first squeeze returns: MAX in rate positions {0, 4, 9} turns one squeeze into two when ten
    indices are wanted; an all-MAX rate yields its first index from the second squeeze"""
    base = oracle.fill_random(16, 0x5F0)
    some, every = base.copy(), base.copy()
    some[[0, 4, 9]] = ref.MAX_RAW
    every[:10] = ref.MAX_RAW
    s_none, i_none = ref.sample_indices(base, 1 << 20, 10)
    assert np.array_equal(s_none, oracle.tip5_permutation(base))
    s_some, i_some = ref.sample_indices(some, 1 << 20, 10)
    p1 = oracle.tip5_permutation(some)
    assert np.array_equal(s_some, oracle.tip5_permutation(p1))
    kept = [ref.value(w) & 0xFFFFF for k, w in enumerate(some[:10]) if k not in (0, 4, 9)] + [ref.value(w) & 0xFFFFF for w in p1[:3]]
    assert i_some.tolist() == kept
    s_every, i_every = ref.sample_indices(every, 1 << 20, 10)
    q1 = oracle.tip5_permutation(every)
    assert np.array_equal(s_every, oracle.tip5_permutation(q1))
    assert i_every.tolist() == [ref.value(w) & 0xFFFFF for w in q1[:10]]
    # p - 1 taken as a raw word is not MAX in Montgomery form: kept
    raw = base.copy()
    raw[0] = 0xFFFFFFFF00000000
    assert ref.value(raw[0]) != ref.P - 1
    assert ref.sample_indices(raw, 1 << 20, 10)[1][0] == ref.value(raw[0]) & 0xFFFFF


# ------------------------------------------------------------------ the C ABI without a device
def _p(a):
    return C.c_void_p(a.ctypes.data)


def test_status_string(tf):
    assert tf.lib().tf_status_string(NOT_POWER_OF_TWO) == b"TF_ERR_UPPER_BOUND_NOT_POWER_OF_TWO"


@pytest.mark.parametrize("dev", [False, True])
def test_count_zero_is_ok(tf, dev):
    L, tail = tf.lib(), ([None] if dev else [])
    sfx = "_dev" if dev else ""
    assert getattr(L, "tf_tip5_sponge_init" + sfx)(None, 0, 1, *tail) == 0
    assert getattr(L, "tf_tip5_sponge_absorb" + sfx)(None, 0, None, 3, *tail) == 0
    assert getattr(L, "tf_tip5_sponge_pad_and_absorb_all" + sfx)(None, 0, None, 7, None, *tail) == 0
    assert getattr(L, "tf_tip5_sponge_squeeze" + sfx)(None, 0, 2, None, *tail) == 0
    assert getattr(L, "tf_tip5_sponge_sample_scalars" + sfx)(None, 0, 2, None, *tail) == 0
    assert getattr(L, "tf_tip5_sponge_sample_indices" + sfx)(None, 0, 8, 2, None, *tail) == 0


@pytest.mark.parametrize("dev", [False, True])
def test_argument_errors_come_before_the_device(tf, dev):
    L, tail = tf.lib(), ([None] if dev else [])
    sfx = "_dev" if dev else ""
    st = np.zeros(32, dtype=np.uint64)
    buf = np.zeros(64, dtype=np.uint64)
    f = lambda name: getattr(L, name + sfx)  # noqa: E731
    assert f("tf_tip5_sponge_init")(None, 2, 0, *tail) == NULL_POINTER
    assert f("tf_tip5_sponge_absorb")(None, 2, _p(buf), 1, *tail) == NULL_POINTER
    assert f("tf_tip5_sponge_absorb")(_p(st), 2, None, 1, *tail) == NULL_POINTER
    assert f("tf_tip5_sponge_pad_and_absorb_all")(None, 2, _p(buf), 3, None, *tail) == NULL_POINTER
    assert f("tf_tip5_sponge_pad_and_absorb_all")(_p(st), 2, None, 3, None, *tail) == NULL_POINTER
    off = np.array([0, 5, 3], dtype=np.uint64)
    assert f("tf_tip5_sponge_pad_and_absorb_all")(_p(st), 2, _p(buf), 0, _p(off), *tail) == INVALID_ARGUMENT
    off = np.array([0, 5, 9], dtype=np.uint64)
    assert f("tf_tip5_sponge_pad_and_absorb_all")(_p(st), 2, None, 0, _p(off), *tail) == NULL_POINTER
    assert f("tf_tip5_sponge_squeeze")(None, 2, 1, _p(buf), *tail) == NULL_POINTER
    assert f("tf_tip5_sponge_squeeze")(_p(st), 2, 1, None, *tail) == NULL_POINTER
    assert f("tf_tip5_sponge_sample_scalars")(None, 2, 1, _p(buf), *tail) == NULL_POINTER
    assert f("tf_tip5_sponge_sample_scalars")(_p(st), 2, 1, None, *tail) == NULL_POINTER
    assert f("tf_tip5_sponge_sample_indices")(None, 2, 8, 1, _p(buf), *tail) == NULL_POINTER
    assert f("tf_tip5_sponge_sample_indices")(_p(st), 2, 8, 1, None, *tail) == NULL_POINTER
    for bad in (0, 3, 6, 12, (1 << 31) + 1, (1 << 32) - 1):
        assert f("tf_tip5_sponge_sample_indices")(_p(st), 2, bad, 1, _p(buf), *tail) == NOT_POWER_OF_TWO
    assert not st.any() and not buf.any()


def test_python_sample_indices_raises_status_26(tf):
    with pytest.raises(tf.TwentyFirstError) as e:
        tf.Tip5Sponge(2).sample_indices(12, 4)
    assert "TF_ERR_UPPER_BOUND_NOT_POWER_OF_TWO" in str(e.value)


def test_cpp_mirror_sponge_selftest_compiles(tf):
    subprocess.check_call(["make", "-C", HOST, "sponge_selftest"], stdout=subprocess.DEVNULL)
    assert os.path.exists(os.path.join(HOST, "sponge_selftest"))
    if tf.lib().tf_device_count() == 0:
        r = subprocess.run([os.path.join(HOST, "sponge_selftest")], capture_output=True, text=True, timeout=120)
        assert r.returncode == 77, r.stdout + r.stderr
