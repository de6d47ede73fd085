"""Device-resident Tip5 sponges on the GPU: init, absorb, pad_and_absorb_all, squeeze, sample_scalars, sample_indices, bit-exact --
states AND outputs -- against tests/sponge_ref.py (the reference's functions restated on the KAT-pinned oracle permutation).

Counts 1, 3, 16, 17 run the latency form on a row pair per sponge, 4096 on a row per sponge, 2^13 + 5 the matrix-pipe form.  Up to
4096 every sponge is checked on the CPU; for the large count the CPU checks the first, the last and a fixed sample of 256, and all
the others are compared between the two GPU forms: the same inputs run once whole (matrix-pipe form) and once in calls of at most
2^13 sponges (latency form), so no sponge is left unchecked."""
import os
import subprocess

import numpy as np
import pytest

from tests import sponge_ref as ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COOP_MAX = 1 << 13
BIG = COOP_MAX + 5
COUNTS = [1, 3, 16, 17, 4096, BIG]
P = ref.P


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(tf):
    assert tf.lib().tf_device_count() > 0, "no HIP device visible: the product has no CPU fallback"


def to_dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).reshape(-1).view(np.int64)).cuda()


def to_host(t):
    import torch

    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint64)


def rand_states(oracle, count, seed):
    return oracle.fill_random(16 * count, seed).reshape(count, 16)


def cpu_checked(count):
    if count <= 4096:
        return range(count)
    rng = np.random.default_rng(0x5A3B1E)
    return sorted({0, count - 1, *rng.choice(count, 256, replace=False).tolist()})


# ---- one GPU call of each kind on sponges [lo, hi) of a batch: (new states, output) ---------------------------------------------
def gpu_squeeze(tf, k):
    def run(st, lo, hi):
        import torch

        d, out = to_dev(st[lo:hi]), torch.full(((hi - lo) * k * 10,), -1, dtype=torch.int64, device="cuda")  # (not canonical: a word never stored shows)
        tf.device.tip5_sponge_squeeze(d, out)
        return to_host(d).reshape(-1, 16), to_host(out).reshape(hi - lo, k, 10)
    return run


def gpu_scalars(tf, n):
    def run(st, lo, hi):
        import torch

        d, out = to_dev(st[lo:hi]), torch.full(((hi - lo) * n * 3,), -1, dtype=torch.int64, device="cuda")
        tf.device.tip5_sponge_sample_scalars(d, out)
        return to_host(d).reshape(-1, 16), to_host(out).reshape(hi - lo, n, 3)
    return run


def gpu_indices(tf, upper_bound, n):
    def run(st, lo, hi):
        import torch

        d, out = to_dev(st[lo:hi]), torch.full(((hi - lo) * n,), -1, dtype=torch.int32, device="cuda")
        tf.device.tip5_sponge_sample_indices(d, upper_bound, out)
        torch.cuda.synchronize()
        return to_host(d).reshape(-1, 16), out.cpu().numpy().view(np.uint32).reshape(hi - lo, n)
    return run


def gpu_absorb(tf, chunks):  # chunks: (count, k, 10)
    def run(st, lo, hi):
        d = to_dev(st[lo:hi])
        tf.device.tip5_sponge_absorb_(d, to_dev(chunks[lo:hi]))
        return to_host(d).reshape(-1, 16), None
    return run


def gpu_pad_uniform(tf, rows):  # rows: (count, len)
    def run(st, lo, hi):
        d = to_dev(st[lo:hi])
        tf.device.tip5_sponge_pad_and_absorb_all_(d, to_dev(rows[lo:hi]))
        return to_host(d).reshape(-1, 16), None
    return run


def gpu_pad_ragged(tf, words, offsets):
    def run(st, lo, hi):
        d = to_dev(st[lo:hi])
        # the whole input stays where it is; the call gets this slice's offsets into it
        tf.device.tip5_sponge_pad_and_absorb_all_(d, to_dev(words), offsets=offsets[lo:hi + 1])
        return to_host(d).reshape(-1, 16), None
    return run


def check(st, gpu, cpu):
    """gpu(st, lo, hi) against cpu(i, state) -> (state, output or None), as the module docstring describes"""
    count = st.shape[0]
    got_s, got_o = gpu(st, 0, count)
    for i in cpu_checked(count):
        want_s, want_o = cpu(i, st[i])
        assert np.array_equal(got_s[i], want_s), f"state of sponge {i} of {count}"
        if want_o is not None:
            assert np.array_equal(got_o[i], want_o), f"output of sponge {i} of {count}"
    if count > COOP_MAX:
        for lo in range(0, count, COOP_MAX):
            hi = min(count, lo + COOP_MAX)
            part_s, part_o = gpu(st, lo, hi)
            assert np.array_equal(part_s, got_s[lo:hi]), "the two kernel forms disagree on a state"
            if got_o is not None:
                assert np.array_equal(part_o, got_o[lo:hi]), "the two kernel forms disagree on an output"


# ---- init --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("fixed", [False, True])
def test_init(tf, count, fixed):
    import torch

    d = torch.full((16 * count,), 0x5555, dtype=torch.int64, device="cuda")
    tf.device.tip5_sponge_init_(d, fixed_length=fixed)
    assert np.array_equal(to_host(d).reshape(count, 16), np.tile(ref.init(fixed), (count, 1)))


# ---- squeeze / sample_scalars ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("k", [0, 1, 7])
def test_squeeze(tf, oracle, count, k):
    st = rand_states(oracle, count, 0x510 + k)
    check(st, gpu_squeeze(tf, k), lambda i, s: ref.squeeze_many(s, k))


@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("n", [0, 1, 3, 4, 10, 100])
def test_sample_scalars(tf, oracle, count, n):
    st = rand_states(oracle, count, 0x520 + n)
    check(st, gpu_scalars(tf, n), lambda i, s: ref.sample_scalars(s, n))


# ---- absorb / pad_and_absorb_all ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("k", [0, 1, 5])
def test_absorb(tf, oracle, count, k):
    st = rand_states(oracle, count, 0x530 + k)
    chunks = oracle.fill_random(count * k * 10, 0x531 + k).reshape(count, k, 10)
    check(st, gpu_absorb(tf, chunks), lambda i, s: (ref.absorb_many(s, chunks[i]), None))


@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("length", [0, 9, 10, 33])
def test_pad_and_absorb_all_uniform(tf, oracle, count, length):
    st = rand_states(oracle, count, 0x540 + length)
    rows = oracle.fill_random(count * length, 0x541 + length).reshape(count, length)
    check(st, gpu_pad_uniform(tf, rows), lambda i, s: (ref.pad_and_absorb_all(s, rows[i]), None))


@pytest.mark.parametrize("count", COUNTS)
def test_pad_and_absorb_all_ragged(tf, oracle, count):
    """lengths i * 7 mod 61: 0 is among them, and the sponges of one wave end after different numbers of steps"""
    lengths = np.array([(i * 7) % 61 for i in range(count)], dtype=np.uint64)
    offsets = np.zeros(count + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum(lengths)
    words = oracle.fill_random(max(int(offsets[-1]), 1), 0x551)
    st = rand_states(oracle, count, 0x550)
    check(st, gpu_pad_ragged(tf, words, offsets),
          lambda i, s: (ref.pad_and_absorb_all(s, words[int(offsets[i]):int(offsets[i + 1])]), None))


@pytest.mark.parametrize("count", [100, BIG])
def test_fresh_sponge_then_pad_and_absorb_all_is_hash_varlen_rows(tf, oracle, count):
    import torch

    rows = to_dev(oracle.fill_random(count * 33, 0x560))
    d = torch.full((16 * count,), -1, dtype=torch.int64, device="cuda")  # (not canonical: a word never stored shows)
    tf.device.tip5_sponge_init_(d)
    tf.device.tip5_sponge_pad_and_absorb_all_(d, rows)
    digests = torch.full((5 * count,), -1, dtype=torch.int64, device="cuda")
    tf.device.tip5_hash_varlen_rows(rows, 33, digests)
    assert np.array_equal(to_host(d).reshape(count, 16)[:, :5], to_host(digests).reshape(count, 5))


# ---- sample_indices ----------------------------------------------------------------------------------------------------------
INDEX_CASES = [(2, 0), (4, 1), (8, 9), (16, 10), (32, 11), (64, 19), (128, 20), (256, 21), (512, 65), (1 << 31, 40), (1, 5)]


@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("upper_bound,num", INDEX_CASES)
def test_sample_indices(tf, oracle, count, upper_bound, num):
    st = rand_states(oracle, count, 0x570 + num)
    check(st, gpu_indices(tf, upper_bound, num), lambda i, s: ref.sample_indices(s, upper_bound, num))


def crafted_states(oracle, count):
    """kind i % 5 -- 0: MAX in rate positions 0, 4, 9 (two squeezes for ten indices); 1: MAX in all ten (two squeezes); 2: none (one);
    3: a rate word whose canonical value has all-ones low 32 bits but is not MAX (kept, one squeeze); 4: the raw word p - 1, which
    is not MAX in Montgomery form (kept, one squeeze).  The kinds alternate, so every wave of every form holds a mix."""
    st = rand_states(oracle, count, 0x580)
    kinds = np.arange(count) % 5
    for k in (0, 4, 9):
        st[kinds == 0, k] = ref.MAX_RAW
    st[kinds == 1, :10] = ref.MAX_RAW
    st[kinds == 3, 2] = oracle.bfe_new(0x12345678FFFFFFFF)
    st[kinds == 4, 2] = 0xFFFFFFFF00000000
    return st, kinds


@pytest.mark.parametrize("count", [40, 4096, BIG])
def test_sample_indices_skips_max(tf, oracle, count):
    st, kinds = crafted_states(oracle, count)
    assert ref.value(oracle.bfe_new(0x12345678FFFFFFFF)) == 0x12345678FFFFFFFF
    check(st, gpu_indices(tf, 1 << 20, 10), lambda i, s: ref.sample_indices(s, 1 << 20, 10))
    # what the reference text says about these states, independent of the restatement's loop
    got_s, got_o = gpu_indices(tf, 1 << 20, 10)(st, 0, count)
    for i in range(10):
        once = oracle.tip5_permutation(st[i])
        assert np.array_equal(got_s[i], oracle.tip5_permutation(once) if kinds[i] < 2 else once)
    assert got_o[1].tolist() == [ref.value(w) & 0xFFFFF for w in oracle.tip5_permutation(st[1])[:10]]
    assert got_o[3, 2] == 0xFFFFF and got_o[4, 2] == ref.value(0xFFFFFFFF00000000) & 0xFFFFF


# ---- the two forms of the ABI, streams, the host classes ---------------------------------------------------------------------
def test_host_pointer_forms_match_the_dev_forms(tf, oracle):
    count = 37
    st = rand_states(oracle, count, 0x590)
    rows = oracle.fill_random(count * 23, 0x591).reshape(count, 23)
    chunks = oracle.fill_random(count * 30, 0x592).reshape(count, 3, 10)
    sp = tf.Tip5Sponge(count)
    sp.state[:] = st
    sp.pad_and_absorb_all(rows)
    s1, _ = gpu_pad_uniform(tf, rows)(st, 0, count)
    assert np.array_equal(sp.state, s1)
    sp.absorb_many(chunks)
    s2, _ = gpu_absorb(tf, chunks)(s1, 0, count)
    assert np.array_equal(sp.state, s2)
    out = sp.squeeze_many(3)
    s3, o3 = gpu_squeeze(tf, 3)(s2, 0, count)
    assert np.array_equal(sp.state, s3) and np.array_equal(out, o3)
    sc = sp.sample_scalars(7)
    s4, o4 = gpu_scalars(tf, 7)(s3, 0, count)
    assert np.array_equal(sp.state, s4) and np.array_equal(sc, o4)
    idx = sp.sample_indices(1 << 10, 33)
    s5, o5 = gpu_indices(tf, 1 << 10, 33)(s4, 0, count)
    assert np.array_equal(sp.state, s5) and np.array_equal(idx, o5) and idx.dtype == np.uint32
    ragged = [rows[i, : (i * 7) % 24] for i in range(count)]
    sp.pad_and_absorb_all(ragged)
    for i in range(count):
        assert np.array_equal(sp.state[i], ref.pad_and_absorb_all(s5[i], ragged[i]))
    sp_before = sp.state.copy()
    # rows without a word: only the states go to the device, every sponge absorbs the padding chunk
    sp.pad_and_absorb_all(np.zeros((count, 0), dtype=np.uint64))
    for i in range(count):
        assert np.array_equal(sp.state[i], ref.pad_and_absorb_all(sp_before[i], np.zeros(0, dtype=np.uint64)))
    # Tip5::new through the host-pointer form
    raw = np.full(16 * 5, 7, dtype=np.uint64)
    assert tf.lib().tf_tip5_sponge_init(raw.ctypes.data, 5, 1) == 0
    assert np.array_equal(raw.reshape(5, 16), np.tile(ref.init(True), (5, 1)))


def test_tip5sponge_existing_methods_keep_their_words(tf, oracle):
    sp = tf.Tip5Sponge(3)
    rows = oracle.fill_random(3 * 25, 0x5A0).reshape(3, 25)
    sp.pad_and_absorb_all(rows)
    for i in range(3):
        assert np.array_equal(sp.state[i, :5], oracle.hash_varlen(rows[i]))
    before = sp.state.copy()
    out = sp.squeeze()
    for i in range(3):
        s, o = ref.squeeze(before[i])
        assert np.array_equal(sp.state[i], s) and np.array_equal(out[i], o)


def test_dev_calls_on_a_non_default_stream(tf, oracle):
    import torch

    count = 300
    st = rand_states(oracle, count, 0x5B0)
    lengths = np.array([(i * 7) % 61 for i in range(count)], dtype=np.uint64)
    offsets = np.zeros(count + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum(lengths)
    words = oracle.fill_random(int(offsets[-1]), 0x5B1)
    d, w = to_dev(st), to_dev(words)
    sc = torch.zeros(count * 4 * 3, dtype=torch.int64, device="cuda")
    idx = torch.zeros(count * 12, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    tf.device.tip5_sponge_pad_and_absorb_all_(d, w, offsets=offsets, stream=stream)
    tf.device.tip5_sponge_sample_scalars(d, sc, stream=stream)
    tf.device.tip5_sponge_sample_indices(d, 1 << 16, idx, stream=stream)
    stream.synchronize()
    got_s, got_sc, got_idx = to_host(d).reshape(count, 16), to_host(sc).reshape(count, 4, 3), idx.cpu().numpy().view(np.uint32).reshape(count, 12)
    for i in range(count):
        s = ref.pad_and_absorb_all(st[i], words[int(offsets[i]):int(offsets[i + 1])])
        s, want_sc = ref.sample_scalars(s, 4)
        s, want_idx = ref.sample_indices(s, 1 << 16, 12)
        assert np.array_equal(got_s[i], s) and np.array_equal(got_sc[i], want_sc) and np.array_equal(got_idx[i], want_idx)


def test_cpp_mirror_sponge_selftest_on_gpu():
    host = os.path.join(ROOT, "twenty-first_amd", "host")
    subprocess.check_call(["make", "-C", host, "sponge_selftest"], stdout=subprocess.DEVNULL)
    r = subprocess.run([os.path.join(host, "sponge_selftest")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
