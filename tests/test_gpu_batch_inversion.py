"""Batch inversion (FiniteField::batch_inversion, math/traits.rs:93-121) and inverse_or_zero (:39-45) on the GPU, both widths.

Small sizes are compared word for word with tests/inversion_ref (pinned against pyref and the oracle by the CPU tests) and with the
oracle's bfe_inverse / xfe_inverse; the sizes sit on every boundary of the kernel (csrc/inverse_kernels.h): one wave's chunk of
64 K elements, one workgroup of four chunks, the grid-stride wrap.  Large inputs are checked with a different kernel (in * out == 1
through tf_hadamard_*_dev), every output word below p, and sampled positions against the oracle."""
import os
import subprocess

import numpy as np
import pytest

from tests import inversion_ref, pyref

pytestmark = pytest.mark.gpu

P = (1 << 64) - (1 << 32) + 1
ONE = 0xFFFFFFFF
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = {1: 16, 3: 8}  # elements per lane, tfk::InvGeom<L>::K
INVERSE_OF_ZERO = 12


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(tf):
    assert tf.lib().tf_device_count() > 0, "no HIP device visible: the product has no CPU fallback"


def _to_dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def _to_host(t):
    return t.cpu().numpy().view(np.uint64)


def _chunk(w):
    return 64 * K[w]


def _wrap(w):
    """elements one launch covers before its grid-stride loop wraps: 8 blocks per compute unit, four waves each"""
    import torch

    return torch.cuda.get_device_properties(0).multi_processor_count * 8 * 4 * _chunk(w)


def _oracle_inverses(oracle, x, w, idx):
    if w == 1:
        return np.array([oracle.bfe_inverse(int(x[i])) for i in idx], dtype=np.uint64)
    return np.concatenate([oracle.xfe_inverse(x[3 * i:3 * i + 3]) for i in idx]) if len(idx) else np.zeros(0, dtype=np.uint64)


def _one(w, n):
    e = np.zeros(w * n, dtype=np.uint64)
    e[::w] = ONE
    return e


def _small_sizes(w):
    c = _chunk(w)
    return sorted({1, 2, 3, 63, 64, 65, c - 1, c, c + 1, 4 * c - 1, 4 * c, 4 * c + 1, (1 << 16) + 7})


# ------------------------------------------------------------------ 1. small sizes, word for word
@pytest.mark.parametrize("w", [1, 3])
def test_small_sizes_word_for_word(tf, oracle, w):
    for n in _small_sizes(w):
        x = oracle.fill_random(w * n, 0x1B00 + n)
        want = inversion_ref.expected(x, w, or_zero=False)
        got = tf.batch_inversion(x, width=w)
        assert np.array_equal(got, want), n
        assert np.array_equal(tf.inverse_or_zero(x, width=w), want), n
        idx = sorted({0, n - 1, n // 2, min(n - 1, 64)})
        assert np.array_equal(_oracle_inverses(oracle, x, w, idx), np.concatenate([want[w * i:w * i + w] for i in idx])), n
    # pyref (Fermat) on the first elements of one size
    x = oracle.fill_random(w * 40, 0x1BFF)
    got = tf.batch_inversion(x, width=w)
    for i in range(40):
        if w == 1:
            assert int(got[i]) == pyref.to_raw(pow(pyref.to_val(int(x[i])), P - 2, P))
        else:
            vals = tuple(pyref.to_val(int(r)) for r in x[3 * i:3 * i + 3])
            assert [int(v) for v in got[3 * i:3 * i + 3]] == [pyref.to_raw(v) for v in pyref.xfe_inv(vals)]


@pytest.mark.parametrize("w", [1, 3])
def test_grid_stride_wrap(tf, oracle, w):
    """sizes where the launch's waves take a second chunk: the inverses checked with a different kernel and at sampled positions"""
    import torch

    for n in (_wrap(w) - 1, _wrap(w) + 1, _wrap(w) + _chunk(w) + 5):
        x = torch.empty(w * n, dtype=torch.int64, device="cuda")
        tf.device.fill_random(x, 0x1C00 + n)
        y = torch.full_like(x, -1)  # (outputs start as 2^64 - 1, not canonical: a word never stored shows)
        tf.device.batch_inversion(x, y, width=w)
        prod = torch.full_like(x, -1)
        tf.device.hadamard(x, y, prod, width=w)
        assert torch.equal(prod, _to_dev(_one(w, n))), n
        xs, ys = _to_host(x), _to_host(y)
        edges = {0, n - 1, _wrap(w) - 1, _wrap(w), _wrap(w) + 1}
        idx = sorted(set(np.random.default_rng(n).integers(0, n, 512).tolist()) | {i for i in edges if i < n})
        assert np.array_equal(_oracle_inverses(oracle, xs, w, idx), np.concatenate([ys[w * i:w * i + w] for i in idx])), n


# ------------------------------------------------------------------ 2. large sizes
@pytest.mark.parametrize("w,n", [(1, (1 << 24) + 5), (3, (1 << 23) + 5)])
def test_large_sizes(tf, oracle, w, n):
    import torch

    x = torch.empty(w * n, dtype=torch.int64, device="cuda")
    tf.device.fill_random(x, 0x1D00 + w)
    y = torch.full_like(x, -1)
    tf.device.batch_inversion(x, y, width=w)
    prod = torch.full_like(x, -1)
    tf.device.hadamard(x, y, prod, width=w)
    assert torch.equal(prod, _to_dev(_one(w, n)))
    ys = _to_host(y)
    assert (ys < np.uint64(P)).all()
    xs = _to_host(x)
    idx = sorted(set(np.random.default_rng(w).integers(0, n, 4096 - 2).tolist()) | {0, n - 1})
    assert np.array_equal(_oracle_inverses(oracle, xs, w, idx), np.concatenate([ys[w * i:w * i + w] for i in idx]))
    # in place: the same words
    tf.device.batch_inversion(x, x, width=w)
    assert torch.equal(x, y)
    # inverse_or_zero of an input without zeros: the same words too
    z = torch.full_like(x, -1)
    tf.device.inverse_or_zero(y, z, width=w)
    torch.cuda.synchronize()
    assert torch.equal(z, _to_dev(xs))


# ------------------------------------------------------------------ 3. zeros under batch_inversion
def _zero_positions(w, n):
    c = _chunk(w)
    return [0, n - 1, c, c - 1, n - 2]


@pytest.mark.parametrize("w", [1, 3])
def test_a_zero_element_panics(tf, oracle, w):
    import torch

    lib = tf.lib()
    n = 3 * _chunk(w) + 5  # a padded tail of 64 K - 5 elements
    for pos in _zero_positions(w, n):
        x = oracle.fill_random(w * n, 0x1E00 + pos)
        x[w * pos:w * pos + w] = 0
        with pytest.raises(tf.NttPanic) as e:
            tf.batch_inversion(x, width=w)
        assert e.value.code == INVERSE_OF_ZERO, pos
        d = _to_dev(x)
        out = torch.full_like(d, -1)  # (not canonical: a word never stored shows)
        with pytest.raises(tf.NttPanic) as e:
            tf.device.batch_inversion(d, out, width=w)
        assert e.value.code == INVERSE_OF_ZERO, pos
        st = torch.zeros(1, dtype=torch.int32, device="cuda")
        tf.device.batch_inversion(d, out, width=w, status=st)
        torch.cuda.synchronize()
        assert int(st.item()) == INVERSE_OF_ZERO, pos
        st.fill_(16)  # an earlier error of the chain stays
        tf.device.batch_inversion(d, out, width=w, status=st)
        torch.cuda.synchronize()
        assert int(st.item()) == 16, pos
        # the other elements of the zero's wave keep their inverses under inverse_or_zero
        want = inversion_ref.expected(x, w)
        assert np.array_equal(tf.inverse_or_zero(x, width=w), want), pos
    # no zero: the status stays 0, and the host form's C status is TF_OK
    x = oracle.fill_random(w * n, 0x1EFF)
    st = torch.zeros(1, dtype=torch.int32, device="cuda")
    out = torch.full((w * n,), -1, dtype=torch.int64, device="cuda")
    tf.device.batch_inversion(_to_dev(x), out, width=w, status=st)
    torch.cuda.synchronize()
    assert int(st.item()) == 0
    fn = lib.tf_batch_inversion_bfe if w == 1 else lib.tf_batch_inversion_xfe
    o = np.empty_like(x)
    import ctypes as C

    assert fn(C.c_void_p(x.ctypes.data), n, C.c_void_p(o.ctypes.data)) == 0


def test_async_forms_never_synchronise(tf, oracle):
    """_dev_async and inverse_or_zero_dev enqueued behind ~40 ms of transforms on one stream return while the stream is still busy
    (torch's Stream.query() = hipStreamQuery); the words are the blocking calls' and a zero reaches the status word."""
    import torch

    n = 3 * _chunk(1) + 7
    xb = torch.empty(n, dtype=torch.int64, device="cuda")
    xx = torch.empty(3 * n, dtype=torch.int64, device="cuda")
    tf.device.fill_random(xb, 0x1F01)
    tf.device.fill_random(xx, 0x1F02)
    xx_zero = xx.clone()
    xx_zero[3 * 17:3 * 18] = 0
    # blocking reference runs (also warm the pool and the code objects)
    rb, rx = torch.full_like(xb, -1), torch.full_like(xx, -1)
    tf.device.batch_inversion(xb, rb)
    tf.device.batch_inversion(xx, rx, width=3)
    rz = torch.full_like(xx, -1)
    tf.device.inverse_or_zero(xx_zero, rz, width=3)
    big = torch.empty(256 << 20, dtype=torch.int64, device="cuda")
    tf.device.fill_random(big, 0x1F03)
    tf.device.ntt_(big, 1 << 20, batch=256)
    torch.cuda.synchronize()

    s = torch.cuda.Stream()
    st = torch.zeros(1, dtype=torch.int32, device="cuda")
    st_bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    ob, ox, oz, junk = torch.full_like(xb, -1), torch.full_like(xx, -1), torch.full_like(xx, -1), torch.full_like(xx, -1)
    s.wait_stream(torch.cuda.current_stream())  # (the fills above are on the default stream)
    with torch.cuda.stream(s):
        for _ in range(20):  # ~40 ms of queued work in front of the calls
            tf.device.ntt_(big, 1 << 20, batch=256, stream=s)
        tf.device.batch_inversion(xb, ob, stream=s, status=st)
        tf.device.batch_inversion(xx, ox, width=3, stream=s, status=st)
        tf.device.inverse_or_zero(xx_zero, oz, width=3, stream=s)
        tf.device.batch_inversion(xx_zero, junk, width=3, stream=s, status=st_bad)
        pending = not s.query()
    s.synchronize()
    assert pending, "an asynchronous entry point waited for the device"
    assert int(st.item()) == 0 and int(st_bad.item()) == INVERSE_OF_ZERO
    assert torch.equal(ob, rb) and torch.equal(ox, rx) and torch.equal(oz, rz)
    del big


# ------------------------------------------------------------------ 4. inverse_or_zero
@pytest.mark.parametrize("w", [1, 3])
def test_inverse_or_zero(tf, oracle, w):
    rng = np.random.default_rng(0x20 + w)
    n = 5 * _chunk(w) + 11
    for frac in (0.01, 0.5):
        x = oracle.fill_random(w * n, 0x2000 + int(frac * 100))
        for i in rng.choice(n, int(frac * n), replace=False):
            x[w * i:w * i + w] = 0
        want = inversion_ref.expected(x, w)
        got = tf.inverse_or_zero(x, width=w)
        assert np.array_equal(got, want), frac
    # a whole wave chunk of zeros, next to chunks without any
    x = oracle.fill_random(w * n, 0x2100)
    c = _chunk(w)
    x[w * c:w * 2 * c] = 0
    got = tf.inverse_or_zero(x, width=w)
    assert not got[w * c:w * 2 * c].any()
    assert np.array_equal(got, inversion_ref.expected(x, w))
    # all zeros
    assert not tf.inverse_or_zero(np.zeros(w * n, dtype=np.uint64), width=w).any()
    # on device, in place
    import torch

    d = _to_dev(x)
    tf.device.inverse_or_zero(d, d, width=w)
    torch.cuda.synchronize()
    assert np.array_equal(_to_host(d), got)


def test_extension_field_zero_is_all_three_words(tf, oracle):
    """(0, 0, 0) is the only zero: (a, 0, 0), (0, a, 0), (0, 0, a) are inverted, and batch_inversion accepts them"""
    a = oracle.fill_random(8, 0x2200)
    elems = []
    for v in a:
        elems += [[0, 0, 0], [int(v), 0, 0], [0, int(v), 0], [0, 0, int(v)]]
    x = np.array(elems, dtype=np.uint64).reshape(-1)
    got = tf.inverse_or_zero(x, width=3)
    assert np.array_equal(got, inversion_ref.expected(x, 3))
    for i in range(len(elems)):
        if i % 4:
            assert np.array_equal(got[3 * i:3 * i + 3], oracle.xfe_inverse(x[3 * i:3 * i + 3]))
        else:
            assert not got[3 * i:3 * i + 3].any()
    nz = np.array([e for i, e in enumerate(elems) if i % 4], dtype=np.uint64).reshape(-1)
    assert np.array_equal(tf.batch_inversion(nz, width=3), inversion_ref.expected(nz, 3))


# ------------------------------------------------------------------ 5. addressing
@pytest.mark.parametrize("w", [1, 3])
def test_pointers_offset_by_one_word_and_empty_calls(tf, oracle, w):
    import ctypes as C

    import torch

    n = 2 * _chunk(w) + 9
    x = oracle.fill_random(w * n + 1, 0x2300)
    want = inversion_ref.expected(x[1:], w)
    d = _to_dev(x)
    out = torch.zeros(w * n + 1, dtype=torch.int64, device="cuda")
    tf.device.batch_inversion(d[1:], out[1:], width=w)
    st = torch.zeros(1, dtype=torch.int32, device="cuda")
    out2 = torch.zeros(w * n + 1, dtype=torch.int64, device="cuda")
    tf.device.batch_inversion(d[1:], out2[1:], width=w, status=st)
    out3 = torch.zeros(w * n + 1, dtype=torch.int64, device="cuda")
    tf.device.inverse_or_zero(d[1:], out3[1:], width=w)
    torch.cuda.synchronize()
    for o in (out, out2, out3):
        h = _to_host(o)
        assert h[0] == 0 and np.array_equal(h[1:], want)
    assert int(st.item()) == 0
    # n = 0: TF_OK, no launch, nothing written (the status word included)
    lib = tf.lib()
    sfx = "bfe" if w == 1 else "xfe"
    keep = out.clone()
    st.fill_(0)
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    assert getattr(lib, f"tf_batch_inversion_{sfx}_dev")(p(d), 0, p(out), s) == 0
    assert getattr(lib, f"tf_batch_inversion_{sfx}_dev_async")(p(d), 0, p(out), s, p(st)) == 0
    assert getattr(lib, f"tf_inverse_or_zero_{sfx}_dev")(p(d), 0, p(out), s) == 0
    torch.cuda.synchronize()
    assert torch.equal(out, keep) and int(st.item()) == 0


# ------------------------------------------------------------------ 6. the C++ mirror
def test_cpp_mirror_inversion_selftest_runs():
    host = os.path.join(ROOT, "twenty-first_amd", "host")
    subprocess.check_call(["make", "-C", host, "inversion_selftest"], stdout=subprocess.DEVNULL)
    r = subprocess.run([os.path.join(host, "inversion_selftest")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("PASS") >= 5, r.stdout
