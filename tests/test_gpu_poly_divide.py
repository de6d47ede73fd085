"""Division with remainder (Polynomial::divide / naive_divide, Div, Rem, reduce; math/polynomial.rs:539-600, :989-1048, :2502-2524) and
formal_power_series_inverse_newton (:1281-1366) on the GPU.

BFieldElement results are compared word for word with the oracle's restatement of naive_divide and with tests/pyref.long_divide;
XFieldElement results with a long division written here over oracle.xfe_mul / xfe_inverse.  At every size the complete
characterisation is checked as well: a == q * b + r with r of nb - 1 coefficients.  Division with remainder is unique, so that
identity is a proof, not a sample.  Shapes sit on both sides of every switch of the implementation: the serial start of the Newton
kernel (16 coefficients), the orders of its one-launch doublings, the one-launch boundary (k = 2048 BFieldElement, 256
XFieldElement), the multi-step folds of a long dividend over a short modulus, and the constant divisor."""
import os
import subprocess

import numpy as np
import pytest

from tests import pyref

pytestmark = pytest.mark.gpu

P = (1 << 64) - (1 << 32) + 1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEWTON_ONE_LAUNCH = {1: 2048, 3: 256}  # NewtonMax<L>::PMAX (csrc/divide_kernels.h)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(tf):
    assert tf.lib().tf_device_count() > 0, "no HIP device visible: the product has no CPU fallback"


# ------------------------------------------------------------------ helpers
def rand(oracle, count, seed):
    return oracle.fill_random(count, seed) if count else np.zeros(0, dtype=np.uint64)


def trim(x, w=1):
    x = np.asarray(x, dtype=np.uint64).reshape(-1)
    n = x.size // w
    while n and not x[(n - 1) * w:n * w].any():
        n -= 1
    return x[:n * w]


def fadd(x, y):
    """Element-wise field addition of canonical raw words (Montgomery form is linear)."""
    s = x + y
    s = np.where(s < x, s + np.uint64(0xFFFFFFFF), s)
    return np.where(s >= np.uint64(P), s - np.uint64(P), s)


def identity_holds(oracle, a, b, q, r, w):
    """a == q * b + r (all zero padded to na), r of nb - 1 coefficients: the definition of division with remainder."""
    na, nb = a.size // w, b.size // w
    assert r.size == (nb - 1) * w
    prod = oracle.poly_mul(q, b, width=w) if q.size else np.zeros(0, dtype=np.uint64)
    lhs = np.zeros(max(na, prod.size // w, nb - 1) * w, dtype=np.uint64)
    lhs[:prod.size] = prod
    lhs[:r.size] = fadd(lhs[:r.size], r)
    return np.array_equal(trim(lhs, w), trim(a, w))


def pad(x, n):
    out = np.zeros(n, dtype=np.uint64)
    x = np.asarray(x, dtype=np.uint64).reshape(-1)
    out[:x.size] = x
    return out


def pyref_divide(a, b):
    q, r = pyref.long_divide([pyref.to_val(int(v)) for v in a], [pyref.to_val(int(v)) for v in b])
    return np.array([pyref.to_raw(v) for v in q], dtype=np.uint64), np.array([pyref.to_raw(v) for v in r], dtype=np.uint64)


def xfe_long_divide(oracle, a, b):
    """Schoolbook division over XFieldElement (3 words per coefficient): (q, r) of na - nb + 1 and nb - 1 coefficients."""
    a = [np.array(a[3 * i:3 * i + 3], dtype=np.uint64) for i in range(a.size // 3)]
    b = [np.array(b[3 * i:3 * i + 3], dtype=np.uint64) for i in range(b.size // 3)]
    na, nb = len(a), len(b)
    inv = oracle.xfe_inverse(b[-1])
    q = [np.zeros(3, dtype=np.uint64) for _ in range(max(na - nb + 1, 0))]
    for k in range(na - nb, -1, -1):
        f = oracle.xfe_mul(a[k + nb - 1], inv)
        q[k] = f
        for j in range(nb):
            a[k + j] = oracle.xfe_sub(a[k + j], oracle.xfe_mul(f, b[j]))
    r = a[:nb - 1]
    cat = lambda v: np.concatenate(v) if v else np.zeros(0, dtype=np.uint64)  # noqa: E731
    return cat(q), cat(r)


def divisor(oracle, nb, w, seed, monic=False):
    b = rand(oracle, nb * w, seed)
    if nb:
        b[(nb - 1) * w:] = 0
        b[(nb - 1) * w] = oracle.bfe_new(1) if monic else oracle.bfe_new(3 + seed % 1000)
    return b


def check_bfe(tf, oracle, a, b, with_pyref=False):
    na, nb = a.size, b.size
    q, r = tf.poly_divide(a, b)
    assert q.size == max(na - nb + 1, 0) and r.size == nb - 1
    wq, wr = oracle.naive_divide(a, b)
    assert np.array_equal(trim(q), wq) and np.array_equal(trim(r), wr), (na, nb)
    if with_pyref:
        pq, pr = pyref_divide(a, b)
        assert np.array_equal(q, pad(pq, q.size)) and np.array_equal(r, pad(pr, r.size))
    assert identity_holds(oracle, a, b, q, r, 1)
    return q, r


# ------------------------------------------------------------------ BFieldElement against the oracle
SMALL = [(0, 1), (0, 3), (1, 2), (2, 3), (1, 1), (5, 1), (1, 3), (4, 4), (5, 4), (17, 2), (100, 3), (33, 33), (40, 7)]


@pytest.mark.parametrize("na,nb", SMALL)
def test_small_shapes_bfe(tf, oracle, na, nb):
    for monic in (False, True):
        check_bfe(tf, oracle, rand(oracle, na, na * 31 + nb), divisor(oracle, nb, 1, nb + 7, monic), with_pyref=True)


def test_zero_and_trailing_zero_dividends(tf, oracle):
    b = divisor(oracle, 9, 1, 3)
    check_bfe(tf, oracle, np.zeros(40, dtype=np.uint64), b, with_pyref=True)
    a = rand(oracle, 60, 4)
    a[45:] = 0  # an unnormalised dividend: the top of q is zero
    q, _ = check_bfe(tf, oracle, a, b, with_pyref=True)
    assert not q[45 - 9 + 1:].any()
    # two dividends without a coefficient: no quotient, the zero remainder twice
    q, r = tf.poly_divide(np.zeros(0, dtype=np.uint64), divisor(oracle, 2, 1, 5), batch=2)
    wq, wr = oracle.naive_divide(np.zeros(0, dtype=np.uint64), divisor(oracle, 2, 1, 5))
    assert q.size == 0 and wq.size == 0 and r.size == 2 and not r.any() and not wr.any()


def test_words_near_p(tf, oracle):
    a = np.array([P - 1 - (i % 5) for i in range(300)], dtype=np.uint64)
    b = np.array([P - 1 - (i % 3) for i in range(21)], dtype=np.uint64)
    check_bfe(tf, oracle, a, b, with_pyref=True)
    check_bfe(tf, oracle, a, np.array([P - 1], dtype=np.uint64))


# quotient lengths k around every switch: the serial start (16), the orders of the one-launch doublings, the one-launch boundary
K_SWITCHES = [15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 4095,
              4096, 4097, 8193]


@pytest.mark.parametrize("k", K_SWITCHES)
def test_quotient_lengths_around_switches_bfe(tf, oracle, k):
    for nb in (2, 40, 1025):
        check_bfe(tf, oracle, rand(oracle, k + nb - 1, k + nb), divisor(oracle, nb, 1, k))


@pytest.mark.parametrize("na,nb", [(5000, 2), (5000, 3), (1 << 15, 2), (1 << 15, 65), (1 << 15, 257), (1 << 15, 258), (1 << 15, (1 << 14) + 1),
                                   (1 << 15, 1 << 14), (1 << 15, 1), (1 << 15, 1 << 15), (3000, 129)])
def test_long_dividends_and_folds_bfe(tf, oracle, na, nb):
    # (5000, 2): the remainder's fold runs in two steps (5000 > 64 x N with N = 1); 257 / 258: m = N and m = N + 1
    check_bfe(tf, oracle, rand(oracle, na, na ^ nb), divisor(oracle, nb, 1, nb))


# ------------------------------------------------------------------ XFieldElement
@pytest.mark.parametrize("na,nb", [(0, 2), (3, 5), (4, 1), (7, 2), (9, 3), (20, 7), (30, 30), (40, 17)])
def test_small_shapes_xfe_against_long_division(tf, oracle, na, nb):
    for monic in (False, True):
        a = rand(oracle, 3 * na, na * 5 + nb)
        b = divisor(oracle, nb, 3, nb + 11, monic)
        q, r = tf.poly_divide(a, b, width=3)
        wq, wr = xfe_long_divide(oracle, a, b) if na >= nb else (np.zeros(0, dtype=np.uint64), pad(a, 3 * (nb - 1)))
        assert np.array_equal(q, wq) and np.array_equal(r, wr)
        assert identity_holds(oracle, a, b, q, r, 3)


@pytest.mark.parametrize("k", [15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 2049])
def test_quotient_lengths_around_switches_xfe(tf, oracle, k):
    for nb in (2, 33):
        a, b = rand(oracle, 3 * (k + nb - 1), k * 3 + nb), divisor(oracle, nb, 3, k)
        q, r = tf.poly_divide(a, b, width=3)
        assert identity_holds(oracle, a, b, q, r, 3)


@pytest.mark.parametrize("na,nb", [(5000, 2), (1 << 14, 129), (1 << 14, (1 << 13) + 1), (1 << 12, 1)])
def test_long_dividends_xfe(tf, oracle, na, nb):
    a, b = rand(oracle, 3 * na, na + nb), divisor(oracle, nb, 3, nb)
    q, r = tf.poly_divide(a, b, width=3)
    assert identity_holds(oracle, a, b, q, r, 3)


# ------------------------------------------------------------------ large shapes (the identity)
@pytest.mark.parametrize("na,nb,w", [(1 << 22, (1 << 21) + 1, 1), (1 << 22, 257, 1), (1 << 20, (1 << 19) + 1, 3)])
def test_large_shapes(tf, oracle, na, nb, w):
    a, b = rand(oracle, na * w, 77 + nb), divisor(oracle, nb, w, 78)
    q, r = tf.poly_divide(a, b, width=w)
    assert identity_holds(oracle, a, b, q, r, w)


def test_issue_minimum_sizes(tf, oracle):
    """At least na = 2^24 (BFieldElement) and 2^23 (XFieldElement) in one call; checked by the remainder of a known product."""
    for na, w in ((1 << 24, 1), (1 << 23, 3)):
        b = divisor(oracle, 65, w, 5)
        r0 = rand(oracle, 64 * w, 6)
        qq = rand(oracle, (na - 64) * w, 7)
        a = pad(oracle.poly_mul(qq, b, width=w), na * w)
        a[:r0.size] = fadd(a[:r0.size], r0)
        q, r = tf.poly_divide(a, b, width=w)
        assert np.array_equal(r, r0) and np.array_equal(q, qq)


# ------------------------------------------------------------------ batches over one divisor
@pytest.mark.parametrize("w", [1, 3])
def test_batch_matches_single_calls(tf, oracle, w):
    na, nb, batch = 200, 37, 300
    a, b = rand(oracle, batch * na * w, 99 + w), divisor(oracle, nb, w, 98)
    q, r = tf.poly_divide(a, b, width=w, batch=batch)
    k, m = na - nb + 1, nb - 1
    for i in range(batch):
        qi, ri = tf.poly_divide(a[i * na * w:(i + 1) * na * w], b, width=w)
        assert np.array_equal(q[i * k * w:(i + 1) * k * w], qi) and np.array_equal(r[i * m * w:(i + 1) * m * w], ri)
    # a dividend's result does not depend on where it sits in the batch
    rows = a.reshape(batch, -1)
    perm = np.random.default_rng(w).permutation(batch)
    q2, r2 = tf.poly_divide(np.ascontiguousarray(rows[perm]).reshape(-1), b, width=w, batch=batch)
    assert np.array_equal(q2.reshape(batch, -1), q.reshape(batch, -1)[perm])
    assert np.array_equal(r2.reshape(batch, -1), r.reshape(batch, -1)[perm])
    # q = NULL and r = NULL give the same words
    q3, r3 = tf.poly_divide(a, b, width=w, batch=batch, quotient=False)
    q4, r4 = tf.poly_divide(a, b, width=w, batch=batch, remainder=False)
    assert q3 is None and r4 is None and np.array_equal(r3, r) and np.array_equal(q4, q)


def test_batch_long_rows(tf, oracle):
    na, nb, batch = 1 << 14, (1 << 12) + 1, 5
    a, b = rand(oracle, batch * na, 123), divisor(oracle, nb, 1, 124)
    q, r = tf.poly_divide(a, b, batch=batch)
    k, m = na - nb + 1, nb - 1
    for i in range(batch):
        assert identity_holds(oracle, a[i * na:(i + 1) * na], b, q[i * k:(i + 1) * k], r[i * m:(i + 1) * m], 1)


# ------------------------------------------------------------------ _dev forms
def _cuda(x):
    import torch

    return torch.from_numpy(np.ascontiguousarray(x).view(np.int64)).cuda()


@pytest.mark.parametrize("na,nb,w,batch", [(300, 20, 1, 3), (5000, 2600, 1, 1), (700, 9, 3, 4), (10, 30, 1, 2), (50, 1, 3, 2)])
def test_dev_matches_host(tf, oracle, na, nb, w, batch):
    import torch

    a, b = rand(oracle, batch * na * w, na + 1), divisor(oracle, nb, w, nb + 2)
    q, r = tf.poly_divide(a, b, width=w, batch=batch)
    dq = torch.full((max(q.size, 1),), -1, dtype=torch.int64, device="cuda")[:q.size]  # (not canonical: a word never stored shows)
    dr = torch.full((max(r.size, 1),), -1, dtype=torch.int64, device="cuda")[:r.size]
    st = torch.zeros(1, dtype=torch.int32, device="cuda")
    tf.device.divide(_cuda(a), na, _cuda(b), dq if q.size else None, dr if r.size else None, batch=batch, width=w, status=st)
    torch.cuda.synchronize()
    assert st.item() == 0
    assert np.array_equal(dq.cpu().numpy().view(np.uint64), q) and np.array_equal(dr.cpu().numpy().view(np.uint64), r)


@pytest.mark.parametrize("w", [1, 3])
def test_dev_unnormalised_divisor_reports_17(tf, oracle, w):
    import torch

    for na, nb in ((100, 10), (100, 1), (5, 10), (5000, 3000)):
        a, b = rand(oracle, na * w, 5), divisor(oracle, nb, w, 6)
        b[(nb - 1) * w:] = 0
        q = torch.zeros(max(na - nb + 1, 0) * w, dtype=torch.int64, device="cuda")
        r = torch.zeros((nb - 1) * w, dtype=torch.int64, device="cuda")
        st = torch.zeros(1, dtype=torch.int32, device="cuda")
        tf.device.divide(_cuda(a), na, _cuda(b), q if q.numel() else None, r if r.numel() else None, width=w, status=st)
        torch.cuda.synchronize()
        assert st.item() == 17, (na, nb)
        with pytest.raises(tf.TwentyFirstError) as e:
            tf.device.divide(_cuda(a), na, _cuda(b), q if q.numel() else None, r if r.numel() else None, width=w)
        assert e.value.code == 17


def test_dev_call_does_not_block(tf, oracle):
    import torch

    na, nb = 1 << 16, (1 << 12) + 1
    a, b = _cuda(rand(oracle, na, 1)), _cuda(divisor(oracle, nb, 1, 2))
    q = torch.zeros(na - nb + 1, dtype=torch.int64, device="cuda")
    r = torch.zeros(nb - 1, dtype=torch.int64, device="cuda")
    f = _cuda(divisor(oracle, 257, 1, 3))
    out = torch.zeros(tf.lib().tf_poly_fps_inverse_newton_len(257, 1024), dtype=torch.int64, device="cuda")
    st = torch.zeros(1, dtype=torch.int32, device="cuda")
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):  # warm-up: tables, pools, LDS attributes
        tf.device.divide(a, na, b, q, r, stream=s, status=st)
        tf.device.fps_inverse_newton(f, 1024, out, stream=s, status=st)
    s.synchronize()
    x = torch.zeros((1 << 22) * 16, dtype=torch.int64, device="cuda")
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(8):
            tf.device.ntt_(x, 1 << 22, batch=16, stream=s)
        tf.device.divide(a, na, b, q, r, stream=s, status=st)
        tf.device.fps_inverse_newton(f, 1024, out, stream=s, status=st)
        busy = not s.query()
    s.synchronize()
    assert busy, "the divide / fps_inverse_newton calls waited for the stream"
    assert st.item() == 0
    del x


# ------------------------------------------------------------------ formal_power_series_inverse_newton
def newton_reference(oracle, g, precision, w):
    """The R-th iterate f <- 2 f - f^2 g from f = g(0)^-1, untruncated, by the recurrence over oracle.poly_mul."""
    d = g.size // w - 1
    f0 = oracle.bfe_inverse(int(g[0])) if w == 1 else oracle.xfe_inverse(g[:3])
    f = np.array([f0], dtype=np.uint64) if w == 1 else np.asarray(f0, dtype=np.uint64)
    if d == 0:
        return f
    R = (1 << (max(precision, 1) - 1).bit_length()).bit_length() - 1
    for _ in range(R):
        sq = oracle.poly_mul(oracle.poly_mul(f, f, width=w), g, width=w)
        twof = fadd(f, f)
        neg = np.where(sq == 0, sq, np.uint64(P) - sq)
        out = neg.copy()
        out[:twof.size] = fadd(out[:twof.size], twof)
        f = out
    return f


@pytest.mark.parametrize("w", [1, 3])
@pytest.mark.parametrize("d", [0, 1, 3, 255, 256, 257, 1000])
def test_fps_inverse_newton(tf, oracle, w, d):
    g = rand(oracle, (d + 1) * w, 1000 + d)
    g[d * w] = oracle.bfe_new(5)
    g[0] = oracle.bfe_new(9)
    for precision in (0, 1, 2, 3, 8, 9, 1024):
        got = tf.Polynomial(g, width=w).formal_power_series_inverse_newton(precision)
        n = tf.lib().tf_poly_fps_inverse_newton_len(d + 1, precision)
        want = newton_reference(oracle, g, precision, w)
        assert n * w == want.size
        assert np.array_equal(got.coefficients, trim(want, w)), (d, precision)
        # f g == 1 mod x^precision
        prod = oracle.poly_mul(pad(got.coefficients, n * w), g, width=w)
        one = np.zeros(max(precision, 1) * w, dtype=np.uint64)
        one[0] = oracle.bfe_new(1)
        assert np.array_equal(pad(prod, max(prod.size, one.size))[:one.size], one)


@pytest.mark.parametrize("w", [1, 3])
def test_fps_zero_constant_term(tf, oracle, w):
    g = rand(oracle, 4 * w, 3)
    g[:w] = 0
    with pytest.raises(tf.NttPanic) as e:
        tf.Polynomial(g, width=w).formal_power_series_inverse_newton(8)
    assert e.value.code == 12
    import torch

    st = torch.zeros(1, dtype=torch.int32, device="cuda")
    out = torch.zeros(tf.lib().tf_poly_fps_inverse_newton_len(4, 8) * w, dtype=torch.int64, device="cuda")
    tf.device.fps_inverse_newton(_cuda(g), 8, out, width=w, status=st)
    torch.cuda.synchronize()
    assert st.item() == 12


def test_fps_dev_matches_host(tf, oracle):
    import torch

    g = divisor(oracle, 300, 1, 8)
    g[0] = oracle.bfe_new(4)
    want = tf.Polynomial(g).formal_power_series_inverse_newton(100)
    out = torch.zeros(tf.lib().tf_poly_fps_inverse_newton_len(300, 100), dtype=torch.int64, device="cuda")
    tf.device.fps_inverse_newton(_cuda(g), 100, out)
    assert np.array_equal(trim(out.cpu().numpy().view(np.uint64)), want.coefficients)


# ------------------------------------------------------------------ Python API and C++ mirror
def test_operators_agree_with_divide(tf, oracle):
    for w in (1, 3):
        a = tf.Polynomial(rand(oracle, 90 * w, 1), width=w)
        b = tf.Polynomial(divisor(oracle, 13, w, 2), width=w)
        q, r = a.divide(b)
        assert np.array_equal((a / b).coefficients, q.coefficients) and np.array_equal((a % b).coefficients, r.coefficients)
        assert np.array_equal(a.reduce(b).coefficients, r.coefficients)
        with pytest.raises(tf.NttPanic) as e:
            a / tf.Polynomial(np.zeros(3 * w, dtype=np.uint64), width=w)
        assert e.value.code == 15
        with pytest.raises(tf.NttPanic) as e:
            a % tf.Polynomial(np.zeros(0, dtype=np.uint64), width=w)
        assert e.value.code == 15


def test_cpp_mirror_divide_selftest_on_gpu():
    host = os.path.join(ROOT, "twenty-first_amd", "host")
    subprocess.check_call(["make", "-C", host, "divide_selftest"], stdout=subprocess.DEVNULL)
    r = subprocess.run([os.path.join(host, "divide_selftest")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("PASS") == 6, r.stdout
