"""The DEEP quotients on the device (twenty_first_amd/deep.py over tf_deep_quotient_dev / tf_deep_quotient_rows_dev) against the literal
model of tests/deep_ref.py, word for word.

Every device output starts as canary words and is compared whole; the inputs are checked unchanged; the padding between a line and
its stride holds a poison that must never reach the result; the work space is exactly workspace() bytes inside a canary.  The shapes
come from deep.plan (csrc/deep_kernels.h, tf_deep.hip): C elements per wave and step, K per lane, the grid cap in chunks:
    n               1, 2, 64 (one lane row), C / 2 (the padded tail of a wave), C, 2 C, 8 C (two workgroups of four waves)
    columns         both sides of the four-column load group of the main table and of the two-column group of the aux table
    points          1 and 2 are one pass (the one- and the two-point kernel), 3 and 4 a second pass that adds into out
    grid stride     n = the smallest power of two with more chunks than the cap: every wave takes a second chunk
"""
import numpy as np
import pytest

from tests import deep_ref as dr
from tests import fence
from tests import field_ref
from tests import pyref
from tests import sponge_ref
from twenty_first_amd import deep as _deep  # noqa: F401  (the feature under test: collection fails without it)

pytestmark = pytest.mark.gpu

P = pyref.P
CANARY64 = np.uint64(0xC0FFEE0000C0FFEE)
POISON = np.uint64(0xFFFFFFFEDEADBEEF)          # a canonical word: were it read as a table word, the result would change
INVERSE_OF_ZERO, INVALID = 12, 17
COLUMNS = [(1, 0), (0, 1), (3, 0), (4, 0), (5, 0), (0, 2), (0, 3), (5, 3), (9, 5)]
OFFSET = pyref.to_raw(7)
ROWS = {}  # the fence rows: callable of deep.py -> (cases, generator of (shape, operands, call)), as tests/test_gpu_scan.py


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(tf):
    assert tf.lib().tf_device_count() > 0, "no HIP device visible: the product has no CPU fallback"


# ------------------------------------------------------------------ plumbing
def dev64(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).reshape(-1).view(np.int64).copy()).cuda()


def dev32(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).reshape(-1).view(np.int32).copy()).cuda()


def host64(t):
    return t.cpu().numpy().view(np.uint64)


def rand_words(rng, count):
    """canonical raw words (any word below p is the raw word of some element)"""
    return (rng.integers(0, 1 << 63, count, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, count, dtype=np.uint64)) % np.uint64(P)


def edge_words(count, shift):
    edge = np.array([x for x in field_ref.edge_words() if x < P], dtype=np.uint64)
    return np.resize(np.roll(edge, shift), count)


def operands(rng, n, k1, k3, n_points):
    """packed main, aux, points, weights, values of random canonical words"""
    k = k1 + k3
    return rand_words(rng, k1 * n), rand_words(rng, 3 * k3 * n), rand_words(rng, 3 * n_points), rand_words(rng, 3 * n_points * k), rand_words(rng, 3 * n_points * k)


def run(tf, n, k1, k3, main, aux, points, weights, values, pad=False, status=0, offset=OFFSET):
    """One codeword call on fresh device buffers: main and aux packed, laid out at strides with poisoned padding when `pad`.  Checks the
    inputs unchanged and the words around the work space untouched.  -> (the n elements of out, the status word, the model's strides)"""
    import torch

    n_points = points.size // 3
    sm, sa = (n + 3, 3 * n + 5) if pad else (n, 3 * n)
    h_main, h_aux = dr.strided(main, k1, n, sm, POISON), dr.strided(aux, k3, 3 * n, sa, POISON)
    inputs = [(h, dev64(h)) for h in (h_main, h_aux, points, weights, values)]
    d_main, d_aux, d_points, d_weights, d_values = (d for _, d in inputs)
    d_out = dev64(np.full(3 * n, CANARY64))
    d_status = torch.full((1,), status, dtype=torch.int32, device="cuda")
    ws = tf.deep.workspace(n, k1, k3, n_points)
    assert ws == (24 * n_points if k1 + k3 else 0)
    d_arena = dev64(np.full(ws // 8 + 16, CANARY64))
    d_work = d_arena[8:8 + ws // 8] if ws else None
    tf.deep.quotient(d_main if k1 else None, d_aux if k3 else None, n, k1, k3, offset, d_points, d_weights if k1 + k3 else None,
                     d_values if k1 + k3 else None, d_out, d_status, d_work, stride_main=sm, stride_aux=sa)
    got = host64(d_out)
    for h, d in inputs:
        assert np.array_equal(host64(d), h), "an input was modified"
    arena = host64(d_arena)
    assert (arena[:8] == CANARY64).all() and (arena[8 + ws // 8:] == CANARY64).all(), "a word outside workspace() bytes was written"
    return got, int(d_status.item()), (h_main, sm, h_aux, sa)


def check(tf, n, k1, k3, main, aux, points, weights, values, pad=False, offset=OFFSET):
    got, status, (h_main, sm, h_aux, sa) = run(tf, n, k1, k3, main, aux, points, weights, values, pad=pad, offset=offset)
    want, bad = dr.codeword(h_main, k1, sm, h_aux, k3, sa, n, offset, points, weights, values)
    assert not bad and status == 0
    assert np.array_equal(got, want), (n, k1, k3, points.size // 3, pad, np.flatnonzero(got != want)[:6])


# ------------------------------------------------------------------ 1. lengths, columns, points, strides
@pytest.mark.parametrize("k1,k3", COLUMNS, ids=[f"{a}-{b}" for a, b in COLUMNS])
def test_lengths_points_and_strides(tf, k1, k3):
    p = tf.deep.plan(1, k1, k3, 1)
    C = p.chunk
    assert C % 64 == 0 and C // 2 >= 64
    rng = np.random.default_rng(100 * k1 + k3)
    for j, n in enumerate((1, 2, 64, C // 2, C, 2 * C, 8 * C)):
        for n_points in (1, 2, 3, 4):
            check(tf, n, k1, k3, *operands(rng, n, k1, k3, n_points), pad=(j + n_points) % 2 == 1)


def test_the_other_stride_form_at_every_length(tf):
    """the loop above alternates packed and padded; here every (n, points) pair runs in the form it did not take there"""
    C = tf.deep.plan(1, 5, 3, 1).chunk
    rng = np.random.default_rng(53)
    for j, n in enumerate((1, 2, 64, C // 2, C, 2 * C, 8 * C)):
        for n_points in (1, 2, 3, 4):
            check(tf, n, 5, 3, *operands(rng, n, 5, 3, n_points), pad=(j + n_points) % 2 == 0)


# ------------------------------------------------------------------ 2. operands
@pytest.mark.parametrize("n_points", [1, 2, 3])
def test_edge_words_under_edge_weights(tf, n_points):
    """0, 1, p - 1, 2^32 +- 1, the single-bit words: the deferred carries and acc_reduce at their extremes"""
    C = tf.deep.plan(1, 5, 3, 1).chunk
    n, k1, k3 = C, 5, 3
    k = k1 + k3
    rng = np.random.default_rng(7)
    check(tf, n, k1, k3, edge_words(k1 * n, 3), edge_words(3 * k3 * n, 11), rand_words(rng, 3 * n_points), edge_words(3 * n_points * k, 5),
          edge_words(3 * n_points * k, 17), pad=True)


def test_zero_weights_and_a_zero_table(tf):
    rng = np.random.default_rng(9)
    n, k1, k3, n_points = 128, 5, 3, 2
    main, aux, points, weights, values = operands(rng, n, k1, k3, n_points)
    got, status, _ = run(tf, n, k1, k3, main, aux, points, np.zeros_like(weights), values)
    assert status == 0 and not got.any()
    check(tf, n, k1, k3, np.zeros_like(main), np.zeros_like(aux), points, weights, values)       # out = -sum_p C_p / (x_i - z_p)
    check(tf, n, k1, k3, main, aux, points, weights, np.zeros_like(values), pad=True)
    # no column at all: zeros, no work space, the status left alone
    got, status, _ = run(tf, n, 0, 0, main[:0], aux[:0], points, weights[:0], values[:0], status=5)
    assert status == 5 and not got.any()


def test_65535_columns_the_counter_bound(tf):
    """k1 + k3 = 65 535 at n = 64: every counter of the carry-deferred accumulators takes as many increments as it ever can -- the
    weights and every other column are the word 0xfffffffe_ffffffff, whose four partial products all carry."""
    n, k1, k3 = 64, 65000, 535
    big = np.uint64(0xFFFFFFFEFFFFFFFF)
    rng = np.random.default_rng(65535)
    main, aux, points, weights, values = operands(rng, n, k1, k3, 1)
    main.reshape(k1, n)[1::2] = big
    aux.reshape(k3, 3 * n)[1::2] = big
    weights[:] = big
    got, status, (h_main, sm, h_aux, sa) = run(tf, n, k1, k3, main, aux, points, weights, values)
    assert status == 0 and np.array_equal(got, dr.codeword_by_sums(h_main, k1, sm, h_aux, k3, sa, n, OFFSET, points, weights, values))


# ------------------------------------------------------------------ 3. the second grid-stride turn
def test_every_wave_takes_a_second_chunk(tf):
    p = tf.deep.plan(1, 1, 0, 1)
    n = 1
    while n // p.chunk <= p.grid_cap:
        n *= 2
    assert n <= 1 << 24 and -(-n // p.chunk) > p.grid_cap
    rng = np.random.default_rng(2)
    main, aux, points, weights, values = operands(rng, n, 1, 0, 1)
    got, status, (h_main, sm, h_aux, sa) = run(tf, n, 1, 0, main, aux, points, weights, values)
    assert status == 0 and not (got.reshape(n, 3) == CANARY64).all(axis=1).any(), "an element was never stored"
    C = p.chunk
    at = np.concatenate([np.arange(C), np.arange(n - C, n), np.arange(p.grid_cap * C, p.grid_cap * C + C),
                         np.random.default_rng(4096).integers(0, n, 4096)])
    want, bad = dr.codeword(h_main, 1, sm, h_aux, 0, sa, n, OFFSET, points, weights, values, at=at)
    assert not bad and np.array_equal(got.reshape(n, 3)[at].reshape(-1), want)


# ------------------------------------------------------------------ 4. zero denominators
def test_a_point_on_the_domain_raises_the_status_and_spares_every_other_element(tf):
    C = tf.deep.plan(1, 3, 2, 2).chunk
    n, k1, k3 = 8 * C, 3, 2
    rng = np.random.default_rng(12)
    main, aux, points, weights, values = operands(rng, n, k1, k3, 2)
    hit = [5, n - 3]                                             # x_5, and an element of the last chunk
    points = dr.words([pyref.xfe(dr.domain_point(n, OFFSET, i)) for i in hit])
    want, bad = dr.codeword(main, k1, n, aux, k3, 3 * n, n, OFFSET, points, weights, values)
    assert bad == hit
    keep = np.ones(n, dtype=bool)
    keep[hit] = False
    for before, after in ((0, INVERSE_OF_ZERO), (99, 99)):       # the first non-zero code stays
        got, status, _ = run(tf, n, k1, k3, main, aux, points, weights, values, status=before)
        assert status == after
        assert np.array_equal(got.reshape(n, 3)[keep], want.reshape(n, 3)[keep])
    # one of the two points off the domain again: the other still raises it, and only its element is lost
    points[3:] = rand_words(rng, 3)
    want, bad = dr.codeword(main, k1, n, aux, k3, 3 * n, n, OFFSET, points, weights, values)
    got, status, _ = run(tf, n, k1, k3, main, aux, points, weights, values)
    keep[n - 3] = True
    assert bad == [5] and status == INVERSE_OF_ZERO and np.array_equal(got.reshape(n, 3)[keep], want.reshape(n, 3)[keep])
    # a clean call leaves the status word at zero
    points[:3] = rand_words(rng, 3)
    check(tf, n, k1, k3, main, aux, points, weights, values)


# ------------------------------------------------------------------ 5. the work space
def test_one_word_less_than_workspace_is_refused(tf):
    import ctypes as C

    import torch

    n, k1, k3, n_points = 64, 2, 1, 3
    rng = np.random.default_rng(3)
    main, aux, points, weights, values = (dev64(x) for x in operands(rng, n, k1, k3, n_points))
    d_out, d_status = dev64(np.full(3 * n, CANARY64)), torch.zeros(1, dtype=torch.int32, device="cuda")
    ws = tf.deep.workspace(n, k1, k3, n_points)
    assert ws == 72
    with pytest.raises(ValueError):
        tf.deep.quotient(main, aux, n, k1, k3, OFFSET, points, weights, values, d_out, d_status, dev64(np.zeros(ws // 8 - 1)))
    with pytest.raises(ValueError):
        tf.deep.quotient(main, aux, n, k1, k3, OFFSET, points, weights, values, d_out, d_status, None)
    # the library itself refuses one BYTE less, before any launch
    d_work = dev64(np.full(ws // 8, CANARY64))
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    rc = tf.lib().tf_deep_quotient_dev(ptr(main), k1, n, ptr(aux), k3, 3 * n, n, C.c_uint64(OFFSET), ptr(points), n_points, ptr(weights), ptr(values),
                                       ptr(d_out), ptr(d_work), ws - 1, None, ptr(d_status))
    torch.cuda.synchronize()
    assert rc == INVALID and (host64(d_out) == CANARY64).all() and (host64(d_work) == CANARY64).all() and int(d_status.item()) == 0


# ------------------------------------------------------------------ 6. the rows form
def opened(rng, n_rows, k1, k3, pad):
    """row-major rows as tf_table_gather_rows_dev leaves them: (main rows, stride, aux rows, stride)"""
    rsm, rsa = (k1 + 2, 3 * k3 + 1) if pad else (k1, 3 * k3)
    return dr.strided(rand_words(rng, n_rows * k1), n_rows if k1 else 0, k1, rsm, POISON), rsm, \
        dr.strided(rand_words(rng, n_rows * 3 * k3), n_rows if k3 else 0, 3 * k3, rsa, POISON), rsa


def run_rows(tf, n, k1, k3, h_main, rsm, h_aux, rsa, idx, points, weights, values, status=0):
    import torch

    inputs = [(h, dev64(h)) for h in (h_main, h_aux, points, weights, values)]
    d_main, d_aux, d_points, d_weights, d_values = (d for _, d in inputs)
    d_idx = dev32(idx)
    d_out = dev64(np.full(3 * idx.size, CANARY64))
    d_status = torch.full((1,), status, dtype=torch.int32, device="cuda")
    tf.deep.quotient_rows(d_main if k1 else None, d_aux if k3 else None, n, k1, k3, OFFSET, d_idx, d_points, d_weights, d_values, d_out, d_status,
                          row_stride_main=rsm, row_stride_aux=rsa)
    got = host64(d_out)
    for h, d in inputs:
        assert np.array_equal(host64(d), h), "an input was modified"
    assert np.array_equal(d_idx.cpu().numpy().view(np.uint32), idx)
    return got, int(d_status.item())


@pytest.mark.parametrize("k1,k3", COLUMNS, ids=[f"{a}-{b}" for a, b in COLUMNS])
def test_rows_against_the_rows_model(tf, k1, k3):
    n = 1 << 12
    rng = np.random.default_rng(1000 + 100 * k1 + k3)
    for j, n_rows in enumerate((1, 63, 64, 65, 257)):
        n_points = 1 + (j + k1) % 4
        idx = rng.integers(0, n, n_rows).astype(np.uint32)
        idx[0] = n - 1
        if n_rows > 3:
            idx[1], idx[2], idx[3] = 0, idx[n_rows - 1], idx[n_rows - 1]          # index 0, and one index three times
        h_main, rsm, h_aux, rsa = opened(rng, n_rows, k1, k3, pad=j % 2 == 0)
        _, _, points, weights, values = operands(rng, 0, k1, k3, n_points)
        got, status = run_rows(tf, n, k1, k3, h_main, rsm, h_aux, rsa, idx, points, weights, values)
        want, bad_zero, bad_index = dr.rows(h_main, k1, rsm, h_aux, k3, rsa, n, OFFSET, idx, points, weights, values)
        assert not bad_zero and not bad_index and status == 0
        assert np.array_equal(got, want), (n_rows, n_points, np.flatnonzero(got != want)[:6])


def test_rows_with_many_columns_per_lane(tf):
    """more columns than a wave has lanes, on both tables: a lane walks several columns, the last turn is ragged"""
    n, n_rows, k1, k3 = 1 << 10, 5, 131, 67
    rng = np.random.default_rng(131)
    idx = rng.integers(0, n, n_rows).astype(np.uint32)
    h_main, rsm, h_aux, rsa = opened(rng, n_rows, k1, k3, pad=True)
    _, _, points, weights, values = operands(rng, 0, k1, k3, 2)
    got, status = run_rows(tf, n, k1, k3, h_main, rsm, h_aux, rsa, idx, points, weights, values)
    want, _, _ = dr.rows(h_main, k1, rsm, h_aux, k3, rsa, n, OFFSET, idx, points, weights, values)
    assert status == 0 and np.array_equal(got, want)


def test_rows_bad_index_and_zero_denominator(tf):
    n, n_rows, k1, k3 = 1 << 10, 65, 5, 3
    rng = np.random.default_rng(77)
    idx = rng.integers(0, n, n_rows).astype(np.uint32)
    h_main, rsm, h_aux, rsa = opened(rng, n_rows, k1, k3, pad=True)
    _, _, points, weights, values = operands(rng, 0, k1, k3, 2)
    # an index = n: the code tf_table_gather_rows_dev stores, the other rows right
    bad = idx.copy()
    bad[40] = n
    got, status = run_rows(tf, n, k1, k3, h_main, rsm, h_aux, rsa, bad, points, weights, values)
    want, bad_zero, bad_index = dr.rows(h_main, k1, rsm, h_aux, k3, rsa, n, OFFSET, bad, points, weights, values)
    keep = np.ones(n_rows, dtype=bool)
    keep[40] = False
    assert bad_index == [40] and not bad_zero and status == INVALID
    assert np.array_equal(got.reshape(-1, 3)[keep], want.reshape(-1, 3)[keep])
    # a point on the domain, at a sampled index
    idx[7] = 333
    idx[idx == 333] = 334
    idx[7] = 333
    points[3:] = dr.words([pyref.xfe(dr.domain_point(n, OFFSET, 333))])
    want, bad_zero, bad_index = dr.rows(h_main, k1, rsm, h_aux, k3, rsa, n, OFFSET, idx, points, weights, values)
    keep = np.ones(n_rows, dtype=bool)
    keep[7] = False
    for before, after in ((0, INVERSE_OF_ZERO), (INVALID, INVALID)):
        got, status = run_rows(tf, n, k1, k3, h_main, rsm, h_aux, rsa, idx, points, weights, values, status=before)
        assert bad_zero == [7] and not bad_index and status == after
        assert np.array_equal(got.reshape(-1, 3)[keep], want.reshape(-1, 3)[keep])
    # no column: zeros
    got, status = run_rows(tf, n, 0, 0, h_main[:0], 0, h_aux[:0], 0, idx, points, weights[:0], values[:0], status=0)
    assert status == 0 and not got.any()


def test_rows_opened_from_the_device_table_are_the_codeword_at_those_indices(tf):
    """the one end-to-end case: table.gather_rows opens the rows, quotient_rows evaluates them, and device.gather_elements of the
    quotient codeword at the same indices gives the same words -- device against device"""
    import torch

    C = tf.deep.plan(1, 5, 3, 2).chunk
    n, k1, k3, n_points, n_rows = 2 * C, 5, 3, 2, 65
    rng = np.random.default_rng(31)
    main, aux, points, weights, values = (dev64(x) for x in operands(rng, n, k1, k3, n_points))
    d_idx = dev32(rng.integers(0, n, n_rows).astype(np.uint32))
    d_status = torch.zeros(1, dtype=torch.int32, device="cuda")
    d_code = dev64(np.full(3 * n, CANARY64))
    d_work = dev64(np.zeros(tf.deep.workspace(n, k1, k3, n_points) // 8))
    tf.deep.quotient(main, aux, n, k1, k3, OFFSET, points, weights, values, d_code, d_status, d_work)
    d_want = dev64(np.full(3 * n_rows, CANARY64))
    tf.device.gather_elements(d_code, d_idx, d_want, width=3, status=d_status)
    rsm, rsa = k1 + 3, 3 * k3 + 2
    d_main_rows, d_aux_rows = dev64(np.full(n_rows * rsm, POISON)), dev64(np.full(n_rows * rsa, POISON))
    tf.table.gather_rows(main, n, k1, d_idx, d_main_rows, width=1, out_stride=rsm, status=d_status)
    tf.table.gather_rows(aux, n, k3, d_idx, d_aux_rows, width=3, out_stride=rsa, status=d_status)
    d_got = dev64(np.full(3 * n_rows, CANARY64))
    tf.deep.quotient_rows(d_main_rows, d_aux_rows, n, k1, k3, OFFSET, d_idx, points, weights, values, d_got, d_status, row_stride_main=rsm,
                          row_stride_aux=rsa)
    assert torch.equal(d_got, d_want) and int(d_status.item()) == 0 and not (host64(d_got) == CANARY64).any()


# ------------------------------------------------------------------ 7. no host in the chain
def test_weights_from_a_sponge_and_values_from_barycentric_evaluate_stay_on_the_device(tf):
    """sample_scalars writes the weights, barycentric_evaluate the values (main columns first, then aux, per point), the quotient reads
    both where they were left; ONE synchronisation at the end."""
    import torch

    C = tf.deep.plan(1, 3, 2, 2).chunk
    n, k1, k3, n_points = 2 * C, 3, 2, 2
    k = k1 + k3
    rng = np.random.default_rng(64)
    one = pyref.to_raw(1)
    main, aux, points, _, _ = operands(rng, n, k1, k3, n_points)
    absorbed = rand_words(rng, 5)
    d_main, d_aux, d_points, d_absorbed = dev64(main), dev64(aux), dev64(points), dev64(absorbed)
    d_states = torch.full((16,), -1, dtype=torch.int64, device="cuda")
    d_weights = torch.full((3 * n_points * k,), -1, dtype=torch.int64, device="cuda")
    d_values = torch.full((3 * n_points * k,), -1, dtype=torch.int64, device="cuda")
    d_out = dev64(np.full(3 * n, CANARY64))
    d_status = torch.zeros(1, dtype=torch.int32, device="cuda")
    d_work = dev64(np.full(tf.deep.workspace(n, k1, k3, n_points) // 8, CANARY64))
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()  # (the uploads above, made on the default stream)
    with torch.cuda.stream(stream):
        tf.device.tip5_sponge_init_(d_states, stream=stream)
        tf.device.tip5_sponge_pad_and_absorb_all_(d_states, d_absorbed, stream=stream)
        tf.device.tip5_sponge_sample_scalars(d_states, d_weights, stream=stream)
        for p in range(n_points):
            z = points[3 * p:3 * p + 3]
            tf.device.barycentric_evaluate(d_main, n, z, d_values[3 * p * k:3 * (p * k + k1)], batch=k1, width=1, stream=stream)
            tf.device.barycentric_evaluate(d_aux, n, z, d_values[3 * (p * k + k1):3 * (p + 1) * k], batch=k3, width=3, stream=stream)
        tf.deep.quotient(d_main, d_aux, n, k1, k3, one, d_points, d_weights, d_values, d_out, d_status, d_work, stream=stream)
    stream.synchronize()
    weights, values = host64(d_weights), host64(d_values)
    assert np.array_equal(weights, sponge_ref.sample_scalars(sponge_ref.pad_and_absorb_all(sponge_ref.init(), absorbed), n_points * k)[1].reshape(-1))
    want, bad = dr.codeword(main, k1, n, aux, k3, 3 * n, n, one, points, weights, values)
    assert not bad and int(d_status.item()) == 0 and np.array_equal(host64(d_out), want)


# ------------------------------------------------------------------ 8. the numpy forms
def test_host_forms(tf):
    rng = np.random.default_rng(900)
    n, k1, k3, n_points = 128, 4, 2, 3
    main, aux, points, weights, values = operands(rng, n, k1, k3, n_points)
    got, status = tf.deep.quotient_host(main, aux, n, k1, k3, OFFSET, points, weights, values)
    want, _ = dr.codeword(main, k1, n, aux, k3, 3 * n, n, OFFSET, points, weights, values)
    assert status == 0 and np.array_equal(got, want)
    idx = np.array([0, n - 1, 17, 17], dtype=np.uint32)
    main_rows = main.reshape(k1, n)[:, idx].T.copy()
    aux_rows = aux.reshape(k3, n, 3)[:, idx].transpose(1, 0, 2).copy()
    got, status = tf.deep.quotient_rows_host(main_rows, aux_rows, n, k1, k3, OFFSET, idx, points, weights, values)
    assert status == 0 and np.array_equal(got, want.reshape(n, 3)[idx].reshape(-1))
    got, status = tf.deep.quotient_host(main[:0], aux[:0], 0, k1, k3, OFFSET, points, weights, values)
    assert got.size == 0 and status == 0


# ------------------------------------------------------------------ 9. fence rows: one per tensor-taking callable of deep.py
def row(name, cases):
    def register(gen):
        assert name not in ROWS, name
        ROWS[name] = (list(cases), gen)
        return gen
    return register


def consts_words(points, weights, values, k):
    """what the call leaves in its work space: C_p = sum_c w[p][c] v[p][c], one XFieldElement per point"""
    w, v = dr.xfes(weights), dr.xfes(values)
    out = []
    for p in range(points.size // 3):
        s = (0, 0, 0)
        for c in range(k):
            s = pyref.xfe_add(s, pyref.xfe_mul(w[p * k + c], v[p * k + c]))
        out.append(s)
    return dr.words(out)


# (n as a function of the plan, k1, k3, points): one lane row; a ragged wave; two workgroups, one and two passes; one table only
@row("quotient", cases=[(lambda p: 64, 5, 3, 1), (lambda p: p.chunk // 2, 4, 2, 2), (lambda p: 8 * p.chunk, 5, 3, 3), (lambda p: 8 * p.chunk, 1, 1, 4),
                        (lambda p: 2 * p.chunk, 6, 0, 2), (lambda p: 2 * p.chunk, 0, 3, 1)])
def _fence_quotient(tf, m, n_of, k1, k3, n_points):
    n = n_of(m.plan(1, k1, k3, n_points))
    k = k1 + k3
    rng = np.random.default_rng(7000 + 10 * k1 + k3 + n_points)
    main, aux, points, weights, values = operands(rng, n, k1, k3, n_points)
    sm, sa = n + 1, 3 * n + 2
    h_main, h_aux = dr.strided(main, k1, n, sm, 0), dr.strided(aux, k3, 3 * n, sa, 0)
    want, bad = dr.codeword(h_main, k1, sm, h_aux, k3, sa, n, OFFSET, points, weights, values)
    assert not bad and m.workspace(n, k1, k3, n_points) == 24 * n_points
    ops = [fence.inp("points", points), fence.inp("weights", weights), fence.inp("values", values), fence.out("out", want),
           fence.out("work", consts_words(points, weights, values, k)), fence.inout("status", np.zeros(1, np.int32), np.zeros(1, np.int32), dtype="int32")]
    if k1:
        ops.append(fence.inp("main", h_main, padding=dr.padding(k1, n, sm)))
    if k3:
        ops.append(fence.inp("aux", h_aux, padding=dr.padding(k3, 3 * n, sa)))

    def call(points, weights, values, out, work, status, main=None, aux=None):
        m.quotient(main, aux, n, k1, k3, OFFSET, points, weights, values, out, status, work, stride_main=sm, stride_aux=sa)

    yield f"n={n} k1={k1} k3={k3} points={n_points}", ops, call


@row("quotient_rows", cases=[(1, 5, 3, 1), (65, 4, 2, 4), (257, 70, 0, 2), (64, 0, 3, 3)])
def _fence_quotient_rows(tf, m, n_rows, k1, k3, n_points):
    n = 1 << 10
    rng = np.random.default_rng(8000 + n_rows + k1)
    idx = rng.integers(0, n, n_rows).astype(np.uint32)
    h_main, rsm, h_aux, rsa = opened(rng, n_rows, k1, k3, pad=True)
    _, _, points, weights, values = operands(rng, 0, k1, k3, n_points)
    want, bad_zero, bad_index = dr.rows(h_main, k1, rsm, h_aux, k3, rsa, n, OFFSET, idx, points, weights, values)
    assert not bad_zero and not bad_index
    ops = [fence.inp("indices", idx.view(np.int32), dtype="int32"), fence.inp("points", points), fence.inp("weights", weights), fence.inp("values", values),
           fence.out("out", want), fence.inout("status", np.zeros(1, np.int32), np.zeros(1, np.int32), dtype="int32")]
    if k1:
        ops.append(fence.inp("main_rows", h_main, padding=dr.padding(n_rows, k1, rsm)))
    if k3:
        ops.append(fence.inp("aux_rows", h_aux, padding=dr.padding(n_rows, 3 * k3, rsa)))

    def call(indices, points, weights, values, out, status, main_rows=None, aux_rows=None):
        m.quotient_rows(main_rows, aux_rows, n, k1, k3, OFFSET, indices, points, weights, values, out, status, row_stride_main=rsm, row_stride_aux=rsa)

    yield f"n_rows={n_rows} k1={k1} k3={k3} points={n_points}", ops, call


def _fence_params():
    return [pytest.param(name, case, id=f"{name}-{i}") for name in ROWS for i, case in enumerate(ROWS[name][0])]


@pytest.mark.parametrize("name,case", _fence_params())
def test_fenced(tf, name, case):
    _, gen = ROWS[name]
    for shape, operands_, call in gen(tf, tf.deep, *case):
        fence.run(name, shape, operands_, call)


def test_every_tensor_taking_callable_of_the_module_has_a_fence_row(tf):
    import inspect

    m = tf.deep
    public = [name for name, f in vars(m).items() if inspect.isfunction(f) and f.__module__ == m.__name__ and not name.startswith("_")]
    assert sorted(public) == sorted(list(ROWS) + ["quotient_host", "quotient_rows_host", "plan", "workspace"]), \
        "numpy forms and host arithmetic need no row; every other call does"


def test_a_workgroup_step_fits_the_guard_words(tf):
    """the condition under fence.G: what one workgroup moves per column and step (four waves of C XFieldElements) stays below the guard"""
    assert 4 * tf.deep.plan(1, 1, 1, 1).chunk * 3 < fence.G


# ------------------------------------------------------------------ 10. the wrapper's own checks
def test_python_argument_checks_come_before_any_launch(tf):
    import torch

    n, k1, k3 = 64, 2, 1
    rng = np.random.default_rng(1)
    main, aux, points, weights, values = (dev64(x) for x in operands(rng, n, k1, k3, 1))
    d_out, d_work = dev64(np.full(3 * n, CANARY64)), dev64(np.full(3, CANARY64))
    d_status = torch.zeros(1, dtype=torch.int32, device="cuda")
    both = dev64(np.full(4 * n, CANARY64))
    with pytest.raises(ValueError):   # out on a table
        tf.deep.quotient(both[:2 * n], aux, n, k1, k3, OFFSET, points, weights, values, both[n:], d_status, d_work)
    with pytest.raises(ValueError):   # a short out
        tf.deep.quotient(main, aux, n, k1, k3, OFFSET, points, weights, values, d_out[:-3], d_status, d_work)
    with pytest.raises(ValueError):   # five points
        tf.deep.quotient(main, aux, n, k1, k3, OFFSET, dev64(np.zeros(15)), weights, values, d_out, d_status, d_work)
    with pytest.raises(TypeError):    # the status is one int32
        tf.deep.quotient(main, aux, n, k1, k3, OFFSET, points, weights, values, d_out, d_out[:1], d_work)
    with pytest.raises(TypeError):
        tf.deep.quotient(main.cpu(), aux, n, k1, k3, OFFSET, points, weights, values, d_out, d_status, d_work)
    with pytest.raises(ValueError):   # indices of 64-bit words
        tf.deep.quotient_rows(main, aux, n, k1, k3, OFFSET, points, points, weights, values, d_out[:9], d_status)
    with pytest.raises(tf.NttPanic):  # what the library itself refuses comes back as its code
        tf.deep.quotient(main[:2 * 48], aux[:3 * 48], 48, k1, k3, OFFSET, points, weights, values, d_out[:3 * 48], d_status, d_work)
    torch.cuda.synchronize()
    assert (host64(d_out) == CANARY64).all() and (host64(both) == CANARY64).all() and (host64(d_work) == CANARY64).all() and int(d_status.item()) == 0
