"""The prefix scans on the device (twenty_first_amd/scan.py over tf_scan_sum_dev / tf_scan_product_dev / tf_scan_affine_dev) against
the sequential loop of tests/scan_ref.py, word for word.

Every device output starts as canary words and is compared whole, the padding between n * width and the stride included.  The shapes
come from scan.plan: T elements per tile, S tile maps per turn of the spine, WAVE elements up to which one wave scans a column
(csrc/scan_kernels.h, tf_scan.hip):
    one wave per column   n <= WAVE: lane l owns K consecutive elements; n in {1, 2, 63, 64, 65} is one lane, less than and more than
                          the K of either width; 257 columns of 5 share workgroups and leave a ragged last one; 65 537 columns of 3 is one
                          column more than the capped grid has waves on 256 compute units, so one wave takes a second column
    one tile per column   WAVE < n <= T: one workgroup per column, the four waves meet in LDS
    three launches        n > T: tile maps, the spine, the tiles from their start values; 2 T + 1 leaves a last tile of one element;
                          S T + T + 1 elements are S + 2 tiles, so the spine takes a second turn with a carry
"""
import numpy as np
import pytest

from tests import fence
from tests import field_ref
from tests import points_ref as pr
from tests import pyref
from tests import scan_ref as sr
from tests import sponge_ref
from twenty_first_amd import scan as _scan  # noqa: F401  (the feature under test: collection fails without it)

pytestmark = pytest.mark.gpu

P = pyref.P
SUM, PRODUCT, AFFINE = sr.SUM, sr.PRODUCT, sr.AFFINE
KINDS = [(SUM, 1, 1), (SUM, 3, 3), (PRODUCT, 1, 1), (PRODUCT, 3, 3), (AFFINE, 1, 1), (AFFINE, 3, 3), (AFFINE, 3, 1)]  # (mode, width_a, width_b)
NAMES = {SUM: "sum", PRODUCT: "product", AFFINE: "affine"}
CANARY64 = np.uint64(0xC0FFEE0000C0FFEE)
ROWS = {}  # the fence rows: callable of scan.py -> (cases, generator of (shape, operands, call)), as tests/test_gpu_fri_fold.py


def _ids(kinds):
    return [f"{NAMES[m]}-{wa}-{wb}" for m, wa, wb in kinds]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(tf):
    assert tf.lib().tf_device_count() > 0, "no HIP device visible: the product has no CPU fallback"


# ------------------------------------------------------------------ plumbing
def dev64(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).reshape(-1).view(np.int64).copy()).cuda()


def host64(t):
    return t.cpu().numpy().view(np.uint64)


def rand_words(rng, count):
    """canonical raw words (any word below p is the raw word of some element)"""
    return (rng.integers(0, 1 << 63, count, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, count, dtype=np.uint64)) % np.uint64(P)


def edge_column(n, w, shift):
    """n elements drawn from the canonical words of field_ref.edge_words(): 0, 1, p - 1, 2^32 +- 1, the single-bit words, ..."""
    edge = np.array([x for x in field_ref.edge_words() if x < P], dtype=np.uint64)
    return np.resize(np.roll(edge, shift), n * w)


def width_out(mode, wa, wb):
    return wb if mode == SUM else wa


def unstrided(words, n, batch, w, stride):
    return np.concatenate([words[c * stride:c * stride + n * w] for c in range(batch)]) if batch else words[:0]


def call_scan(m, mode, wa, wb, n, batch, d_a, d_b, d_out, a_len, a_sets, sa, sb, so, d_init, d_work, stream=None):
    if mode == SUM:
        m.sum_(d_b, n, d_out, batch=batch, width=wb, stride_in=sb, stride_out=so, init=d_init, work=d_work, stream=stream)
    elif mode == PRODUCT:
        m.product(d_a, n, d_out, batch=batch, width=wa, stride_in=sa, stride_out=so, init=d_init, work=d_work, stream=stream)
    else:
        m.affine(d_a, d_b, n, d_out, batch=batch, width_a=wa, width_b=wb, a_len=a_len, a_sets=a_sets, stride_a=sa, stride_b=sb, stride_out=so,
                 init=d_init, work=d_work, stream=stream)


def run(tf, mode, wa, wb, n, batch, a=None, b=None, a_len=None, a_sets=1, init=None, pads=(1, 2, 3), inplace=False):
    """One call on fresh device buffers.  a, b: packed raw words (batch x n elements; a with a_len = 1: a_sets elements); the strides
    are `pads` words above the minimum, one pad per operand.  Returns the packed result after checking that the padding of out still
    holds its canary, that the inputs are unchanged and (inside workspace()) that nothing else was needed."""
    w = width_out(mode, wa, wb)
    packed_a = mode == AFFINE and a_len == 1   # asked for as such, also at n = 1
    sa, sb, so = n * w + pads[0], n * wb + pads[1], n * w + pads[2]
    h_a = None if mode == SUM else (np.asarray(a, dtype=np.uint64) if packed_a else sr.strided(a, n, batch, w, sa, fill=CANARY64))
    h_b = None if mode == PRODUCT else sr.strided(b, n, batch, wb, sb, fill=CANARY64)
    d_a, d_b = (None if h is None else dev64(h) for h in (h_a, h_b))
    if inplace:
        d_out, so = (d_a, sa) if mode == PRODUCT else (d_b, sb)
    else:
        d_out = dev64(np.full((batch - 1) * so + n * w, CANARY64))
    ws = tf.scan.workspace(mode, n, batch, w)
    assert (ws > 0) == (tf.scan.plan(mode, n, batch, w).launches == 3)
    d_work = dev64(np.full(ws // 8, CANARY64)) if ws else None
    d_init = None if init is None else dev64(init)
    call_scan(tf.scan, mode, wa, wb, n, batch, d_a, d_b, d_out, a_len, a_sets, sa, sb, so, d_init, d_work)
    got = host64(d_out)
    assert (got[sr.padding(n, batch, w, so)] == CANARY64).all(), "a word between n * width and the stride was written"
    for h, d in ((h_a, d_a), (h_b, d_b)):
        if h is not None and d is not d_out:
            assert np.array_equal(host64(d), h), "an input was modified"
    return unstrided(got, n, batch, w, so)


def inputs(rng, mode, wa, wb, n, batch, edge=True):
    """packed a and b of `batch` columns: random canonical words, the last column drawn from the edge words"""
    w = width_out(mode, wa, wb)
    a, b = rand_words(rng, batch * n * w), rand_words(rng, batch * n * wb)
    if edge and batch > 1:
        a[(batch - 1) * n * w:] = edge_column(n, w, 3)
        b[(batch - 1) * n * wb:] = edge_column(n, wb, 11)
    return (None if mode == SUM else a), (None if mode == PRODUCT else b)


# ------------------------------------------------------------------ 1. lengths
@pytest.mark.parametrize("mode,wa,wb", KINDS, ids=_ids(KINDS))
def test_lengths_around_every_boundary(tf, mode, wa, wb):
    w = width_out(mode, wa, wb)
    p = tf.scan.plan(mode, 1, 3, w)
    T, WAVE = p.tile, p.wave
    rng = np.random.default_rng(100 * mode + 10 * wa + wb)
    for n in sorted({1, 2, 63, 64, 65, WAVE - 1, WAVE, WAVE + 1, T - 1, T, T + 1, 2 * T + 1}):
        a, b = inputs(rng, mode, wa, wb, n, 3)
        want, _ = sr.scan(mode, n, 3, a=a, b=b, wa=wa, wb=wb)
        assert np.array_equal(run(tf, mode, wa, wb, n, 3, a=a, b=b), want), n


# ------------------------------------------------------------------ 2. the spine past its first turn
DENSE = [(SUM, 1, 1), (SUM, 3, 3), (PRODUCT, 1, 1), (AFFINE, 1, 1)]
SPARSE = [(PRODUCT, 3, 3), (AFFINE, 3, 3), (AFFINE, 3, 1)]


@pytest.mark.parametrize("mode,wa,wb", DENSE, ids=_ids(DENSE))
def test_spine_takes_a_second_turn_dense(tf, mode, wa, wb):
    """n = S T + T + 1 dense random elements: S + 2 tiles, the last of one element.  The loop reference in pure Python takes about a
    second per 2^19 steps for these four kinds (no XFieldElement product), so every element is random."""
    w = width_out(mode, wa, wb)
    p = tf.scan.plan(mode, 1, 1, w)
    n = p.turn * p.tile + p.tile + 1
    assert tf.scan.plan(mode, n, 1, w).tiles == p.turn + 2
    rng = np.random.default_rng(7 + 10 * mode + w)
    a, b = inputs(rng, mode, wa, wb, n, 1)
    init = rand_words(rng, w)
    want, _ = sr.scan(mode, n, 1, a=a, b=b, wa=wa, wb=wb, init=init)
    assert np.array_equal(run(tf, mode, wa, wb, n, 1, a=a, b=b, init=init), want)


@pytest.mark.parametrize("mode,wa,wb", SPARSE, ids=_ids(SPARSE))
def test_spine_takes_a_second_turn_sparse(tf, mode, wa, wb):
    """The same n for the kinds with an XFieldElement product per step.  NOT dense: the loop reference takes 2.2 s per 2^18 such steps
    in pure Python, more than 5 s at this n.  Instead a_i = 1, b_i = 0 everywhere but at the first and the last element of every
    wave's chunk (the tiles' ends among them), which are dense random: no wave and no tile is an identity that a dropped or
    misplaced map could hide behind, and the reference only has to step at those elements."""
    w = wa
    p = tf.scan.plan(mode, 1, 1, w)
    n = p.turn * p.tile + p.tile + 1
    rng = np.random.default_rng(70 + 10 * mode + wb)
    at = np.array(sorted({q for k in range(0, n, p.wave) for q in (k, min(k + p.wave, n) - 1)}))
    a = np.tile(pr.words([pr.one(w)], w), n).reshape(n, w)
    b = np.zeros((n, wb), dtype=np.uint64)
    a[at] = rand_words(rng, at.size * w).reshape(-1, w)
    if mode == AFFINE:
        b[at] = rand_words(rng, at.size * wb).reshape(-1, wb)
    init = rand_words(rng, w)
    ea, eb = pr.elements(a[at], w), [pr.lift(x, wb, w) for x in pr.elements(b[at], wb)]
    steps = pr.words(sr.loop(ea, eb if mode == AFFINE else None, pr.elements(init, w)[0], w), w).reshape(-1, w)
    want = np.repeat(steps, np.diff(np.append(at, n)), axis=0).reshape(-1)   # y stays where a = 1 and b = 0
    got = run(tf, mode, wa, wb, n, 1, a=a.reshape(-1), b=b.reshape(-1), init=init)
    assert np.array_equal(got, want)


# ------------------------------------------------------------------ 3. multiplier and init forms, special elements
@pytest.mark.parametrize("mode,wa,wb", KINDS, ids=_ids(KINDS))
def test_init_and_multiplier_forms(tf, mode, wa, wb):
    w = width_out(mode, wa, wb)
    T, batch = tf.scan.plan(mode, 1, 3, w).tile, 3
    rng = np.random.default_rng(300 + 10 * mode + wb)
    for n in (1, 65, T + 1):   # n = 1: the table of one row at its stride, and the packed forms, which stride_a = 0 tells apart
        a, b = inputs(rng, mode, wa, wb, n, batch)
        forms = [(None, 1, a)] + ([(1, 1, rand_words(rng, w)), (1, batch, rand_words(rng, batch * w))] if mode == AFFINE else [])
        for a_len, a_sets, a_words in forms:
            for n_init in (0, 1, batch):
                init = rand_words(rng, n_init * w) if n_init else None
                want, _ = sr.scan(mode, n, batch, a=a_words, b=b, wa=wa, wb=wb, a_len=a_len, a_sets=a_sets, init=init)
                got = run(tf, mode, wa, wb, n, batch, a=a_words, b=b, a_len=a_len, a_sets=a_sets, init=init)
                assert np.array_equal(got, want), (n, a_len, a_sets, n_init)


@pytest.mark.parametrize("wa,wb", sr.PAIRS)
def test_affine_special_elements(tf, wa, wb):
    """a = 0 forgets everything before it; a = 1 throughout is the sum; b = 0 throughout is the product"""
    w = wa
    n, batch = 2 * tf.scan.plan(AFFINE, 1, 3, w).tile + 1, 3
    rng = np.random.default_rng(40 + wb)
    a, b = inputs(rng, AFFINE, wa, wb, n, batch, edge=False)
    a, b = a.reshape(batch, n, w), b.reshape(batch, n, wb)
    k = n // 2 + 7
    a[0, k] = 0
    a[1] = pr.words([pr.one(w)], w)
    b[2] = 0
    init = rand_words(rng, batch * w)
    want, _ = sr.scan(AFFINE, n, batch, a=a.reshape(-1), b=b.reshape(-1), wa=wa, wb=wb, init=init)
    got = run(tf, AFFINE, wa, wb, n, batch, a=a.reshape(-1), b=b.reshape(-1), init=init)
    assert np.array_equal(got, want)
    got = got.reshape(batch, n, w)
    assert np.array_equal(got[0, k, :wb], b[0, k]) and not got[0, k, wb:].any()
    assert np.array_equal(got[1], sr.scan(SUM, n, 1, b=pr.words([pr.lift(x, wb, w) for x in pr.elements(b[1], wb)], w), wa=w, wb=w, init=init[w:2 * w])[0].reshape(n, w))
    assert np.array_equal(got[2], sr.scan(PRODUCT, n, 1, a=a[2].reshape(-1), wa=w, wb=w, init=init[2 * w:])[0].reshape(n, w))


@pytest.mark.parametrize("w", [1, 3])
def test_a_zero_in_a_product_column_stays_in_its_column(tf, w):
    n, batch = 2 * tf.scan.plan(PRODUCT, 1, 3, w).tile + 1, 3
    rng = np.random.default_rng(50 + w)
    a = rand_words(rng, batch * n * w).reshape(batch, n, w)
    k = 1234
    a[1, k] = 0
    want, _ = sr.scan(PRODUCT, n, batch, a=a.reshape(-1), wa=w, wb=w)
    got = run(tf, PRODUCT, w, w, n, batch, a=a.reshape(-1))
    assert np.array_equal(got, want)
    got = got.reshape(batch, n, w)
    assert not got[1, k:].any() and got[1, :k].any(axis=1).all() and got[0].any(axis=1).all() and got[2].any(axis=1).all()


# ------------------------------------------------------------------ 4. batches
BATCHED = [(SUM, 1, 1), (PRODUCT, 3, 3), (AFFINE, 1, 1)]


@pytest.mark.parametrize("mode,wa,wb", BATCHED, ids=_ids(BATCHED))
def test_65537_columns_of_three(tf, mode, wa, wb):
    n, batch = 3, 65537
    rng = np.random.default_rng(65537 + mode)
    a, b = inputs(rng, mode, wa, wb, n, batch, edge=False)
    init = rand_words(rng, batch * width_out(mode, wa, wb))
    want, _ = sr.scan(mode, n, batch, a=a, b=b, wa=wa, wb=wb, init=init)
    assert np.array_equal(run(tf, mode, wa, wb, n, batch, a=a, b=b, init=init), want)


@pytest.mark.parametrize("mode,wa,wb", KINDS, ids=_ids(KINDS))
def test_257_short_columns_share_workgroups(tf, mode, wa, wb):
    n, batch = 5, 257
    rng = np.random.default_rng(257 + 10 * mode + wb)
    a, b = inputs(rng, mode, wa, wb, n, batch)
    want, _ = sr.scan(mode, n, batch, a=a, b=b, wa=wa, wb=wb)
    assert np.array_equal(run(tf, mode, wa, wb, n, batch, a=a, b=b), want)


@pytest.mark.parametrize("wa,wb", sr.PAIRS)
def test_two_long_columns_with_a_multiplier_each(tf, wa, wb):
    n, batch = 2 * tf.scan.plan(AFFINE, 1, 2, wa).tile + 1, 2
    rng = np.random.default_rng(2 + wb)
    _, b = inputs(rng, AFFINE, wa, wb, n, batch)
    a, init = rand_words(rng, batch * wa), rand_words(rng, batch * wa)
    want, _ = sr.scan(AFFINE, n, batch, a=a, b=b, wa=wa, wb=wb, a_len=1, a_sets=batch, init=init)
    assert np.array_equal(run(tf, AFFINE, wa, wb, n, batch, a=a, b=b, a_len=1, a_sets=batch, init=init), want)


# ------------------------------------------------------------------ 5. splitting a scan in two
@pytest.mark.parametrize("mode,wa,wb", KINDS, ids=_ids(KINDS))
def test_two_scans_chained_through_init_are_the_whole_scan(tf, mode, wa, wb):
    """[0, k) and then [k, n) from the last element of the first, device against device, nothing read back in between"""
    import torch

    w = width_out(mode, wa, wb)
    T = tf.scan.plan(mode, 1, 2, w).tile
    n, batch = 2 * T + 1, 2
    rng = np.random.default_rng(500 + 10 * mode + wb)
    a, b = inputs(rng, mode, wa, wb, n, batch)
    sa, sb, so = n * w + 1, n * wb + 2, n * w + 3
    d_a = None if a is None else dev64(sr.strided(a, n, batch, w, sa, fill=CANARY64))
    d_b = None if b is None else dev64(sr.strided(b, n, batch, wb, sb, fill=CANARY64))
    d_init = dev64(rand_words(rng, batch * w))
    work = lambda m: dev64(np.full(tf.scan.workspace(mode, m, batch, w) // 8, CANARY64)) if tf.scan.workspace(mode, m, batch, w) else None  # noqa: E731
    d_whole = dev64(np.full((batch - 1) * so + n * w, CANARY64))
    call_scan(tf.scan, mode, wa, wb, n, batch, d_a, d_b, d_whole, n, 1, sa, sb, so, d_init, work(n))
    for k in (T, T + 1):
        d_parts = dev64(np.full((batch - 1) * so + n * w, CANARY64))
        call_scan(tf.scan, mode, wa, wb, k, batch, d_a, d_b, d_parts, k, 1, sa, sb, so, d_init, work(k))
        d_mid = torch.cat([d_parts[c * so + (k - 1) * w:c * so + k * w] for c in range(batch)])
        call_scan(tf.scan, mode, wa, wb, n - k, batch, None if d_a is None else d_a[k * w:], None if d_b is None else d_b[k * wb:], d_parts[k * w:], n - k, 1,
                  sa, sb, so, d_mid, work(n - k))
        assert torch.equal(d_parts, d_whole), k
    want, _ = sr.scan(mode, n, batch, a=a, b=b, wa=wa, wb=wb, init=host64(d_init))
    assert np.array_equal(unstrided(host64(d_whole), n, batch, w, so), want)


# ------------------------------------------------------------------ 6. the exact in-place forms
@pytest.mark.parametrize("mode,wa,wb", [k for k in KINDS if k[1] == k[2]], ids=_ids([k for k in KINDS if k[1] == k[2]]))
def test_in_place_equals_out_of_place(tf, mode, wa, wb):
    w = width_out(mode, wa, wb)
    p = tf.scan.plan(mode, 1, 2, w)
    rng = np.random.default_rng(600 + 10 * mode + w)
    for n in (p.wave - 3, p.tile - 3, 2 * p.tile + 1):
        a, b = inputs(rng, mode, wa, wb, n, 2)
        init = rand_words(rng, w)
        apart = run(tf, mode, wa, wb, n, 2, a=a, b=b, init=init)
        assert np.array_equal(run(tf, mode, wa, wb, n, 2, a=a, b=b, init=init, inplace=True), apart), n
        assert np.array_equal(apart, sr.scan(mode, n, 2, a=a, b=b, wa=wa, wb=wb, init=init)[0]), n


# ------------------------------------------------------------------ 7. no host in the chain
def test_sample_and_scan_without_a_host_round_trip(tf):
    """init -> pad_and_absorb_all of different words -> sample_scalars (one per sponge) -> the running evaluation of two columns, each
    under its own sponge's challenge, the sampler's output tensor handed straight on as the multipliers; ONE synchronisation at the
    end and no intermediate copy."""
    import torch

    n, n_sponges = 2 * tf.scan.plan(AFFINE, 1, 2, 3).tile + 1, 2
    rng = np.random.default_rng(64)
    absorbed = rand_words(rng, n_sponges * 5).reshape(n_sponges, 5)
    v = rand_words(rng, n_sponges * n)
    d_v, d_absorbed = dev64(v), dev64(absorbed)
    d_states = torch.full((16 * n_sponges,), -1, dtype=torch.int64, device="cuda")
    d_ch = torch.full((n_sponges * 3,), -1, dtype=torch.int64, device="cuda")
    d_out = dev64(np.full(n_sponges * n * 3, CANARY64))
    d_work = dev64(np.full(tf.scan.workspace(AFFINE, n, n_sponges, 3) // 8, CANARY64))
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()  # (the uploads above, made on the default stream)
    with torch.cuda.stream(stream):
        tf.device.tip5_sponge_init_(d_states, stream=stream)
        tf.device.tip5_sponge_pad_and_absorb_all_(d_states, d_absorbed, stream=stream)
        tf.device.tip5_sponge_sample_scalars(d_states, d_ch, stream=stream)
        tf.scan.affine(d_ch, d_v, n, d_out, batch=n_sponges, width_a=3, width_b=1, a_len=1, a_sets=n_sponges, work=d_work, stream=stream)
    stream.synchronize()
    ch = np.stack([sponge_ref.sample_scalars(sponge_ref.pad_and_absorb_all(sponge_ref.init(), absorbed[s]), 1)[1] for s in range(n_sponges)])
    assert np.array_equal(host64(d_ch), ch.reshape(-1)) and not np.array_equal(ch[0], ch[1])
    want, _ = sr.scan(AFFINE, n, n_sponges, a=ch.reshape(-1), b=v, wa=3, wb=1, a_len=1, a_sets=n_sponges)
    assert np.array_equal(host64(d_out), want)


# ------------------------------------------------------------------ 8. against the library itself, device against device
@pytest.mark.parametrize("w", [1, 3])
def test_product_of_a_constant_column_is_tf_powers(tf, w):
    import torch

    n = 3 * tf.scan.plan(PRODUCT, 1, 1, w).tile + 17
    rng = np.random.default_rng(80 + w)
    first, ratio = rand_words(rng, w), rand_words(rng, w)
    d_want = dev64(np.full((n + 1) * w, CANARY64))
    tf.device.powers(first if w == 3 else int(first[0]), ratio if w == 3 else int(ratio[0]), d_want, width=w)
    d_got = dev64(np.full(n * w, CANARY64))
    d_work = dev64(np.full(tf.scan.workspace(PRODUCT, n, 1, w) // 8, CANARY64))
    tf.scan.product(dev64(np.tile(ratio, n)), n, d_got, width=w, init=dev64(first), work=d_work)
    assert torch.equal(d_got, d_want[w:])   # powers starts at `first`, the scan one step further


def test_horner_form_is_evaluate_bfe_at_xfe(tf):
    import torch

    n = 2 * tf.scan.plan(AFFINE, 1, 1, 3).tile + 5
    rng = np.random.default_rng(90)
    coeffs, x = rand_words(rng, n), rand_words(rng, 3)
    d_want = dev64(np.full(3, CANARY64))
    tf.device.evaluate_bfe_at_xfe(dev64(coeffs), n, dev64(x), d_want)
    d_got = dev64(np.full(n * 3, CANARY64))
    d_work = dev64(np.full(tf.scan.workspace(AFFINE, n, 1, 3) // 8, CANARY64))
    tf.scan.affine(dev64(x), dev64(coeffs[::-1].copy()), n, d_got, width_a=3, width_b=1, a_len=1, work=d_work)
    assert torch.equal(d_got[-3:], d_want)


# ------------------------------------------------------------------ 9. the numpy forms
@pytest.mark.parametrize("mode,wa,wb", KINDS, ids=_ids(KINDS))
def test_host_forms(tf, mode, wa, wb):
    w = width_out(mode, wa, wb)
    rng = np.random.default_rng(900 + 10 * mode + wb)
    for n in (9, tf.scan.plan(mode, 1, 2, w).tile + 9):
        a, b = inputs(rng, mode, wa, wb, n, 2)
        init = rand_words(rng, 2 * w)
        want, _ = sr.scan(mode, n, 2, a=a, b=b, wa=wa, wb=wb, init=init)
        if mode == SUM:
            got = tf.scan.sum_host(b, n, batch=2, width=w, init=init)
        elif mode == PRODUCT:
            got = tf.scan.product_host(a, n, batch=2, width=w, init=init)
        else:
            got = tf.scan.affine_host(a, b, n, batch=2, width_a=wa, width_b=wb, init=init)
        assert np.array_equal(got, want), n
    assert tf.scan.sum_host(np.zeros(0, np.uint64), 0).size == 0


# ------------------------------------------------------------------ 10. fence rows: one per tensor-taking callable of scan.py
def row(name, cases):
    def register(gen):
        assert name not in ROWS, name
        ROWS[name] = (list(cases), gen)
        return gen
    return register


def _fence_case(m, mode, wa, wb, n_of, batch, a_form, n_init, inplace):
    """One fenced shape.  n_of: function of the plan -> n.  Operands: the inputs with their padding poisoned, out with its padding as
    kept slots, init, and the work space as a pure output of exactly workspace() bytes whose every word is known: the tile maps and
    start values of the blocked model, the slot of each column's last tile kept."""
    w = width_out(mode, wa, wb)
    p = m.plan(mode, 1, batch, w)
    n = n_of(p)
    rng = np.random.default_rng(1000 * mode + 100 * wb + n % 97 + batch)
    a, b = inputs(rng, mode, wa, wb, n, batch)
    a_len, a_sets = (n, 1) if a_form is None else (1, a_form)
    if a_len != n and mode == AFFINE:
        a = rand_words(rng, a_sets * w)
    init = rand_words(rng, n_init * w) if n_init else None
    tiled = n > p.tile
    want, inner = sr.scan(mode, n, batch, a=a, b=b, wa=wa, wb=wb, a_len=a_len, a_sets=a_sets, init=init, tile=p.tile if tiled else None, turn=p.turn)
    if not tiled:
        assert m.workspace(mode, n, batch, w) == 0
    sa, sb, so = n * w + 1, n * wb + 2, n * w + 3
    if inplace:
        so = sa if mode == PRODUCT else sb
    ops, names = [], {}
    pad_out = sr.padding(n, batch, w, so)
    for key, words, width, stride in (("a", a, w, sa), ("b", b, wb, sb)):
        if words is None:
            continue
        if key == "a" and mode == AFFINE and a_len != n:
            ops.append(fence.inp("a", words))
        elif inplace and key == ("a" if mode == PRODUCT else "b"):
            ops.append(fence.Operand(key, pad_out.size, data=sr.strided(words, n, batch, width, stride), poisoned=pad_out,
                                     expect=sr.strided(want, n, batch, w, so), kept=pad_out))
        else:
            ops.append(fence.inp(key, sr.strided(words, n, batch, width, stride), padding=sr.padding(n, batch, width, stride)))
    if not inplace:
        ops.append(fence.out("out", sr.strided(want, n, batch, w, so), kept=pad_out))
    if init is not None:
        ops.append(fence.inp("init", init))
    if tiled:
        words, kept = sr.work_words(mode, inner, w)
        assert words.size * 8 == m.workspace(mode, n, batch, w)
        ops.append(fence.out("work", words, kept=kept))

    def call(a=None, b=None, out=None, init=None, work=None):
        if out is None:
            out = a if mode == PRODUCT else b
        call_scan(m, mode, wa, wb, n, batch, a, b, out, a_len, a_sets, sa, sb, so, init, work)

    shape = f"({wa}, {wb}) n={n} batch={batch} a_len={a_len} a_sets={a_sets} n_init={n_init}{' in place' if inplace else ''}"
    return shape, ops, call


_ONE_WAVE, _ONE_TILE, _THREE_TILES = (lambda p: 65), (lambda p: p.tile - 1), (lambda p: 2 * p.tile + 1)
# (width, n, batch, n_init, in place): one wave per column; one tile; three launches, with and without in place
_ONE_OPERAND_CASES = [(1, _ONE_WAVE, 3, 0, False), (3, _ONE_WAVE, 3, 3, True), (1, _ONE_TILE, 2, 1, False), (3, _ONE_TILE, 2, 0, True),
                      (1, _THREE_TILES, 2, 2, False), (3, _THREE_TILES, 2, 1, False), (1, _THREE_TILES, 1, 0, True)]


@row("sum_", cases=_ONE_OPERAND_CASES)
def _fence_sum(tf, m, w, n_of, batch, n_init, inplace):
    yield _fence_case(m, SUM, w, w, n_of, batch, None, n_init, inplace)


@row("product", cases=_ONE_OPERAND_CASES)
def _fence_product(tf, m, w, n_of, batch, n_init, inplace):
    yield _fence_case(m, PRODUCT, w, w, n_of, batch, None, n_init, inplace)


# (width_a, width_b, n, batch, a_sets with a_len = 1 or None for a_len = n, n_init, in place)
@row("affine", cases=[(1, 1, _ONE_WAVE, 3, None, 0, False), (3, 1, _ONE_WAVE, 3, 3, 1, False), (3, 3, _ONE_TILE, 2, 1, 2, True), (3, 1, _ONE_TILE, 2, None, 0, False),
                      (1, 1, _THREE_TILES, 2, None, 2, True), (3, 3, _THREE_TILES, 2, 2, 1, False), (3, 1, _THREE_TILES, 2, 1, 0, False),
                      (3, 3, _THREE_TILES, 1, None, 1, False)])
def _fence_affine(tf, m, wa, wb, n_of, batch, a_form, n_init, inplace):
    yield _fence_case(m, AFFINE, wa, wb, n_of, batch, a_form, n_init, inplace)


def _fence_params():
    return [pytest.param(name, case, id=f"{name}-{i}") for name in ROWS for i, case in enumerate(ROWS[name][0])]


@pytest.mark.parametrize("name,case", _fence_params())
def test_fenced(tf, name, case):
    _, gen = ROWS[name]
    for shape, operands, call in gen(tf, tf.scan, *case):
        fence.run(name, shape, operands, call)


def test_every_tensor_taking_callable_of_the_module_has_a_fence_row(tf):
    import inspect

    m = tf.scan
    public = [name for name, f in vars(m).items() if inspect.isfunction(f) and f.__module__ == m.__name__ and not name.startswith("_")]
    assert sorted(public) == sorted(list(ROWS) + ["sum_host", "product_host", "affine_host", "plan", "workspace"]), \
        "numpy forms and host arithmetic need no row; every other call does"


def test_a_tile_fits_the_guard_words(tf):
    """the condition under fence.G: what one workgroup moves per operand stays below the guard, so a workgroup one tile off lands
    in a guard and not in a neighbouring allocation"""
    for mode, wa, wb in KINDS:
        w = width_out(mode, wa, wb)
        assert tf.scan.plan(mode, 1, 1, w).tile * w < fence.G


# ------------------------------------------------------------------ 11. the wrapper's own checks
def test_python_argument_checks_come_before_any_launch(tf):
    import torch

    T = tf.scan.plan(SUM, 1, 1, 1).tile
    d_x, d_out = dev64(np.zeros(24)), dev64(np.full(24, CANARY64))
    both = dev64(np.full(48, CANARY64))
    with pytest.raises(ValueError):  # overlapping, not exactly in place
        tf.scan.sum_(both[:24], 8, both[1:25], batch=3)
    with pytest.raises(ValueError):  # out on the multipliers
        tf.scan.affine(both[:3], d_x, 8, both[:24], a_len=1)
    with pytest.raises(ValueError):  # a short out
        tf.scan.product(d_x, 8, d_out[:-1], batch=3)
    with pytest.raises(ValueError):  # two tiles and no work space
        tf.scan.sum_(dev64(np.zeros(T + 1)), T + 1, dev64(np.zeros(T + 1)))
    with pytest.raises(ValueError):
        tf.scan.affine(d_x, d_x, 8, d_out, width_a=1, width_b=3)
    with pytest.raises(TypeError):
        tf.scan.sum_(d_x.to(torch.int32), 8, d_out, batch=3)
    with pytest.raises(TypeError):
        tf.scan.sum_(d_x.cpu(), 8, d_out, batch=3)
    torch.cuda.synchronize()
    assert (host64(d_out) == CANARY64).all() and (host64(both) == CANARY64).all()
