"""The FRI fold on the device (twenty_first_amd/fri.py over tf_fri_fold_dev / tf_fri_fold) against tests/fri_ref.py, word for word.

Every device output starts as canary words and is compared whole.  What the shapes are for (csrc/fri_kernels.h, tf_fri.hip):
    one pass            up to R_max levels in registers; levels in {1, R_max} are one launch, R_max + 1 splits with a remainder of 1,
                        levels = k leaves one element per codeword
    the launch          256-thread workgroups over batch x n / 2^R outputs, flattened: n = 2 ... 2^13 is one pair, less than a wave, one
                        workgroup, several workgroups; 257 codewords of 4 elements share waves and leave a ragged last one
    the walk            a thread takes a second output only above 8 workgroups per compute unit (2^19 threads on 256 compute units):
                        the long codewords are the first sizes at which it does, with and without a product on the way
The model folds a codeword of n elements in pure Python; where n is large it is asked for single outputs instead: output i of r
levels depends on the inputs i + t n / 2^r alone, which are a codeword of 2^r elements on the offset g w_n^i."""
import numpy as np
import pytest

from tests import fence
from tests import field_ref
from tests import fri_ref
from tests import points_ref as pr
from tests import pyref
from tests import sponge_ref

pytestmark = pytest.mark.gpu

P = pyref.P
PAIRS = pr.PAIRS  # (width_c, width_a)
CANARY64 = np.uint64(0xC0FFEE0000C0FFEE)
ROWS = {}  # the fence rows: callable of fri.py -> (cases, generator of (shape, operands, call)), as tests/test_gpu_merkle_sampled.py


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(tf):
    assert tf.lib().tf_device_count() > 0, "no HIP device visible: the product has no CPU fallback"


@pytest.fixture(scope="module")
def rmax(tf):
    return max(tf.fri.plan(1 << 12, 12))


# ------------------------------------------------------------------ plumbing
def dev64(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).reshape(-1).view(np.int64).copy()).cuda()


def host64(t):
    return t.cpu().numpy().view(np.uint64)


def rand_words(rng, count):
    """canonical raw words (any word below p is the raw word of some element)"""
    return (rng.integers(0, 1 << 63, count, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, count, dtype=np.uint64)) % np.uint64(P)


def run_fold(tf, cw, n, g_raw, ch, batch=1, levels=1, n_sets=1, wc=3, wa=3):
    d_out = dev64(np.full(batch * (n >> levels) * wa, CANARY64))
    tf.fri.fold(dev64(cw), n, g_raw, dev64(ch), d_out, batch=batch, levels=levels, n_sets=n_sets, width_c=wc, width_a=wa)
    return host64(d_out)


def model_prefixes(cw, n, wc, g, alphas, wa):
    """{r: words after r levels} for every r <= len(alphas): the chain of the model, each level computed once"""
    c, out = pr.elements(cw, wc), {}
    for r, alpha in enumerate(alphas, 1):
        c = fri_ref.fold_level(c, n, wc, g, alpha, wa)
        n, wc, g = n // 2, wa, g * g % P
        out[r] = pr.words(c, wa)
    return out


# ------------------------------------------------------------------ 1. the sweep
@pytest.mark.parametrize("wc,wa", PAIRS)
@pytest.mark.parametrize("k", range(1, 14))
def test_sweep_of_lengths_and_levels(tf, rmax, k, wc, wa):
    n = 1 << k
    rng = np.random.default_rng(100 * k + 10 * wc + wa)
    g = int(rand_words(rng, 1)[0]) or 1
    cw, ch = rand_words(rng, n * wc), rand_words(rng, k * wa)
    want = model_prefixes(cw, n, wc, pyref.to_val(g), pr.elements(ch, wa), wa)
    for levels in sorted({1, rmax, rmax + 1, k} & set(range(1, k + 1))):
        assert tf.fri.plan(n, levels, wc, wa) == [rmax] * (levels // rmax) + ([levels % rmax] if levels % rmax else [])
        assert np.array_equal(run_fold(tf, cw, n, g, ch[:levels * wa], levels=levels, wc=wc, wa=wa), want[levels]), levels
    if k == 5:  # the host form, once per width pair
        assert np.array_equal(tf.fri_fold(cw, n, g, ch[:4 * wa], levels=4, width_c=wc, width_a=wa), want[4])


# ------------------------------------------------------------------ 2. batches and challenge sets
@pytest.mark.parametrize("wc,wa", PAIRS)
def test_batches_with_one_set_and_with_a_set_per_codeword(tf, rmax, wc, wa):
    n, batch = 1 << 9, 3
    rng = np.random.default_rng(9 + wc + wa)
    g = pyref.to_raw(7)
    cw = rand_words(rng, batch * n * wc)
    for levels in (1, rmax + 1):
        for n_sets in (1, 3):
            ch = rand_words(rng, n_sets * levels * wa)
            want = fri_ref.fold(cw, n, batch, wc, g, ch, levels, n_sets, wa)
            assert np.array_equal(run_fold(tf, cw, n, g, ch, batch, levels, n_sets, wc, wa), want), (levels, n_sets)


@pytest.mark.parametrize("wc,wa", PAIRS)
def test_257_tiny_codewords_share_waves(tf, wc, wa):
    n, batch, levels = 4, 257, 2
    rng = np.random.default_rng(257 + wc + wa)
    g = int(rand_words(rng, 1)[0]) or 1
    cw = rand_words(rng, batch * n * wc)
    for n_sets in (1, batch):
        ch = rand_words(rng, n_sets * levels * wa)
        want = fri_ref.fold(cw, n, batch, wc, g, ch, levels, n_sets, wa)
        assert np.array_equal(run_fold(tf, cw, n, g, ch, batch, levels, n_sets, wc, wa), want), n_sets


# ------------------------------------------------------------------ 3. edge words
@pytest.mark.parametrize("wc,wa", PAIRS)
@pytest.mark.parametrize("g", [1, 7, P - 1])
def test_edge_words_and_special_challenges(tf, g, wc, wa):
    """the canonical words of field_ref.edge_words() as raw codeword words (a codeword holds canonical words by contract); the
    challenges 0, 1, all limbs p - 1, and the two that lie on the line's own points and must hand back c[j] and c[j + n/2] exactly"""
    n, j = 1 << 8, 37
    edge = np.array([w for w in field_ref.edge_words() if w < P], dtype=np.uint64)
    cw = np.resize(edge, n * wc)
    xs = fri_ref.domain(g, n)
    c = np.array([cw[i * wc:(i + 1) * wc].tolist() + [0] * (wa - wc) for i in range(n)], dtype=np.uint64)  # lifted, raw words
    alphas = {"zero": pr.zero(wa), "one": pr.one(wa), "max": P - 1 if wa == 1 else (P - 1,) * 3, "x_j": pr.lift(xs[j], 1, wa),
              "-x_j": pr.lift(P - xs[j], 1, wa)}
    for name, alpha in alphas.items():
        ch = pr.words([alpha], wa)
        got = run_fold(tf, cw, n, pyref.to_raw(g), ch, wc=wc, wa=wa)
        assert np.array_equal(got, fri_ref.fold(cw, n, 1, wc, pyref.to_raw(g), ch, 1, 1, wa)), name
        if name == "x_j":
            assert np.array_equal(got.reshape(-1, wa)[j], c[j])
        if name == "-x_j":
            assert np.array_equal(got.reshape(-1, wa)[j], c[j + n // 2])


# ------------------------------------------------------------------ 4. long codewords: the walk
@pytest.mark.parametrize("wc,wa,k", [(3, 3, 21), (1, 1, 22)])
def test_long_codeword(tf, rmax, wc, wa, k):
    """2^21 XFieldElements: a thread of the one-level fold takes two outputs 2^19 apart (one product on the way); 2^22 BFieldElements:
    the same for the two-level pass.  The multi-level calls equal the chain of single-level device calls; 256 sampled outputs of each
    equal the model."""
    import torch

    n = 1 << k
    rng = np.random.default_rng(k)
    g = int(rand_words(rng, 1)[0]) or 1
    d_cw = torch.empty(n * wc, dtype=torch.int64, device="cuda")
    tf.device.fill_random(d_cw, 0xF01D + k)
    ch = rand_words(rng, (rmax + 1) * wa)
    d_ch = dev64(ch)
    chain, cur, w, off = {}, d_cw, wc, pyref.to_val(g)
    for r in range(1, rmax + 2):
        nxt = dev64(np.full((n >> r) * wa, CANARY64))
        tf.fri.fold(cur, n >> (r - 1), pyref.to_raw(off), d_ch[(r - 1) * wa:r * wa], nxt, width_c=w, width_a=wa)
        chain[r], cur, w, off = nxt, nxt, wa, off * off % P
    picks = np.unique(np.concatenate([[0, 1, 63, 64, 255, 256], rng.integers(0, n >> (rmax + 1), 250)]))
    w_n = pyref.root_of_unity(n)
    for levels in (1, 2, rmax + 1):
        m = n >> levels
        d_out = dev64(np.full(m * wa, CANARY64))
        tf.fri.fold(d_cw, n, g, d_ch[:levels * wa], d_out, levels=levels, width_c=wc, width_a=wa)
        assert torch.equal(d_out, chain[levels]), levels
        idx = np.unique(np.concatenate([picks, m - 1 - picks]))  # both ends: the first and the second step of the walk
        rows = (idx[:, None] + m * np.arange(1 << levels)[None, :]).reshape(-1)
        sub = host64(d_cw.view(-1, wc)[torch.from_numpy(rows).cuda()].reshape(-1)).reshape(idx.size, -1)
        got = host64(d_out).reshape(-1, wa)
        alphas = pr.elements(ch[:levels * wa], wa)
        for q, i in enumerate(idx):
            off_i = pyref.to_val(g) * pow(w_n, int(i), P) % P
            want = fri_ref.fold_elements(pr.elements(sub[q], wc), 1 << levels, wc, off_i, alphas, wa)
            assert np.array_equal(got[i], pr.words(want, wa)), (levels, int(i))


# ------------------------------------------------------------------ 5. against the composition it replaces, device against device
@pytest.mark.parametrize("wc,wa", [(1, 3), (3, 3)])
def test_equals_two_powers_and_get_colinear_y(tf, wc, wa):
    import torch

    n, h = 1 << 12, 1 << 11
    rng = np.random.default_rng(12 + wc)
    g = int(rand_words(rng, 1)[0]) or 1
    cw, ch = rand_words(rng, n * wc), rand_words(rng, wa)
    d_x0, d_x1 = torch.empty(h, dtype=torch.int64, device="cuda"), torch.empty(h, dtype=torch.int64, device="cuda")
    w_raw = pyref.to_raw(pyref.root_of_unity(n))
    tf.device.powers(g, w_raw, d_x0)
    tf.device.powers(pyref.to_raw(P - pyref.to_val(g)), w_raw, d_x1)
    lifted = np.zeros((n, wa), dtype=np.uint64)
    lifted[:, :wc] = cw.reshape(n, wc)
    d_y = dev64(lifted)
    d_want, d_got = dev64(np.full(h * wa, CANARY64)), dev64(np.full(h * wa, CANARY64))
    tf.device.get_colinear_y(d_x0, d_y[:h * wa], d_x1, d_y[h * wa:], dev64(ch), d_want, width_x=1, width_y=wa)
    tf.fri.fold(dev64(cw), n, g, dev64(ch), d_got, width_c=wc, width_a=wa)
    assert torch.equal(d_got, d_want)


# ------------------------------------------------------------------ 6. on polynomials
def test_fold_of_a_coset_evaluation_is_the_coset_evaluation_of_even_plus_alpha_odd(tf):
    import torch

    n, g = 1 << 10, 7
    rng = np.random.default_rng(1010)
    F = pyref.Field(3)
    coeffs, ch = rand_words(rng, n * 3), rand_words(rng, 3)
    p, alpha = pr.elements(coeffs, 3), pr.elements(ch, 3)[0]
    folded = pr.words([F.add(p[2 * i], F.mul(alpha, p[2 * i + 1])) for i in range(n // 2)], 3)
    d_c, d_want = torch.empty(n * 3, dtype=torch.int64, device="cuda"), torch.empty(n // 2 * 3, dtype=torch.int64, device="cuda")
    tf.device.coset_evaluate(dev64(coeffs), n, pyref.to_raw(g), d_c, n, width=3)
    tf.device.coset_evaluate(dev64(folded), n // 2, pyref.to_raw(g * g % P), d_want, n // 2, width=3)
    d_got = dev64(np.full(n // 2 * 3, CANARY64))
    tf.fri.fold(d_c, n, pyref.to_raw(g), dev64(ch), d_got)
    assert torch.equal(d_got, d_want)


# ------------------------------------------------------------------ 7. no host in the chain
def test_sample_and_fold_without_a_host_round_trip(tf):
    """init -> pad_and_absorb_all of different words -> sample_scalars (two per sponge) -> fold of two codewords by two levels, the
    sampler's output tensor handed straight on as the challenges; ONE synchronisation at the end and no intermediate copy."""
    import torch

    n, levels, n_sponges = 64, 2, 2
    rng = np.random.default_rng(64)
    absorbed = rand_words(rng, n_sponges * 5).reshape(n_sponges, 5)
    cw = rand_words(rng, n_sponges * n * 3)
    g = pyref.to_raw(7)
    d_cw, d_absorbed = dev64(cw), dev64(absorbed)
    d_states = torch.full((16 * n_sponges,), -1, dtype=torch.int64, device="cuda")
    d_ch = torch.full((n_sponges * levels * 3,), -1, dtype=torch.int64, device="cuda")
    d_out = dev64(np.full(n_sponges * (n >> levels) * 3, CANARY64))
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()  # (the uploads above, made on the default stream)
    with torch.cuda.stream(stream):
        tf.device.tip5_sponge_init_(d_states, stream=stream)
        tf.device.tip5_sponge_pad_and_absorb_all_(d_states, d_absorbed, stream=stream)
        tf.device.tip5_sponge_sample_scalars(d_states, d_ch, stream=stream)
        tf.fri.fold(d_cw, n, g, d_ch, d_out, batch=n_sponges, levels=levels, n_sets=n_sponges, stream=stream)
    stream.synchronize()
    ch = np.stack([sponge_ref.sample_scalars(sponge_ref.pad_and_absorb_all(sponge_ref.init(), absorbed[s]), levels)[1] for s in range(n_sponges)])
    assert np.array_equal(host64(d_ch), ch.reshape(-1)) and not np.array_equal(ch[0], ch[1])
    assert np.array_equal(host64(d_out), fri_ref.fold(cw, n, n_sponges, 3, g, ch.reshape(-1), levels, n_sponges, 3))


# ------------------------------------------------------------------ 8. fence rows: one per tensor-taking callable of fri.py
def row(name, cases):
    def register(gen):
        assert name not in ROWS, name
        ROWS[name] = (list(cases), gen)
        return gen
    return register


# (width_c, width_a, log n, batch, levels - R_max or None for all log n levels, n_sets): a full pass; two passes with one intermediate;
# four passes that take both intermediates in turn; single pairs
@row("fold", cases=[(1, 3, 9, 3, 0, 1), (3, 3, 9, 3, 0, 3), (1, 3, 9, 3, 1, 3), (3, 3, 9, 3, 1, 1), (3, 3, 10, 2, None, 2), (1, 1, 1, 5, None, 1)])
def _fence_fold(tf, m, rmax, wc, wa, k, batch, extra, n_sets):
    n = 1 << k
    levels = k if extra is None else rmax + extra
    rng = np.random.default_rng(1000 * k + levels)
    g = int(rand_words(rng, 1)[0]) or 1
    cw, ch = rand_words(rng, batch * n * wc), rand_words(rng, n_sets * levels * wa)
    want = fri_ref.fold(cw, n, batch, wc, g, ch, levels, n_sets, wa)
    assert (m.workspace(n, batch, levels, wc, wa) > 0) == (levels > rmax)
    ops = [fence.inp("codewords", cw), fence.inp("challenges", ch), fence.out("out", want)]
    yield (f"({wc}, {wa}) n=2^{k} batch={batch} levels={levels} n_sets={n_sets}", ops,
           lambda codewords, challenges, out: m.fold(codewords, n, g, challenges, out, batch=batch, levels=levels, n_sets=n_sets, width_c=wc, width_a=wa))


def _fence_params():
    return [pytest.param(name, case, id=f"{name}-{i}") for name in ROWS for i, case in enumerate(ROWS[name][0])]


@pytest.mark.parametrize("name,case", _fence_params())
def test_fenced(tf, rmax, name, case):
    _, gen = ROWS[name]
    for shape, operands, call in gen(tf, tf.fri, rmax, *case):
        fence.run(name, shape, operands, call)


def test_every_tensor_taking_callable_of_the_module_has_a_fence_row(tf):
    import inspect

    m = tf.fri
    public = [name for name, f in vars(m).items() if inspect.isfunction(f) and f.__module__ == m.__name__ and not name.startswith("_")]
    assert sorted(public) == sorted(list(ROWS) + ["fold_host", "plan", "workspace"]), "numpy and host arithmetic need no row; every other call does"


# ------------------------------------------------------------------ 9. the wrapper's own checks
def test_python_argument_checks_come_before_any_launch(tf):
    import torch

    n, g = 16, pyref.to_raw(7)
    d_cw, d_ch = dev64(np.zeros(n * 3)), dev64(np.zeros(3))
    d_out = dev64(np.full(n // 2 * 3, CANARY64))
    both = dev64(np.zeros(n * 3 + n // 2 * 3))
    with pytest.raises(ValueError):  # out inside the codeword's words
        tf.fri.fold(both[:n * 3], n, g, d_ch, both[n * 3 - 3:n * 3 - 3 + n // 2 * 3])
    with pytest.raises(ValueError):  # out on the challenges
        tf.fri.fold(d_cw, 2, g, both[21:24], both[:24], batch=n // 2)
    with pytest.raises(TypeError):
        tf.fri.fold(d_cw.to(torch.int32), n, g, d_ch, d_out)
    with pytest.raises(TypeError):
        tf.fri.fold(d_cw, n, g, d_ch.cpu(), d_out)
    with pytest.raises(ValueError):  # a short out
        tf.fri.fold(d_cw, n, g, d_ch, d_out[:-3])
    with pytest.raises(ValueError):  # out sized for one level, two asked for
        tf.fri.fold(d_cw, n, g, dev64(np.zeros(6)), d_out, levels=2)
    with pytest.raises(ValueError):
        tf.fri.fold(d_cw, n, g, d_ch, d_out, width_c=3, width_a=1)
    torch.cuda.synchronize()
    assert (host64(d_out) == CANARY64).all()
