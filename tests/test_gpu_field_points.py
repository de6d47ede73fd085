"""get_colinear_y, are_colinear, mod_pow, powers and gather_elements on the GPU, host and _dev forms, compared word for word with
tests/points_ref (pinned to the reference's doc examples, pyref and the oracle by tests/test_field_points_cpu.py).

The sizes sit on the boundaries of the kernels (csrc/points_kernels.h): C, the triples one wave covers per step of get_colinear_y;
the grid-stride wraps; T, the group size at which are_colinear changes from one lane per group to one wave per group; the element
count at which a workgroup of the broadcast-base mod_pow reuses its table; the thread count of a powers launch.  Large outputs are
checked with a different kernel and at sampled positions.  Zero dx and out-of-range indices are handled values: the kernels replace
the one and never read through the other."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import field_ref, points_ref as ref, pyref

pytestmark = pytest.mark.gpu

P = ref.P
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = ref.PAIRS
CHUNK = {(1, 1): 64 * 8, (1, 3): 64 * 8, (3, 3): 64 * 4}  # 64 K, tfk::ColinearGeom<WX, WY>::CHUNK
T = 16                # tf_points.hip: kLaneGroup, the largest group that takes one lane
TABLE_ITEMS = 4       # tf_points.hip: kTableItems, elements per thread before a broadcast-base mod_pow launch adds workgroups
INVERSE_OF_ZERO, INVALID = 12, 17
EXPONENTS = [0, 1, 2, (1 << 32) - 1, 1 << 32, 1 << 63, (1 << 64) - 1, P - 1, P - 2]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(tf):
    assert tf.lib().tf_device_count() > 0, "no HIP device visible: the product has no CPU fallback"


def _to_dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def _to_host(t):
    return t.cpu().numpy().view(np.uint64)


def _p(a):
    return C.c_void_p(a.ctypes.data)


def _cus():
    import torch

    return torch.cuda.get_device_properties(0).multi_processor_count


def _status(v=0):
    import torch

    return torch.full((1,), v, dtype=torch.int32, device="cuda")


def _edges():
    return np.array([w for w in field_ref.edge_words() if w < P], dtype=np.uint64)


# ------------------------------------------------------------------ 1. get_colinear_y
def _colinear_sizes(pair):
    c = CHUNK[pair]
    return sorted({1, 2, 63, 64, 65, c - 1, c, c + 1, 4 * c - 1, 4 * c, 4 * c + 1})


def _colinear_inputs(oracle, n, wx, wy, seed, each):
    x0, x1 = oracle.fill_random(n * wx, seed), oracle.fill_random(n * wx, seed + 1)
    y0, y1 = oracle.fill_random(n * wy, seed + 2), oracle.fill_random(n * wy, seed + 3)
    p2x = oracle.fill_random((n if each else 1) * wy, seed + 4)
    return x0, y0, x1, y1, p2x


def _run_colinear_both(tf, ins, wx, wy, want):
    import torch

    x0, y0, x1, y1, p2x = ins
    assert np.array_equal(tf.get_colinear_y(x0, y0, x1, y1, p2x, width_x=wx, width_y=wy), want)
    out = torch.full((want.size,), -1, dtype=torch.int64, device="cuda")  # (not canonical: a word never stored shows)
    st = _status()
    tf.device.get_colinear_y(*[_to_dev(a) for a in ins], out, width_x=wx, width_y=wy, status=st)
    torch.cuda.synchronize()
    assert np.array_equal(_to_host(out), want) and int(st.item()) == 0


@pytest.mark.parametrize("wx,wy", PAIRS)
def test_get_colinear_y_sizes_word_for_word(tf, oracle, wx, wy):
    for n in _colinear_sizes((wx, wy)):
        for each in (False, True):
            ins = _colinear_inputs(oracle, n, wx, wy, 0x3A00 + 16 * n + each, each)
            want, bad = ref.get_colinear_y(*ins, wx, wy)
            assert not bad
            _run_colinear_both(tf, ins, wx, wy, want)


@pytest.mark.parametrize("wx,wy", PAIRS)
def test_get_colinear_y_edge_words_in_every_operand(tf, oracle, wx, wy):
    """block p of the call has operand p (x0, y0, x1, y1, p2x) built from 0, 1, p - 1 and the carry-edge words, limb k rotated by 17 k"""
    e = _edges()
    m = e.size
    n = 5 * m
    ins = [a.copy() for a in _colinear_inputs(oracle, n, wx, wy, 0x3B00 + wx + wy, True)]
    for p, w in enumerate((wx, wy, wx, wy, wy)):
        blk = ins[p].reshape(n, w)
        for k in range(w):
            blk[p * m:(p + 1) * m, k] = np.roll(e, 17 * k)
    want, bad = ref.get_colinear_y(*ins, wx, wy)
    assert not bad
    _run_colinear_both(tf, ins, wx, wy, want)


@pytest.mark.parametrize("wx,wy", PAIRS)
def test_get_colinear_y_zero_dx(tf, oracle, wx, wy):
    import torch

    lib = tf.lib()
    c = CHUNK[(wx, wy)]
    n = 4 * c + 1
    planted = [0, n - 1, 2 * c + 64 * 1 + 37]  # the first and the last triple, and lane 37 in the middle of the third wave's chunk
    for each in (False, True):
        ins = [a.copy() for a in _colinear_inputs(oracle, n, wx, wy, 0x3C00 + each, each)]
        for i in planted:
            ins[2][wx * i:wx * i + wx] = ins[0][wx * i:wx * i + wx]
        want, bad = ref.get_colinear_y(*ins, wx, wy)
        assert bad == sorted(planted)
        keep = np.ones(n, dtype=bool)
        keep[bad] = False
        keep = np.repeat(keep, wy)
        dev = [_to_dev(a) for a in ins]
        out = torch.zeros(n * wy, dtype=torch.int64, device="cuda")
        st = _status()
        tf.device.get_colinear_y(*dev, out, width_x=wx, width_y=wy, status=st)
        torch.cuda.synchronize()
        assert int(st.item()) == INVERSE_OF_ZERO
        assert np.array_equal(_to_host(out)[keep], want[keep])
        st.fill_(16)  # an earlier error of the chain stays
        tf.device.get_colinear_y(*dev, out, width_x=wx, width_y=wy, status=st)
        torch.cuda.synchronize()
        assert int(st.item()) == 16
        with pytest.raises(tf.NttPanic) as err:
            tf.device.get_colinear_y(*dev, out, width_x=wx, width_y=wy)
        assert err.value.code == INVERSE_OF_ZERO
        with pytest.raises(tf.NttPanic) as err:
            tf.get_colinear_y(*ins, width_x=wx, width_y=wy)
        assert err.value.code == INVERSE_OF_ZERO
        # the host form returns the code and still delivers the other triples
        o = np.zeros(n * wy, dtype=np.uint64)
        rc = lib.tf_get_colinear_y(_p(ins[0]), _p(ins[1]), _p(ins[2]), _p(ins[3]), n, _p(ins[4]), n if each else 1, wx, wy, _p(o))
        assert rc == INVERSE_OF_ZERO and np.array_equal(o[keep], want[keep])
    # a clean call leaves a zeroed status at 0 and a pre-set one untouched
    ins = _colinear_inputs(oracle, n, wx, wy, 0x3CFF, False)
    want, bad = ref.get_colinear_y(*ins, wx, wy)
    assert not bad
    dev = [_to_dev(a) for a in ins]
    for preset in (0, 16):
        st = _status(preset)
        out = torch.zeros(n * wy, dtype=torch.int64, device="cuda")
        tf.device.get_colinear_y(*dev, out, width_x=wx, width_y=wy, status=st)
        torch.cuda.synchronize()
        assert int(st.item()) == preset and np.array_equal(_to_host(out), want)


def test_get_colinear_y_large_checked_by_are_colinear(tf):
    """one chunk and three triples past the launch's grid-stride wrap (8 workgroups per compute unit, four waves each): the
    result checked by a different kernel -- (p0, p1, (p2x, out)) must be colinear, which also runs the lane-per-group form of
    are_colinear across its own wrap -- and at 64 sampled positions against the model"""
    import torch

    c = CHUNK[(1, 1)]
    wrap = _cus() * 8 * 4 * c
    n = wrap + c + 3
    assert n > _cus() * 8 * 256  # the wrap of are_colinear's lane-per-group launch
    bufs = [torch.empty(n, dtype=torch.int64, device="cuda") for _ in range(5)]
    for i, b in enumerate(bufs):
        tf.device.fill_random(b, 0x3D00 + i)
    x0, y0, x1, y1, p2x = bufs
    out = torch.full_like(x0, -1)  # (not canonical: a word never stored shows)
    st = _status()
    tf.device.get_colinear_y(x0, y0, x1, y1, p2x, out, status=st)
    xs = torch.stack((x0, x1, p2x), dim=1).reshape(-1).contiguous()
    ys = torch.stack((y0, y1, out), dim=1).reshape(-1).contiguous()
    flags = torch.zeros(n, dtype=torch.int32, device="cuda")
    tf.device.are_colinear(xs, ys, 3, flags)
    torch.cuda.synchronize()
    assert int(st.item()) == 0
    assert int(flags.sum().item()) == n
    idx = sorted(set(np.random.default_rng(7).integers(0, n, 58).tolist()) | {0, n - 1, wrap - 1, wrap, wrap + c, wrap + c + 2})
    sel = torch.tensor(idx, device="cuda")
    got = _to_host(out[sel])
    want, bad = ref.get_colinear_y(*[_to_host(b[sel]) for b in bufs], 1, 1)
    assert not bad and np.array_equal(got, want)
    # one point moved off its line is found, wherever it sits
    ys[3 * (wrap + 1) + 2] ^= 1
    tf.device.are_colinear(xs, ys, 3, flags)
    torch.cuda.synchronize()
    assert int(flags.sum().item()) == n - 1 and int(flags[wrap + 1].item()) == 0


# ------------------------------------------------------------------ 2. are_colinear
K_VALUES = [0, 1, 2, 3, 4, T, T + 1, 64, 65, 1024]


def _groups(rng, n_groups, k, wx, wy):
    """canonical values: per group a random line and k distinct x-coordinates on it, then one of seven variations by g % 7:
    0 on the line; 1 / 2 / 3 the first / a middle / the last further point off the line; 4 the last x equal to the first (its y
    too: still on the line); 5 two middle points with one x; 6 two middle x-coordinates that differ in one limb only (on the line)"""
    rnd = lambda w: int(rng.integers(1, 1 << 62)) % P if w == 1 else tuple(int(v) % P for v in rng.integers(1, 1 << 62, 3))  # noqa: E731
    xs, ys = [], []
    a_mid = k // 2
    b_mid = a_mid + 1 if a_mid + 1 < k else a_mid - 1
    for g in range(n_groups):
        slope, icpt = rnd(wy), rnd(wy)
        gx = []
        while len(gx) < k:
            x = rnd(wx)
            if x not in gx:
                gx.append(x)
        var = g % 7
        if k >= 2 and var == 4:
            gx[k - 1] = gx[0]
        if k >= 3 and var == 5:
            gx[b_mid] = gx[a_mid]
        if k >= 3 and var == 6 and wx == 3:
            gx[b_mid] = (gx[a_mid][0], gx[a_mid][1], (gx[a_mid][2] + 1) % P)
        gy = [ref.f_add(ref.f_mul(slope, ref.lift(x, wx, wy), wy), icpt, wy) for x in gx]
        if k >= 3 and var in (1, 2, 3):
            j = {1: 2, 2: max(2, k // 2), 3: k - 1}[var]
            gy[j] = ref.f_add(gy[j], ref.one(wy), wy)
        xs += gx
        ys += gy
    return ref.words(xs, wx), ref.words(ys, wy)


@pytest.mark.parametrize("wx,wy", PAIRS)
def test_are_colinear_shapes(tf, wx, wy):
    import torch

    rng = np.random.default_rng(0x4A00 + wx + wy)
    for k in K_VALUES:
        for n_groups in ((1, 3) if k == 1024 else (1, 63, 64, 65, 257)):
            xs, ys = _groups(rng, n_groups, k, wx, wy)
            want = ref.are_colinear(xs, ys, n_groups, k, wx, wy)
            if k >= 3:
                assert want[0] == 1 and (n_groups < 7 or set(want[:7].tolist()) == {0, 1}), (k, n_groups)
                if n_groups >= 7:  # the variations give what they were built for
                    assert want[:7].tolist() == [1, 0, 0, 0, 0, 0, 1], (k, n_groups)
            else:
                assert not want.any()
            if k:
                assert np.array_equal(tf.are_colinear(xs, ys, k, width_x=wx, width_y=wy), want.astype(bool)), (k, n_groups)
            flags = torch.full((n_groups,), 7, dtype=torch.int32, device="cuda")
            if k:
                tf.device.are_colinear(_to_dev(xs), _to_dev(ys), k, flags, width_x=wx, width_y=wy)
            else:
                empty = torch.empty(0, dtype=torch.int64, device="cuda")
                tf.device.are_colinear(empty, empty, 0, flags, width_x=wx, width_y=wy)
            torch.cuda.synchronize()
            assert np.array_equal(flags.cpu().numpy(), want), (k, n_groups)


# ------------------------------------------------------------------ 3. mod_pow
def _pow_pools(oracle, w, seed):
    """(raw words of the base pool as rows, exponent pool): 0, 1, p - 1, (0, a, 0), (0, 0, a) and random elements; the CPU list of
    exponents and random 32-bit ones"""
    r = oracle.fill_random(8 * w, seed).reshape(8, w)
    one, a = pyref.to_raw(1), int(r[0, 0])
    if w == 1:
        special = [[0], [one], [pyref.to_raw(P - 1)]]
    else:
        special = [[0, 0, 0], [one, 0, 0], [pyref.to_raw(P - 1), 0, 0], [0, a, 0], [0, 0, a]]
    bases = np.concatenate([np.array(special, dtype=np.uint64), r])
    exps = np.array(EXPONENTS + np.random.default_rng(seed).integers(0, 1 << 32, 8).tolist(), dtype=np.uint64)
    return bases, exps


@pytest.mark.parametrize("w", [1, 3])
def test_mod_pow_broadcasts_and_routes(tf, oracle, w):
    import torch

    pool_b, pool_e = _pow_pools(oracle, w, 0x5A00 + w)
    elems = ref.elements(pool_b.reshape(-1), w)
    memo = {}

    def want_for(bi, ei):
        out = []
        for b, e in zip(bi, ei):
            if (b, e) not in memo:
                memo[(b, e)] = ref.f_pow(elems[b], int(pool_e[e]), w)
            out.append(memo[(b, e)])
        return ref.words(out, w)

    rng = np.random.default_rng(0x5B00 + w)
    # (one workgroup serves 256 TABLE_ITEMS elements of the broadcast-base route: past it a launch has several workgroups, and every
    # thread of them takes its table a second time)
    for n in (1, 63, 64, 65, 255, 256, 257, 256 * TABLE_ITEMS + 1, 3 * 256 * TABLE_ITEMS + 5):
        bi_n, ei_n = rng.integers(0, len(pool_b), n), rng.integers(0, len(pool_e), n)
        bi_n[:len(pool_b)] = np.arange(len(pool_b))[:n]  # every special base ...
        ei_n[:len(pool_e)] = np.arange(len(pool_e))[:n]  # ... and every listed exponent, mixed within one wave
        for nb, ne in ((n, n), (1, n), (n, 1), (1, 1)):
            bi = bi_n if nb == n else np.full(n, bi_n[n // 2])
            ei = ei_n if ne == n else np.full(n, ei_n[n // 3])
            want = want_for(bi.tolist(), ei.tolist())
            bases = np.ascontiguousarray(pool_b[bi[:nb]].reshape(-1))
            exps = np.ascontiguousarray(pool_e[ei[:ne]])
            assert np.array_equal(tf.mod_pow(bases, exps, width=w), want if max(nb, ne) == n else want[:w]), (n, nb, ne)
            out = torch.zeros(n * w, dtype=torch.int64, device="cuda")
            tf.device.mod_pow(_to_dev(bases), _to_dev(exps), out, width=w)
            if nb == 1:  # the same inputs through the general route: the base written out n times
                out2 = torch.zeros_like(out)
                tf.device.mod_pow(_to_dev(np.tile(bases, n)), _to_dev(exps), out2, width=w)
                assert torch.equal(out, out2), (n, nb, ne)
            torch.cuda.synchronize()
            assert np.array_equal(_to_host(out), want), (n, nb, ne)


def test_mod_pow_past_the_grid_stride_wrap(tf, oracle):
    """base field, g^index as a FRI round forms it: a size past the wrap of the broadcast-base launch; the two routes against each
    other, and 64 sampled positions against the model"""
    import torch

    n = _cus() * 8 * 256 * TABLE_ITEMS + 261
    g = pyref.root_of_unity(1 << 32)
    base = _to_dev(np.array([pyref.to_raw(g)], dtype=np.uint64))
    exps = torch.empty(n, dtype=torch.int64, device="cuda")
    tf.device.fill_random(exps, 0x5C00)
    exps &= 0xFFFFFFFF
    out, out2 = torch.full_like(exps, -1), torch.full_like(exps, -1)  # (not canonical: a word never stored shows)
    tf.device.mod_pow(base, exps, out)
    tf.device.mod_pow(base.repeat(n), exps, out2)
    torch.cuda.synchronize()
    assert torch.equal(out, out2)
    idx = sorted(set(np.random.default_rng(9).integers(0, n, 62).tolist()) | {0, n - 1})
    sel = torch.tensor(idx, device="cuda")
    e = _to_host(exps[sel])
    assert _to_host(out[sel]).tolist() == [pyref.to_raw(pow(g, int(x), P)) for x in e]


# ------------------------------------------------------------------ 4. powers
def _powers_threads_max():
    """the largest launch of powers_kernel: the largest power of two of threads within 8 workgroups per compute unit"""
    cap = _cus() * 8 * 256
    return 1 << (cap.bit_length() - 1)


@pytest.mark.parametrize("w", [1, 3])
def test_powers(tf, oracle, w):
    import torch

    rnd = oracle.fill_random(2 * w, 0x6A00 + w)
    lift = lambda v: [pyref.to_raw(v)] + [0] * (w - 1)  # noqa: E731
    ratios = {"zero": lift(0), "one": lift(1), "minus one": lift(P - 1), "root of order 2^10": lift(pyref.root_of_unity(1 << 10)),
              "random": rnd[:w].tolist()}
    firsts = {"zero": lift(0), "random": rnd[w:].tolist()}
    for n in (1, 2, 64, 65, (1 << 16) + 7):
        for rname, ratio in ratios.items():
            for fname, first in firsts.items():
                f, r = np.array(first, dtype=np.uint64), np.array(ratio, dtype=np.uint64)
                if n > 65 and (fname == "zero" or rname in ("zero", "one")):
                    want = np.tile(f, n) if rname == "one" else np.concatenate([f, np.zeros((n - 1) * w, dtype=np.uint64)])
                else:
                    want = ref.powers(f, r, w, n)
                assert np.array_equal(tf.powers(f, r, n, width=w), want), (n, rname, fname)
                out = torch.zeros(n * w, dtype=torch.int64, device="cuda")
                tf.device.powers(f, r, out, width=w)
                torch.cuda.synchronize()
                assert np.array_equal(_to_host(out), want), (n, rname, fname)
    # the root of unity's sequence wraps: element 2^10 is `first` again
    f, r = np.array(firsts["random"], dtype=np.uint64), np.array(ratios["root of order 2^10"], dtype=np.uint64)
    seq = tf.powers(f, r, 1025, width=w)
    assert np.array_equal(seq[1024 * w:], f) and not np.array_equal(seq[512 * w:513 * w], f)


@pytest.mark.parametrize("w", [1, 3])
def test_powers_around_one_launch_thread_count(tf, oracle, w):
    """n = the largest launch's thread count - 1 and + 1 (the first thread then takes a second element) and two elements per thread
    and five: every element against its neighbour with a different kernel (out[i + 1] = out[i] * ratio, tf_poly_scalar_mul_dev),
    element 0 = first, and sampled positions against first * ratio^i of the model"""
    import torch

    s_max = _powers_threads_max()
    rnd = oracle.fill_random(2 * w, 0x6B00 + w)
    f, r = rnd[:w], rnd[w:]
    fe, re_ = ref.elements(f, w)[0], ref.elements(r, w)[0]
    for n in (s_max - 1, s_max + 1, 2 * s_max + 5):
        out = torch.full((n * w,), -1, dtype=torch.int64, device="cuda")  # (not canonical: a word never stored shows)
        tf.device.powers(f, r, out, width=w)
        nxt = torch.full(((n - 1) * w,), -1, dtype=torch.int64, device="cuda")
        tf.device.poly_scalar_mul(out[:(n - 1) * w], n - 1, r, nxt, width=w, width_s=w)
        torch.cuda.synchronize()
        assert torch.equal(nxt, out[w:]), n
        assert np.array_equal(_to_host(out[:w]), f), n
        idx = sorted(set(np.random.default_rng(n).integers(0, n, 28).tolist()) | {i for i in (n - 1, n - 2, s_max - 1, s_max) if i < n})
        for i in idx:
            want = ref.words([ref.f_mul(fe, ref.f_pow(re_, i, w), w)], w)
            assert np.array_equal(_to_host(out[i * w:(i + 1) * w]), want), (n, i)


# ------------------------------------------------------------------ 5. gather
@pytest.mark.parametrize("width", [1, 3, 5, 16])
def test_gather_elements(tf, oracle, width):
    import torch

    src_len, n = 301, 1000
    src = oracle.fill_random(src_len * width, 0x7A00 + width)
    idx = np.random.default_rng(width).integers(0, src_len, n).astype(np.uint32)
    idx[:6] = [0, src_len - 1, 5, 5, 5, 0]  # the two ends, repeated indices
    want, bad = ref.gather(src, width, idx)
    assert not bad
    d_src, d_idx = _to_dev(src), torch.from_numpy(idx.view(np.int32)).cuda()
    out = torch.zeros(n * width, dtype=torch.int64, device="cuda")
    st = _status()
    tf.device.gather_elements(d_src, d_idx, out, width=width, status=st)
    out2 = torch.zeros_like(out)
    tf.device.gather_elements(d_src, d_idx, out2, width=width)  # the wrapper's own status word
    torch.cuda.synchronize()
    assert np.array_equal(_to_host(out), want) and torch.equal(out, out2) and int(st.item()) == 0
    # the second half of a fold is a pointer offset on src
    half = src_len // 2
    low = torch.from_numpy((idx % half).astype(np.uint32).view(np.int32)).cuda()
    tf.device.gather_elements(d_src[half * width:], low, out, width=width, status=st)
    torch.cuda.synchronize()
    assert np.array_equal(_to_host(out), ref.gather(src[half * width:], width, idx % half)[0]) and int(st.item()) == 0
    # out-of-range indices (src_len itself, the largest u32) set the status and are never read; the other outputs are right
    idx2 = idx.copy()
    idx2[[3, 500, n - 1]] = [src_len, 0xFFFFFFFF, src_len + 7]
    want2, bad2 = ref.gather(src, width, idx2)
    assert bad2 == [3, 500, n - 1]
    d_idx2 = torch.from_numpy(idx2.view(np.int32)).cuda()
    out.fill_(-1)
    tf.device.gather_elements(d_src, d_idx2, out, width=width, status=st)
    torch.cuda.synchronize()
    assert int(st.item()) == INVALID
    got = _to_host(out).reshape(n, width)
    keep = np.ones(n, dtype=bool)
    keep[bad2] = False
    assert np.array_equal(got[keep], want2.reshape(n, width)[keep])
    assert (got[~keep] == np.uint64((1 << 64) - 1)).all()  # the slots of the bad indices are as they were
    with pytest.raises(tf.TwentyFirstError) as err:
        tf.device.gather_elements(d_src, d_idx2, out, width=width)
    assert err.value.code == INVALID
    st.fill_(12)  # an earlier error of the chain stays
    tf.device.gather_elements(d_src, d_idx2, out, width=width, status=st)
    torch.cuda.synchronize()
    assert int(st.item()) == 12


# ------------------------------------------------------------------ 6. a FRI query round without a host round trip
def test_fri_query_round_stays_on_the_device(tf, oracle):
    """f of degree < 2^9 over XFieldElements on the coset offset * <g> of order 2^10.  One sponge samples 80 indices below 2^9 and
    the folding challenge alpha; two gathers fetch f(x) and f(-x) (g^(2^9) = -1: the second half of the codeword), mod_pow and
    scalar_mul form x = offset * g^index, neg forms -x, and get_colinear_y (1, 3) evaluates the line through (x, f(x)), (-x, f(-x))
    at alpha.  That is the folded polynomial f_even + alpha f_odd at x^2, computed on the host with pyref."""
    import torch

    order, half, queries = 1 << 10, 1 << 9, 80
    coeffs = oracle.fill_random(3 * half, 0x8A00)
    offset = tf.BFieldElement.new(7)
    g_raw = tf.BFieldElement.primitive_root_of_unity(order)
    codeword = tf.fast_coset_evaluate(coeffs, offset, order, width=3)
    # ---- the one upload
    cw = _to_dev(codeword)
    g = _to_dev(np.array([g_raw], dtype=np.uint64))
    # ---- on the device
    st = _status()
    sponge = torch.zeros(16, dtype=torch.int64, device="cuda")
    tf.device.tip5_sponge_init_(sponge)
    tf.device.tip5_sponge_pad_and_absorb_all_(sponge, cw[:30])
    idx = torch.zeros(queries, dtype=torch.int32, device="cuda")
    tf.device.tip5_sponge_sample_indices(sponge, half, idx)
    alpha = torch.zeros(3, dtype=torch.int64, device="cuda")
    tf.device.tip5_sponge_sample_scalars(sponge, alpha)
    y0, y1 = torch.zeros(3 * queries, dtype=torch.int64, device="cuda"), torch.zeros(3 * queries, dtype=torch.int64, device="cuda")
    tf.device.gather_elements(cw, idx, y0, width=3, status=st)
    tf.device.gather_elements(cw[3 * half:], idx, y1, width=3, status=st)
    x0, x1 = torch.zeros(queries, dtype=torch.int64, device="cuda"), torch.zeros(queries, dtype=torch.int64, device="cuda")
    tf.device.mod_pow(g, idx.to(torch.int64), x0)
    tf.device.poly_scalar_mul(x0, queries, offset, x0)
    tf.device.poly_neg_(x0, queries, out=x1)
    folded = torch.zeros(3 * queries, dtype=torch.int64, device="cuda")
    tf.device.get_colinear_y(x0, y0, x1, y1, alpha, folded, width_x=1, width_y=3, status=st)
    # ---- the one download
    torch.cuda.synchronize()
    assert int(st.item()) == 0
    got, h_idx, h_alpha = _to_host(folded), idx.cpu().numpy(), _to_host(alpha)
    assert len(set(h_idx.tolist())) > 1 and (h_idx >= 0).all() and (h_idx < half).all()
    F = pyref.Field(3)
    c = ref.elements(coeffs, 3)
    a = ref.elements(h_alpha, 3)[0]
    folded_poly = [F.add(c[2 * j], F.mul(a, c[2 * j + 1])) for j in range(half // 2)]
    w_val, off_val = pyref.to_val(g_raw), pyref.to_val(offset)
    want = []
    for i in h_idx.tolist():
        x = off_val * pow(w_val, i, P) % P
        want.append(pyref.poly_eval(F, folded_poly, pyref.xfe(x * x % P)))
    assert np.array_equal(got, ref.words(want, 3))


# ------------------------------------------------------------------ 7. the C++ mirror
def test_cpp_mirror_points_selftest_runs():
    host = os.path.join(ROOT, "twenty-first_amd", "host")
    subprocess.check_call(["make", "-C", host, "points_selftest"], stdout=subprocess.DEVNULL)
    r = subprocess.run(["timeout", "-k", "10", "120", os.path.join(host, "points_selftest")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.count("PASS") >= 6, r.stdout
