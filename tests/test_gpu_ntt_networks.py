"""The register networks of the NTT kernels (csrc/ntt_network.h: dit_half, dit_level, DitRange, class_fused, leftover_fused, tw_operand)
and the glue that hands lazy words to their first level (csrc/ntt_kernels.h: pre2_combine8, pre2_shift, c8_combine8), one composition
per call through the very functions the kernels call (tf_debug_ntt_network_dev), WORD FOR WORD against the integer model of
tests/network_ref.py -- on blocks built to put a word in [p, 2^64), a carry or a rippling correction on every butterfly of every level,
which uniform data does about once in 2^32 words.  A lazy output that is congruent to the model's but not the same word means that the
network took another path than its comments document: the Montgomery product behind it would forgive that, the v <= p contract of the
next level may not.

Then the one family of product kernels whose whole network is a direct function of the words it loads, the wave-private short
transforms (ntt_rows32w_kernel, n <= 64), on the same blocks: every steered block in every lane of a tile that is not its wave's first
(the prefetched one), against the plain Python-integer DFT and the oracle.

tests/test_network_cpu.py pins the model to the plain DFT and checks that the operand sets reach what they are built to reach.
"""
import numpy as np
import pytest

from tests import network_ref as nr

pytestmark = pytest.mark.gpu

GUARD = 64  # canary words behind the buffer
CANARY = 0xA5A5A5A5A5A5A5A5
THREADS = 256  # per workgroup of tf_debug_ntt_network_dev: one block of 32 (or 64) words per thread
P = nr.P


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(tf):
    assert tf.lib().tf_device_count() > 0, "no HIP device visible: the product has no CPU fallback"


@pytest.fixture(scope="module")
def config(tf):
    return tf.device.debug_ntt_network_config()


def _arrays(form, config):
    """(blocks [N, words], want [N, 32], indices of the constructed blocks) as uint64 arrays"""
    blocks, want = nr.expected(form, config)
    sets = nr.operand_sets(form, config)
    built = sum(len(v) for k, v in sets.items() if k not in ("edge", "uniform"))  # (the sets come in this order: built ones first)
    assert list(sets)[-2:] == ["edge", "uniform"]
    return np.array(blocks, dtype=np.uint64), np.array(want, dtype=np.uint64), built


def _run(tf, form, x):
    """one call on the blocks x [n, words] -> the words left in their place, after checking the canaries behind the buffer"""
    import torch

    n = x.size
    buf = np.concatenate([x.ravel(), np.full(GUARD, CANARY, dtype=np.uint64)]).view(np.int64)
    d = torch.from_numpy(buf).cuda()
    tf.device.debug_ntt_network_(form.name, d[:n])
    torch.cuda.synchronize()
    got = d.cpu().numpy().view(np.uint64)
    assert np.array_equal(got[n:], np.full(GUARD, CANARY, dtype=np.uint64)), f"{form}: words behind the buffer were written ({n} words)"
    return got[:n].reshape(x.shape)


def _compare(form, config, x, got, want):
    if form.words == 64:
        assert np.array_equal(got[:, 32:], x[:, 32:]), f"{form}: the partner words were written"
    bad = np.nonzero((got[:, :32] != want).any(axis=1))[0]
    if bad.size:
        t = int(bad[0])
        block, words = [int(w) for w in x[t]], [int(w) for w in got[t, :32]]
        lvl, i, slot, label, a, b, v = nr.locate(form, block, words, config)
        congruent = [w % P for w in words] == [int(w) % P for w in want[t]]
        raise AssertionError(
            f"{form}: {bad.size} of {len(x)} blocks differ; first in thread {t} (lane {t % 64}): level {lvl}, butterfly {i}, slot {slot} ({label}): "
            f"a = {a:#018x}, b = {b:#018x} (twiddled {v:#018x}), got {words[slot]:#018x}, want {int(want[t, slot]):#018x}; slots that differ: "
            f"{[q for q in range(32) if words[q] != int(want[t, q])]}; the block is {'' if congruent else 'NOT '}congruent to the model mod p; "
            f"block = {[hex(w) for w in block]}")


@pytest.mark.parametrize("name", list(nr.FORMS))
def test_form_word_for_word_on_steered_blocks(tf, config, name):
    """the whole operand set of the form in one call.  Wave w of the launch holds constructed block w (mod their number) in lane 0 and
    constructed block w + 1 in lane 63 (so every constructed block rides the first and the last lane of a wave); the lanes between walk through all the
    blocks of all the sets."""
    form = nr.FORMS[name]
    blocks, want, built = _arrays(form, config)
    waves = max(built, -(-len(blocks) // 62))
    idx = (np.arange(waves)[:, None] * 62 + np.arange(64)[None, :] - 1) % len(blocks)
    idx[:, 0] = np.arange(waves) % built
    idx[:, 63] = (np.arange(waves) + 1) % built
    idx = idx.ravel()
    assert set(idx.tolist()) == set(range(len(blocks)))
    x = blocks[idx]
    _compare(form, config, x, _run(tf, form, x), want[idx])


@pytest.mark.parametrize("name", list(nr.FORMS))
def test_ragged_block_counts(tf, config, name):
    """one block, and one block short of, exactly and one block past a workgroup's worth: nothing behind the count is touched"""
    form = nr.FORMS[name]
    blocks, want, _ = _arrays(form, config)
    for count in (1, THREADS - 1, THREADS, THREADS + 1):
        x = blocks[:count]
        _compare(form, config, x, _run(tf, form, x), want[:count])


# ------------------------------------------------------------------------------------------------------- the short-transform kernels
def _tiles_before_the_second(torch):
    """tiles the wave-private kernel's grid walks in its first round: 4 waves in each of at most 2 workgroups per compute unit"""
    return 8 * torch.cuda.get_device_properties(0).multi_processor_count


def _diagonal(n_blocks, lanes, first_round):
    """block index per (tile, lane): `first_round` tiles of filler, then tile first_round + t holds block t - l in lane l -- every block
    rides every lane, in a tile its wave has prefetched -- and five more lane rows that end the data inside a tile"""
    t = np.arange(first_round + n_blocks + lanes - 1)[:, None]
    ids = (t - np.arange(lanes)[None, :]) % n_blocks
    return np.concatenate([ids.ravel(), np.arange(5) % n_blocks])


def _device_ntt(tf, x, n, batch, width, inverse):
    """the whole batch in ONE launch (the host entry points may cut a batch into pipelined pieces)"""
    import torch

    d = torch.from_numpy(x.view(np.int64)).cuda()
    tf.device.ntt_(d, n, batch=batch, width=width, inverse=inverse)
    torch.cuda.synchronize()
    return d.cpu().numpy().view(np.uint64)


@pytest.mark.parametrize("width", [1, 3])
@pytest.mark.parametrize("n", [2, 4, 8, 16, 32])
def test_short_transforms_on_steered_blocks(tf, oracle, config, n, width):
    """ntt_rows32w_kernel<INV, L, LOGN>, both directions: every lane's 32 words are one steered block of LEVELS<INV, INV, log n>
    (slot q's word at element (q / n) n + brev(q % n) of the lane's row); expected words from the plain DFT and from the oracle"""
    import torch

    logn = n.bit_length() - 1
    lanes = 64 if width == 1 else 63
    for inverse in (False, True):
        form, blocks = nr.steered_rows(logn, inverse, config)
        rows = np.array([nr.rows32_row(b, logn) for b in blocks], dtype=np.uint64)
        outs = np.array([nr.short_transform_row(r, logn, inverse) for r in rows.tolist()], dtype=np.uint64)
        ids = _diagonal(len(blocks), lanes, _tiles_before_the_second(torch))
        if width == 3:  # lane 3 r + limb of a tile holds limb `limb` of element row r: five spare rows keep whole elements
            ids = np.concatenate([ids[:-5], np.arange(6) % len(blocks)])
            x = rows[ids].reshape(-1, 3, 32).transpose(0, 2, 1).ravel()
            want = outs[ids].reshape(-1, 3, 32).transpose(0, 2, 1).ravel()
        else:
            x, want = rows[ids].ravel(), outs[ids].ravel()
        assert x.size % (2048 if width == 1 else 2016) != 0
        batch = x.size // (n * width)
        got = _device_ntt(tf, x, n, batch, width, inverse)
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, (f"n = {n}, width {width}, inverse {inverse}: {bad.size} words differ from the plain DFT, first at word {int(bad[0])} "
                               f"(lane row {int(bad[0]) // 32 if width == 1 else '-'}): got {int(got[bad[0]]):#018x}, want {int(want[bad[0]]):#018x}")
        assert np.array_equal(oracle.ntt(x, width=width, inverse=inverse, batch=batch, threads=8), want), "the oracle disagrees with the plain DFT"


def test_n64_transforms_on_steered_blocks(tf, oracle, config):
    """n = 64 (BFieldElement): lanes 2 t and 2 t + 1 share transform t; its 64 words are solved backwards through rows64_dif_stage so
    that the even lane's network sees steered block k and the odd lane's block k + 1"""
    import torch

    for inverse in (False, True):
        form, blocks = nr.steered_rows(6, inverse, config)
        scale = pow(64, P - 2, P) if inverse else 1
        nb = len(blocks)
        ins = [nr.rows64_elements(blocks[k], blocks[(k + 1) % nb], inverse) for k in range(nb)]
        outs = np.array([[y * scale % P for y in nr.dft(u, inverse)] for u in ins], dtype=np.uint64)
        ids = _diagonal(nb, 32, _tiles_before_the_second(torch))
        x, want = np.array(ins, dtype=np.uint64)[ids].ravel(), outs[ids].ravel()
        assert x.size % 2048 != 0
        got = _device_ntt(tf, x, 64, x.size // 64, 1, inverse)
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, (f"n = 64, inverse {inverse}: {bad.size} words differ from the plain DFT, first at word {int(bad[0])}: "
                               f"got {int(got[bad[0]]):#018x}, want {int(want[bad[0]]):#018x}")
        assert np.array_equal(oracle.ntt(x, inverse=inverse, batch=x.size // 64, threads=8), want), "the oracle disagrees with the plain DFT"
