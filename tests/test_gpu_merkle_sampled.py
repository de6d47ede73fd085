"""Merkle openings at leaf indices held in device memory (twenty_first_amd/merkle_sampled.py over tf_merkle_auth_structure_indices_dev,
tf_merkle_authentication_structure_sampled_dev, tf_merkle_auth_structure_from_leafs_sampled_dev) against the CPU oracle.

Expected node indices: oracle.auth_structure_indices (pinned by tests/test_oracle_kat.py::test_merkle_structure); expected run ends:
its per-level histogram; expected digests: oracle.merkle_build(leafs).reshape(2n, 5)[ids], row 1 the root, as
tests/test_gpu_merkle_open.py builds them.  Every comparison is np.array_equal on WHOLE buffers that start as canary words, so a store
beyond `count` entries or into another tree's slot shows.

The constants of the planner kernel (csrc/merkle_plan_kernels.h, launch_plan of tf_merkle_open.hip) behind the list lengths K:
    one wave            k <= 64: 64 threads, no workgroup barrier                          63, 64, 65
    256 threads         k <= 1024; a round of the scans is 256 items                       255, 256, 257, 1023, 1024, 1025
    1024 threads        k <= 8192; a round is 1024 items                                   2047 ... 8191, 8192
    bitonic padding     the list is padded to the next power of two with 0xFFFFFFFF        2^j - 1, 2^j, 2^j + 1 for j = 0 ... 13
    the limit           8192 indices per list (8193 is refused on the host: tests/test_merkle_sampled_cpu.py)
At height 31 the lists hold the leafs 0 and 2^31 - 1: node indices reach 2^32 - 1, the value of the padding word.
The sweep's heights and batches are those of tests/test_gpu_merkle_open.py (where it changes shape), its index lists cut to 8192."""
import numpy as np
import pytest

from tests import fence
from tests import sponge_ref
from tests.test_gpu_merkle_open import index_sets  # the host-index sweep's own lists: the sampled sweep opens at the same ones

pytestmark = pytest.mark.gpu

LEAF_INDEX_INVALID, BUFFER_TOO_SMALL = 11, 13
CANARY32 = np.uint32(0xCA11AB1E)
CANARY64 = np.uint64(0xC0FFEE0000C0FFEE)
MAX_K = 8192
K = sorted({k for j in range(14) for k in ((1 << j) - 1, 1 << j, (1 << j) + 1) if k <= MAX_K})
PLAN_HEIGHTS = [0, 1, 2, 6, 14, 31]
NODE_HEIGHTS = [0, 1, 2, 6, 10]
NODE_BATCHES = [(1, 1), (1, 3), (5, 2)]
LEAF_HEIGHTS = [0, 1, 2, 6, 7, 10, 14, 15, 16, 17]
LEAF_BATCHES = [(1 << 13, 2, 2), (1 << 14, 2, 2), (1 << 6, 3, 1), (1 << 10, 1, 5)]
ROWS = {}  # the fence rows: callable of merkle_sampled.py -> (cases, generator of (shape, operands, call)), as tests/test_gpu_table.py


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(tf):
    assert tf.lib().tf_device_count() > 0, "no HIP device visible: the product has no CPU fallback"


# ------------------------------------------------------------------ plumbing
def dev32(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).reshape(-1).view(np.int32).copy()).cuda()


def dev64(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).reshape(-1).view(np.int64).copy()).cuda()


def host32(t):
    return t.cpu().numpy().view(np.uint32)


def host64(t):
    return t.cpu().numpy().view(np.uint64)


def new_status(v=0):
    import torch

    return torch.full((1,), v, dtype=torch.int32, device="cuda")


_trees = {}


def trees(oracle, n, batch=1):
    """(leafs (batch, n, 5), nodes (batch, 2n, 5)) of `batch` trees with distinct leafs, built once by the oracle and never written."""
    if (n, batch) not in _trees:
        leafs = oracle.fill_random(batch * n * 5, 0x5A3D + 31 * n + batch).reshape(batch, n, 5)
        nodes = np.stack([oracle.merkle_build(leafs[t], threads=8 if n >= 1 << 13 else 0).reshape(2 * n, 5) for t in range(batch)])
        leafs.setflags(write=False)
        nodes.setflags(write=False)
        _trees[(n, batch)] = (leafs, nodes)
    return _trees[(n, batch)]


def node_ids(oracle, n, idx):
    return oracle.auth_structure_indices(n, np.asarray(idx, dtype=np.uint64)).astype(np.uint64)


def level_ends(n, ids):
    """entry j: the structure nodes on the levels of n, n / 2, ..., n >> j nodes -- the histogram of the oracle's list"""
    return np.array([int((ids >= np.uint64(n >> j)).sum()) for j in range(32)], dtype=np.uint32)


def special_lists(n):
    """the issue's lists, each cut to MAX_K indices"""
    rng = np.random.default_rng(n % 1000003 + 17)
    lists = [[], [n // 3], [n - 1] * 5, [2 % n, 3 % n], [0, n - 1], [3 % n, 3 % n, 5 % n, 0, 3 % n, (n - 1) // 2],
             list(range(0, min(n, 2 * MAX_K), 2)), list(range(min(n, MAX_K))), rng.integers(0, n, size=17).tolist(),
             [0, n - 1] + rng.integers(0, n, size=15).tolist()]
    return [np.array(s, dtype=np.uint64) for s in lists]


def random_list(n, k, seed):
    idx = np.random.default_rng(seed).integers(0, n, size=k).astype(np.uint64)
    if k >= 2:
        idx[k // 2], idx[0] = 0, n - 1  # the first and the last leaf: the smallest and the largest node index of the leaf level
    return idx


def list_group(n, n_lists, k, seed):
    """n_lists lists of k indices each, of different kinds: random, all equal, bunched, random again, ..."""
    rng = np.random.default_rng(seed)
    out = np.zeros((n_lists, k), dtype=np.uint64)
    for l in range(n_lists):
        kind = l % 4
        if kind == 1:
            out[l] = rng.integers(0, n)
        elif kind == 2:
            out[l] = (np.arange(k) + rng.integers(0, n)) % n
        else:
            out[l] = rng.integers(0, n, size=k)
    return out


# ------------------------------------------------------------------ 1. the planner alone
def run_plan(tf, n, lists, capacity, with_ends=True, status=None):
    """lists: (n_lists, k) -> (node indices (n_lists, capacity), counts, run ends (n_lists, 32) or None, status) after ONE synchronisation"""
    import torch

    lists = np.asarray(lists, dtype=np.uint64)
    n_lists = lists.shape[0]
    d_nodes = dev32(np.full(n_lists * capacity, CANARY32))
    d_counts = dev32(np.full(n_lists, CANARY32))
    d_ends = dev32(np.full(n_lists * 32, CANARY32)) if with_ends else None
    st = new_status() if status is None else status
    tf.merkle_sampled.structure_indices(n, dev32(lists), d_nodes, d_counts, n_lists=n_lists, level_ends=d_ends, status=st)
    torch.cuda.synchronize()
    return (host32(d_nodes).reshape(n_lists, capacity), host32(d_counts), host32(d_ends).reshape(n_lists, 32) if with_ends else None,
            int(st.item()))


def check_plan(tf, oracle, n, lists, slack=3):
    lists = np.asarray(lists, dtype=np.uint64)
    n_lists, k = lists.shape
    want = [node_ids(oracle, n, l) for l in lists]
    capacity = tf.merkle_sampled.max_nodes(n, k) + slack
    assert max(len(w) for w in want) <= capacity - slack, "the bound"
    nodes, counts, ends, status = run_plan(tf, n, lists, capacity)
    want_nodes = np.full((n_lists, capacity), CANARY32)
    for l, w in enumerate(want):
        want_nodes[l, :len(w)] = w.astype(np.uint32)
    assert status == 0
    assert np.array_equal(counts, np.array([len(w) for w in want], dtype=np.uint32)), (n, k)
    assert np.array_equal(nodes, want_nodes), (n, k)
    assert np.array_equal(ends, np.stack([level_ends(n, w) for w in want])), (n, k)


@pytest.mark.parametrize("height", PLAN_HEIGHTS)
def test_plan_special_lists(tf, oracle, height):
    n = 1 << height
    for idx in special_lists(n):
        check_plan(tf, oracle, n, idx[None, :])
    every = special_lists(n)[7]
    if n <= MAX_K:
        assert every.size == n and node_ids(oracle, n, every).size == 0, "every leaf opened: nothing left to send"


@pytest.mark.parametrize("k", K)
def test_plan_random_lists_at_every_boundary_of_the_kernel(tf, oracle, k):
    for height in (6, 14, 31):  # 6: far more indices than leafs; 14: many repeats at the long lists; 31: nearly all distinct
        check_plan(tf, oracle, 1 << height, random_list(1 << height, k, 1000 * height + k)[None, :])


def test_plan_last_node_equals_the_padding_word(tf, oracle):
    """n = 2^31 and the leaf 2^31 - 1: the node 2^32 - 1 is the word the bitonic network pads with; k one below a power of two, so
    exactly one padding word joins it."""
    n = 1 << 31
    for k in (1, 3, 63, 255, 8191):
        idx = random_list(n, k, k)
        idx[-1] = n - 1
        ids = node_ids(oracle, n, idx)
        assert int(ids[0]) == (1 << 32) - 2, "the sibling of the last node comes first"
        check_plan(tf, oracle, n, idx[None, :])


def test_plan_257_lists_in_one_call(tf, oracle):
    n, k, n_lists = 1 << 14, 80, 257
    lists = list_group(n, n_lists, k, 257)
    assert len({l.tobytes() for l in lists}) == n_lists
    check_plan(tf, oracle, n, lists)
    # without run ends, and a longer list on the 1024-thread kernel
    want = [node_ids(oracle, n, l) for l in lists]
    cap = tf.merkle_sampled.max_nodes(n, k)
    nodes, counts, ends, status = run_plan(tf, n, lists, cap, with_ends=False)
    assert status == 0 and ends is None and counts.tolist() == [len(w) for w in want]
    assert all(np.array_equal(nodes[l, :len(w)], w.astype(np.uint32)) and (nodes[l, len(w):] == CANARY32).all() for l, w in enumerate(want))
    check_plan(tf, oracle, n, list_group(n, 5, 1500, 5))


def test_plan_errors_one_kind_per_call(tf, oracle):
    n, k = 1 << 10, 40
    lists = list_group(n, 3, k, 99)
    lists[0] = np.random.default_rng(1).integers(0, n, size=k)
    want = [node_ids(oracle, n, l) for l in lists]
    capacity = tf.merkle_sampled.max_nodes(n, k)
    # an index == num_leafs in list 1
    bad = lists.copy()
    bad[1, 7] = n
    nodes, counts, ends, status = run_plan(tf, n, bad, capacity)
    assert status == LEAF_INDEX_INVALID and counts.tolist() == [len(want[0]), 0, len(want[2])]
    assert (nodes[1] == CANARY32).all() and not ends[1].any()
    for l in (0, 2):
        assert np.array_equal(nodes[l, :len(want[l])], want[l].astype(np.uint32)) and (nodes[l, len(want[l]):] == CANARY32).all()
        assert np.array_equal(ends[l], level_ends(n, want[l]))
    # one node short for list 0, which has the most
    assert len(want[0]) > max(len(want[1]), len(want[2]))
    short = len(want[0]) - 1
    nodes, counts, ends, status = run_plan(tf, n, lists, short)
    assert status == BUFFER_TOO_SMALL and counts.tolist() == [len(w) for w in want], "the full count is reported"
    assert np.array_equal(nodes[0], want[0][:short].astype(np.uint32)), "the plan alone keeps the first `capacity` node indices"
    for l in (1, 2):
        assert np.array_equal(nodes[l, :len(want[l])], want[l].astype(np.uint32)) and (nodes[l, len(want[l]):] == CANARY32).all()
    # the first non-zero code stays, and without a status word the wrapper raises after one synchronisation
    _, _, _, status = run_plan(tf, n, bad, capacity, status=new_status(12))
    assert status == 12
    with pytest.raises(tf.MerkleTreeError) as e:
        tf.merkle_sampled.structure_indices(n, dev32(bad), dev32(np.zeros(3 * capacity)), dev32(np.zeros(3)), n_lists=3)
    assert e.value.code == LEAF_INDEX_INVALID


# ------------------------------------------------------------------ 2. digests: from node arrays and from the leafs
def expected_digests(oracle, nodes, n, lists, tpl, capacity, skip=()):
    """(trees, capacity, 5) canary words with the structure of every tree in front (lists in `skip` write nothing), counts per list"""
    n_lists = len(lists)
    want = np.full((n_lists * tpl, capacity, 5), CANARY64)
    counts = []
    for l, idx in enumerate(lists):
        ids = node_ids(oracle, n, idx).astype(np.int64)
        counts.append(len(ids))
        for t in range(l * tpl, (l + 1) * tpl):
            if l not in skip:
                want[t, :len(ids)] = nodes[t][ids]
    return want, np.array(counts, dtype=np.uint32)


def open_sampled(tf, which, d_trees, n, lists, tpl, capacity, with_roots=False, status=None):
    """-> (digests (trees, capacity, 5), counts, roots (trees, 5) or None, status), read back after ONE synchronisation"""
    import torch

    lists = np.asarray(lists, dtype=np.uint64)
    n_lists, n_trees = lists.shape[0], lists.shape[0] * tpl
    d_out = dev64(np.full(n_trees * capacity * 5, CANARY64))
    d_counts = dev32(np.full(n_lists, CANARY32))
    d_roots = dev64(np.full(n_trees * 5, CANARY64)) if with_roots else None
    st = new_status() if status is None else status
    kw = dict(n_lists=n_lists, trees_per_list=tpl, status=st)
    if which == "leafs":
        tf.merkle_sampled.structure_from_leafs(d_trees, n, dev32(lists), d_out, d_counts, roots=d_roots, **kw)
    else:
        tf.merkle_sampled.structure_from_nodes(d_trees, n, dev32(lists), d_out, d_counts, **kw)
    torch.cuda.synchronize()
    return (host64(d_out).reshape(n_trees, capacity, 5), host32(d_counts), host64(d_roots).reshape(n_trees, 5) if with_roots else None,
            int(st.item()))


def check_open(tf, oracle, which, d_trees, nodes, n, lists, tpl, with_roots=True, slack=2):
    lists = np.asarray(lists, dtype=np.uint64)
    capacity = tf.merkle_sampled.max_nodes(n, lists.shape[1]) + slack
    want, want_counts = expected_digests(oracle, nodes, n, lists, tpl, capacity)
    got, counts, roots, status = open_sampled(tf, which, d_trees, n, lists, tpl, capacity, with_roots=with_roots and which == "leafs")
    assert status == 0 and np.array_equal(counts, want_counts), (which, n, lists.shape, tpl)
    assert np.array_equal(got, want), (which, n, lists.shape, tpl)
    if roots is not None:
        assert np.array_equal(roots, nodes[:, 1]), (which, n, lists.shape, tpl)


def groups(n, n_lists):
    """lists for n_lists lists at once: each special list and each list of tests/test_gpu_merkle_open.py (cut to MAX_K) beside shifted
    copies of itself, then random groups"""
    for idx in special_lists(n) + [s[:MAX_K] for s in index_sets(n)]:
        yield np.stack([(idx + np.uint64(l * 5)) % np.uint64(n) for l in range(n_lists)]) if idx.size else np.zeros((n_lists, 0), dtype=np.uint64)
    yield list_group(n, n_lists, 17, n + n_lists)
    yield list_group(n, n_lists, 80, n + n_lists + 1)


@pytest.mark.parametrize("n_lists,tpl", NODE_BATCHES)
@pytest.mark.parametrize("height", NODE_HEIGHTS)
def test_from_node_arrays(tf, oracle, height, n_lists, tpl):
    n = 1 << height
    _, nodes = trees(oracle, n, n_lists * tpl)
    d_nodes = dev64(nodes)
    for lists in groups(n, n_lists):
        check_open(tf, oracle, "nodes", d_nodes, nodes, n, lists, tpl)
    assert np.array_equal(host64(d_nodes), nodes.reshape(-1)), "the node arrays are read only"


@pytest.mark.parametrize("height", LEAF_HEIGHTS)
def test_from_leafs_one_tree(tf, oracle, height):
    n = 1 << height
    leafs, nodes = trees(oracle, n)
    d_leafs = dev64(leafs)
    for i, lists in enumerate(groups(n, 1)):
        check_open(tf, oracle, "leafs", d_leafs, nodes, n, lists, 1, with_roots=i % 3 != 2)  # (every third list with d_roots = NULL)
    assert np.array_equal(host64(d_leafs), leafs.reshape(-1)), "the leafs are read only"


@pytest.mark.parametrize("n,n_lists,tpl", LEAF_BATCHES)
def test_from_leafs_batches(tf, oracle, n, n_lists, tpl):
    leafs, nodes = trees(oracle, n, n_lists * tpl)
    assert not np.array_equal(nodes[0, 1], nodes[1, 1])
    d_leafs = dev64(leafs)
    for i, lists in enumerate(groups(n, n_lists)):
        check_open(tf, oracle, "leafs", d_leafs, nodes, n, lists, tpl, with_roots=i % 3 != 2)
    assert np.array_equal(host64(d_leafs), leafs.reshape(-1))


def test_from_leafs_roots_only_and_a_long_list(tf, oracle):
    n = 1 << 15
    leafs, nodes = trees(oracle, n)
    d_leafs = dev64(leafs)
    # k == 0 with roots: the sweep runs for the roots alone; capacity 0 is then enough
    got, counts, roots, status = open_sampled(tf, "leafs", d_leafs, n, np.zeros((1, 0)), 1, 0, with_roots=True)
    assert status == 0 and counts.tolist() == [0] and got.size == 0 and np.array_equal(roots, nodes[:, 1])
    # 8192 indices: the 1024-thread planner drives the sweep
    check_open(tf, oracle, "leafs", d_leafs, nodes, n, random_list(n, MAX_K, 8)[None, :], 1)
    check_open(tf, oracle, "nodes", dev64(nodes), nodes, n, random_list(n, MAX_K, 9)[None, :], 1)


@pytest.mark.parametrize("which", ["nodes", "leafs"])
def test_errors_leave_the_slots_of_their_trees_and_spare_the_other_lists(tf, oracle, which):
    n, k, tpl = 1 << 10, 40, 2
    leafs, nodes = trees(oracle, n, 3 * tpl)
    d_trees = dev64(leafs if which == "leafs" else nodes)
    lists = list_group(n, 3, k, 98)
    lists[0], lists[1] = lists[0, 0], np.random.default_rng(2).integers(0, n, size=k)  # (one leaf k times; list 1 has the most nodes)
    capacity = tf.merkle_sampled.max_nodes(n, k)
    # one index == num_leafs in list 2: status 11, count 0, its trees' slots still canary, the other two lists exact
    bad = lists.copy()
    bad[2, k - 1] = n
    want, want_counts = expected_digests(oracle, nodes, n, lists, tpl, capacity, skip=(2,))
    want_counts[2] = 0
    got, counts, roots, status = open_sampled(tf, which, d_trees, n, bad, tpl, capacity, with_roots=which == "leafs")
    assert status == LEAF_INDEX_INVALID and np.array_equal(counts, want_counts)
    assert np.array_equal(got, want) and (got[2 * tpl:] == CANARY64).all()
    if roots is not None:
        assert np.array_equal(roots, nodes[:, 1]), "the roots are written whatever the status"
    # capacity = count - 1 for list 1 (it has the most): status 13, the full count reported, its slots canary, the others exact
    _, full = expected_digests(oracle, nodes, n, lists, tpl, capacity)
    assert full[1] > max(full[0], full[2])
    short = int(full[1]) - 1
    want, _ = expected_digests(oracle, nodes, n, lists, tpl, short, skip=(1,))
    got, counts, roots, status = open_sampled(tf, which, d_trees, n, lists, tpl, short, with_roots=which == "leafs")
    assert status == BUFFER_TOO_SMALL and np.array_equal(counts, full)
    assert np.array_equal(got, want) and (got[tpl:2 * tpl] == CANARY64).all()
    if roots is not None:
        assert np.array_equal(roots, nodes[:, 1])
    # without a status word the wrapper raises after one synchronisation
    with pytest.raises(tf.MerkleTreeError) as e:
        open_fn = tf.merkle_sampled.structure_from_leafs if which == "leafs" else tf.merkle_sampled.structure_from_nodes
        open_fn(d_trees, n, dev32(bad), dev64(np.zeros(3 * tpl * capacity * 5)), dev32(np.zeros(3)), n_lists=3, trees_per_list=tpl)
    assert e.value.code == LEAF_INDEX_INVALID


# ------------------------------------------------------------------ 3. no host in the chain
def test_sample_and_open_without_a_host_round_trip(tf, oracle):
    """init -> pad_and_absorb_all of a root -> sample_indices for 4 sponges -> structure_from_leafs on 4 x 2 trees, the sampler's output
    tensor handed straight on; ONE synchronisation at the end and no intermediate copy."""
    import torch

    n, k, n_sponges, tpl = 1 << 12, 80, 4, 2
    leafs, nodes = trees(oracle, n, n_sponges * tpl)
    absorbed = np.stack([nodes[tpl * s, 1] for s in range(n_sponges)])  # each transcript absorbs the root of its first tree
    capacity = tf.merkle_sampled.max_nodes(n, k)
    d_leafs, d_absorbed = dev64(leafs), dev64(absorbed)
    d_states = torch.full((16 * n_sponges,), -1, dtype=torch.int64, device="cuda")
    d_indices = torch.full((n_sponges * k,), -1, dtype=torch.int32, device="cuda")
    d_out = dev64(np.full(n_sponges * tpl * capacity * 5, CANARY64))
    d_counts, d_roots, st = dev32(np.full(n_sponges, CANARY32)), dev64(np.full(n_sponges * tpl * 5, CANARY64)), new_status()
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()  # (the uploads above, made on the default stream)
    with torch.cuda.stream(stream):
        tf.device.tip5_sponge_init_(d_states, stream=stream)
        tf.device.tip5_sponge_pad_and_absorb_all_(d_states, d_absorbed, stream=stream)
        tf.device.tip5_sponge_sample_indices(d_states, n, d_indices, stream=stream)
        tf.merkle_sampled.structure_from_leafs(d_leafs, n, d_indices, d_out, d_counts, n_lists=n_sponges, trees_per_list=tpl, roots=d_roots,
                                               stream=stream, status=st)
    stream.synchronize()
    lists = []
    for s in range(n_sponges):
        state = sponge_ref.pad_and_absorb_all(sponge_ref.init(), absorbed[s])
        lists.append(sponge_ref.sample_indices(state, n, k)[1])
    lists = np.stack(lists)
    assert np.array_equal(host32(d_indices).reshape(n_sponges, k), lists)
    want, want_counts = expected_digests(oracle, nodes, n, lists, tpl, capacity)
    assert int(st.item()) == 0 and np.array_equal(host32(d_counts), want_counts)
    assert np.array_equal(host64(d_out).reshape(want.shape), want)
    assert np.array_equal(host64(d_roots).reshape(-1, 5), nodes[:, 1])


# ------------------------------------------------------------------ 4. fence rows: one per tensor-taking callable of merkle_sampled.py
def row(name, cases):
    def register(gen):
        assert name not in ROWS, name
        ROWS[name] = (list(cases), gen)
        return gen
    return register


def _kept_behind(counts, per_list, width=1):
    """mask over n_lists x per_list x width words: True behind the first counts[l] entries of list l"""
    m = np.zeros((len(counts), per_list, width), dtype=bool)
    for l, c in enumerate(counts):
        m[l, int(c):] = True
    return m.reshape(-1)


def _status_ok():
    return fence.out("status", np.zeros(1, np.int32), dtype="int32", kept=[True])


@row("structure_indices", cases=[(6, 3, 17), (14, 2, 300), (31, 1, 2000)])
def _fence_structure_indices(tf, oracle, m, height, n_lists, k):
    n = 1 << height
    lists = list_group(n, n_lists, k, height)
    lists[0, :2] = (0, n - 1)
    want = [node_ids(oracle, n, l) for l in lists]
    capacity = m.max_nodes(n, k) + 5
    nodes = np.zeros((n_lists, capacity), np.uint32)
    for l, w in enumerate(want):
        nodes[l, :len(w)] = w.astype(np.uint32)
    counts = np.array([len(w) for w in want], np.uint32)
    ops = [fence.inp("leaf_indices", lists.astype(np.uint32), dtype="int32"),
           fence.out("node_indices", nodes, dtype="int32", kept=_kept_behind(counts, capacity)),
           fence.out("counts", counts, dtype="int32"),
           fence.out("level_ends", np.stack([level_ends(n, w) for w in want]), dtype="int32"), _status_ok()]
    yield (f"height={height} n_lists={n_lists} k={k}", ops,
           lambda leaf_indices, node_indices, counts, level_ends, status: m.structure_indices(
               n, leaf_indices, node_indices, counts, n_lists=n_lists, level_ends=level_ends, status=status))


def _fence_open(tf, oracle, m, which, height, n_lists, tpl, k):
    n = 1 << height
    leafs, nodes = trees(oracle, n, n_lists * tpl)
    lists = list_group(n, n_lists, k, height + k)
    capacity = m.max_nodes(n, k) + 3
    canary, counts = expected_digests(oracle, nodes, n, lists, tpl, capacity)
    kept = _kept_behind(np.repeat(counts, tpl), capacity, 5)
    ops = [fence.inp(which, leafs if which == "leafs" else nodes), fence.inp("leaf_indices", lists.astype(np.uint32), dtype="int32"),
           fence.out("out", canary, kept=kept), fence.out("counts", counts, dtype="int32")]
    shape = f"height={height} n_lists={n_lists} trees_per_list={tpl} k={k}"
    if which == "nodes":
        yield (shape, ops + [_status_ok()], lambda nodes, leaf_indices, out, counts, status: m.structure_from_nodes(
            nodes, n, leaf_indices, out, counts, n_lists=n_lists, trees_per_list=tpl, status=status))
        return
    yield (shape, ops + [fence.out("roots", nodes[:, 1]), _status_ok()], lambda leafs, leaf_indices, out, counts, roots, status: m.structure_from_leafs(
        leafs, n, leaf_indices, out, counts, n_lists=n_lists, trees_per_list=tpl, roots=roots, status=status))
    # one list with an index == num_leafs: 11 in the status, count 0, the slots of its trees as they were, the roots all the same
    bad = lists.copy()
    bad[n_lists - 1, 0] = n
    counts = counts.copy()
    counts[n_lists - 1] = 0
    ops = [ops[0], fence.inp("leaf_indices", bad.astype(np.uint32), dtype="int32"),
           fence.out("out", canary, kept=_kept_behind(np.repeat(counts, tpl), capacity, 5)), fence.out("counts", counts, dtype="int32"),
           fence.out("roots", nodes[:, 1]), fence.inout("status", np.zeros(1, np.int32), np.array([LEAF_INDEX_INVALID], np.int32), dtype="int32")]
    yield (shape + " one index out of range", ops, lambda leafs, leaf_indices, out, counts, roots, status: m.structure_from_leafs(
        leafs, n, leaf_indices, out, counts, n_lists=n_lists, trees_per_list=tpl, roots=roots, status=status))


@row("structure_from_nodes", cases=[(6, 3, 2, 17), (10, 2, 1, 80)])
def _fence_structure_from_nodes(tf, oracle, m, height, n_lists, tpl, k):
    yield from _fence_open(tf, oracle, m, "nodes", height, n_lists, tpl, k)


@row("structure_from_leafs", cases=[(6, 3, 1, 17), (10, 1, 5, 80), (14, 2, 2, 160)])
def _fence_structure_from_leafs(tf, oracle, m, height, n_lists, tpl, k):
    yield from _fence_open(tf, oracle, m, "leafs", height, n_lists, tpl, k)


def _ids():
    return [pytest.param(name, case, id=f"{name}-{i}") for name in ROWS for i, case in enumerate(ROWS[name][0])]


@pytest.mark.parametrize("name,case", _ids())
def test_fenced(tf, oracle, name, case):
    _, gen = ROWS[name]
    for shape, operands, call in gen(tf, oracle, tf.merkle_sampled, *case):
        fence.run(name, shape, operands, call)


def test_every_tensor_taking_callable_of_the_module_has_a_fence_row(tf):
    import inspect

    m = tf.merkle_sampled
    public = [name for name, f in vars(m).items() if inspect.isfunction(f) and f.__module__ == m.__name__ and not name.startswith("_")]
    assert sorted(public) == sorted(list(ROWS) + ["max_nodes", "from_leafs_workspace"]), "host arithmetic needs no row; every other call does"
