"""Authentication structures and roots straight from the leafs on the GPU (MerkleTree::{sequential,par}_authentication_structure_from_leafs,
util_types/merkle_tree.rs:506-542) against the CPU oracle.

Expected structure: oracle.merkle_build(leafs).reshape(2n, 5)[oracle.auth_structure_indices(n, idx)]; expected root: row 1 of the same
array.  Every comparison is np.array_equal on raw words.  One test pins the reference's own definition at height 7: every structure
node is the frugal root of its subtree_leafs (:565-575).

Heights, for one tree: 0, 1, 2; 6 (one top launch); 7 (two narrow launches); 10; 14 (the largest tree that is narrow from its leafs);
15 (one wide level, leafs -> buffer a); 16 (two wide levels, both ping-pong buffers); 17 (three: buffer a written again after its
nodes must be out).  Batches: (2^13, 4) one wide level that only the batch makes wide, (2^14, 4) two, (2^6, 3), (2^10, 5)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "twenty-first_amd", "host")
HEIGHTS = [0, 1, 2, 6, 7, 10, 14, 15, 16, 17]
BATCHES = [(1 << 13, 4), (1 << 14, 4), (1 << 6, 3), (1 << 10, 5)]
ROOT_MISMATCH = 21


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(tf):
    assert tf.lib().tf_device_count() > 0, "no HIP device visible: the product has no CPU fallback"


_trees = {}


def trees(oracle, n, batch=1):
    """(leafs (batch, n, 5), nodes (batch, 2n, 5)) of `batch` trees with distinct leafs, built once by the oracle and never written."""
    if (n, batch) not in _trees:
        leafs = oracle.fill_random(batch * n * 5, 0x0FE0 + 31 * n + batch).reshape(batch, n, 5)
        nodes = np.stack([oracle.merkle_build(leafs[t], threads=8 if n >= 1 << 13 else 0).reshape(2 * n, 5) for t in range(batch)])
        leafs.setflags(write=False)
        nodes.setflags(write=False)
        _trees[(n, batch)] = (leafs, nodes)
    return _trees[(n, batch)]


def index_sets(n):
    rng = np.random.default_rng(n + 17)
    sets = [[], [0], [n - 1], [0, n - 1], [2 % n, 3 % n], [3 % n, 3 % n, 5 % n], rng.integers(0, n, size=17).tolist(),
            list(range(0, n, 2)), list(range(n))]
    return [np.array(s, dtype=np.uint64) for s in sets]


def on_device(a):
    import torch

    return torch.from_numpy(np.array(a, dtype=np.uint64).reshape(-1).view(np.int64)).cuda()  # (a copy: the shared reference stays untouched)


def host_words(t):
    return t.cpu().numpy().view(np.uint64)


def open_dev(tf, d_leafs, n, idx, batch=1, with_roots=True, stream=None):
    """The device call -> (structure (batch, count, 5), roots (batch, 5) or None), read back after a synchronisation."""
    import torch

    d_roots = torch.full((batch * 5,), -1, dtype=torch.int64, device="cuda") if with_roots else None  # (not canonical: a word never stored shows)
    d_out = tf.device.authentication_structure_from_leafs(d_leafs, n, idx, roots=d_roots, batch=batch, stream=stream)
    torch.cuda.synchronize()
    return host_words(d_out).reshape(batch, -1, 5), host_words(d_roots).reshape(batch, 5) if with_roots else None


def expected(oracle, nodes, n, idx):
    node_ids = oracle.auth_structure_indices(n, idx).astype(np.int64)
    return nodes[:, node_ids], nodes[:, 1]


@pytest.mark.parametrize("height", HEIGHTS)
def test_one_tree_every_index_set(tf, oracle, height):
    n = 1 << height
    leafs, nodes = trees(oracle, n)
    d_leafs = on_device(leafs)
    for idx in index_sets(n):
        want, want_roots = expected(oracle, nodes, n, idx)
        got, roots = open_dev(tf, d_leafs, n, idx)
        assert got.shape == want.shape, (height, idx[:8])
        assert np.array_equal(got, want), (height, idx[:8])
        assert np.array_equal(roots, want_roots), (height, idx[:8])
    assert np.array_equal(host_words(d_leafs), leafs.reshape(-1)), "the leafs are read only"
    count_all, _ = open_dev(tf, d_leafs, n, index_sets(n)[-1])
    assert count_all.shape[1] == 0, "every leaf opened: nothing left to send"


def test_each_node_is_the_frugal_root_of_its_subtree(tf, oracle):
    """The reference's definition (merkle_tree.rs:514-522 over subtree_leafs :565-575), directly, at height 7."""
    height, n = 7, 1 << 7
    leafs, _ = trees(oracle, n)
    d_leafs = on_device(leafs)
    for idx in index_sets(n):
        got, _ = open_dev(tf, d_leafs, n, idx)
        node_ids = oracle.auth_structure_indices(n, idx).tolist()
        assert got.shape[1] == len(node_ids)
        for slot, node in enumerate(node_ids):
            sub_height = height - (int(node).bit_length() - 1)
            left = int(node) * (1 << sub_height) - n
            sub = leafs[0, left:left + (1 << sub_height)]
            want = sub[0] if sub_height == 0 else oracle.merkle_frugal_root(np.ascontiguousarray(sub))
            assert np.array_equal(got[0, slot], want), (idx[:8], node)


@pytest.mark.parametrize("n,batch", BATCHES)
def test_batches_every_tree_against_its_own_oracle_tree(tf, oracle, n, batch):
    leafs, nodes = trees(oracle, n, batch)
    assert not np.array_equal(nodes[0, 1], nodes[1, 1])
    d_leafs = on_device(leafs)
    for idx in index_sets(n):
        want, want_roots = expected(oracle, nodes, n, idx)
        got, roots = open_dev(tf, d_leafs, n, idx, batch=batch)
        for t in range(batch):
            assert np.array_equal(got[t], want[t]), (n, batch, t, idx[:8])
            assert np.array_equal(roots[t], want_roots[t]), (n, batch, t, idx[:8])
    assert np.array_equal(host_words(d_leafs), leafs.reshape(-1))


@pytest.mark.parametrize("n,batch", [(1 << 10, 1), (1 << 16, 1), (1 << 13, 4)])
def test_roots_are_optional_and_equal_the_frugal_roots(tf, oracle, n, batch):
    import torch

    leafs, nodes = trees(oracle, n, batch)
    d_leafs = on_device(leafs)
    idx = index_sets(n)[6]
    with_roots, roots = open_dev(tf, d_leafs, n, idx, batch=batch)
    without, _ = open_dev(tf, d_leafs, n, idx, batch=batch, with_roots=False)
    assert np.array_equal(with_roots, without) and with_roots.shape[1] > 0
    d_frugal = torch.zeros(batch * 5, dtype=torch.int64, device="cuda")
    tf.device.merkle_root(d_leafs, n, d_frugal, batch=batch)
    torch.cuda.synchronize()
    assert np.array_equal(roots.reshape(-1), host_words(d_frugal))
    # roots only: no index at all
    empty, roots_only = open_dev(tf, d_leafs, n, np.zeros(0, dtype=np.uint64), batch=batch)
    assert empty.shape[1] == 0 and np.array_equal(roots_only, roots)


@pytest.mark.parametrize("n,batch", [(1, 1), (1 << 7, 1), (1 << 15, 1), (1 << 10, 5)])
def test_host_pointer_form_equals_the_device_form(tf, oracle, n, batch):
    leafs, nodes = trees(oracle, n, batch)
    d_leafs = on_device(leafs)
    for idx in (index_sets(n)[6], index_sets(n)[-1], index_sets(n)[5]):
        dev, dev_roots = open_dev(tf, d_leafs, n, idx, batch=batch)
        host, host_roots = tf.MerkleTree.authentication_structure_from_leafs(leafs, idx, batch=batch, with_root=True)
        plain = tf.MerkleTree.par_authentication_structure_from_leafs(leafs, idx, batch=batch)
        assert host.shape == ((dev.shape[1], 5) if batch == 1 else dev.shape)
        assert np.array_equal(host.reshape(dev.shape), dev) and np.array_equal(plain, host)
        assert np.array_equal(host_roots.reshape(dev_roots.shape), dev_roots)
        assert np.array_equal(dev_roots, nodes[:, 1])
    assert np.array_equal(tf.MerkleTree.sequential_authentication_structure_from_leafs(leafs, idx, batch=batch), host)


@pytest.mark.parametrize("height", [6, 10, 16])
def test_same_words_in_the_same_order_as_build_and_gather(tf, oracle, height):
    import torch

    n = 1 << height
    leafs, _ = trees(oracle, n)
    d_leafs = on_device(leafs)
    d_nodes = torch.zeros(n * 10, dtype=torch.int64, device="cuda")
    tf.device.merkle_build(d_leafs, n, d_nodes)
    for idx in index_sets(n)[:8]:
        got, _ = open_dev(tf, d_leafs, n, idx)
        assert np.array_equal(got[0], tf.device.authentication_structure(d_nodes, n, idx)), (height, idx[:8])


def test_two_calls_on_one_stream_before_any_synchronisation(tf, oracle):
    """The _dev form returns with its work enqueued; a second, different call right behind it must not disturb the first one's plan."""
    import torch

    stream = torch.cuda.Stream()
    calls = []
    for n, batch, which in ((1 << 16, 1, 7), (1 << 10, 5, 6), (1 << 16, 1, 6), (1 << 14, 4, 7)):
        leafs, nodes = trees(oracle, n, batch)
        calls.append((n, batch, index_sets(n)[which], on_device(leafs), nodes))
    torch.cuda.synchronize()
    outs = []
    with torch.cuda.stream(stream):
        for n, batch, idx, d_leafs, _ in calls:
            d_roots = torch.zeros(batch * 5, dtype=torch.int64, device="cuda")
            outs.append((tf.device.authentication_structure_from_leafs(d_leafs, n, idx, roots=d_roots, batch=batch, stream=stream), d_roots))
    stream.synchronize()
    for (n, batch, idx, _, nodes), (d_out, d_roots) in zip(calls, outs):
        want, want_roots = expected(oracle, nodes, n, idx)
        assert np.array_equal(host_words(d_out).reshape(want.shape), want), (n, batch)
        assert np.array_equal(host_words(d_roots).reshape(batch, 5), want_roots), (n, batch)


def test_caller_buffer_and_capacity(tf, oracle):
    """`out` may be larger than the structure: the trees stay count digests apart and nothing behind them is written."""
    import torch

    n, batch = 1 << 10, 5
    leafs, nodes = trees(oracle, n, batch)
    idx = index_sets(n)[6]
    want, _ = expected(oracle, nodes, n, idx)
    d_out = torch.full((want.size + 40,), 7, dtype=torch.int64, device="cuda")
    got = tf.device.authentication_structure_from_leafs(on_device(leafs), n, idx, out=d_out, batch=batch)
    torch.cuda.synchronize()
    assert got.numel() == want.size and got.data_ptr() == d_out.data_ptr()
    assert np.array_equal(host_words(got).reshape(want.shape), want)
    assert (host_words(d_out)[want.size:] == 7).all()


def test_round_trip_through_the_batched_verifier(tf, oracle):
    n, batch, height = 1 << 10, 3, 10
    leafs, _ = trees(oracle, n, batch)
    idx = index_sets(n)[6]
    structure, roots = tf.MerkleTree.authentication_structure_from_leafs(leafs, idx, batch=batch, with_root=True)
    proofs = [tf.MerkleTreeInclusionProof(height, idx, leafs[t][idx.astype(np.int64)], structure[t]) for t in range(batch)]
    assert (tf.MerkleTreeInclusionProof.try_verify_batch(proofs, roots) == 0).all()
    bent = structure.copy()
    bent[1, 2, 3] ^= np.uint64(1)
    proofs[1] = tf.MerkleTreeInclusionProof(height, idx, leafs[1][idx.astype(np.int64)], bent[1])
    assert tf.MerkleTreeInclusionProof.try_verify_batch(proofs, roots).tolist() == [0, ROOT_MISMATCH, 0]


def test_raw_abi_sizing_and_too_small_on_the_device(tf, oracle):
    """The sizing rule with a device present: the count, nothing written; one digest short is TF_ERR_BUFFER_TOO_SMALL."""
    import torch

    n = 1 << 10
    leafs, nodes = trees(oracle, n)
    idx = index_sets(n)[6]
    want, _ = expected(oracle, nodes, n, idx)
    d_leafs = on_device(leafs)
    d_out = torch.full((want.size,), 7, dtype=torch.int64, device="cuda")
    d_roots = torch.full((5,), 7, dtype=torch.int64, device="cuda")
    fn = tf.lib().tf_merkle_auth_structure_from_leafs_dev
    cnt = C.c_size_t(0)
    args = (C.c_void_p(d_leafs.data_ptr()), n, 1, C.c_void_p(idx.ctypes.data), idx.size)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    assert fn(*args, C.c_void_p(d_out.data_ptr()), 0, C.byref(cnt), C.c_void_p(d_roots.data_ptr()), stream) == 0 and cnt.value == want.shape[1]
    assert fn(*args, C.c_void_p(d_out.data_ptr()), cnt.value - 1, C.byref(cnt), C.c_void_p(d_roots.data_ptr()), stream) == 13
    torch.cuda.synchronize()
    assert (host_words(d_out) == 7).all() and (host_words(d_roots) == 7).all()
    assert fn(*args, C.c_void_p(d_out.data_ptr()), cnt.value, C.byref(cnt), C.c_void_p(d_roots.data_ptr()), stream) == 0
    torch.cuda.synchronize()
    assert np.array_equal(host_words(d_out).reshape(want.shape), want) and np.array_equal(host_words(d_roots), nodes[0, 1])


def test_cpp_mirror_merkle_open_selftest_on_gpu():
    subprocess.check_call(["make", "-C", HOST, "merkle_open_selftest"], stdout=subprocess.DEVNULL)
    r = subprocess.run([os.path.join(HOST, "merkle_open_selftest")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
