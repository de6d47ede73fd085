"""Merkle openings at sampled indices in device memory, the part that needs no GPU: the bound tf_merkle_auth_structure_max_nodes
against brute force over the oracle, the return codes of the four new entry points and their order (decided before any HIP call, so
they hold without a device), the work-space rule, and the argument checks of twenty_first_amd/merkle_sampled.py.

The bound is sum over the levels l below the root of min(k, (num_leafs >> l) / 2).  Brute force over the subsets of leafs at heights
0 ... 6 never exceeds it: every subset at heights 0 ... 4; at height 5 one subset of every class under the tree's symmetries (swapping
the two children of a node maps a structure onto one of the same size: 26796 classes stand for the 2^32 subsets); at height 6, where
even the classes are 3.6 * 10^8, every subset of up to 3 leafs, every subset missing up to 3, and seeded random, spread and bunched
ones of every size.  It is NOT attained in general: from height 2 on only k <= 1 reaches it (two paths share a node
below the root at the latest), so the header calls it an upper bound and TRUE_MAXIMUM below states what the oracle gives."""
import ctypes as C
import itertools

import numpy as np
import pytest

OK, TOO_FEW, NOT_POW2, TOO_HIGH, LEN_TOO_LARGE, NULL = 0, 1, 2, 3, 5, 7
MAX_K = 8192

# height -> the largest structure over all subsets of exactly k leafs, k = 0 ... 2^height (from the oracle, exhaustively)
TRUE_MAXIMUM = {
    0: [0, 0],
    1: [0, 1, 0],
    2: [0, 2, 2, 1, 0],
    3: [0, 3, 4, 4, 4, 3, 2, 1, 0],
    4: [0, 4, 6, 7, 8, 8, 8, 8, 8, 7, 6, 5, 4, 3, 2, 1, 0],
}


def bound(n, k):
    return sum(min(k, (n >> level) // 2) for level in range(n.bit_length() - 1))


def count(oracle, n, leafs):
    return len(oracle.auth_structure_indices(n, np.array(leafs, dtype=np.uint64)))


def test_the_bound_is_the_stated_sum(tf):
    lib = tf.lib()
    for height in range(0, 32):
        n = 1 << height
        for k in (0, 1, 2, 3, 63, 64, 65, 80, 160, 1024, 8191, MAX_K):
            assert lib.tf_merkle_auth_structure_max_nodes(n, k) == bound(n, k), (height, k)
            assert tf.merkle_sampled.max_nodes(n, k) == bound(n, k)
    # arguments the calls reject
    for n, k in ((0, 1), (3, 1), (12, 4), (1 << 32, 1), (1 << 40, 1), (16, MAX_K + 1)):
        assert lib.tf_merkle_auth_structure_max_nodes(n, k) == 0, (n, k)


@pytest.mark.parametrize("height", [0, 1, 2, 3, 4])
def test_no_subset_exceeds_the_bound_and_the_true_maximum_is_as_stated(tf, oracle, height):
    n = 1 << height
    best = [0] * (n + 1)
    for mask in range(1 << n):
        leafs = [i for i in range(n) if mask >> i & 1]
        c = count(oracle, n, leafs)
        assert c <= bound(n, len(leafs)), (height, leafs)
        best[len(leafs)] = max(best[len(leafs)], c)
    assert best == TRUE_MAXIMUM[height]
    # a list of k indices may repeat leafs: its structure is that of its distinct leafs, and the bound grows with k
    attained = [k for k in range(n + 1) if max(best[:k + 1]) == bound(n, k)]
    # an upper bound only: from height 2 on, two paths or more stay below it (height 1: a list of 2 may open the same leaf twice)
    assert attained == ([0, 1, 2] if height == 1 else [0, 1]), attained


def _classes(height):
    """one subset (as a bit mask) of every class of subsets of 2^height leafs under swaps of the two children of any node"""
    if height == 0:
        return [0, 1]
    sub, half = _classes(height - 1), 1 << (height - 1)
    return [(a << half) | b for i, a in enumerate(sub) for b in sub[i:]]


def test_no_subset_exceeds_the_bound_at_height_5_up_to_symmetry(tf, oracle):
    n = 32
    classes = _classes(5)
    assert len(classes) == 26796 and len(_classes(4)) == 231
    # (the symmetry itself, on the oracle: a swap of two sibling subtrees keeps the size of the structure)
    rng = np.random.default_rng(5)
    for _ in range(200):
        leafs = np.flatnonzero(rng.integers(0, 2, size=n))
        level = int(rng.integers(0, 5))
        assert count(oracle, n, leafs) == count(oracle, n, leafs ^ (1 << level))
    sizes = set()
    for mask in classes:
        leafs = [i for i in range(n) if mask >> i & 1]
        assert count(oracle, n, leafs) <= bound(n, len(leafs)), leafs
        sizes.add(len(leafs))
    assert sizes == set(range(n + 1))


def test_no_subset_exceeds_the_bound_at_height_6(tf, oracle):
    height, n = 6, 64
    everything = set(range(n))
    for size in range(0, 4):
        for leafs in itertools.combinations(range(n), size):
            assert count(oracle, n, leafs) <= bound(n, size), (height, leafs)
            rest = sorted(everything - set(leafs))
            assert count(oracle, n, rest) <= bound(n, n - size), (height, "all but", leafs)
    rng = np.random.default_rng(height)
    for size in range(4, n - 3):
        for _ in range(40):
            leafs = rng.choice(n, size=size, replace=False)
            assert count(oracle, n, leafs) <= bound(n, size), (height, leafs.tolist())
        # evenly spread and bunched leafs: the extremes of how paths share nodes
        assert count(oracle, n, [(i * n) // size for i in range(size)]) <= bound(n, size)
        assert count(oracle, n, list(range(size))) <= bound(n, size)


def _dummies():
    buf = (C.c_uint64 * 64)()
    p = C.cast(buf, C.c_void_p)
    return buf, p


def _calls(lib, p, n, k=4, n_lists=1, tpl=1, idx="p", out="p", counts="p", trees="p", status="p", capacity=8):
    """the three status-returning entry points on dummy pointers; a keyword set to None passes a null pointer"""
    g = lambda v: p if v == "p" else None  # noqa: E731
    return [
        ("indices_dev", lambda: lib.tf_merkle_auth_structure_indices_dev(n, g(idx), k, n_lists, g(out), capacity, g(counts), None, None, g(status))),
        ("sampled_dev", lambda: lib.tf_merkle_authentication_structure_sampled_dev(g(trees), n, g(idx), k, n_lists, tpl, g(out), capacity, g(counts),
                                                                                  None, g(status))),
        ("from_leafs_sampled_dev", lambda: lib.tf_merkle_auth_structure_from_leafs_sampled_dev(g(trees), n, g(idx), k, n_lists, tpl, g(out), capacity,
                                                                                              g(counts), None, None, g(status))),
    ]


def test_argument_errors_and_their_order_without_a_device(tf):
    """Every code below is returned before any HIP call, so this runs on a machine without a GPU (the pointers are never followed)."""
    lib = tf.lib()
    buf, p = _dummies()
    for name, call in _calls(lib, p, 0):
        assert call() == TOO_FEW, name
    for name, call in _calls(lib, p, 3):
        assert call() == NOT_POW2, name
    for name, call in _calls(lib, p, 1 << 32):
        assert call() == TOO_HIGH, name
    for name, call in _calls(lib, p, 16, k=MAX_K + 1):
        assert call() == LEN_TOO_LARGE, name
    for name, call in _calls(lib, p, 16, n_lists=1 << 31):
        assert call() == LEN_TOO_LARGE, name
    for name, call in _calls(lib, p, 16, status=None):
        assert call() == NULL, name
    for name, call in _calls(lib, p, 16, idx=None):
        assert call() == NULL, name
    for name, call in _calls(lib, p, 16, counts=None):
        assert call() == NULL, name
    for name, call in _calls(lib, p, 16, out=None):
        assert call() == NULL, name
    for name, call in _calls(lib, p, 16, trees=None)[1:]:
        assert call() == NULL, name
    # the order: the tree's shape, then its height, then the list length, then the pointers
    for name, call in _calls(lib, p, 0, k=MAX_K + 1, status=None):
        assert call() == TOO_FEW, name
    for name, call in _calls(lib, p, 12, k=MAX_K + 1, status=None):
        assert call() == NOT_POW2, name
    for name, call in _calls(lib, p, 1 << 33, k=MAX_K + 1, status=None):
        assert call() == TOO_HIGH, name
    for name, call in _calls(lib, p, 1 << 31, k=MAX_K + 1, status=None):
        assert call() == LEN_TOO_LARGE, name
    for name, call in _calls(lib, p, 1 << 31, k=MAX_K, status=None):
        assert call() == NULL, name
    # no list: nothing to do, whatever the other pointers are -- but the status word is always needed
    for name, call in _calls(lib, p, 16, n_lists=0, idx=None, out=None, counts=None, trees=None):
        assert call() == OK, name
    for name, call in _calls(lib, p, 16, n_lists=0, status=None):
        assert call() == NULL, name
    for name, call in _calls(lib, p, 16, tpl=0, trees=None, out=None)[1:]:
        assert call() == OK, name
    # an empty list needs no index pointer, a capacity of 0 no output: these reach the device and fail there, or run
    assert all(v == 0 for v in buf)


def test_workspace_is_the_host_index_request_plus_the_plan_and_monotone_in_trees(tf):
    lib = tf.lib()
    ws = lib.tf_merkle_auth_structure_from_leafs_sampled_workspace
    old = lib.tf_merkle_auth_structure_from_leafs_workspace
    for height in (0, 1, 6, 10, 13, 14, 16, 20):
        n = 1 << height
        for k, n_lists in ((0, 1), (1, 1), (80, 4), (160, 1), (MAX_K, 2)):
            plan = (n_lists * (bound(n, k) + 32) * 4 + 7) // 8 * 8
            last = 0
            for trees in list(range(1, 40)) + [64, 100, 1000]:
                got = ws(n, trees, k, n_lists)
                assert got == old(n, trees, 0) + plan, (height, k, n_lists, trees)
                assert got >= last, (height, k, n_lists, trees)
                last = got
                assert tf.merkle_sampled.from_leafs_workspace(n, trees, k, n_lists) == got
    for args in ((0, 1, 1, 1), (3, 1, 1, 1), (1 << 32, 1, 1, 1), (16, 0, 1, 1), (16, 1, MAX_K + 1, 1), (16, 1, 1, 0)):
        assert ws(*args) == 0, args


def test_python_argument_checks_raise_value_error(tf):
    """Sizes and shapes are refused before the ABI sees a pointer; no CUDA tensor is needed to get that far."""
    import torch

    m = tf.merkle_sampled
    idx = torch.zeros(8, dtype=torch.int32)
    words = torch.zeros(80, dtype=torch.int64)
    for n in (0, 3, 12, 1 << 32, -4):
        with pytest.raises(ValueError):
            m.structure_indices(n, idx, idx, idx)
        with pytest.raises(ValueError):
            m.structure_from_nodes(words, n, idx, words, idx)
        with pytest.raises(ValueError):
            m.structure_from_leafs(words, n, idx, words, idx)
    with pytest.raises(ValueError):
        m.structure_indices(16, idx, idx, idx, n_lists=0)
    with pytest.raises(ValueError):
        m.structure_indices(16, idx, idx, idx)  # (host tensors: not CUDA)
    with pytest.raises(ValueError):
        m.structure_indices(16, idx.to(torch.int64), idx, idx)
    with pytest.raises(ValueError):
        m.structure_from_leafs(words, 16, idx, words, idx, n_lists=3)  # 8 indices are not 3 lists
    assert m.MAX_INDICES == MAX_K and m.LEVELS == 32
    assert "merkle_sampled" in tf.__all__
