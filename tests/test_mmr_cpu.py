"""Merkle Mountain Range: host-side checks that need no GPU -- the index helpers against the literal tables of the reference's unit
tests (util_types/mmr/shared_basic.rs:148-346, shared_advanced.rs:286-618), the status strings, and every argument error the MMR
calls return before they touch a device."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_leaf_index_to_node_index_table(tf):
    m = tf.mmr_index
    want = [1, 2, 4, 5, 8, 9, 11, 12, 16, 17, 19, 20, 23, 24, 26, 27, 32, 33, 35, 36, 39, 40]
    assert [m.leaf_index_to_node_index(i) for i in range(22)] == want
    for leaf, node in enumerate(want):
        assert m.node_index_to_leaf_index(node) == leaf


def test_node_indices_added_by_append_table(tf):
    m = tf.mmr_index
    want = {0: [1], 1: [2, 3], 2: [4], 3: [5, 6, 7], 4: [8], 5: [9, 10], 6: [11], 7: [12, 13, 14, 15], 8: [16], 9: [17, 18],
            10: [19], 11: [20, 21, 22], 12: [23], 13: [24, 25], 14: [26], 15: [27, 28, 29, 30, 31], 16: [32], 17: [33, 34], 18: [35],
            19: [36, 37, 38], 31: [58, 59, 60, 61, 62, 63], 32: [64]}
    for n, nodes in want.items():
        assert m.node_indices_added_by_append(n) == nodes


def test_right_lineage_length_from_leaf_index_table(tf):
    m = tf.mmr_index
    assert [m.right_lineage_length_from_leaf_index(i) for i in range(11)] == [0, 1, 0, 2, 0, 1, 0, 3, 0, 1, 0]
    assert m.right_lineage_length_from_leaf_index((1 << 32) - 1) == 32
    assert m.right_lineage_length_from_leaf_index((1 << 63) - 1) == 63


def test_leaf_index_to_mt_index_and_peak_index_table(tf):
    f = tf.mmr_index.leaf_index_to_mt_index_and_peak_index
    assert f(0, 1) == (1, 0)
    assert [f(i, 2) for i in range(2)] == [(2, 0), (3, 0)]
    assert [f(i, 3) for i in range(3)] == [(2, 0), (3, 0), (1, 1)]
    assert [f(i, 4) for i in range(4)] == [(4, 0), (5, 0), (6, 0), (7, 0)]
    assert [f(i, 14) for i in range(12)] == [(8 + i, 0) for i in range(8)] + [(4, 1), (5, 1), (6, 1), (7, 1)]
    with pytest.raises(ValueError):
        f(3, 3)


def test_right_lineage_length_and_own_height_table(tf):
    """right_ancestor_count_test, shared_advanced.rs:359-419"""
    f = tf.mmr_index.right_lineage_length_and_own_height
    want = [(0, 0), (1, 0), (0, 1), (0, 0), (2, 0), (1, 1), (0, 2), (0, 0), (1, 0), (0, 1), (0, 0), (3, 0), (2, 1), (1, 2), (0, 3), (0, 0),
            (1, 0), (0, 1), (0, 0), (2, 0), (1, 1), (0, 2), (0, 0), (1, 0), (0, 1), (0, 0), (4, 0), (3, 1), (2, 2), (1, 3), (0, 4), (0, 0),
            (1, 0), (0, 1), (0, 0), (2, 0), (1, 1), (0, 2), (0, 0), (1, 0), (0, 1)]
    assert [f(i) for i in range(1, 42)] == want
    half = ((1 << 64) - 1) // 2
    assert f(half - 61) == (61, 1)
    assert f(half - 3) == (3, 59)
    assert f(half - 2) == (2, 60)
    assert f(half - 1) == (1, 61)
    assert f(half) == (0, 62)
    assert tf.mmr_index.right_lineage_length_from_node_index(half - 3) == 3


def test_leftmost_ancestor_table(tf):
    """shared_advanced.rs:429-447"""
    f = tf.mmr_index.leftmost_ancestor
    want = [(1, 0), (3, 1), (3, 1)] + [(7, 2)] * 4 + [(15, 3)] * 8 + [(31, 4)]
    assert [f(i) for i in range(1, 17)] == want


def test_left_sibling_table(tf):
    """shared_advanced.rs:449-457"""
    f = tf.mmr_index.left_sibling
    assert [f(6, 1), f(2, 0), f(5, 0), f(30, 3), f(29, 2), f(14, 2)] == [3, 1, 4, 15, 22, 7]
    for node, h in ((3, 1), (1, 0), (4, 0), (15, 3), (22, 2), (7, 2)):
        assert tf.mmr_index.left_sibling(tf.mmr_index.right_sibling(node, h), h) == node


def test_node_index_to_leaf_index_table(tf):
    """shared_advanced.rs:459-482"""
    want = [0, 1, None, 2, 3, None, None, 4, 5, None, 6, 7, None, None, None, 8, 9, None, 10, 11, None, None]
    assert [tf.mmr_index.node_index_to_leaf_index(i) for i in range(1, 23)] == want


def test_leaf_count_to_node_count_table(tf):
    """shared_advanced.rs:485-494"""
    want = [0, 1, 3, 4, 7, 8, 10, 11, 15, 16, 18, 19, 22, 23, 25, 26, 31, 32, 34, 35, 38, 39, 41, 42, 46, 47, 49, 50, 53, 54, 56, 57, 63, 64]
    assert [tf.mmr_index.num_leafs_to_num_nodes(i) for i in range(len(want))] == want


def test_get_peak_heights_and_peak_node_indices_table(tf):
    """shared_advanced.rs:496-529"""
    m = tf.mmr_index
    want = {0: ([], []), 1: ([0], [1]), 2: ([1], [3]), 3: ([1, 0], [3, 4]), 4: ([2], [7]), 5: ([2, 0], [7, 8]), 6: ([2, 1], [7, 10]),
            7: ([2, 1, 0], [7, 10, 11]), 8: ([3], [15]), 9: ([3, 0], [15, 16]), 10: ([3, 1], [15, 18]), 11: ([3, 1, 0], [15, 18, 19]),
            12: ([3, 2], [15, 22]), 13: ([3, 2, 0], [15, 22, 23]), 14: ([3, 2, 1], [15, 22, 25]), 15: ([3, 2, 1, 0], [15, 22, 25, 26]),
            16: ([4], [31]), 17: ([4, 0], [31, 32]), 18: ([4, 1], [31, 34]), 19: ([4, 1, 0], [31, 34, 35])}
    for n, (heights, nodes) in want.items():
        assert m.get_peak_heights_and_peak_node_indices(n) == (heights, nodes)
        assert m.get_peak_heights(n) == heights
    assert m.get_peak_heights(0b1010) == [3, 1] and m.get_peak_heights(0b1011) == [3, 1, 0]


def test_get_authentication_path_node_indices_table(tf):
    """shared_advanced.rs:531-551"""
    f = tf.mmr_index.get_authentication_path_node_indices
    cases = [((1, 31, 31), [2, 6, 14, 30]), ((2, 31, 31), [1, 6, 14, 30]), ((3, 31, 31), [6, 14, 30]), ((4, 31, 31), [5, 3, 14, 30]),
             ((21, 31, 31), [18, 29, 15]), ((21, 31, 32), [18, 29, 15]), ((32, 32, 32), []), ((1, 32, 32), None)]
    for args, want in cases:
        assert f(*args) == want, args


def test_auth_path_node_indices_table(tf):
    """auth_path_indices_unit_test and auth_path_indices_out_of_bounds_unit_test, shared_advanced.rs:553-602"""
    m = tf.mmr_index
    want16 = [[2, 6, 14, 30], [1, 6, 14, 30], [5, 3, 14, 30], [4, 3, 14, 30], [9, 13, 7, 30], [8, 13, 7, 30], [12, 10, 7, 30],
              [11, 10, 7, 30], [17, 21, 29, 15], [16, 21, 29, 15], [20, 18, 29, 15], [19, 18, 29, 15], [24, 28, 22, 15],
              [23, 28, 22, 15], [27, 25, 22, 15], [26, 25, 22, 15]]
    assert [m.auth_path_node_indices(16, i) for i in range(16)] == want16
    assert m.auth_path_node_indices(1, 0) == [] and m.auth_path_node_indices(2, 0) == [2] and m.auth_path_node_indices(2, 1) == [1]
    expected = []
    for i in range(1, 63):
        expected.append((1 << (i + 1)) - 2)
        assert m.auth_path_node_indices(1 << i, 0) == expected, i
    with pytest.raises(ValueError, match="Leaf index out-of-bounds: 5/5"):
        m.auth_path_node_indices(5, 5)
    # auth_path_indices_prop: a proof's node indices are the same walk
    rng = np.random.default_rng(7)
    for n in [int(x) for x in rng.integers(1, 1 << 62, size=200, dtype=np.uint64)]:
        i = int(rng.integers(0, n))
        want = m.auth_path_node_indices(n, i)
        assert m.membership_proof_node_indices(i, len(want)) == want


def test_node_relations_agree_with_the_leaf_level_arithmetic(tf):
    """parent / siblings in node indices against (level, index) arithmetic: node (l, x) is a right child iff x is odd."""
    m = tf.mmr_index
    for leaf in range(200):
        node = m.leaf_index_to_node_index(leaf)
        for level in range(8):
            right, height = m.right_lineage_length_and_own_height(node)
            assert height == level and (right != 0) == bool((leaf >> level) & 1)
            node = m.parent(node)


def test_status_strings(tf):
    lib = tf.lib()
    assert [lib.tf_status_string(c) for c in (22, 23, 24, 25)] == [b"TF_ERR_MMR_LEAF_INDEX_OUT_OF_RANGE", b"TF_ERR_MMR_PEAK_COUNT_MISMATCH",
                                                                  b"TF_ERR_MMR_AUTH_PATH_LENGTH_MISMATCH", b"TF_ERR_MMR_PEAK_MISMATCH"]


def _p(a):
    return C.c_void_p(a.ctypes.data)


def test_argument_errors_precede_any_device_work(tf):
    lib = tf.lib()
    INVALID, NULL, LEAF = 17, 7, 11
    d = np.zeros(64 * 5, dtype=np.uint64)
    big = C.c_uint64((1 << 63) + 1)
    # leaf counts above 2^63
    assert lib.tf_mmr_append(big, _p(d), _p(d), 1, _p(d), None) == INVALID
    assert lib.tf_mmr_append(C.c_uint64(1 << 63), _p(d), _p(d), 1, _p(d), None) == INVALID  # 2^63 + 1 after the append
    assert lib.tf_mmr_append_dev(big, _p(d), _p(d), 1, _p(d), None, None) == INVALID
    lc = np.array([3, (1 << 63) + 1], dtype=np.uint64)
    assert lib.tf_mmr_bag_peaks(_p(lc), 2, _p(d), _p(d)) == INVALID
    assert lib.tf_mmr_bag_peaks_dev(_p(lc), 2, _p(d), _p(d), None) == INVALID
    off = np.array([0, 1], dtype=np.uint64)
    st = np.zeros(4, dtype=np.int32)
    assert lib.tf_mmr_verify_membership_proofs(big, _p(d), 1, 1, _p(d), _p(d), _p(off), _p(d), _p(st)) == INVALID
    assert lib.tf_mmr_verify_membership_proofs_dev(big, _p(d), 1, 1, _p(d), _p(d), _p(off), _p(d), _p(st), None) == INVALID
    one = np.array([0], dtype=np.uint64)
    for fn, extra in ((lib.tf_mmr_batch_mutate_leafs, ()), (lib.tf_mmr_batch_mutate_leafs_dev, (None,))):
        assert fn(big, _p(d), 1, _p(one), _p(d), _p(off), _p(d), 0, None, None, None, None, *extra) == INVALID
    # NULL pointers
    assert lib.tf_mmr_append(C.c_uint64(1), _p(d), _p(d), 1, None, None) == NULL
    assert lib.tf_mmr_append(C.c_uint64(1), None, _p(d), 1, _p(d), None) == NULL
    assert lib.tf_mmr_append_dev(C.c_uint64(0), None, None, 1, _p(d), None, None) == NULL
    assert lib.tf_mmr_bag_peaks(None, 1, _p(d), _p(d)) == NULL
    assert lib.tf_mmr_bag_peaks_dev(_p(lc), 1, None, _p(d), None) == NULL
    assert lib.tf_mmr_verify_membership_proofs(C.c_uint64(3), _p(d), 2, 1, _p(d), _p(d), None, _p(d), _p(st)) == NULL
    assert lib.tf_mmr_verify_membership_proofs_dev(C.c_uint64(3), _p(d), 2, 1, _p(d), _p(d), _p(off), None, _p(st), None) == NULL
    # decreasing offsets
    dec = np.array([2, 1], dtype=np.uint64)
    assert lib.tf_mmr_verify_membership_proofs(C.c_uint64(3), _p(d), 2, 1, _p(d), _p(d), _p(dec), _p(d), _p(st)) == INVALID
    assert lib.tf_mmr_verify_membership_proofs_dev(C.c_uint64(3), _p(d), 2, 1, _p(d), _p(d), _p(dec), _p(d), _p(st), None) == INVALID
    mod = np.zeros(4, dtype=np.int32)
    idx2 = np.array([1, 1], dtype=np.uint64)
    off2 = np.array([0, 1, 2], dtype=np.uint64)
    for fn, extra in ((lib.tf_mmr_batch_mutate_leafs, ()), (lib.tf_mmr_batch_mutate_leafs_dev, (None,))):
        # duplicate mutation indices (the reference panics)
        assert fn(C.c_uint64(4), _p(d), 2, _p(idx2), _p(d), _p(off2), _p(d), 0, None, None, None, None, *extra) == INVALID
        # a mutation index or an own index out of range, with and without peaks
        for peaks in (_p(d), None):
            assert fn(C.c_uint64(1), peaks, 1, _p(np.array([1], dtype=np.uint64)), _p(d), _p(off), _p(d), 0, None, None, None, None,
                      *extra) == LEAF
            assert fn(C.c_uint64(4), peaks, 0, None, None, None, None, 1, _p(np.array([4], dtype=np.uint64)), _p(off), _p(d), _p(mod),
                      *extra) == LEAF
        assert fn(C.c_uint64(4), _p(d), 1, _p(one), _p(d), _p(dec), _p(d), 0, None, None, None, None, *extra) == INVALID
        assert fn(C.c_uint64(4), _p(d), 0, None, None, None, None, 1, _p(one), _p(dec), _p(d), _p(mod), *extra) == INVALID
        assert fn(C.c_uint64(4), _p(d), 1, None, _p(d), _p(off), _p(d), 0, None, None, None, None, *extra) == NULL
        # a mutation path of 64 digests: no MMR node is that high (the header's second divergence), with and without peaks
        long_path = np.array([0, 64], dtype=np.uint64)
        big_d = np.zeros(64 * 5, dtype=np.uint64)
        for peaks in (_p(d), None):
            assert fn(C.c_uint64(4), peaks, 1, _p(one), _p(d), _p(long_path), _p(big_d), 0, None, None, None, None, *extra) == INVALID


def test_python_front_rejects_mismatched_lists(tf):
    # an accumulator's peak list must have popcount(leaf_count) digests: the host calls read and write that many
    with pytest.raises(ValueError):
        tf.MmrAccumulator(5, np.zeros((1, 5), dtype=np.uint64))
    with pytest.raises(ValueError):
        tf.MmrAccumulator(4, np.zeros((2, 5), dtype=np.uint64))
    tf.MmrAccumulator(5, np.zeros((2, 5), dtype=np.uint64))
    acc = tf.MmrAccumulator(0)
    with pytest.raises(ValueError):
        acc.batch_mutate_leaf_and_update_mps([tf.MmrMembershipProof(np.zeros((0, 5), dtype=np.uint64))], [], [])
    with pytest.raises(ValueError):
        tf.MmrAccumulator((1 << 63) + 1)


def test_cpp_mirror_self_test_compiles_and_runs():
    """twenty-first_amd/host/mmr_selftest.cpp builds against the header and the library; without a device it reports the skip (77),
    with one it passes (0)."""
    if shutil.which("make") is None or shutil.which(os.environ.get("CXX", "g++")) is None:
        pytest.skip("no C++ toolchain")
    host = os.path.join(ROOT, "twenty-first_amd", "host")
    subprocess.check_call(["make", "-C", host, "mmr_selftest"], stdout=subprocess.DEVNULL)
    rc = subprocess.run([os.path.join(host, "mmr_selftest")], capture_output=True, timeout=300).returncode
    assert rc in (0, 77)
