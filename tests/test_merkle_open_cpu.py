"""Authentication structures straight from the leafs (MerkleTree::{sequential,par}_authentication_structure_from_leafs,
util_types/merkle_tree.rs:506-542): the parts that need no GPU -- the entry points, the argument errors in the documented order, the
sizing rule, the work-space arithmetic and the C++ mirror's self-test program."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "twenty-first_amd", "host")

OK, TOO_FEW, INCORRECT, NULL, NO_DEVICE, INDEX_INVALID, TOO_SMALL = 0, 1, 2, 7, 8, 11, 13


def p(a):
    return C.c_void_p(a.ctypes.data)


def u64(values):
    return np.array(values, dtype=np.uint64)


def index_sets(n):
    """The index lists of the sizing checks: empty, the two ends, both, all leafs, every second leaf, repeats."""
    return [[], [0], [n - 1], [0, n - 1], list(range(n)), list(range(0, n, 2)), [3 % n, 3 % n, 5 % n, 0, 3 % n]]


def test_version_and_entry_points(tf):
    lib = tf.lib()
    assert lib.tf_version() == 1002
    for name in ("tf_merkle_auth_structure_from_leafs", "tf_merkle_auth_structure_from_leafs_dev", "tf_merkle_auth_structure_from_leafs_workspace"):
        assert hasattr(lib, name)
    assert lib.tf_status_string(TOO_SMALL) == b"TF_ERR_BUFFER_TOO_SMALL" and lib.tf_status_string(INDEX_INVALID) == b"TF_ERR_LEAF_INDEX_INVALID"


@pytest.mark.parametrize("dev", [False, True])
def test_argument_errors_in_order_before_any_device(tf, dev):
    """num_leafs == 0, not a power of two, an index out of range, NULL leafs, NULL indices with k > 0, NULL out_count: each wins
    over everything after it, and none needs a device (they are the return value on a machine without one)."""
    lib = tf.lib()
    fn = lib.tf_merkle_auth_structure_from_leafs_dev if dev else lib.tf_merkle_auth_structure_from_leafs
    tail = (None,) if dev else ()  # the stream
    leafs, out = np.zeros(8 * 5, dtype=np.uint64), np.zeros(8 * 5, dtype=np.uint64)
    good, bad = u64([0, 2]), u64([0, 8])
    cnt = C.c_size_t(0)

    def call(leafs_p, n, batch, idx_p, k, out_p, cap, cnt_p):
        return fn(leafs_p, n, batch, idx_p, k, out_p, cap, cnt_p, None, *tail)

    # every later error is present as well: the earlier one is reported
    assert call(None, 0, 1, p(bad), 2, p(out), 8, None) == TOO_FEW
    assert call(None, 6, 1, p(bad), 2, p(out), 8, None) == INCORRECT
    assert call(None, 12, 1, None, 2, p(out), 8, None) == INCORRECT
    assert call(None, 8, 1, p(bad), 2, p(out), 8, None) == INDEX_INVALID
    assert call(p(leafs), 8, 0, p(bad), 2, None, 0, C.byref(cnt)) == INDEX_INVALID  # ... before batch == 0 returns
    assert call(None, 8, 1, p(good), 2, p(out), 8, C.byref(cnt)) == NULL
    assert call(p(leafs), 8, 1, None, 2, p(out), 8, C.byref(cnt)) == NULL
    assert call(p(leafs), 8, 1, p(good), 2, p(out), 8, None) == NULL
    # k == 0 needs no index array; batch == 0 is TF_OK with the count set
    cnt.value = 99
    assert call(p(leafs), 8, 1, None, 0, None, 0, C.byref(cnt)) == OK and cnt.value == 0
    cnt.value = 99
    assert call(p(leafs), 8, 0, p(good), 2, p(out), 8, C.byref(cnt)) == OK and cnt.value == 3
    assert not out.any()
    # with every argument in order the call needs a device
    if lib.tf_device_count() == 0:
        assert call(p(leafs), 8, 1, p(good), 2, p(out), 8, C.byref(cnt)) == NO_DEVICE


def test_errors_raise_the_existing_variants(tf):
    leafs = np.zeros(8 * 5, dtype=np.uint64)
    for args, variant in (((leafs, [8]), "LeafIndexInvalid"), ((leafs[:30], [0]), "IncorrectNumberOfLeafs"), ((leafs[:0], []), "TooFewLeafs")):
        for fn in (tf.MerkleTree.authentication_structure_from_leafs, tf.MerkleTree.par_authentication_structure_from_leafs,
                   tf.MerkleTree.sequential_authentication_structure_from_leafs):
            with pytest.raises(tf.MerkleTreeError) as e:
                fn(*args)
            assert e.value.variant == variant


@pytest.mark.parametrize("n", [1, 2, 8, 1 << 10])
def test_sizing_call_counts_what_the_oracle_counts(tf, oracle, n):
    lib = tf.lib()
    leafs = np.zeros(5, dtype=np.uint64)  # never read: the sizing call touches no digest
    roots = np.full(5, 7, dtype=np.uint64)
    for indices in index_sets(n):
        idx = u64(indices)
        want = len(oracle.auth_structure_indices(n, idx))
        for batch in (1, 3):
            for fn, tail in ((lib.tf_merkle_auth_structure_from_leafs, ()), (lib.tf_merkle_auth_structure_from_leafs_dev, (None,))):
                cnt = C.c_size_t(12345)
                assert fn(p(leafs), n, batch, p(idx) if idx.size else None, idx.size, None, 0, C.byref(cnt), p(roots), *tail) == OK
                assert cnt.value == want, (n, indices)
                cnt.value = 12345
                assert fn(p(leafs), n, batch, p(idx) if idx.size else None, idx.size, p(leafs), 0, C.byref(cnt), p(roots), *tail) == OK
                assert cnt.value == want
        # the count of the index-only entry point
        cnt = C.c_size_t(0)
        assert lib.tf_merkle_auth_structure_indices(n, p(idx) if idx.size else None, idx.size, None, 0, C.byref(cnt)) == OK
        assert cnt.value == want
    assert (roots == 7).all(), "the sizing call writes nothing, roots included"


def test_buffer_too_small_still_reports_the_count(tf, oracle):
    lib = tf.lib()
    n = 1 << 10
    leafs = np.zeros(5, dtype=np.uint64)
    out = np.full(5 * 64, 7, dtype=np.uint64)
    roots = np.full(5, 7, dtype=np.uint64)
    idx = u64([5, 77, 78, 1000])
    want = len(oracle.auth_structure_indices(n, idx))
    assert 2 <= want <= 64
    for fn, tail in ((lib.tf_merkle_auth_structure_from_leafs, ()), (lib.tf_merkle_auth_structure_from_leafs_dev, (None,))):
        cnt = C.c_size_t(0)
        assert fn(p(leafs), n, 2, p(idx), idx.size, p(out), want - 1, C.byref(cnt), p(roots), *tail) == TOO_SMALL
        assert cnt.value == want
    assert (out == 7).all() and (roots == 7).all(), "nothing is written"


def layout_digests(n, batch):
    """The digests in use as include/tf_hip.h and DESIGN.md describe them, from the project's constants kCoopMaxCount = 2^13 and
    kTopWidth = 64: wide levels (not narrow: more than 64 nodes and more than 2^13 pairs over the batch) ping-pong through n / 2 and
    n / 4 digests per tree, the levels from the first narrow one (w nodes) on are a block of 2 w per tree."""
    narrow = lambda w: w <= 64 or (w // 2) * batch <= (1 << 13)  # noqa: E731
    w, wide = n, 0
    while not narrow(w):
        w, wide = w // 2, wide + 1
    return batch * ((n // 2 if wide >= 1 else 0) + (n // 4 if wide >= 2 else 0) + 2 * w)


def documented_workspace(n, batch, k_nodes):
    """... and the request: the largest use of any batch up to this one, 8 * 5 bytes per digest, 8 bytes per plan entry."""
    return 8 * 5 * max(layout_digests(n, b) for b in range(1, batch + 1)) + 8 * k_nodes


def test_workspace_arithmetic(tf):
    ws = tf.device.authentication_structure_from_leafs_workspace
    assert ws(1, 1, 0) == 8 * 5 * 2 and ws(64, 1, 3) == 8 * 5 * 128 + 8 * 3
    assert ws(1 << 14, 1, 5) == 8 * 5 * (1 << 15) + 40  # the largest tree that is narrow from its leafs: all top block
    assert ws(1 << 15, 1, 0) == 8 * 5 * ((1 << 14) + (1 << 15))  # one wide level
    assert ws(1 << 20, 1, 80) == 8 * 5 * ((1 << 19) + (1 << 18) + (1 << 15)) + 8 * 80
    assert ws(1 << 20, 1, 80) < 0.8 * (1 << 20) * 40, "under 0.8 n digests where a node array takes 2 n"
    for n, batch, k in ((1 << 20, 1, 80), (1 << 14, 4, 17), (64, 1000, 3)):
        assert ws(n, batch, k) == documented_workspace(n, batch, k)
        assert ws(n, batch, k) <= 40 * (batch * (3 * n // 4) + (1 << 15) + 128 * batch) + 16 * k
    for log_n in range(0, 22):
        n, prev = 1 << log_n, 0
        for batch in list(range(1, 70)) + [127, 128, 129, 255, 256, 257, 1000, 4096, 4097, (1 << 14) + 1]:
            got = ws(n, batch, 9)
            if batch < 70:
                assert got == documented_workspace(n, batch, 9), (n, batch)
            assert got >= 40 * layout_digests(n, batch) + 72, "the request covers what the batch uses"
            assert got <= 40 * 2 * n * batch + 72, (n, batch)
            assert got <= 40 * (batch * (3 * n // 4) + (1 << 15) + 128 * batch) + 16 * 9, (n, batch)
            assert got >= prev, f"not monotone in batch at n = {n}, batch = {batch}"
            prev = got
    # arguments the call rejects have no work space
    assert ws(0, 1, 0) == 0 and ws(12, 1, 0) == 0 and ws(8, 0, 0) == 0 and ws(1 << 32, 1, 0) == 0


def test_cpp_mirror_merkle_open_selftest_compiles(tf):
    subprocess.check_call(["make", "-C", HOST, "merkle_open_selftest"], stdout=subprocess.DEVNULL)
    assert os.path.exists(os.path.join(HOST, "merkle_open_selftest"))
    if tf.lib().tf_device_count() == 0:
        r = subprocess.run([os.path.join(HOST, "merkle_open_selftest")], capture_output=True, text=True, timeout=120)
        assert r.returncode == 77, r.stdout + r.stderr
