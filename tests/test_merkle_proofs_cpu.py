"""Inclusion-proof verification (MerkleTreeInclusionProof, util_types/merkle_tree.rs:90-113, :683-931): the parts that need no GPU --
the new status codes, their MerkleTreeError variants, the ABI version and the C++ mirror's self-test program."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "twenty-first_amd", "host")

NEW_CODES = {19: ("TF_ERR_AUTH_STRUCTURE_LENGTH_MISMATCH", "AuthenticationStructureLengthMismatch"),
             20: ("TF_ERR_REPEATED_LEAF_DIGEST_MISMATCH", "RepeatedLeafDigestMismatch"),
             21: ("TF_ERR_ROOT_MISMATCH", "RootMismatch")}


def test_status_strings(tf):
    for code, (name, _) in NEW_CODES.items():
        assert tf.lib().tf_status_string(code).decode() == name


def test_merkle_tree_error_variants(tf):
    for code, (_, variant) in NEW_CODES.items():
        assert tf.MerkleTreeError.VARIANTS[code] == variant
        with pytest.raises(tf.MerkleTreeError) as e:
            tf._check(code, "MerkleTreeInclusionProof::try_verify")
        assert e.value.variant == variant and e.value.code == code


def test_version_and_entry_points(tf):
    lib = tf.lib()
    assert lib.tf_version() == 1002
    for name in ("tf_merkle_verify_proofs", "tf_merkle_verify_proofs_dev", "tf_merkle_authentication_paths", "tf_merkle_authentication_paths_dev"):
        assert hasattr(lib, name)


def test_proof_layout_checks_without_device(tf):
    """Argument errors are the call's return value and come before any device is touched."""
    import ctypes as C

    import numpy as np

    h = np.array([3], dtype=np.uint32)
    lo = np.array([1, 0], dtype=np.uint64)  # decreasing
    ao = np.array([0, 0], dtype=np.uint64)
    st = np.zeros(1, dtype=np.int32)
    p = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
    root = np.zeros(5, dtype=np.uint64)
    assert tf.lib().tf_merkle_verify_proofs(p(h), 1, p(lo), p(root), p(root), p(ao), p(root), p(root), p(st)) == 17
    assert tf.lib().tf_merkle_verify_proofs(None, 1, p(lo), None, None, p(ao), None, p(root), p(st)) == 7
    assert tf.lib().tf_merkle_verify_proofs(None, 0, None, None, None, None, None, None, None) == 0


def test_proof_objects_are_checked_on_the_host(tf):
    import numpy as np

    with pytest.raises(ValueError):
        tf.MerkleTreeInclusionProof(3, [0, 1], np.zeros((1, 5), dtype=np.uint64), np.zeros((0, 5), dtype=np.uint64))
    with pytest.raises(ValueError):
        tf.MerkleTreeInclusionProof(1 << 32, [], np.zeros((0, 5), dtype=np.uint64), np.zeros((0, 5), dtype=np.uint64))
    nodes = np.arange(80, dtype=np.uint64).reshape(16, 5)
    with pytest.raises(tf.MerkleTreeError) as e:
        tf.MerkleTree(nodes).indexed_leafs([2, 8])
    assert e.value.variant == "LeafIndexInvalid"


def test_cpp_mirror_proof_selftest_compiles(tf):
    subprocess.check_call(["make", "-C", HOST, "proof_selftest"], stdout=subprocess.DEVNULL)
    assert os.path.exists(os.path.join(HOST, "proof_selftest"))
    if tf.lib().tf_device_count() == 0:
        r = subprocess.run([os.path.join(HOST, "proof_selftest")], capture_output=True, text=True, timeout=120)
        assert r.returncode == 77, r.stdout + r.stderr


@pytest.mark.gpu
def test_cpp_mirror_proof_selftest_on_gpu():
    subprocess.check_call(["make", "-C", HOST, "proof_selftest"], stdout=subprocess.DEVNULL)
    r = subprocess.run([os.path.join(HOST, "proof_selftest")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
