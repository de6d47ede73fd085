"""MMR successor proofs and membership-proof updates under appends: what needs no GPU -- the proof length against the loop of
MmrSuccessorProof::new_from_batch_append (util_types/mmr/mmr_successor_proof.rs:34-91), the status strings, the offsets and flags of
the update's sizing call, and every argument error the calls return before they touch a device."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, NULL, LEAF, TOO_SMALL, PATH_LEN = 17, 7, 11, 13, 24
NAMES = ["tf_mmr_successor_proof_len", "tf_mmr_successor_proof_new", "tf_mmr_successor_proof_new_dev", "tf_mmr_verify_successor_proofs",
         "tf_mmr_verify_successor_proofs_dev", "tf_mmr_update_proofs_from_append", "tf_mmr_update_proofs_from_append_dev"]


def _p(a):
    return C.c_void_p(a.ctypes.data)


def u64(x):
    return C.c_uint64(x)


def model_len(tf, n, k):
    """The loop of new_from_batch_append, counting instead of hashing."""
    if n == 0:
        return 0
    t = (n & -n).bit_length() - 1
    if k < 1 << t:
        return 0
    mt = tf.mmr_index.leaf_index_to_mt_index_and_peak_index(n, n + k)[0] >> t
    count = 1
    while mt > 1:
        count += mt % 2 == 0
        mt //= 2
    return count


def test_successor_proof_len_is_the_reference_loop(tf):
    f = tf.lib().tf_mmr_successor_proof_len
    for n in range(65):
        for k in range(65):
            assert f(u64(n), u64(k)) == model_len(tf, n, k), (n, k)
    assert f(u64(42), u64(8)) == 2 and f(u64(8), u64(3)) == 0 and f(u64(0), u64(0)) == 0 and f(u64(0), u64(1)) == 0
    for n, k in (((1 << 62) + (1 << 40), 1 << 40), ((1 << 63) - 1, 1)):
        assert f(u64(n), u64(k)) == model_len(tf, n, k) > 0, (n, k)
    # arguments the calls reject
    assert f(u64((1 << 63) + 1), u64(0)) == 0 and f(u64(1 << 63), u64(1)) == 0 and f(u64(3), u64((1 << 64) - 2)) == 0
    assert tf.device.mmr_successor_proof_len(42, 8) == 2


def test_status_strings(tf):
    lib = tf.lib()
    want = [b"TF_ERR_MMR_INCONSISTENT_OLD", b"TF_ERR_MMR_INCONSISTENT_NEW", b"TF_ERR_MMR_OLD_HAS_MORE_LEAFS", b"TF_ERR_MMR_SUCCESSOR_PATH_TOO_SHORT",
            b"TF_ERR_MMR_SUCCESSOR_PATH_TOO_LONG", b"TF_ERR_MMR_DIFFERENT_SHARED_PEAK", b"TF_ERR_MMR_DIFFERENT_UNSHARED_PEAK"]
    assert [lib.tf_status_string(c) for c in range(27, 34)] == want
    assert lib.tf_status_string(26) == b"TF_ERR_UPPER_BOUND_NOT_POWER_OF_TWO" and lib.tf_status_string(34) == b"TF_ERR_UNKNOWN"
    header = open(os.path.join(ROOT, "include", "tf_hip.h")).read()
    for code, name in zip(range(27, 34), want):
        assert re.search(rf"\b{name.decode()} = {code}\b", header), name


@pytest.mark.parametrize("dev", [False, True])
@pytest.mark.parametrize("n", [1, 2, 3, 7, 8, 21, 42])
def test_sizing_call_writes_offsets_and_flags(tf, n, dev):
    """out_offsets and modified are arithmetic on (leaf index, old count, new count): no pointer to a digest is needed for them."""
    lib = tf.lib()
    fn, extra = (lib.tf_mmr_update_proofs_from_append_dev, (None,)) if dev else (lib.tf_mmr_update_proofs_from_append, ())
    idx = np.array(list(range(n)) + [0, n - 1], dtype=np.uint64)  # every leaf, two of them twice
    old_len = [(int(i) ^ n).bit_length() - 1 for i in idx]
    off = np.zeros(idx.size + 1, dtype=np.uint64)
    off[1:] = np.cumsum(old_len)
    for k in (0, 1, 2, 5, 8, 64):
        new_len = [max(a, ((int(i) ^ (n + k)).bit_length() - 1)) for i, a in zip(idx, old_len)]
        assert new_len == [(int(i) ^ (n + k)).bit_length() - 1 for i in idx]  # (the old path is a prefix: the length never shrinks)
        out_off = np.full(idx.size + 1, 99, dtype=np.uint64)
        mod = np.full(idx.size, 7, dtype=np.int32)
        assert fn(u64(n), None, None, k, idx.size, _p(idx), _p(off), None, _p(out_off), None, 0, _p(mod), None, *extra) == 0
        assert out_off.tolist() == [0] + np.cumsum(new_len).tolist(), (n, k)
        assert mod.tolist() == [int(b > a) for a, b in zip(old_len, new_len)], (n, k)
        # modified may be NULL
        out_off[:] = 99
        assert fn(u64(n), None, None, k, idx.size, _p(idx), _p(off), None, _p(out_off), None, 0, None, None, *extra) == 0
        assert out_off.tolist() == [0] + np.cumsum(new_len).tolist()


def test_argument_errors_precede_any_device_work(tf):
    lib = tf.lib()
    d = np.zeros(64 * 5, dtype=np.uint64)
    st = np.zeros(4, dtype=np.int32)
    big = (1 << 63) + 1
    # ---- tf_mmr_successor_proof_new
    for fn, extra in ((lib.tf_mmr_successor_proof_new, ()), (lib.tf_mmr_successor_proof_new_dev, (None,))):
        assert fn(u64(big), _p(d), _p(d), 1, _p(d), _p(d), *extra) == INVALID
        assert fn(u64(1 << 63), _p(d), _p(d), 1, _p(d), _p(d), *extra) == INVALID  # 2^63 + 1 after the append
        assert fn(u64(big), None, None, 1, None, None, *extra) == INVALID  # the count comes first
        assert fn(u64(1), None, _p(d), 1, None, None, *extra) == NULL  # one digest, no paths_out
        assert fn(u64(1), None, None, 1, _p(d), None, *extra) == NULL  # no leafs
        assert fn(u64(1), None, _p(d), 1, _p(d), _p(d), *extra) == NULL  # new_peaks wanted, no old_peaks
        assert fn(u64(8), None, None, 3, None, None, *extra) == 0  # an empty proof and nothing else asked for: no pointer is needed
        assert fn(u64(0), None, None, 0, None, None, *extra) == 0
    # ---- tf_mmr_verify_successor_proofs
    one, two, off = np.array([1], dtype=np.uint64), np.array([2], dtype=np.uint64), np.array([0, 1], dtype=np.uint64)
    zero, dec = np.array([0, 0], dtype=np.uint64), np.array([2, 1], dtype=np.uint64)
    huge = np.array([big], dtype=np.uint64)
    for fn, extra in ((lib.tf_mmr_verify_successor_proofs, ()), (lib.tf_mmr_verify_successor_proofs_dev, (None,))):
        assert fn(0, None, None, None, None, None, None, None, None, None, *extra) == 0
        assert fn(1, None, _p(two), _p(off), _p(d), _p(off), _p(d), _p(zero), _p(d), _p(st), *extra) == NULL
        assert fn(1, _p(one), _p(two), _p(off), _p(d), _p(off), _p(d), None, _p(d), _p(st), *extra) == NULL
        assert fn(1, _p(one), _p(two), _p(off), _p(d), _p(off), _p(d), _p(zero), _p(d), None, *extra) == NULL
        assert fn(1, _p(huge), _p(two), _p(off), _p(d), _p(off), _p(d), _p(zero), _p(d), _p(st), *extra) == INVALID
        assert fn(1, _p(one), _p(huge), _p(off), _p(d), _p(off), _p(d), _p(zero), _p(d), _p(st), *extra) == INVALID
        for bad in range(3):
            offs = [off, off, zero]
            offs[bad] = dec
            assert fn(1, _p(one), _p(two), _p(offs[0]), _p(d), _p(offs[1]), _p(d), _p(offs[2]), _p(d), _p(st), *extra) == INVALID
        assert fn(1, _p(huge), _p(two), _p(dec), None, _p(off), _p(d), _p(zero), _p(d), _p(st), *extra) == INVALID  # counts and offsets before pointers
        assert fn(1, _p(one), _p(two), _p(off), None, _p(off), _p(d), _p(zero), _p(d), _p(st), *extra) == NULL
        assert fn(1, _p(one), _p(two), _p(off), _p(d), _p(off), None, _p(zero), _p(d), _p(st), *extra) == NULL
        assert fn(1, _p(one), _p(two), _p(off), _p(d), _p(off), _p(d), _p(off), None, _p(st), *extra) == NULL
    # ---- tf_mmr_update_proofs_from_append: count, host arrays, leaf index, path length, offsets -- in that order
    idx = np.array([0, 5], dtype=np.uint64)  # in an MMR of 6 leafs: peaks of height 2 and 1
    good = np.array([0, 2, 3], dtype=np.uint64)
    out_off = np.zeros(3, dtype=np.uint64)
    for fn, extra in ((lib.tf_mmr_update_proofs_from_append, ()), (lib.tf_mmr_update_proofs_from_append_dev, (None,))):
        args = lambda n, i, o, oo=out_off: (u64(n), _p(d), _p(d), 1, 2, None if i is None else _p(i), None if o is None else _p(o), _p(d),
                                            None if oo is None else _p(oo), _p(d), 64, None, None) + extra
        assert fn(*args(big, idx, good)) == INVALID
        assert fn(*args(1 << 63, idx, good)) == INVALID
        assert fn(*args(big, None, None, None)) == INVALID  # the count comes first
        assert fn(*args(6, None, good)) == NULL
        assert fn(*args(6, idx, None)) == NULL
        assert fn(*args(6, idx, good, None)) == NULL
        assert fn(*args(6, np.array([0, 6], dtype=np.uint64), good)) == LEAF
        assert fn(*args(5, idx, good)) == LEAF
        assert fn(*args(6, np.array([0, 6], dtype=np.uint64), np.array([0, 1, 3], dtype=np.uint64))) == LEAF  # the index before the length
        assert fn(*args(6, idx, np.array([0, 1, 2], dtype=np.uint64))) == PATH_LEN
        assert fn(*args(6, idx, np.array([0, 2, 5], dtype=np.uint64))) == PATH_LEN
        assert fn(*args(6, idx, np.array([3, 2, 3], dtype=np.uint64))) == INVALID
        assert fn(*args(6, idx, np.array([3, 2, 5], dtype=np.uint64))) == PATH_LEN  # a wrong length before a decreasing offset
        # a capacity that is too small, decided before any pointer is read
        assert fn(u64(6), None, None, 1, 2, _p(idx), _p(good), None, _p(out_off), _p(d), 2, None, None, *extra) == TOO_SMALL
        assert out_off.tolist() == [0, 2, 3]
        # an empty call
        assert fn(u64(0), None, None, 0, 0, None, None, None, _p(out_off), None, 0, None, None, *extra) == 0 and out_off[0] == 0
        assert fn(u64(0), None, None, 0, 0, None, None, None, None, None, 0, None, None, *extra) == NULL


def test_header_signatures_and_exports_stay_in_step(tf):
    header = open(os.path.join(ROOT, "include", "tf_hip.h")).read()
    abi = open(os.path.join(ROOT, "twenty-first_amd", "csrc", "tf_abi.hip")).read()
    for name in NAMES:
        m = re.search(rf"^(?:int|size_t) {name}\((.*?)\);", header, flags=re.M | re.S)
        assert m, name
        assert len(m.group(1).split(",")) == len(tf._lib.SIGNATURES[name][1]), name
        assert re.search(rf"^(?:int|size_t) {name}\(", abi, flags=re.M), name
        assert hasattr(tf.lib(), name), name
    assert tf._lib.SIGNATURES["tf_mmr_successor_proof_len"][0] is C.c_size_t
    nm = shutil.which("nm")
    if nm:
        exported = {ln.split()[-1] for ln in subprocess.check_output([nm, "-D", "--defined-only", tf._lib.SO_PATH], text=True).splitlines() if ln.strip()}
        assert set(NAMES) <= exported
    for doc in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        text = open(os.path.join(ROOT, doc)).read()
        for name in ("tf_mmr_successor_proof_new", "tf_mmr_verify_successor_proofs", "tf_mmr_update_proofs_from_append"):
            assert name in text, (doc, name)


def test_python_front_rejects_mismatched_lists(tf):
    with pytest.raises(ValueError):
        tf.MmrMembershipProof.batch_update_from_append_many([tf.MmrMembershipProof(np.zeros((0, 5), dtype=np.uint64))], [], 1,
                                                            np.zeros((1, 5), dtype=np.uint64), np.zeros((1, 5), dtype=np.uint64))
    with pytest.raises(ValueError):
        tf.MmrSuccessorProof.verify_status_batch([tf.MmrSuccessorProof(np.zeros((0, 5), dtype=np.uint64))], [], [])
    with pytest.raises(ValueError):
        tf.MmrSuccessorProof.new_from_batch_append(tf.MmrAccumulator(1 << 63, np.zeros((1, 5), dtype=np.uint64)), np.zeros((1, 5), dtype=np.uint64))


def test_cpp_mirror_self_test_compiles_and_runs():
    """twenty-first_amd/host/mmr_successor_selftest.cpp builds against the header and the library; without a device it reports the skip
    (77), with one it passes (0)."""
    if shutil.which("make") is None or shutil.which(os.environ.get("CXX", "g++")) is None:
        pytest.skip("no C++ toolchain")
    host = os.path.join(ROOT, "twenty-first_amd", "host")
    subprocess.check_call(["make", "-C", host, "mmr_successor_selftest"], stdout=subprocess.DEVNULL)
    rc = subprocess.run([os.path.join(host, "mmr_successor_selftest")], capture_output=True, timeout=300).returncode
    assert rc in (0, 77)
