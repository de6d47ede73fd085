"""MMR successor proofs (util_types/mmr/mmr_successor_proof.rs) and membership proofs carried over appends
(MmrMembershipProof::batch_update_from_append, mmr_membership_proof.rs:224-331) on the GPU, word for word against short Python
restatements built on the oracle's hash_pair / merkle_build / hash_varlen.  Host forms and _dev forms, the latter on a side stream."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HOST = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "twenty-first_amd", "host")
OK, BUFFER_TOO_SMALL = 0, 13
INC_OLD, INC_NEW, OLD_MORE, TOO_SHORT, TOO_LONG, SHARED, UNSHARED = range(27, 34)
FORMS = ["host", "dev"]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(tf):
    assert tf.lib().tf_device_count() > 0, "no HIP device visible: the product has no CPU fallback"


def popcount(x):
    return bin(x).count("1")


def digests(x):
    return np.ascontiguousarray(x, dtype=np.uint64).reshape(-1, 5)


# ------------------------------------------------------------------ leafs and the honest structures, computed once
@functools.lru_cache(maxsize=None)
def random_leafs():
    return np.random.default_rng(20).integers(0, 0xFFFFFFFF00000001, size=(1 << 14, 5), dtype=np.uint64)


@functools.lru_cache(maxsize=None)
def numbered_leafs():
    """Tip5::hash(&i) of the reference's tests: the u64 encodes as [low word, high word]."""
    from oracle import tfo

    return np.array([tfo.hash_varlen([tfo.bfe_new(i), tfo.bfe_new(0)]) for i in range(64)], dtype=np.uint64)


def root(oracle, chunk):
    chunk = digests(chunk)
    return chunk[0] if chunk.shape[0] == 1 else oracle.merkle_build(chunk).reshape(-1, 5)[1]


def model_peaks(oracle, leafs):
    """new_from_leafs: one Merkle tree per set bit of the count, highest first."""
    leafs = digests(leafs)
    n, peaks, start = leafs.shape[0], [], 0
    for h in range(63, -1, -1):
        if (n >> h) & 1:
            peaks.append(root(oracle, leafs[start: start + (1 << h)]))
            start += 1 << h
    return digests(np.array(peaks, dtype=np.uint64))


@functools.lru_cache(maxsize=None)
def random_peaks(count):
    from oracle import tfo

    return model_peaks(tfo, random_leafs()[:count])


@functools.lru_cache(maxsize=None)
def honest_proofs(count):
    """The membership proof of every one of the first `count` random leafs, from the peak trees."""
    from oracle import tfo

    leafs, out, start = random_leafs()[:count], [], 0
    for h in range(63, -1, -1):
        if (count >> h) & 1:
            nodes = tfo.merkle_build(leafs[start: start + (1 << h)]).reshape(-1, 5) if h else None
            for i in range(1 << h):
                out.append(digests(np.array([nodes[(((1 << h) + i) >> lv) ^ 1] for lv in range(h)], dtype=np.uint64)))
            start += 1 << h
    return out


# ------------------------------------------------------------------ the models
def model_successor_new(oracle, m, n, new_leafs):
    """new_from_batch_append (:34-91): the roots of a run of subtrees of the new leafs, chosen by the bits of the Merkle tree index."""
    new_leafs = digests(new_leafs)
    k = new_leafs.shape[0]
    if n == 0:
        return digests([])
    lowest = (n & -n).bit_length() - 1
    if k < 1 << lowest:
        return digests([])
    mt, _ = m.leaf_index_to_mt_index_and_peak_index(n, n + k)
    new_peak_height = mt.bit_length() - 1
    mt >>= lowest
    paths, used = [root(oracle, new_leafs[: 1 << lowest])], 1 << lowest
    while mt > 1:
        if mt % 2 == 0:
            h = new_peak_height - (mt.bit_length() - 1)
            paths.append(root(oracle, new_leafs[used: used + (1 << h)]))
            used += 1 << h
        mt //= 2
    return digests(np.array(paths, dtype=np.uint64))


def model_verify(oracle, m, n, old, N, new, paths):
    """verify_internal (:142-223) line by line."""
    old, new, paths = list(digests(old)), list(digests(new)), list(digests(paths))
    if len(old) != popcount(n):
        return INC_OLD
    if len(new) != popcount(N):
        return INC_NEW
    path_is_empty = OK if not paths else TOO_LONG
    if n == 0:
        return path_is_empty
    if n == N:
        return path_is_empty if all(np.array_equal(a, b) for a, b in zip(old, new)) else SHARED
    if n > N:
        return OLD_MORE
    mt, unchanged = m.leaf_index_to_mt_index_and_peak_index(n, N)
    for _ in range(unchanged):
        if not np.array_equal(old.pop(0), new.pop(0)):
            return SHARED
    lowest = (n & -n).bit_length() - 1
    if N - n < 1 << lowest:
        return path_is_empty
    if not paths:
        return TOO_SHORT
    node = paths.pop(0)
    mt >>= lowest
    while mt > 1:
        if mt % 2 == 0:
            if not paths:
                return TOO_SHORT
            node = oracle.hash_pair(node, paths.pop(0))
        else:
            node = oracle.hash_pair(old.pop(), node)
        mt //= 2
    assert not old
    if paths:
        return TOO_LONG
    return OK if np.array_equal(node, new.pop(0)) else UNSHARED


def model_append(oracle, n, peaks, leaf):
    """calculate_new_peaks_from_append (shared_basic.rs:75-105)."""
    peaks = list(digests(peaks)) + [np.asarray(leaf, dtype=np.uint64)]
    while n & 1:
        right, left = peaks.pop(), peaks.pop()
        peaks.append(oracle.hash_pair(left, right))
        n >>= 1
    return digests(np.array(peaks, dtype=np.uint64))


def model_update_from_append(oracle, m, paths, indices, n, new_leaf, old_peaks):
    """batch_update_from_append (mmr_membership_proof.rs:224-331) line by line; paths: lists of digests, extended in place."""
    added = m.node_indices_added_by_append(n)
    if len(added) == 1:
        return []
    known = dict(zip(m.get_peak_heights_and_peak_node_indices(n)[1], digests(old_peaks)))
    acc = np.asarray(new_leaf, dtype=np.uint64)
    for count, (node, old_peak) in enumerate(zip(added, digests(old_peaks)[::-1])):
        known[node] = acc
        if count == len(added) - 2:
            break
        acc = oracle.hash_pair(old_peak, acc)
    modified, new_peak, node_count = [], added[-1], m.num_leafs_to_num_nodes(n + 1)
    for i, (path, leaf_index) in enumerate(zip(paths, indices)):
        peak = m.leaf_index_to_node_index(leaf_index)
        for _ in path:
            peak = m.parent(peak)
        if peak + (1 << (len(path) + 1)) not in added:
            continue
        modified.append(i)
        path.extend(known[x] for x in m.get_authentication_path_node_indices(peak, new_peak, node_count))
    return modified


# ------------------------------------------------------------------ both forms of every call
def _cuda(a):
    import torch

    a = np.ascontiguousarray(a, dtype=np.uint64).reshape(-1)
    return torch.from_numpy(a.view(np.int64).copy()).cuda() if a.size else torch.zeros(5, dtype=torch.int64, device="cuda")


def _back(t, n_digests):
    return t.cpu().numpy().view(np.uint64)[: 5 * n_digests].reshape(-1, 5)


def _side_stream():
    import torch

    torch.cuda.synchronize()  # the inputs were written on the default stream
    return torch.cuda.Stream()


def successor_new(tf, form, n, old_peaks, new_leafs, with_peaks=True):
    """-> (paths, new_peaks or None)"""
    new_leafs = digests(new_leafs)
    k = new_leafs.shape[0]
    length, n_new = tf.device.mmr_successor_proof_len(n, k), popcount(n + k)
    if form == "host":
        acc = tf.MmrAccumulator(n, old_peaks)
        proof = tf.MmrSuccessorProof.new_from_batch_append(acc, new_leafs)  # without the peaks: old_peaks is not even passed
        if not with_peaks:
            return proof.paths, None
        out, new = np.zeros(max(5 * length, 1), dtype=np.uint64), np.zeros(max(5 * n_new, 1), dtype=np.uint64)
        flat = np.ascontiguousarray(new_leafs.reshape(-1))
        p = lambda a: C.c_void_p(a.ctypes.data)
        assert tf.lib().tf_mmr_successor_proof_new(C.c_uint64(n), p(np.ascontiguousarray(digests(old_peaks).reshape(-1))) if n else None,
                                                   p(flat) if k else None, k, p(out), p(new)) == 0
        assert np.array_equal(out[: 5 * length].reshape(-1, 5), proof.paths)
        return proof.paths, new[: 5 * n_new].reshape(-1, 5)
    import torch

    d_out = torch.zeros(max(5 * length, 5), dtype=torch.int64, device="cuda")
    d_new = torch.zeros(max(5 * n_new, 5), dtype=torch.int64, device="cuda") if with_peaks else None
    d_old, d_leafs = _cuda(old_peaks) if with_peaks else None, _cuda(new_leafs)
    if k == 0:
        d_leafs = d_leafs[:0]
    s = _side_stream()
    assert tf.device.mmr_successor_proof_new(n, d_old, d_leafs, d_out, d_new, stream=s) == length
    s.synchronize()
    return _back(d_out, length), (_back(d_new, n_new) if with_peaks else None)


def verify_successors(tf, form, cases):
    """cases: (n, old peaks, N, new peaks, paths) -> statuses, all in ONE call"""
    if form == "host":
        return tf.MmrSuccessorProof.verify_status_batch([tf.MmrSuccessorProof(c[4]) for c in cases], [(c[0], c[1]) for c in cases],
                                                        [(c[2], c[3]) for c in cases]).tolist()
    import torch

    off = lambda col: np.concatenate([[0], np.cumsum([digests(c[col]).shape[0] for c in cases])]).astype(np.uint64)
    flat = lambda col: np.concatenate([digests(c[col]) for c in cases])
    st = torch.full((len(cases),), -1, dtype=torch.int32, device="cuda")
    d_old, d_new, d_paths = _cuda(flat(1)), _cuda(flat(3)), _cuda(flat(4))
    s = _side_stream()
    tf.device.mmr_verify_successor_proofs([c[0] for c in cases], [c[2] for c in cases], off(1), d_old, off(3), d_new, off(4), d_paths, st, stream=s)
    s.synchronize()
    return st.cpu().tolist()


def update_proofs(tf, form, n, old_peaks, new_leafs, indices, paths):
    """-> (updated paths, modified flags, new peaks)"""
    new_leafs, k = digests(new_leafs), digests(new_leafs).shape[0]
    if form == "host":
        proofs = [tf.MmrMembershipProof(p) for p in paths]
        grown = tf.MmrMembershipProof.batch_update_from_append_many(proofs, indices, n, new_leafs, old_peaks)
        acc = tf.MmrAccumulator(n, old_peaks)
        acc.append_many(new_leafs, proofs=False)
        flags = np.zeros(len(paths), dtype=np.int32)
        flags[grown] = 1
        return [p.authentication_path for p in proofs], flags.tolist(), acc.peaks()
    import torch

    own_off = np.concatenate([[0], np.cumsum([p.shape[0] for p in paths])]).astype(np.uint64)
    d_own, d_old, d_leafs = _cuda(np.concatenate(paths) if paths else []), _cuda(old_peaks), _cuda(new_leafs)
    out_off, _ = tf.device.mmr_update_proofs_from_append(n, d_old, d_leafs, indices, own_off, d_own)  # sizes
    d_out = torch.full((max(5 * int(out_off[-1]), 5),), -1, dtype=torch.int64, device="cuda")
    d_new = torch.zeros(5 * popcount(n + k), dtype=torch.int64, device="cuda")
    s = _side_stream()
    out_off2, mod = tf.device.mmr_update_proofs_from_append(n, d_old, d_leafs, indices, own_off, d_own, d_out, d_new, stream=s)
    s.synchronize()
    assert np.array_equal(out_off, out_off2)
    out = _back(d_out, int(out_off[-1]))
    return [out[int(a): int(b)] for a, b in zip(out_off[:-1], out_off[1:])], mod.tolist(), _back(d_new, popcount(n + k))


# ------------------------------------------------------------------ successor proofs: construction
@pytest.mark.parametrize("form", FORMS)
def test_the_reference_literal_42_plus_8(tf, oracle, form):
    leafs = numbered_leafs()
    old, new = model_peaks(oracle, leafs[:42]), model_peaks(oracle, leafs[:50])
    paths, peaks = successor_new(tf, form, 42, old, leafs[42:50])
    assert paths.shape == (2, 5)
    assert np.array_equal(paths[0], root(oracle, leafs[42:44])) and np.array_equal(paths[1], root(oracle, leafs[44:48]))
    assert np.array_equal(peaks, new)
    assert verify_successors(tf, form, [(42, old, 50, new, paths)]) == [OK]
    for n, k in ((8, 3), (0, 0), (0, 1)):
        assert successor_new(tf, form, n, model_peaks(oracle, leafs[:n]), leafs[n: n + k])[0].shape == (0, 5)


@pytest.mark.parametrize("form", FORMS)
def test_unit_tests_all_n_m_below_18(tf, oracle, form):
    """The reference's `unit_tests` (:385-392): proof and peaks against the model, then all 324 triples verified in one call."""
    leafs, m = numbered_leafs(), tf.mmr_index
    cases = []
    for n in range(18):
        old = model_peaks(oracle, leafs[:n])
        for k in range(18):
            paths, peaks = successor_new(tf, form, n, old, leafs[n: n + k], with_peaks=(n + k) % 3 != 1)
            assert np.array_equal(paths, model_successor_new(oracle, m, n, leafs[n: n + k])), (n, k)
            new = tf.MmrAccumulator(n, old)
            new.append_many(leafs[n: n + k], proofs=False)  # tf_mmr_append
            assert np.array_equal(new.peaks(), model_peaks(oracle, leafs[: n + k])), (n, k)
            if peaks is not None:
                assert np.array_equal(peaks, new.peaks()), (n, k)
            cases.append((n, old, n + k, new.peaks(), paths))
    assert len(cases) == 324
    assert verify_successors(tf, form, cases) == [OK] * 324
    assert [model_verify(oracle, m, *c) for c in cases[::7]] == [OK] * len(cases[::7])


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n,k", [((1 << 12) + (1 << 5) + 1, (1 << 13) + 77), (1 << 10, 1 << 10)])
def test_sweep_shapes(tf, oracle, form, n, k):
    """An odd count (the pair of level 1 that starts with an old peak), gaps between the peaks and both level buffers; and a proof of
    one digest whose every step takes an old peak."""
    leafs, m = random_leafs(), tf.mmr_index
    old = random_peaks(n)
    paths, peaks = successor_new(tf, form, n, old, leafs[n: n + k])
    assert np.array_equal(paths, model_successor_new(oracle, m, n, leafs[n: n + k]))
    assert paths.shape[0] == tf.device.mmr_successor_proof_len(n, k) >= 1
    if (n, k) == (1 << 10, 1 << 10):
        assert paths.shape[0] == 1
    new = tf.MmrAccumulator(n, old)
    new.append_many(leafs[n: n + k], proofs=False)
    assert np.array_equal(peaks, new.peaks()) and np.array_equal(peaks, random_peaks(n + k))
    assert np.array_equal(successor_new(tf, form, n, old, leafs[n: n + k], with_peaks=False)[0], paths)
    assert verify_successors(tf, form, [(n, old, n + k, peaks, paths)]) == [OK]


# ------------------------------------------------------------------ successor proofs: verification
def corrupt(d, i=0, w=2):
    d = digests(d).copy()
    d[i, w] ^= np.uint64(1)
    return d


def triple(oracle, m, n, k):
    """An honest (n, old peaks, N, new peaks, proof) of the random leafs."""
    leafs = random_leafs()
    return (n, random_peaks(n), n + k, random_peaks(n + k), model_successor_new(oracle, m, n, leafs[n: n + k]))


@pytest.mark.parametrize("form", FORMS)
def test_statuses_follow_verify_internal(tf, oracle, form):
    m = tf.mmr_index
    n, old, N, new, paths = triple(oracle, m, 42, 8)  # two digests, one shared peak
    n2, old2, N2, new2, paths2 = triple(oracle, m, 0b1000101, 0b1000000 - 0b101)  # 69 -> 128: five digests, three old peaks on the left
    assert paths.shape[0] == 2 and paths2.shape[0] == 5
    swapped_old = old[[0, 2, 1]]
    swapped_new = new[[1, 0, 2]]
    extra = np.concatenate([paths, paths[:1]])
    pinned = [
        ((n, old[:2], N, new, paths), INC_OLD),  # wrong old peak count
        ((n, np.concatenate([old, old[:1]]), N, new, paths), INC_OLD),
        ((n, old, N, new[:2], paths), INC_NEW),  # wrong new peak count
        ((n, old[:2], N, new[:2], paths), INC_OLD),  # old is looked at first
        ((N, new, n, old, paths), OLD_MORE),  # old and new swapped
        ((n, old, n, old, digests([])), OK),  # equal counts
        ((n, old, n, corrupt(old, 2), digests([])), SHARED),  # ... with one unequal peak
        ((n, old, n, old, paths[:1]), TOO_LONG),
        ((n, old, n, corrupt(old, 1), paths[:1]), SHARED),  # the peaks come before the length
        ((0, digests([]), N, new, digests([])), OK),  # anything succeeds the empty accumulator
        ((0, digests([]), N, new, paths[:1]), TOO_LONG),
        ((0, digests([]), 0, digests([]), digests([])), OK),
        ((n, swapped_old, N, new, paths), UNSHARED),  # two unshared old peaks swapped
        ((n, old, N, swapped_new, paths), SHARED),  # the first new peak is the shared one
        ((n, old, N, corrupt(new, 1), paths), UNSHARED),
        ((n, old, N, corrupt(new, 2), paths), OK),  # the new peaks after the first unshared one are not looked at
        ((n, old, N, new, paths[:1]), TOO_SHORT),  # one digest removed
        ((n, old, N, new, digests([])), TOO_SHORT),
        ((n, old, N, new, extra), TOO_LONG),  # one digest appended
        ((8, random_peaks(8), 11, random_peaks(11), paths[:1]), TOO_LONG),  # k < 2^t with a proof
        ((8, random_peaks(8), 11, random_peaks(11), digests([])), OK),
        ((8, corrupt(random_peaks(8)), 11, random_peaks(11), digests([])), SHARED),
        # the order-pinning pairs
        ((n, corrupt(old, 0), N, new, paths[:1]), SHARED),  # shared-peak mismatch and a wrong length
        ((n, corrupt(old, 0), N, new, extra), SHARED),
        ((n, old, N, new, corrupt(extra, 0)), TOO_LONG),  # too long and a corrupt digest
        ((n, old, N, new, corrupt(paths, 0)[:1]), TOO_SHORT),  # too short and a corrupt digest
        ((n2, old2, N2, new2, paths2), OK),
        ((n2, old2, N2, new2, paths2[:3]), TOO_SHORT),
    ]
    cases, want = [c for c, _ in pinned], [w for _, w in pinned]
    for c in ((n, old, N, new, paths), (n2, old2, N2, new2, paths2)):  # each path digest corrupted in turn, each word of it once
        for i in range(c[4].shape[0]):
            for w in range(5):
                cases.append(c[:4] + (corrupt(c[4], i, w),))
                want.append(UNSHARED)
    for i in range(old2.shape[0]):  # every old peak of the second triple is on the chain
        cases.append((n2, corrupt(old2, i, 4), N2, new2, paths2))
        want.append(UNSHARED)
    assert [model_verify(oracle, m, *c) for c in cases] == want
    assert verify_successors(tf, form, cases) == want


@pytest.mark.parametrize("form", FORMS)
def test_mixed_chain_lengths_land_at_their_own_index(tf, oracle, form):
    """Valid proofs of chain lengths 0..12 with invalid ones between them, ascending then descending: several waves, and the sort by
    length moves every chain."""
    m = tf.mmr_index
    valid = []
    for s in range(1, 13):
        valid.append(triple(oracle, m, (1 << s) - 1, 1))  # s steps, all old peaks
        valid.append(triple(oracle, m, (1 << (s - 1)) + 1, (1 << (s - 1)) - 1) if s > 1 else triple(oracle, m, 3, 1))  # path digests between two peaks
        valid.append(triple(oracle, m, (1 << s) + (1 << (s - 1)), 1 << (s - 1)))  # one step
        valid.append(triple(oracle, m, 1 << s, (1 << s) - 1))  # no chain: the new leafs do not fill the old peak's sibling
    valid += [triple(oracle, m, 0, 5), triple(oracle, m, 77, 0)]
    assert len(valid) >= 40
    steps = lambda c: 0 if c[0] in (0, c[2]) or c[4].shape[0] == 0 else (c[0] ^ c[2]).bit_length() - 1 - ((c[0] & -c[0]).bit_length() - 1)
    assert {steps(c) for c in valid} == set(range(13))
    valid.sort(key=steps)
    cases = []
    for i, c in enumerate(valid + valid[::-1]):
        cases.append(c)
        if i % 3 == 0 and c[4].shape[0]:
            cases.append((c[0], c[1], c[2], c[3], corrupt(c[4], c[4].shape[0] - 1, i % 5)))
        if i % 4 == 1 and c[0]:
            cases.append((c[0], c[1][:-1], c[2], c[3], c[4]))
        if i % 5 == 2 and c[0] != c[2]:
            cases.append((c[2], c[3], c[0], c[1], c[4]))
    want = [model_verify(oracle, m, *c) for c in cases]
    assert want.count(OK) >= 80 and {UNSHARED, INC_OLD, OLD_MORE} <= set(want) and len(cases) > 128
    assert verify_successors(tf, form, cases) == want


# ------------------------------------------------------------------ membership proofs under appends
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n", [1, 2, 3, 7, 8, 21, 42, 333])
def test_all_proofs_updated_in_one_call(tf, oracle, form, n):
    leafs = random_leafs()
    for k in (1, 2, 5, 8, 64, 300):
        got, flags, peaks = update_proofs(tf, form, n, random_peaks(n), leafs[n: n + k], np.arange(n), honest_proofs(n))
        want = honest_proofs(n + k)[:n]
        assert len(got) == n and all(np.array_equal(a, b) for a, b in zip(got, want)), (n, k)
        assert flags == [int(b.shape[0] > a.shape[0]) for a, b in zip(honest_proofs(n), want)], (n, k)
        assert np.array_equal(peaks, random_peaks(n + k)), (n, k)
        st = tf.MmrMembershipProof.verify_status_batch([tf.MmrMembershipProof(p) for p in got], np.arange(n), leafs[:n], peaks, n + k)
        assert st.tolist() == [OK] * n, (n, k)


@pytest.mark.parametrize("form", FORMS)
def test_against_the_literal_loop_of_update_and_append(tf, oracle, form):
    m, leafs = tf.mmr_index, random_leafs()
    for n in (1, 2, 3, 7, 8, 21):
        for k in (1, 2, 5, 8):
            paths, peaks, union = [list(p) for p in honest_proofs(n)], random_peaks(n), set()
            for j in range(k):
                union |= set(model_update_from_append(oracle, m, paths, range(n), n + j, leafs[n + j], peaks))
                peaks = model_append(oracle, n + j, peaks, leafs[n + j])
            got, flags, new_peaks = update_proofs(tf, form, n, random_peaks(n), leafs[n: n + k], np.arange(n), honest_proofs(n))
            assert all(np.array_equal(a, digests(np.array(b, dtype=np.uint64))) for a, b in zip(got, paths)), (n, k)
            assert {i for i, f in enumerate(flags) if f} == union, (n, k)
            assert np.array_equal(new_peaks, peaks), (n, k)


@pytest.mark.parametrize("form", FORMS)
def test_5000_proofs_with_repeated_indices(tf, oracle, form):
    n, k = 333, 300
    idx = np.random.default_rng(5).integers(0, n, size=5000).astype(np.uint64)
    idx[:4] = [0, n - 1, n - 1, 0]
    got, flags, _ = update_proofs(tf, form, n, random_peaks(n), random_leafs()[n: n + k], idx, [honest_proofs(n)[i] for i in idx])
    want = [honest_proofs(n + k)[i] for i in idx]
    assert np.array_equal(np.concatenate(got), np.concatenate(want))
    assert [g.shape[0] for g in got] == [w.shape[0] for w in want]
    assert flags == [int(honest_proofs(n + k)[i].shape[0] > honest_proofs(n)[i].shape[0]) for i in idx]


def test_sizing_then_a_capacity_that_is_too_small(tf, oracle):
    import torch

    n, k, lib = 21, 8, tf.lib()
    paths = honest_proofs(n)
    own_off = np.concatenate([[0], np.cumsum([p.shape[0] for p in paths])]).astype(np.uint64)
    idx = np.arange(n, dtype=np.uint64)
    d_own, d_old, d_leafs = _cuda(np.concatenate(paths)), _cuda(random_peaks(n)), _cuda(random_leafs()[n: n + k])
    out_off, mod = tf.device.mmr_update_proofs_from_append(n, d_old, d_leafs, idx, own_off, d_own)
    total = int(out_off[-1])
    assert total == sum(p.shape[0] for p in honest_proofs(n + k)[:n])
    assert mod.tolist() == [int(b.shape[0] > a.shape[0]) for a, b in zip(paths, honest_proofs(n + k))] and 0 < sum(mod.tolist()) < n
    d_out = torch.full((5 * total,), 0x5A5A, dtype=torch.int64, device="cuda")
    d_new = torch.full((5 * popcount(n + k),), 0x5A5A, dtype=torch.int64, device="cuda")
    p = lambda a: C.c_void_p(a.ctypes.data)
    d = lambda t: C.c_void_p(t.data_ptr())
    off2 = np.zeros(n + 1, dtype=np.uint64)
    rc = lib.tf_mmr_update_proofs_from_append_dev(C.c_uint64(n), d(d_old), d(d_leafs), k, n, p(idx), p(own_off), d(d_own), p(off2), d(d_out), total - 1,
                                                  None, d(d_new), None)
    torch.cuda.synchronize()
    assert rc == BUFFER_TOO_SMALL and np.array_equal(off2, out_off)
    assert bool((d_out == 0x5A5A).all()) and bool((d_new == 0x5A5A).all())
    rc = lib.tf_mmr_update_proofs_from_append_dev(C.c_uint64(n), d(d_old), d(d_leafs), k, n, p(idx), p(own_off), d(d_own), p(off2), d(d_out), total, None,
                                                  d(d_new), None)
    torch.cuda.synchronize()
    assert rc == 0 and np.array_equal(_back(d_out, total), np.concatenate(honest_proofs(n + k)[:n]))
    assert np.array_equal(_back(d_new, popcount(n + k)), random_peaks(n + k))


def test_append_is_unchanged_by_the_shared_sweep(tf, oracle):
    """tf_mmr_append runs through the sweep the new calls share: peaks and proofs of an odd count with gaps, against the model."""
    n, k, leafs = (1 << 7) + (1 << 3) + 1, 200, random_leafs()
    acc = tf.MmrAccumulator(n, random_peaks(n))
    proofs = acc.append_many(leafs[n: n + k])
    assert np.array_equal(acc.peaks(), random_peaks(n + k))
    assert np.array_equal(proofs[-1].authentication_path, honest_proofs(n + k)[n + k - 1])
    peaks = random_peaks(n)
    for i in range(k):
        assert proofs[i].authentication_path.shape[0] == tf.mmr_index.trailing_ones(n + i)
        peaks = model_append(oracle, n + i, peaks, leafs[n + i])
    assert np.array_equal(acc.peaks(), peaks)


def test_cpp_mirror_mmr_successor_selftest_on_gpu():
    subprocess.check_call(["make", "-C", HOST, "mmr_successor_selftest"], stdout=subprocess.DEVNULL)
    r = subprocess.run([os.path.join(HOST, "mmr_successor_selftest")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "mmr successor: PASS" in r.stdout, r.stdout + r.stderr
