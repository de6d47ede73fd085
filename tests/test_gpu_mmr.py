"""Merkle Mountain Range accumulators and membership proofs on the GPU (util_types/mmr/), word for word against a short Python
restatement built on the oracle's hash_pair / hash_10 / merkle_build (pinned by the reference's known-answer vectors)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

OK, OUT_OF_RANGE, PEAK_COUNT, PATH_LEN, PEAK = 0, 22, 23, 24, 25


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(tf):
    assert tf.lib().tf_device_count() > 0, "no HIP device visible: the product has no CPU fallback"


def rand_digests(rng, n):
    return rng.integers(0, 0xFFFFFFFF00000001, size=(n, 5), dtype=np.uint64)


# ------------------------------------------------------------------ the model
def popcount(x):
    return bin(x).count("1")


def model_peaks(oracle, leafs):
    """new_from_leafs: one Merkle tree per set bit of the count, highest first."""
    leafs = np.asarray(leafs, dtype=np.uint64).reshape(-1, 5)
    n, peaks, start = leafs.shape[0], [], 0
    for h in range(63, -1, -1):
        if (n >> h) & 1:
            chunk = leafs[start: start + (1 << h)]
            peaks.append(chunk[0] if h == 0 else oracle.merkle_build(chunk, threads=16).reshape(-1, 5)[1])
            start += 1 << h
    return np.array(peaks, dtype=np.uint64).reshape(-1, 5)


def model_append(oracle, n, peaks, leaf):
    """calculate_new_peaks_from_append (shared_basic.rs:75-105)."""
    peaks = [p for p in np.asarray(peaks, dtype=np.uint64).reshape(-1, 5)] + [np.asarray(leaf, dtype=np.uint64)]
    path = []
    while n & 1:
        right, left = peaks.pop(), peaks.pop()
        path.append(left)
        peaks.append(oracle.hash_pair(left, right))
        n >>= 1
    return np.array(peaks, dtype=np.uint64).reshape(-1, 5), np.array(path, dtype=np.uint64).reshape(-1, 5)


def honest_proofs(oracle, leafs):
    """The membership proof of every leaf, from the peak trees."""
    leafs = np.asarray(leafs, dtype=np.uint64).reshape(-1, 5)
    n, out, start = leafs.shape[0], [], 0
    for h in range(63, -1, -1):
        if (n >> h) & 1:
            nodes = oracle.merkle_build(leafs[start: start + (1 << h)]).reshape(-1, 5) if h else None
            for i in range(1 << h):
                out.append(np.array([nodes[(((1 << h) + i) >> lv) ^ 1] for lv in range(h)], dtype=np.uint64).reshape(-1, 5))
            start += 1 << h
    return out


def model_verify(oracle, idx, leaf, path, peaks, n, m):
    if idx >= n:
        return OUT_OF_RANGE
    mt, pk = m.leaf_index_to_mt_index_and_peak_index(idx, n)
    if popcount(n) != len(peaks):
        return PEAK_COUNT
    if mt.bit_length() - 1 != len(path):
        return PATH_LEN
    acc = np.asarray(leaf, dtype=np.uint64)
    for sib in path:
        acc = oracle.hash_pair(acc, sib) if mt % 2 == 0 else oracle.hash_pair(sib, acc)
        mt //= 2
    return OK if np.array_equal(np.asarray(peaks[pk]), acc) else PEAK


def model_mutate(oracle, m, peaks, n, own_paths, own_idx, mutations):
    """batch_mutate_leaf_and_update_mps (mmr_accumulator.rs:180-302) line by line; peaks None: batch_update_from_batch_leaf_mutation."""
    peaks = None if peaks is None else [np.array(p) for p in peaks]
    new = {}
    for leaf_index, new_leaf, path in reversed(mutations):
        node = m.leaf_index_to_node_index(leaf_index)
        assert node not in new
        new[node] = new_leaf
        acc = new_leaf
        for count, h in enumerate(path):
            rc, height = m.right_lineage_length_and_own_height(node)
            if rc != 0:
                acc = oracle.hash_pair(new.get(m.left_sibling(node, height), h), acc)
                node += 1
            else:
                acc = oracle.hash_pair(acc, new.get(m.right_sibling(node, height), h))
                node += 1 << (height + 1)
            if count < len(path) - 1:
                new[node] = acc
        if peaks is not None:
            peaks[m.leaf_index_to_mt_index_and_peak_index(leaf_index, n)[1]] = acc
    paths, flags = [], []
    for path, i in zip(own_paths, own_idx):
        path = [np.array(d) for d in path]
        flag = False
        for e, node in enumerate(m.membership_proof_node_indices(i, len(path))):
            if node in new and not np.array_equal(path[e], new[node]):
                path[e] = new[node]
                flag = True
        paths.append(np.array(path, dtype=np.uint64).reshape(-1, 5))
        flags.append(flag)
    return (None if peaks is None else np.array(peaks, dtype=np.uint64).reshape(-1, 5)), paths, flags


# ------------------------------------------------------------------ bag_peaks
def test_bag_peaks_of_the_empty_accumulator_is_the_reference_snapshot(tf):
    acc = tf.MmrAccumulator.new_from_leafs(np.zeros((0, 5), dtype=np.uint64))
    assert tf.Digest.to_hex(acc.bag_peaks()) == "cd65052100640f0d27e5654f97c47e49899add2f265967ccbefee7264e9bc08f588542d9dc3d5ac5"


def test_bag_peaks_batch(tf, oracle):
    rng = np.random.default_rng(1)
    counts = [0, 1, 2, 3, 7, 8, 1000, (1 << 32) - 1, 1 << 32, (1 << 40) + 12345, (1 << 63) - 1, 1 << 63] + \
        [int(x) for x in rng.integers(0, 1 << 62, size=300, dtype=np.uint64)]
    peaks = [rand_digests(rng, popcount(c)) for c in counts]
    got = tf.bag_peaks_batch(counts, np.concatenate(peaks))
    for c, p, g in zip(counts, peaks, got):
        acc = oracle.hash_10(np.array([oracle.bfe_new(c & 0xFFFFFFFF), oracle.bfe_new(c >> 32)] + [0] * 8, dtype=np.uint64))
        for d in p[::-1]:
            acc = oracle.hash_pair(d, acc)
        assert np.array_equal(g, acc), c


# ------------------------------------------------------------------ build / append
@pytest.mark.parametrize("n", list(range(0, 71)) + [(1 << k) + d for k in range(7, 21) for d in (-1, 0, 1)])
def test_new_from_leafs(tf, oracle, n):
    rng = np.random.default_rng(n)
    leafs = rand_digests(rng, n)
    acc = tf.MmrAccumulator.new_from_leafs(leafs)
    assert acc.num_leafs() == n
    assert np.array_equal(acc.peaks(), model_peaks(oracle, leafs))


def test_new_from_leafs_2_24_minus_1(tf, oracle):
    n = (1 << 24) - 1
    leafs = np.asarray(oracle.fill_random(5 * n, 77), dtype=np.uint64).reshape(-1, 5)
    acc = tf.MmrAccumulator.new_from_leafs(leafs)
    assert np.array_equal(acc.peaks(), model_peaks(oracle, leafs))


@pytest.mark.parametrize("n,k", [(0, 0), (0, 1), (0, 5), (1, 1), (1, 6), (3, 1), (3, 13), (5, 0), (6, 2), (7, 1), (7, 9), (12, 20),
                                 (31, 33), (64, 64), (100, 157), (255, 1), (1000, 300)])
def test_append_many_with_proofs(tf, oracle, n, k):
    rng = np.random.default_rng(1000 * n + k)
    old = rand_digests(rng, n)
    acc = tf.MmrAccumulator.new_from_leafs(old)
    new = rand_digests(rng, k)
    proofs = acc.append_many(new)
    peaks = model_peaks(oracle, old)
    for i in range(k):
        peaks, path = model_append(oracle, n + i, peaks, new[i])
        assert np.array_equal(proofs[i].authentication_path, path), i
    assert acc.num_leafs() == n + k and np.array_equal(acc.peaks(), peaks)
    # every proof of the final accumulator verifies only in its own accumulator; the last one is valid now
    if k:
        assert proofs[-1].verify(n + k - 1, new[-1], acc.peaks(), n + k)


@pytest.mark.parametrize("n", [(1 << 40) - 3, (1 << 40) + 5, (1 << 63) - 40, (1 << 63) - 7])
def test_append_to_synthetic_large_accumulators(tf, oracle, n):
    rng = np.random.default_rng(n & 0xFFFF)
    k = min(37, (1 << 63) - n)
    old_peaks = rand_digests(rng, popcount(n))
    acc = tf.MmrAccumulator(n, old_peaks)
    new = rand_digests(rng, k)
    proofs = acc.append_many(new)
    peaks = old_peaks
    for i in range(k):
        peaks, path = model_append(oracle, n + i, peaks, new[i])
        assert np.array_equal(proofs[i].authentication_path, path), i
    assert np.array_equal(acc.peaks(), peaks)


# ------------------------------------------------------------------ verification
def test_honest_proofs_verify(tf, oracle):
    for n in (1, 2, 3, 7, 8, 13, 64, 100, 257):
        rng = np.random.default_rng(n)
        leafs = rand_digests(rng, n)
        peaks = model_peaks(oracle, leafs)
        proofs = [tf.MmrMembershipProof(p) for p in honest_proofs(oracle, leafs)]
        st = tf.MmrMembershipProof.verify_status_batch(proofs, np.arange(n), leafs, peaks, n)
        assert st.tolist() == [OK] * n


def test_failing_proofs_give_their_codes(tf, oracle):
    m = tf.mmr_index
    rng = np.random.default_rng(3)
    cases = []  # (leaf_count, peaks, idx, leaf, path)
    for n in (1, 5, 13, 100):
        leafs = rand_digests(rng, n)
        peaks = model_peaks(oracle, leafs)
        paths = honest_proofs(oracle, leafs)
        for i in range(0, n, max(1, n // 7)):
            cases.append((n, peaks, i, leafs[i], paths[i]))
            cases.append((n, peaks, n + i, leafs[i], paths[i]))                      # out of range
            cases.append((n, peaks[:-1], i, leafs[i], paths[i]))                     # one peak short
            cases.append((n, np.concatenate([peaks, peaks[:1]]), i, leafs[i], paths[i]))  # one peak too many
            cases.append((n, peaks, i, leafs[i], np.concatenate([paths[i], paths[i][:1] if len(paths[i]) else leafs[:1]])))
            if len(paths[i]):
                cases.append((n, peaks, i, leafs[i], paths[i][:-1]))
                bad = paths[i].copy()
                bad[rng.integers(len(bad)), rng.integers(5)] ^= np.uint64(1)
                cases.append((n, peaks, i, leafs[i], bad))
            bad_leaf = leafs[i].copy()
            bad_leaf[2] ^= np.uint64(1 << 20)
            cases.append((n, peaks, i, bad_leaf, paths[i]))
            bad_peaks = peaks.copy()
            bad_peaks[m.leaf_index_to_mt_index_and_peak_index(i, n)[1], 4] ^= np.uint64(7)
            cases.append((n, bad_peaks, i, leafs[i], paths[i]))
    # leaf_count = 2^63: one peak of height 63; paths of 63 random digests hashed up to synthetic peaks
    for i in (0, 12345, (1 << 63) - 1, 1 << 62):
        leaf, path = rand_digests(rng, 1)[0], rand_digests(rng, 63)
        acc = leaf
        for lv, sib in enumerate(path):
            acc = oracle.hash_pair(sib, acc) if (i >> lv) & 1 else oracle.hash_pair(acc, sib)
        cases.append((1 << 63, acc.reshape(1, 5), i, leaf, path))
        cases.append((1 << 63, acc.reshape(1, 5), i, leaf, path[:-1]))
        wrong = acc.copy()
        wrong[0] ^= np.uint64(1)
        cases.append((1 << 63, wrong.reshape(1, 5), i, leaf, path))
    seen = set()
    for n, peaks, i, leaf, path in cases:
        want = model_verify(oracle, i, leaf, path, peaks, n, m)
        got = tf.MmrMembershipProof.verify_status_batch([tf.MmrMembershipProof(path)], [i], leaf, peaks, n)[0]
        assert got == want, (n, i, len(path))
        seen.add(want)
    assert seen == {OK, OUT_OF_RANGE, PEAK_COUNT, PATH_LEN, PEAK}


def test_batched_verification_of_one_accumulator_matches_one_by_one(tf, oracle):
    """one call with ragged path lengths and mixed verdicts, against one call per proof"""
    rng = np.random.default_rng(11)
    n = 1000
    leafs = rand_digests(rng, n)
    peaks = model_peaks(oracle, leafs)
    paths = honest_proofs(oracle, leafs)
    idx = rng.integers(0, n + 20, size=500)
    proofs, digs, want = [], [], []
    for i in idx:
        i = int(i)
        path = paths[i % n].copy()
        leaf = leafs[i % n].copy()
        if rng.random() < 0.2 and len(path):
            path[rng.integers(len(path)), 0] ^= np.uint64(3)
        proofs.append(tf.MmrMembershipProof(path))
        digs.append(leaf)
        want.append(model_verify(oracle, i, leaf, path, peaks, n, tf.mmr_index))
    st = tf.MmrMembershipProof.verify_status_batch(proofs, idx.astype(np.uint64), np.array(digs), peaks, n)
    assert st.tolist() == want


# ------------------------------------------------------------------ batch mutation
def _setup(oracle, rng, n):
    leafs = rand_digests(rng, n)
    return leafs, model_peaks(oracle, leafs), honest_proofs(oracle, leafs)


@pytest.mark.parametrize("n,n_mut,n_own", [(1, 1, 1), (2, 1, 2), (7, 3, 7), (13, 5, 13), (100, 17, 40), (1000, 64, 200), (1023, 300, 100)])
def test_consistent_batch_mutation(tf, oracle, n, n_mut, n_own):
    m = tf.mmr_index
    rng = np.random.default_rng(n * 7 + n_mut)
    leafs, peaks, paths = _setup(oracle, rng, n)
    mut_idx = [int(x) for x in rng.choice(n, size=n_mut, replace=False)]
    own_idx = [int(x) for x in rng.choice(n, size=n_own, replace=n_own > n)]
    new_leafs = rand_digests(rng, n_mut)
    muts = [tf.LeafMutation(i, new_leafs[j], tf.MmrMembershipProof(paths[i])) for j, i in enumerate(mut_idx)]
    own = [tf.MmrMembershipProof(paths[i]) for i in own_idx]
    acc = tf.MmrAccumulator(n, peaks)
    flagged = acc.batch_mutate_leaf_and_update_mps(own, own_idx, muts)
    mutated = leafs.copy()
    for j, i in enumerate(mut_idx):
        mutated[i] = new_leafs[j]
    assert np.array_equal(acc.peaks(), model_peaks(oracle, mutated))
    assert tf.MmrMembershipProof.verify_batch(own, own_idx, mutated[own_idx], acc.peaks(), n).all()
    want_peaks, want_paths, want_flags = model_mutate(oracle, m, peaks, n, [paths[i] for i in own_idx], own_idx,
                                                      [(i, new_leafs[j], paths[i]) for j, i in enumerate(mut_idx)])
    assert flagged == [p for p, f in enumerate(want_flags) if f]
    assert all(np.array_equal(a.authentication_path, b) for a, b in zip(own, want_paths))


@pytest.mark.parametrize("with_peaks", [True, False])
def test_inconsistent_batch_mutation_is_the_reference_hashmap_loop(tf, oracle, with_peaks):
    m = tf.mmr_index
    for seed in range(6):
        rng = np.random.default_rng(100 + seed)
        n = int(rng.integers(20, 300))
        leafs, peaks, paths = _setup(oracle, rng, n)
        n_mut = int(rng.integers(1, 30))
        mut_idx = [int(x) for x in rng.choice(n, size=n_mut, replace=False)]
        muts = []
        for i in mut_idx:
            path = paths[i].copy()
            r = rng.random()
            if r < 0.25:  # stale: a random digest
                if len(path):
                    path[rng.integers(len(path))] = rand_digests(rng, 1)[0]
            elif r < 0.45:  # one digest short
                path = path[:-1]
            elif r < 0.6:  # too long
                path = np.concatenate([path, rand_digests(rng, int(rng.integers(1, 4)))])
            muts.append((i, rand_digests(rng, 1)[0], path))
        own_idx = [int(x) for x in rng.integers(0, n, size=40)]
        own_paths = []
        for i in own_idx:
            p = paths[i].copy()
            if rng.random() < 0.3:
                p = np.concatenate([p, rand_digests(rng, 2)]) if rng.random() < 0.5 else p[: max(0, len(p) - 2)]
            own_paths.append(p)
        want_peaks, want_paths, want_flags = model_mutate(oracle, m, peaks if with_peaks else None, n, own_paths, own_idx, muts)
        own = [tf.MmrMembershipProof(p) for p in own_paths]
        lm = [tf.LeafMutation(i, leaf, tf.MmrMembershipProof(p)) for i, leaf, p in muts]
        if with_peaks:
            acc = tf.MmrAccumulator(n, peaks)
            flagged = acc.batch_mutate_leaf_and_update_mps(own, own_idx, lm)
            assert np.array_equal(acc.peaks(), want_peaks), seed
        else:
            flagged = tf.MmrMembershipProof.batch_update_from_batch_leaf_mutation(own, own_idx, lm, n)
        assert flagged == [p for p, f in enumerate(want_flags) if f], seed
        assert all(np.array_equal(a.authentication_path, b) for a, b in zip(own, want_paths)), seed


def test_mutate_leaf(tf, oracle):
    rng = np.random.default_rng(9)
    leafs, peaks, paths = _setup(oracle, rng, 77)
    acc = tf.MmrAccumulator(77, peaks)
    new = rand_digests(rng, 1)[0]
    acc.mutate_leaf(tf.LeafMutation(40, new, tf.MmrMembershipProof(paths[40])))
    leafs[40] = new
    assert np.array_equal(acc.peaks(), model_peaks(oracle, leafs))


# ------------------------------------------------------------------ _dev forms
def _cuda(a):
    import torch

    a = np.ascontiguousarray(a, dtype=np.uint64).reshape(-1)
    return torch.from_numpy(a.view(np.int64).copy()).cuda() if a.size else torch.zeros(1, dtype=torch.int64, device="cuda")


def _host(t, words):
    return t.cpu().numpy().view(np.uint64)[:words]


def test_dev_forms_match_host_forms(tf, oracle):
    import torch

    rng = np.random.default_rng(21)
    n = 300
    leafs, peaks, paths = _setup(oracle, rng, n)
    # append
    new = rand_digests(rng, 50)
    acc = tf.MmrAccumulator(n, peaks)
    proofs = acc.append_many(new)
    words = sum(p.authentication_path.size for p in proofs)
    np_out = torch.zeros(5 * popcount(n + 50), dtype=torch.int64, device="cuda")
    pr_out = torch.zeros(max(words, 1), dtype=torch.int64, device="cuda")
    tf.device.mmr_append(n, _cuda(peaks), _cuda(new), np_out, pr_out)
    torch.cuda.synchronize()
    assert np.array_equal(_host(np_out, np_out.numel()).reshape(-1, 5), acc.peaks())
    assert np.array_equal(_host(pr_out, words), np.concatenate([p.authentication_path.reshape(-1) for p in proofs]))
    # bag
    counts = [n, 5, 0, 1 << 63]
    pk = np.concatenate([peaks, rand_digests(rng, 2), rand_digests(rng, 1)])
    out = torch.zeros(20, dtype=torch.int64, device="cuda")
    tf.device.mmr_bag_peaks(counts, _cuda(pk), out)
    torch.cuda.synchronize()
    assert np.array_equal(_host(out, 20).reshape(-1, 5), tf.bag_peaks_batch(counts, pk))
    # verify
    idx = np.array([0, 5, 299, 400], dtype=np.uint64)
    off = np.cumsum([0] + [len(paths[int(i) % n]) for i in idx]).astype(np.uint64)
    st = torch.full((4,), -1, dtype=torch.int32, device="cuda")
    tf.device.mmr_verify_membership_proofs(n, _cuda(peaks), _cuda(idx), _cuda(leafs[idx % n]), off,
                                           _cuda(np.concatenate([paths[int(i) % n] for i in idx])), st)
    torch.cuda.synchronize()
    assert st.cpu().tolist() == [OK, OK, OK, OUT_OF_RANGE]
    # mutate
    mut_idx, own_idx = [3, 100, 250], [3, 4, 101, 299]
    nl = rand_digests(rng, 3)
    mo = np.cumsum([0] + [len(paths[i]) for i in mut_idx]).astype(np.uint64)
    oo = np.cumsum([0] + [len(paths[i]) for i in own_idx]).astype(np.uint64)
    d_peaks, d_own = _cuda(peaks), _cuda(np.concatenate([paths[i] for i in own_idx]))
    mod = torch.full((4,), -1, dtype=torch.int32, device="cuda")
    tf.device.mmr_batch_mutate_leafs(n, d_peaks, mut_idx, _cuda(nl), mo, _cuda(np.concatenate([paths[i] for i in mut_idx])), own_idx, oo,
                                     d_own, mod)
    torch.cuda.synchronize()
    acc = tf.MmrAccumulator(n, peaks)
    own = [tf.MmrMembershipProof(paths[i]) for i in own_idx]
    flagged = acc.batch_mutate_leaf_and_update_mps(own, own_idx, [tf.LeafMutation(i, nl[j], tf.MmrMembershipProof(paths[i]))
                                                                   for j, i in enumerate(mut_idx)])
    assert np.array_equal(_host(d_peaks, peaks.size).reshape(-1, 5), acc.peaks())
    assert np.array_equal(_host(d_own, int(oo[-1]) * 5), np.concatenate([p.authentication_path.reshape(-1) for p in own]))
    assert [p for p, f in enumerate(mod.cpu().tolist()) if f] == flagged


def test_dev_call_does_not_block(tf, oracle):
    import torch

    rng = np.random.default_rng(5)
    n = 1 << 10
    leafs, peaks, paths = _setup(oracle, rng, n)
    idx = np.arange(0, n, 37, dtype=np.uint64)
    off = np.cumsum([0] + [len(paths[int(i)]) for i in idx]).astype(np.uint64)
    d_pk, d_idx, d_leaf = _cuda(peaks), _cuda(idx), _cuda(leafs[idx])
    d_paths = _cuda(np.concatenate([paths[int(i)] for i in idx]))
    st = torch.full((idx.size,), -1, dtype=torch.int32, device="cuda")
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        tf.device.mmr_verify_membership_proofs(n, d_pk, d_idx, d_leaf, off, d_paths, st, stream=s)  # warm-up
    s.synchronize()
    x = torch.zeros((1 << 22) * 16, dtype=torch.int64, device="cuda")
    st.fill_(-1)
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(8):
            tf.device.ntt_(x, 1 << 22, batch=16, stream=s)
        tf.device.mmr_verify_membership_proofs(n, d_pk, d_idx, d_leaf, off, d_paths, st, stream=s)
        busy = not s.query()
    s.synchronize()
    assert busy, "the verify call waited for the stream"
    assert st.cpu().tolist() == [OK] * idx.size
    del x
