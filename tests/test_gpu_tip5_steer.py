"""Every Tip5 kernel form on the inputs of tests/tip5_steer.py, which take the rare carry and lazy-word paths of the hand-written
reductions in every round at every output word (tests/test_tip5_steer_cpu.py holds the set to that), bit-exact against the oracle.

Launch sizes: a batch entry point runs the row pair up to 8 chains per compute unit, the 16-lane form up to 2^13, the matrix pipe
above; every call below runs on both sides of both switches.  The counts come from windows of the state set that start at different
offsets and wrap around, so a state visits several chain positions of a workgroup and several columns of a wave, and the last
workgroup / wave of most launches is ragged.  Expected words are computed once per distinct state."""
import numpy as np
import pytest

from tests import tip5_steer as ts

pytestmark = pytest.mark.gpu

P = ts.P
COOP_MAX = 1 << 13


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(tf):
    assert tf.lib().tf_device_count() > 0, "no HIP device visible: the product has no CPU fallback"


@pytest.fixture(scope="module")
def pair_max():
    import torch

    n = 8 * torch.cuda.get_device_properties(0).multi_processor_count
    assert 16 < n < COOP_MAX - 16
    return n


@pytest.fixture(scope="module")
def steered(oracle):
    """S as an (n, 16) array, its classes, and the oracle's trace of every state (n, 6, 16)"""
    states, classes = ts.steered_states()
    s = np.array(states, dtype=np.uint64)
    tr = np.empty((len(states), 6, 16), dtype=np.uint64)
    for i in range(len(states)):
        t, after = oracle.tip5_trace(s[i].copy())
        tr[i] = np.asarray(t).reshape(6, 16)
        assert np.array_equal(tr[i, 5], after)
    s.setflags(write=False)
    tr.setflags(write=False)
    return s, classes, tr


@pytest.fixture(scope="module")
def fixed(oracle):
    """{cap: (H as an (n, 10) array, its classes)}, and for cap = 1 the digests oracle.hash_pairs gives"""
    out = {}
    for cap in (0, 1):
        inputs, classes = ts.fixed_inputs(cap)
        h = np.array(inputs, dtype=np.uint64)
        h.setflags(write=False)
        out[cap] = (h, classes)
    digests = oracle.hash_pairs(out[1][0].reshape(-1).copy()).reshape(-1, 5)
    digests.setflags(write=False)
    return out, digests


def window(n, start, count):
    """indices of `count` consecutive states of a set of n, from `start`, wrapping around"""
    return (start + np.arange(count)) % n


def plans(n, pair_max):
    """{form: [index arrays]}: every state in every form, at several positions, on both sides of both switches"""
    pair = [window(n, start - o, pair_max) for o in (0, 5) for start in range(0, n, pair_max)] + [window(n, 11, 1), window(n, 3, pair_max - 3)]
    lanes = [window(n, 0, pair_max + 1), window(n, -3, min(COOP_MAX, max(n, pair_max + 1))), window(n, -9, COOP_MAX)]
    mx = [window(n, 0, COOP_MAX + 1), window(n, -6, max(3 * n, COOP_MAX + 16) + 5)]
    for idx in lanes + mx:
        assert idx.size < n or len(set(idx.tolist())) == n
    assert all(i.size <= pair_max for i in pair) and all(pair_max < i.size <= COOP_MAX for i in lanes) and all(i.size > COOP_MAX for i in mx)
    assert len(set(np.concatenate(pair).tolist())) == n and len(set(np.concatenate(lanes).tolist())) == n
    return {"row pair": pair, "16 lanes": lanes, "matrix pipe": mx}


def to_dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).reshape(-1).view(np.int64)).cuda()


def to_host(t):
    import torch

    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint64)


def explain(steered, i, word, form, r=None):
    """class and model events of state i for a failure message"""
    s, classes, tr = steered
    model = "coop" if form in ("row pair", "16 lanes") else "mx_trace" if form == "trace" else "mx"
    events, _ = ts.classify([int(v) for v in s[i]])
    if r is None:  # a final word: every round may have led to it
        ev = {rr: sorted(events[model][rr][word]) for rr in range(5) if events[model][rr][word] - {"none", "lazy none"}}
        return f"state {i} (class {classes[i]}), word {word}, {form} form; model events of this word by round: {ev or 'none'}"
    return (f"state {i} (class {classes[i]}), after round {r}, word {word}, {form} form; model event: {sorted(events[model][r][word])}; "
            f"events of the whole round: {[sorted(e) for e in events[model][r]]}")


def check_states(steered, idx, got, form, what):
    s, _, tr = steered
    got = got.reshape(-1, 16)
    want = tr[idx, 5]
    if not np.array_equal(got, want):
        k, word = np.argwhere(got != want)[0]
        raise AssertionError(f"{what}, launch of {idx.size}, position {k}: " + explain(steered, int(idx[k]), int(word), form))
    assert (got < np.uint64(P)).all(), f"{what}: a returned word is >= p"


# ------------------------------------------------------------------------------------------------ permutation and trace on S
@pytest.mark.parametrize("form", ["row pair", "16 lanes", "matrix pipe"])
def test_permutation_of_the_steered_states(tf, steered, pair_max, form):
    s = steered[0]
    for k, idx in enumerate(plans(len(s), pair_max)[form]):
        if k % 2:  # the device-resident call and the host call are the same kernels: alternate
            d = to_dev(s[idx])
            tf.device.tip5_permute_(d)
            got = to_host(d)
        else:
            got = s[idx].reshape(-1).copy()
            tf.Tip5.permute_states(got)
        check_states(steered, idx, got, form, "Tip5::permutation")


def test_trace_of_the_steered_states(tf, steered):
    """all six states of every permutation (the trace kernel makes every round canonical: mx_fold4_tail<true> in rounds 0..3 too)"""
    import torch

    s, _, tr = steered
    n = len(s)
    for idx in (window(n, 0, n), window(n, -7, n + 9), window(n, 4, 33)):
        d = to_dev(s[idx])
        out = torch.empty(idx.size * 96, dtype=torch.int64, device="cuda")
        tf.device.tip5_trace_(d, out)
        got = to_host(out).reshape(-1, 6, 16)
        if not np.array_equal(got, tr[idx]):
            k, r, word = np.argwhere(got != tr[idx])[0]
            raise AssertionError(f"Tip5::trace, launch of {idx.size}, position {k}: " + explain(steered, int(idx[k]), int(word), "trace", int(r) - 1))
        assert (got < np.uint64(P)).all()
        check_states(steered, idx, to_host(d), "trace", "Tip5::trace, the state it leaves")


# ------------------------------------------------------------------------------------------------ device-resident sponges on S
@pytest.mark.parametrize("form", ["row pair", "16 lanes", "matrix pipe"])
def test_sponge_squeeze_of_the_steered_states(tf, steered, pair_max, form):
    """squeeze, one block: the rate words come out, the state is permuted (mod.rs:693-698)"""
    import torch

    s = steered[0]
    for idx in plans(len(s), pair_max)[form]:
        d, out = to_dev(s[idx]), torch.zeros(idx.size * 10, dtype=torch.int64, device="cuda")
        tf.device.tip5_sponge_squeeze(d, out)
        assert np.array_equal(to_host(out).reshape(-1, 10), s[idx, :10])
        check_states(steered, idx, to_host(d), form, "Sponge::squeeze")


@pytest.mark.parametrize("form", ["row pair", "16 lanes", "matrix pipe"])
def test_sponge_absorb_into_the_steered_states(tf, steered, pair_max, form):
    """absorb, one chunk: a sponge that holds the capacity of a steered state (and other rate words) absorbs that state's rate, so
    what is permuted is exactly the steered state (mod.rs:684-691)"""
    s = steered[0]
    for idx in plans(len(s), pair_max)[form]:
        before = s[idx].copy()
        before[:, :10] = s[(idx + 1) % len(s), :10]
        d = to_dev(before)
        tf.device.tip5_sponge_absorb_(d, to_dev(s[idx, :10]))
        check_states(steered, idx, to_host(d), form, "Sponge::absorb")


# ------------------------------------------------------------------------------------------------ fixed-capacity forms on H
def check_digests(got, want, idx, classes, what):
    got = got.reshape(-1, 5)
    assert (got < np.uint64(P)).all(), f"{what}: a returned word is >= p"
    if not np.array_equal(got, want):
        k, word = np.argwhere(got != want)[0]
        raise AssertionError(f"{what}, launch of {idx.size}, position {k}, digest word {word}: input {idx[k]} (class {classes[idx[k]]})")


@pytest.mark.parametrize("form", ["row pair", "16 lanes", "matrix pipe"])
def test_hash_pairs_of_the_fixed_inputs(tf, fixed, pair_max, form):
    """capacity words 1: hash_10 / hash_pair; in the matrix pipe round 0 runs with the cf starts (tip5_permutation_mx_fixed)"""
    (h, classes), digests = fixed[0][1], fixed[1]
    for idx in plans(len(h), pair_max)[form]:
        check_digests(tf.Tip5.hash_pairs(h[idx].reshape(-1).copy()), digests[idx], idx, classes, "Tip5::hash_pair")


@pytest.mark.parametrize("row_len", [10, 20])
@pytest.mark.parametrize("form", ["row pair", "16 lanes", "matrix pipe"])
def test_hash_varlen_rows_of_the_fixed_inputs(tf, oracle, fixed, pair_max, form, row_len):
    """capacity words 0: the first permutation of hash_varlen absorbs the steered ten words (cz starts in the matrix pipe); row_len 20
    puts a generic permutation between it and the padding block"""
    h, classes = fixed[0][0]
    rows = h if row_len == 10 else np.concatenate([h, np.roll(h, 1, axis=0)], axis=1)
    want = oracle.hash_varlen_rows(rows.reshape(-1).copy(), row_len).reshape(-1, 5)
    for idx in plans(len(h), pair_max)[form]:
        check_digests(tf.Tip5.hash_varlen_rows(rows[idx].reshape(-1).copy(), row_len), want[idx], idx, classes, f"Tip5::hash_varlen, {row_len} words")


def test_hash_table_rows_of_the_fixed_inputs(tf, oracle, fixed):
    """the same rows as the columns of a column-major table, at a matrix-pipe size"""
    h, classes = fixed[0][0]
    idx = window(len(h), -2, COOP_MAX + len(h) + 3)
    want = oracle.hash_varlen_rows(h.reshape(-1).copy(), 10).reshape(-1, 5)
    got = tf.Tip5.hash_table_rows(np.ascontiguousarray(h[idx].T), idx.size)
    check_digests(got, want[idx], idx, classes, "Tip5::hash_varlen of table rows")


# ------------------------------------------------------------------------------------------------ trees: H as sibling pairs of leafs
def leafs_of(fixed, start, pairs):
    """2 * pairs leaf digests whose sibling pairs are the cap-1 inputs window(start, pairs)"""
    h = fixed[0][1][0]
    return h[window(len(h), start, pairs)].reshape(2 * pairs, 5).copy()


def oracle_trees(oracle, leafs, n):
    return np.stack([oracle.merkle_build(np.ascontiguousarray(t)).reshape(2 * n, 5) for t in leafs.reshape(-1, n, 5)])


def check_nodes(got, want, what):
    assert (got < np.uint64(P)).all(), f"{what}: a returned word is >= p"
    if not np.array_equal(got, want):
        t, node, word = np.argwhere(got != want)[0]
        raise AssertionError(f"{what}: tree {t}, node {node} (of {want.shape[1]}), word {word}")


@pytest.mark.parametrize("n,batch,what", [(2048, 9, "the level sweep in the matrix pipe"), (2048, 1, "the subtree kernel on 16 lanes"),
                                          (64, 32, "the top kernel on 16 lanes"), (16, 74, "the top kernel on row pairs")])
def test_merkle_build_with_steered_sibling_pairs(tf, oracle, fixed, n, batch, what):
    """the leaf level of each way a tree is built: batch n / 2 pairs above 2^13 is a level sweep, a single tree of 2^11 leafs starts in
    merkle_subtree_kernel, trees of at most 64 leafs are one merkle_top_kernel launch (row pairs for 8 pairs per workgroup)"""
    leafs = leafs_of(fixed, 61 * batch, batch * n // 2)
    want = oracle_trees(oracle, leafs, n)
    check_nodes(tf.MerkleTree.build_batch(leafs.reshape(-1), n), want, what)
    roots = tf.MerkleTree.roots_batch(leafs.reshape(-1), n)
    assert np.array_equal(roots, want[:, 1]), what + " (roots only)"


@pytest.mark.parametrize("n,batch", [(2048, 1), (2048, 9)])
def test_auth_structure_from_leafs_with_steered_sibling_pairs(tf, oracle, fixed, n, batch):
    leafs = leafs_of(fixed, 17, batch * n // 2)
    want = oracle_trees(oracle, leafs, n)
    idx = np.array([0, 1, 2, 77, 600, 601, 1023, 1024, 2047], dtype=np.uint64)
    node_ids = oracle.auth_structure_indices(n, idx).astype(np.int64)
    got, roots = tf.MerkleTree.authentication_structure_from_leafs(leafs.reshape(-1), idx, batch=batch, with_root=True)
    assert np.array_equal(got.reshape(batch, -1, 5), want[:, node_ids]) and np.array_equal(roots.reshape(batch, 5), want[:, 1])
    assert (got < np.uint64(P)).all() and (roots < np.uint64(P)).all()


def test_inclusion_proofs_with_steered_sibling_pairs(tf, oracle, fixed):
    """one proof per left leaf: the first hash of its verification is hash_pair of a steered input"""
    n = 2048
    leafs = leafs_of(fixed, 0, n // 2)
    nodes = oracle_trees(oracle, leafs, n)[0]
    tree = tf.MerkleTree(nodes)
    proofs = [tree.inclusion_proof_for_leaf_indices([i]) for i in range(0, n, 2)]
    proofs.append(tree.inclusion_proof_for_leaf_indices(list(range(0, n, 2))))  # and all of them in one proof
    status = tf.MerkleTreeInclusionProof.try_verify_batch(proofs, np.tile(nodes[1], len(proofs)))
    assert not status.any(), f"proofs {np.flatnonzero(status).tolist()} fail with {sorted(set(status.tolist()))}"


def test_mmr_with_steered_sibling_pairs(tf, oracle, fixed):
    """new_from_leafs, append and membership-proof verification: the MMR kernels hash every pair in the matrix-pipe form with the cf
    starts at every size"""
    from tests.test_gpu_mmr import honest_proofs, model_append, model_peaks

    for pairs in (1024, 9 * 1024 + 3):  # one peak; peaks of 2^14, 2^11, 4 and 2 leafs
        leafs = leafs_of(fixed, 29, pairs)
        acc = tf.MmrAccumulator.new_from_leafs(leafs)
        assert np.array_equal(acc.peaks(), model_peaks(oracle, leafs)), pairs
        assert (acc.peaks() < np.uint64(P)).all()
    n = 2048
    leafs = leafs_of(fixed, 0, n // 2)
    acc = tf.MmrAccumulator.new_from_leafs(leafs[:n - 256])
    peaks = model_peaks(oracle, leafs[:n - 256])
    got_paths = acc.append_many(leafs[n - 256:])
    for i in range(256):
        peaks, path = model_append(oracle, n - 256 + i, peaks, leafs[n - 256 + i])
        assert np.array_equal(got_paths[i].authentication_path, path), i
    assert np.array_equal(acc.peaks(), peaks) and np.array_equal(peaks, model_peaks(oracle, leafs))
    paths = honest_proofs(oracle, leafs)
    proofs = [tf.MmrMembershipProof(paths[i]) for i in range(0, n, 2)]
    status = tf.MmrMembershipProof.verify_status_batch(proofs, np.arange(0, n, 2), leafs[0::2], peaks, n)
    assert not status.any(), f"proofs {np.flatnonzero(status).tolist()} fail with {sorted(set(status.tolist()))}"
