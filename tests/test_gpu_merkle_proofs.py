"""Batched verification of Merkle inclusion proofs on the GPU (MerkleTreeInclusionProof, util_types/merkle_tree.rs:90-113, :683-931)
against a small, independent checker of the same semantics.

The checker follows the decision order of try_verify: trivial proof -> Ok; height >= 64 -> TreeTooHigh; a leaf index >= 2^h ->
LeafIndexInvalid; structure length != number of node indices the oracle's authentication_structure_node_indices returns ->
AuthenticationStructureLengthMismatch; a repeated leaf index with another digest -> RepeatedLeafDigestMismatch; then the partial tree
is filled level by level (every level's known nodes pair up into hash_pair inputs) and node 1 is compared with the root.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

OK, TOO_HIGH, LEAF_INVALID, LEN, REPEATED, ROOT = 0, 3, 11, 19, 20, 21


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(tf):
    assert tf.lib().tf_device_count() > 0, "no HIP device visible: the product has no CPU fallback"


# ------------------------------------------------------------------ the checker
def check(oracle, height, indices, digests, auth, root=None, paths=False):
    """-> (status, root or paths).  indices: leaf indices; digests: (k, 5); auth: (a, 5)."""
    indices = [int(i) for i in indices]
    digests = np.asarray(digests, dtype=np.uint64).reshape(-1, 5)
    auth = np.asarray(auth, dtype=np.uint64).reshape(-1, 5)
    if not paths and not indices and auth.shape[0] == 0:
        return OK, None
    if height >= 64:
        return TOO_HIGH, None
    n = 1 << height
    if any(i >= n for i in indices):
        return LEAF_INVALID, None
    node_ids = oracle.auth_structure_indices(n, np.array(indices, dtype=np.uint64)) if indices else np.zeros(0, dtype=np.uint64)
    if len(node_ids) != auth.shape[0]:
        return LEN, None
    known = {int(v): auth[j] for j, v in enumerate(node_ids)}
    for i, d in zip(indices, digests):
        if n + i in known:
            if not np.array_equal(known[n + i], d):
                return REPEATED, None
        else:
            known[n + i] = d
    if not indices:
        return OK, np.zeros((0, height, 5), dtype=np.uint64) if paths else None
    # level by level: the known nodes of a level (revealed / computed ones and structure digests) pair up as (2q, 2q + 1)
    level_ids = sorted({n + i for i in indices})
    for _ in range(height):
        sibs = sorted(set(level_ids) | {v ^ 1 for v in level_ids})
        ins = np.concatenate([known[v] for v in sibs])
        outs = oracle.hash_pairs(ins).reshape(-1, 5)
        level_ids = [sibs[2 * j] >> 1 for j in range(len(sibs) // 2)]
        for q, d in zip(level_ids, outs):
            known[q] = d
    if paths:
        return OK, np.array([[known[((n + i) >> lv) ^ 1] for lv in range(height)] for i in indices], dtype=np.uint64).reshape(len(indices), height, 5)
    got = known[1]
    return (OK if root is None or np.array_equal(got, np.asarray(root, dtype=np.uint64)) else ROOT), got


def honest(oracle, rng, height, k):
    """A proof of k (distinct or not) random leafs of a tree of the given height and its root, without building the tree: any
    leaf and structure digests are the partial tree of some tree, whose root the checker computes."""
    n = 1 << height
    idx = rng.integers(0, n, size=k, dtype=np.uint64) if n > 1 else np.zeros(k, dtype=np.uint64)
    uniq = {}
    for i in idx.tolist():
        uniq.setdefault(i, oracle.fill_random(5, int(rng.integers(1 << 62))))
    dig = np.array([uniq[i] for i in idx.tolist()], dtype=np.uint64).reshape(-1, 5)
    na = len(oracle.auth_structure_indices(n, idx)) if k else 0
    auth = oracle.fill_random(5 * na, int(rng.integers(1 << 62))).reshape(-1, 5)
    st, root = check(oracle, height, idx, dig, auth)
    assert st == OK
    return idx, dig, auth, root


def proof(tf, h, idx, dig, auth):
    return tf.MerkleTreeInclusionProof(h, np.asarray(idx, dtype=np.uint64), np.asarray(dig, dtype=np.uint64).reshape(-1, 5),
                                       np.asarray(auth, dtype=np.uint64).reshape(-1, 5))


def tree(oracle, height, seed):
    leaves = oracle.fill_random(5 << height, seed)
    return oracle.merkle_build(leaves).reshape(-1, 5)


def tree_proof(tf, oracle, nodes, indices):
    n = nodes.shape[0] // 2
    ids = oracle.auth_structure_indices(n, np.array(indices, dtype=np.uint64)) if len(indices) else np.zeros(0, dtype=np.uint64)
    return proof(tf, n.bit_length() - 1, indices, nodes[n + np.array(indices, dtype=np.int64)] if len(indices) else np.zeros((0, 5)),
                 nodes[ids.astype(np.int64)])


def corrupt(x, rng):
    y = np.array(x, dtype=np.uint64, copy=True).reshape(-1, 5)
    r, w = int(rng.integers(y.shape[0])), int(rng.integers(5))
    y[r, w] = (int(y[r, w]) + 1) % 0xFFFFFFFF00000001
    return y


# ------------------------------------------------------------------ reference examples
def test_doc_example_paths(tf, oracle):
    """merkle_tree.rs:1518-1535 / :749-772: leafs 0 and 2 of 8 -> structure [11, 9, 3], paths [9, 5, 3] and [11, 4, 3]"""
    nodes = tree(oracle, 3, 0xD0C)
    p = tree_proof(tf, oracle, nodes, [0, 2])
    assert np.array_equal(p.authentication_structure, nodes[[11, 9, 3]])
    assert p.verify(nodes[1])
    paths = p.into_authentication_paths()
    assert paths.shape == (2, 3, 5)
    assert np.array_equal(paths[0], nodes[[9, 5, 3]]) and np.array_equal(paths[1], nodes[[11, 4, 3]])


@pytest.mark.parametrize("height", [2, 3])
def test_every_single_leaf_path(tf, oracle, height):
    """merkle_tree.rs:1309-1354: the path of every single leaf is its siblings bottom-up"""
    nodes = tree(oracle, height, 0x5117 + height)
    n = 1 << height
    for i in range(n):
        p = tree_proof(tf, oracle, nodes, [i])
        want = [nodes[((n + i) >> lv) ^ 1] for lv in range(height)]
        assert np.array_equal(p.into_authentication_paths()[0], np.array(want, dtype=np.uint64).reshape(height, 5))
        assert p.verify(nodes[1])


# ------------------------------------------------------------------ the reference's property tests (:1139-1306), seeded
def test_honest_proofs_verify(tf, oracle):
    rng = np.random.default_rng(1)
    for h in range(0, 11):
        nodes = tree(oracle, h, 0xA000 + h)
        for k in (1, 2, 5, 17):
            idx = rng.integers(0, 1 << h, size=k).tolist()
            p = tree_proof(tf, oracle, nodes, idx)
            assert p.verify(nodes[1]), (h, idx)
            p.try_verify(nodes[1])


def test_corruptions_give_root_mismatch(tf, oracle):
    rng = np.random.default_rng(2)
    nodes = tree(oracle, 9, 0xC0)
    for _ in range(20):
        idx = rng.integers(0, 512, size=int(rng.integers(1, 12))).tolist()
        p = tree_proof(tf, oracle, nodes, idx)
        bad_root = corrupt(nodes[1], rng).reshape(-1)
        cases = [(p, bad_root)]
        if p.authentication_structure.shape[0]:
            cases.append((proof(tf, p.tree_height, p.leaf_indices, p.leaf_digests, corrupt(p.authentication_structure, rng)), nodes[1]))
        d = corrupt(p.leaf_digests, rng)
        # a corrupted digest of a repeated index is a repeated-leaf mismatch, not a root mismatch
        cases.append((proof(tf, p.tree_height, p.leaf_indices, d, p.authentication_structure), nodes[1]))
        for q, r in cases:
            want, _ = check(oracle, q.tree_height, q.leaf_indices, q.leaf_digests, q.authentication_structure, r)
            assert want in (ROOT, REPEATED)
            with pytest.raises(tf.MerkleTreeError) as e:
                q.try_verify(r)
            assert e.value.code == want and e.value.variant == tf.MerkleTreeError.VARIANTS[want]
            assert not q.verify(r)


def test_removed_and_spurious_leafs_and_every_wrong_height(tf, oracle):
    rng = np.random.default_rng(3)
    nodes = tree(oracle, 8, 0x8E)
    proofs, roots = [], []
    for _ in range(10):
        idx = sorted(set(rng.integers(0, 256, size=int(rng.integers(2, 10))).tolist()))
        p = tree_proof(tf, oracle, nodes, idx)
        keep = np.ones(len(idx), dtype=bool)
        keep[int(rng.integers(len(idx)))] = False
        proofs.append(proof(tf, 8, p.leaf_indices[keep], p.leaf_digests[keep], p.authentication_structure))  # a leaf removed
        extra = int(rng.integers(0, 256))
        proofs.append(proof(tf, 8, np.append(p.leaf_indices, extra), np.vstack([p.leaf_digests, nodes[256 + extra]]),
                            p.authentication_structure))  # a spurious extra leaf
        for h in range(64):
            proofs.append(proof(tf, h, p.leaf_indices, p.leaf_digests, p.authentication_structure))
    roots = np.vstack([nodes[1]] * len(proofs))
    got = tf.MerkleTreeInclusionProof.try_verify_batch(proofs, roots)
    want = [check(oracle, q.tree_height, q.leaf_indices, q.leaf_digests, q.authentication_structure, nodes[1])[0] for q in proofs]
    assert got.tolist() == want
    assert set(want) - {OK} and OK in want


def test_duplicate_leafs(tf, oracle):
    rng = np.random.default_rng(4)
    nodes = tree(oracle, 7, 0xD1)
    for _ in range(10):
        idx = rng.integers(0, 128, size=4).tolist()
        idx = idx + idx[:2]
        p = tree_proof(tf, oracle, nodes, idx)
        assert p.verify(nodes[1])  # equal digests
        d = p.leaf_digests.copy()
        d[-1, int(rng.integers(5))] ^= 1
        q = proof(tf, 7, p.leaf_indices, d, p.authentication_structure)
        with pytest.raises(tf.MerkleTreeError) as e:
            q.try_verify(nodes[1])
        assert e.value.variant == "RepeatedLeafDigestMismatch"


def test_all_leafs_revealed(tf, oracle):
    for h in range(0, 14):
        nodes = tree(oracle, h, 0xA11 + h)
        p = tree_proof(tf, oracle, nodes, list(range(1 << h)))
        assert p.authentication_structure.shape[0] == 0
        assert p.verify(nodes[1]), h
        assert not p.verify(corrupt(nodes[1], np.random.default_rng(h)).reshape(-1))


def test_small_edge_cases(tf, oracle):
    nodes = tree(oracle, 4, 0xE)
    mt = tf.MerkleTree(nodes)
    with pytest.raises(tf.MerkleTreeError) as e:
        mt.inclusion_proof_for_leaf_indices([3, 16])
    assert e.value.variant == "LeafIndexInvalid"
    p = mt.inclusion_proof_for_leaf_indices([3, 9])
    assert p.verify(nodes[1]) and [i for i, _ in mt.indexed_leafs([3, 9])] == [3, 9]
    trivial = proof(tf, 200, [], np.zeros((0, 5)), np.zeros((0, 5)))
    assert trivial.verify(nodes[1]) and trivial.verify(np.zeros(5, dtype=np.uint64))
    # a batch of proofs without any leaf or digest: nothing but the roots goes to the device
    pair = [trivial, proof(tf, 3, [], np.zeros((0, 5)), np.zeros((0, 5)))]
    got = tf.MerkleTreeInclusionProof.try_verify_batch(pair, np.vstack([nodes[1], nodes[2]]))
    assert got.tolist() == [check(oracle, p.tree_height, [], np.zeros((0, 5)), np.zeros((0, 5)))[0] for p in pair] == [OK, OK]
    with pytest.raises(tf.MerkleTreeError) as e:
        proof(tf, 64, [0], nodes[16:17], np.zeros((0, 5))).try_verify(nodes[1])
    assert e.value.variant == "TreeTooHigh"
    with pytest.raises(tf.MerkleTreeError) as e:
        proof(tf, 4, [], np.zeros((0, 5)), nodes[2:3]).try_verify(nodes[1])
    assert e.value.variant == "AuthenticationStructureLengthMismatch"
    one = proof(tf, 0, [0, 0], np.vstack([nodes[5], nodes[5]]), np.zeros((0, 5)))
    assert one.verify(nodes[5]) and one.into_authentication_paths().shape == (2, 0, 5)


# ------------------------------------------------------------------ a ragged batch over both routes
def ragged_batch(tf, oracle, count, seed):
    rng = np.random.default_rng(seed)
    proofs, roots = [], []
    for _ in range(count):
        h = int(rng.integers(0, 25))
        k = int(rng.integers(0, 301)) if rng.random() < 0.1 else int(rng.integers(0, 41))
        idx, dig, auth, root = honest(oracle, rng, h, k)
        root = root if root is not None else oracle.fill_random(5, int(rng.integers(1 << 62)))
        kind = int(rng.integers(0, 16)) if rng.random() < 0.65 else -1
        if kind in (0, 1) or (kind == 2 and k == 0):
            root = corrupt(root, rng).reshape(-1)
        elif kind == 2 and auth.shape[0]:
            auth = corrupt(auth, rng)
        elif kind == 3 and k:
            dig = corrupt(dig, rng)
        elif kind == 4 and k:
            idx, dig = idx[1:], dig[1:]
        elif kind == 5:
            extra = int(rng.integers(0, 1 << h))
            idx, dig = np.append(idx, np.uint64(extra)), np.vstack([dig, oracle.fill_random(5, extra).reshape(1, 5)])
        elif kind == 6:
            h = int(rng.integers(0, 70))
        elif kind == 7 and k:
            idx, dig = np.append(idx, idx[0]), np.vstack([dig, corrupt(dig[:1], rng)])
        elif kind == 8 and k:
            idx, dig = np.append(idx, idx[-1]), np.vstack([dig, dig[-1:]])
        elif kind == 9 and auth.shape[0]:
            auth = auth[:-1]
        elif kind == 10:
            auth = np.vstack([auth, oracle.fill_random(5, 7).reshape(1, 5)])
        elif kind == 11 and k:
            idx = idx.copy()
            idx[int(rng.integers(k))] = np.uint64((1 << h) + int(rng.integers(0, 5)))
        proofs.append(proof(tf, h, idx, dig, auth))
        roots.append(np.asarray(root, dtype=np.uint64).reshape(5))
    return proofs, np.vstack(roots)


def test_ragged_batch(tf, oracle):
    proofs, roots = ragged_batch(tf, oracle, 3000, 0x4A6)
    got = tf.MerkleTreeInclusionProof.try_verify_batch(proofs, roots)
    want = [check(oracle, p.tree_height, p.leaf_indices, p.leaf_digests, p.authentication_structure, r)[0] for p, r in zip(proofs, roots)]
    assert got.tolist() == want
    assert {OK, ROOT, LEN, REPEATED, LEAF_INVALID, TOO_HIGH} <= set(want)
    assert 0.3 < sum(w != OK for w in want) / len(want) < 0.7
    assert any(p.leaf_indices.size > 256 and w == OK for p, w in zip(proofs, want))  # the device-scratch route, verified
    alone = [tf.MerkleTreeInclusionProof.try_verify_batch([p], r)[0] for p, r in zip(proofs, roots)]
    assert list(alone) == want


def test_authentication_paths_batch(tf, oracle):
    proofs, _ = ragged_batch(tf, oracle, 600, 0x9A7)
    paths, st = tf.MerkleTreeInclusionProof.authentication_paths_batch(proofs)
    n_ok = 0
    for p, got, s in zip(proofs, paths, st.tolist()):
        want_st, want = check(oracle, p.tree_height, p.leaf_indices, p.leaf_digests, p.authentication_structure, paths=True)
        assert s == want_st
        if s == OK:
            n_ok += 1
            assert got.shape == (p.leaf_indices.size, p.tree_height, 5)
            assert np.array_equal(got, want.reshape(got.shape))
    assert n_ok > 100


# ------------------------------------------------------------------ large device-resident trees through the _dev API
@pytest.mark.parametrize("height,k", [(20, 40), (24, 160)])
def test_large_tree_dev(tf, oracle, height, k):
    import torch

    n = 1 << height
    leaves = torch.empty(5 * n, dtype=torch.int64, device="cuda")
    tf.device.fill_random(leaves, 0x1A26E + height)
    nodes = torch.empty(10 * n, dtype=torch.int64, device="cuda")
    tf.device.merkle_build(leaves, n, nodes)
    rng = np.random.default_rng(height)
    proofs_idx = [rng.integers(0, n, size=k, dtype=np.uint64) for _ in range(3)]
    nv = nodes.view(-1, 5)
    li, ld, ad, lo, ao = [], [], [], [0], [0]
    for idx in proofs_idx:
        ids = tf.MerkleTree.authentication_structure_node_indices(n, idx)
        li.append(torch.from_numpy(idx.astype(np.int64)).cuda())
        ld.append(nv[torch.from_numpy((idx + n).astype(np.int64)).cuda()].reshape(-1))
        ad.append(nv[torch.from_numpy(ids.astype(np.int64)).cuda()].reshape(-1))
        lo.append(lo[-1] + k)
        ao.append(ao[-1] + len(ids))
    li, ld, ad = torch.cat(li), torch.cat(ld), torch.cat(ad)
    ad_bad = ad.clone()
    ad_bad[7] = (ad_bad[7] + 1) % 0xFFFFFFFF
    root = nv[1].clone()
    roots = root.repeat(3)
    st = torch.full((3,), -1, dtype=torch.int32, device="cuda")
    tf.device.verify_inclusion_proofs([height] * 3, lo, li, ld, ao, ad, roots, st)
    st_bad = torch.full((3,), -1, dtype=torch.int32, device="cuda")
    tf.device.verify_inclusion_proofs([height] * 3, lo, li, ld, ao, ad_bad, roots, st_bad)
    torch.cuda.synchronize()
    assert st.cpu().tolist() == [OK] * 3
    assert st_bad.cpu().tolist() == [ROOT, OK, OK]
    # the checker, from the first proof alone, reaches the same root
    st0, r0 = check(oracle, height, proofs_idx[0], ld[: 5 * k].cpu().numpy().view(np.uint64), ad[: 5 * ao[1]].cpu().numpy().view(np.uint64))
    assert st0 == OK and np.array_equal(r0, root.cpu().numpy().view(np.uint64))
    del leaves, nodes


def test_dev_call_does_not_block(tf, oracle):
    import torch

    rng = np.random.default_rng(5)
    idx, dig, auth, root = honest(oracle, rng, 20, 40)
    li = torch.from_numpy(idx.astype(np.int64)).cuda()
    ld = torch.from_numpy(dig.reshape(-1).view(np.int64)).cuda()
    ad = torch.from_numpy(auth.reshape(-1).view(np.int64)).cuda()
    rt = torch.from_numpy(np.asarray(root, dtype=np.uint64).view(np.int64)).cuda()
    st = torch.full((1,), -1, dtype=torch.int32, device="cuda")
    lo, ao = [0, 40], [0, auth.shape[0]]
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        tf.device.verify_inclusion_proofs([20], lo, li, ld, ao, ad, rt, st, stream=s)  # warm-up: constants, pools, staging
    s.synchronize()
    x = torch.zeros((1 << 22) * 16, dtype=torch.int64, device="cuda")
    st.fill_(-1)
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(8):
            tf.device.ntt_(x, 1 << 22, batch=16, stream=s)
        tf.device.verify_inclusion_proofs([20], lo, li, ld, ao, ad, rt, st, stream=s)
        busy = not s.query()
    s.synchronize()
    assert busy, "the verify call waited for the stream"
    assert st.cpu().tolist() == [OK]
    del x


def test_dev_paths_match_host(tf, oracle):
    import torch

    proofs, _ = ragged_batch(tf, oracle, 200, 0xBEE)
    h, lo, li, ld, ao, ad = tf.MerkleTreeInclusionProof._pack(proofs)
    words = tf.device.authentication_path_words(h, lo)
    out = torch.zeros(max(words, 1), dtype=torch.int64, device="cuda")
    st = torch.full((len(proofs),), -1, dtype=torch.int32, device="cuda")
    cuda = lambda a: torch.from_numpy(a.view(np.int64)).cuda() if a.size else torch.zeros(1, dtype=torch.int64, device="cuda")  # noqa: E731
    tf.device.authentication_paths(h, lo, cuda(li), cuda(ld), ao, cuda(ad), out, st)
    torch.cuda.synchronize()
    paths, st_host = tf.MerkleTreeInclusionProof.authentication_paths_batch(proofs)
    assert st.cpu().numpy().tolist() == st_host.tolist()
    got = out.cpu().numpy().view(np.uint64)
    off = 0
    for p, want, s in zip(proofs, paths, st_host.tolist()):
        size = 5 * p.leaf_indices.size * p.tree_height if p.tree_height < 64 else 0
        if s == OK:
            assert np.array_equal(got[off: off + size], want.reshape(-1))
        off += size
