"""Merkle openings at leaf indices that are device data (include/tf_hip.h, "The same openings with the leaf indices in DEVICE memory").

The device-pointer API of device.py for the last link of a device-resident opening: the indices a batch of Tip5 sponges sampled
(device.tip5_sponge_sample_indices: n_lists x k 32-bit words) go straight into the authentication structure.  Digest tensors are
1-D contiguous int64 / uint64 CUDA tensors of raw Montgomery words; index, count and run-end tensors are contiguous int32 / uint32
CUDA tensors whose bits are the u32 values.  Every call only enqueues on torch's current stream (or the given one).

A count is device data, so outputs are sized by `capacity` digests (or node indices) per tree, at most max_nodes(num_leafs, k).
With `status` (a one-element int32 CUDA tensor, see device._status) nothing is synchronised and a data error writes its code there:
11 (LeafIndexInvalid) for a list with an index >= num_leafs, which gets count 0; 13 (buffer too small) for a list with more than
`capacity` nodes, which gets its full count.  Neither list writes a digest and the other lists are unaffected.  Without `status`
the call synchronises once and raises.
"""
from __future__ import annotations

from . import _lib
from .device import _chk, _need, _own_status, _p, _raise_own_status, _status, _stream, _t
from .table import _apart_bytes, _counts

MAX_INDICES = 8192
LEVELS = 32


def _u32(t, name: str):
    import torch

    _need(isinstance(t, torch.Tensor) and t.is_cuda and t.is_contiguous() and t.dtype in (torch.int32, torch.uint32),
          f"{name} must be a contiguous CUDA tensor of 32-bit words")
    return t


def _lists(num_leafs: int, leaf_indices, n_lists: int) -> int:
    """the indices per list, after the checks every call shares"""
    _counts(num_leafs=num_leafs, n_lists=n_lists)
    _need(num_leafs >= 1 and num_leafs & (num_leafs - 1) == 0 and num_leafs <= 1 << 31, "num_leafs must be a power of two, at most 2^31")
    _u32(leaf_indices, "leaf_indices")
    _need(n_lists >= 1 and leaf_indices.numel() % n_lists == 0, "leaf_indices must hold n_lists lists of equal length")
    k = leaf_indices.numel() // n_lists
    _need(k <= MAX_INDICES, f"a list holds at most {MAX_INDICES} indices")
    return k


def _run(call, status, like, others, stream, where: str) -> None:
    own = _own_status(status, like)
    _status(own)  # (its type, before its address is compared)
    for other, name in others:
        if other is not None:
            _apart_bytes(own, other, f"status must not overlap {name}")
    _chk(call(_status(own)), where)
    if status is None:
        _raise_own_status(own, stream, where)


def max_nodes(num_leafs: int, k: int) -> int:
    """No list of k indices into a tree of num_leafs leafs has more structure nodes than this (tf_merkle_auth_structure_max_nodes:
    host arithmetic, no device needed); 0 for arguments the calls reject."""
    return int(_lib.lib().tf_merkle_auth_structure_max_nodes(num_leafs, k))


def structure_indices(num_leafs: int, leaf_indices, node_indices, counts, n_lists: int = 1, level_ends=None, stream=None, status=None) -> None:
    """MerkleTree::authentication_structure_node_indices (util_types/merkle_tree.rs:449-504) of n_lists index lists
    (tf_merkle_auth_structure_indices_dev): list l writes its node indices, descending, to node_indices[l * capacity:] with
    capacity = node_indices.numel() // n_lists, their number to counts[l] and, when level_ends (n_lists x 32) is given, the ends of
    its per-level runs there."""
    k = _lists(num_leafs, leaf_indices, n_lists)
    _u32(node_indices, "node_indices"), _u32(counts, "counts")
    _need(node_indices.numel() % n_lists == 0, "node_indices must hold the same number of slots for every list")
    _need(counts.numel() == n_lists, "counts must hold one entry per list")
    tensors = [(leaf_indices, "leaf_indices"), (node_indices, "node_indices"), (counts, "counts")]
    if level_ends is not None:
        _need(_u32(level_ends, "level_ends").numel() == n_lists * LEVELS, f"level_ends must hold {LEVELS} entries per list")
        tensors.append((level_ends, "level_ends"))
    for i, (a, na) in enumerate(tensors[1:], 1):
        for b, nb in tensors[:i]:
            _apart_bytes(a, b, f"{na} must not overlap {nb}")
    capacity = node_indices.numel() // n_lists
    fn = _lib.lib().tf_merkle_auth_structure_indices_dev
    _run(lambda st: fn(num_leafs, _p(leaf_indices), k, n_lists, _p(node_indices), capacity, _p(counts),
                       _p(level_ends) if level_ends is not None else None, _stream(stream), st),
         status, counts, tensors, stream, "MerkleTree::authentication_structure_node_indices")


def _open(fn, where, trees, words_per_tree: int, what: str, num_leafs, leaf_indices, out, counts, n_lists, trees_per_list, roots, stream, status):
    k = _lists(num_leafs, leaf_indices, n_lists)
    _counts(trees_per_list=trees_per_list)
    _need(trees_per_list >= 1, "trees_per_list must be at least 1")
    n_trees = n_lists * trees_per_list
    trees, out = _t(trees, what), _t(out, "out")
    _need(trees.numel() == n_trees * num_leafs * words_per_tree, f"{what} must hold n_lists * trees_per_list trees of num_leafs leafs")
    _need(out.numel() % (5 * n_trees) == 0, "out must hold the same whole number of digests for every tree")
    _need(_u32(counts, "counts").numel() == n_lists, "counts must hold one entry per list")
    tensors = [(trees, what), (leaf_indices, "leaf_indices"), (out, "out"), (counts, "counts")]
    if roots is not None:
        _need(_t(roots, "roots").numel() == 5 * n_trees, "roots must hold one digest per tree")
        tensors.append((roots, "roots"))
    for i, (a, na) in enumerate(tensors[2:], 2):
        for b, nb in tensors[:i]:
            _apart_bytes(a, b, f"{na} must not overlap {nb}")
    capacity = out.numel() // (5 * n_trees)
    tail = (_p(roots) if roots is not None else None,) if fn is _lib.lib().tf_merkle_auth_structure_from_leafs_sampled_dev else ()
    _run(lambda st: fn(_p(trees), num_leafs, _p(leaf_indices), k, n_lists, trees_per_list, _p(out), capacity, _p(counts), *tail,
                       _stream(stream), st),
         status, counts, tensors, stream, where)


def structure_from_nodes(nodes, num_leafs: int, leaf_indices, out, counts, n_lists: int = 1, trees_per_list: int = 1, stream=None,
                         status=None) -> None:
    """The authentication structures of n_lists * trees_per_list trees given as node arrays (2 * num_leafs digests each, as
    device.merkle_build leaves them), tree t opened at list t // trees_per_list (tf_merkle_authentication_structure_sampled_dev).
    out is tree-major, capacity = out.numel() // (5 * trees) digests per tree: the first counts[list] are the structure in the
    reference's order, the words behind them stay as they were."""
    _open(_lib.lib().tf_merkle_authentication_structure_sampled_dev, "MerkleTree::authentication_structure", nodes, 10, "nodes", num_leafs,
          leaf_indices, out, counts, n_lists, trees_per_list, None, stream, status)


def structure_from_leafs(leafs, num_leafs: int, leaf_indices, out, counts, n_lists: int = 1, trees_per_list: int = 1, roots=None, stream=None,
                         status=None) -> None:
    """Commit and open: the same structures straight from the leafs (num_leafs digests per tree), without a node array
    (tf_merkle_auth_structure_from_leafs_sampled_dev); `roots` (one digest per tree), when given, receives the roots, whatever
    the status.  Work space comes from the library's pool: from_leafs_workspace."""
    _open(_lib.lib().tf_merkle_auth_structure_from_leafs_sampled_dev, "MerkleTree::authentication_structure_from_leafs", leafs, 5, "leafs",
          num_leafs, leaf_indices, out, counts, n_lists, trees_per_list, roots, stream, status)


def from_leafs_workspace(num_leafs: int, trees: int, k: int, n_lists: int) -> int:
    """Bytes structure_from_leafs requests from the library's pool for `trees` trees in all, opened at n_lists lists of k indices
    (tf_merkle_auth_structure_from_leafs_sampled_workspace: host arithmetic, no device needed); 0 for arguments the call rejects."""
    return int(_lib.lib().tf_merkle_auth_structure_from_leafs_sampled_workspace(num_leafs, trees, k, n_lists))
