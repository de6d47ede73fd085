"""Index arithmetic of the Merkle Mountain Range in pure Python (util_types/mmr/shared_basic.rs, shared_advanced.rs).

Node indices are the reference's: 1-based, in the order an append-only MMR creates its nodes (post-order over the peaks).  Leaf
indices are 0-based.  All arguments and results are Python ints in [0, 2^64)."""
from __future__ import annotations

MAX_LEAFS = 1 << 63  # mmr.rs:12-13


def _ilog2(x: int) -> int:
    return x.bit_length() - 1


def trailing_ones(x: int) -> int:
    return ((x ^ (x + 1)).bit_length() - 1)


# ---- shared_basic.rs
def left_child(node_index: int, height: int) -> int:  # :6-9
    return node_index - (1 << height)


def right_child(node_index: int) -> int:  # :11-14
    return node_index - 1


def leaf_index_to_mt_index_and_peak_index(leaf_index: int, num_leafs: int):  # :24-62
    if not leaf_index < num_leafs:
        raise ValueError("Leaf index must be strictly smaller than the number of leafs")
    h = _ilog2(leaf_index ^ num_leafs)
    local = leaf_index & ((1 << h) - 1)
    peak_index = bin(num_leafs).count("1") - bin(num_leafs & ((1 << h) - 1)).count("1") - 1
    return local + (1 << h), peak_index


def right_lineage_length_from_leaf_index(leaf_index: int) -> int:  # :65-68
    return trailing_ones(leaf_index)


# ---- shared_advanced.rs
def leftmost_ancestor(node_index: int):  # :8-17 -> (node index, height)
    if node_index >> 63:
        return (1 << 64) - 1, 63
    h = _ilog2(node_index)
    return (1 << (h + 1)) - 1, h


def right_lineage_length_and_own_height(node_index: int):  # :21-44
    candidate, height = leftmost_ancestor(node_index)
    right_count = 0
    while candidate != node_index:
        left = left_child(candidate, height)
        if left < node_index:
            candidate = right_child(candidate)
            right_count += 1
        else:
            candidate = left
            right_count = 0
        height -= 1
    return right_count, height


def right_lineage_length_from_node_index(node_index: int) -> int:  # :46-60
    return right_lineage_length_and_own_height(node_index)[0]


def leaf_index_to_node_index(leaf_index: int) -> int:  # :62-67
    return 2 * leaf_index - bin(leaf_index).count("1") + 1


def parent(node_index: int) -> int:  # :69-80
    right_count, height = right_lineage_length_and_own_height(node_index)
    return node_index + 1 if right_count != 0 else node_index + (1 << (height + 1))


def left_sibling(node_index: int, height: int) -> int:  # :82-87
    return node_index - (1 << (height + 1)) + 1


def right_sibling(node_index: int, height: int) -> int:  # :89-92
    return node_index + (1 << (height + 1)) - 1


def num_leafs_to_num_nodes(num_leafs: int) -> int:  # :94-99
    return 0 if num_leafs == 0 else 2 * num_leafs - bin(num_leafs).count("1")


def get_authentication_path_node_indices(start_node_index: int, peak_node_index: int, node_count: int):  # :155-187
    """The node indices of the path from start_node_index up to peak_node_index, or None if the walk leaves the first node_count."""
    out, node = [], start_node_index
    while node <= node_count and node != peak_node_index:
        right_count, height = right_lineage_length_and_own_height(node)
        if right_count != 0:
            out.append(left_sibling(node, height))
            node += 1
        else:
            out.append(right_sibling(node, height))
            node += 1 << (height + 1)
    return out if node == peak_node_index else None


def get_peak_heights(leaf_count: int):  # :198-220 (highest first)
    return [h for h in range(63, -1, -1) if (leaf_count >> h) & 1]


def get_peak_heights_and_peak_node_indices(leaf_count: int):  # :222-254
    heights, nodes, acc = [], [], 0
    for h in get_peak_heights(leaf_count):
        acc += (1 << (h + 1)) - 1
        heights.append(h)
        nodes.append(acc)
    return heights, nodes


def node_index_to_leaf_index(node_index: int):  # :256-277 -> leaf index, or None for an inner node
    if right_lineage_length_and_own_height(node_index)[1] != 0:
        return None
    node, height = leftmost_ancestor(node_index)
    leaf_index = 0
    while height > 0:
        left = left_child(node, height)
        height -= 1
        if node_index <= left:
            node = left
        else:
            node = right_child(node)
            leaf_index += 1 << height
    return leaf_index


def node_indices_added_by_append(old_leaf_count: int):  # :101-119
    node_index = leaf_index_to_node_index(old_leaf_count)
    added = [node_index]
    for _ in range(right_lineage_length_from_leaf_index(old_leaf_count)):
        node_index += 1
        added.append(node_index)
    return added


def auth_path_node_indices(num_leafs: int, leaf_index: int):  # :121-153
    if not leaf_index < num_leafs:
        raise ValueError(f"Leaf index out-of-bounds: {leaf_index}/{num_leafs}")
    mt_index, _ = leaf_index_to_mt_index_and_peak_index(leaf_index, num_leafs)
    node = leaf_index_to_node_index(leaf_index)
    out = []
    for _ in range(_ilog2(mt_index)):
        right_count, height = right_lineage_length_and_own_height(node)
        if right_count != 0:
            out.append(left_sibling(node, height))
            node += 1
        else:
            out.append(right_sibling(node, height))
            node += 1 << (height + 1)
    return out


def membership_proof_node_indices(leaf_index: int, path_len: int):  # MmrMembershipProof::get_node_indices, mmr_membership_proof.rs:80-99
    node, out = leaf_index_to_node_index(leaf_index), []
    for _ in range(path_len):
        right_count, height = right_lineage_length_and_own_height(node)
        if right_count != 0:
            out.append(left_sibling(node, height))
            node += 1
        else:
            out.append(right_sibling(node, height))
            node += 1 << (height + 1)
    return out
