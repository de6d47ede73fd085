"""tests/field_ref.py checked against itself and against exact field arithmetic, without a GPU: the expected words are congruent to the
field result, canonical where the primitive promises it, 64 bits wide and equal to a step-by-step model of the primitive; the operand
sets reach every carry path of every output at every block position; and tf_debug_field_op_dev checks its arguments before it
touches a device.  tests/test_gpu_field_primitives.py compares the kernels with these words."""
import collections

import pytest

from tests import field_ref as ref

MIN_OCCURRENCES = 8


def test_op_table_matches_the_binding(tf):
    assert ref.OPS == tf.device.FIELD_OPS
    assert sorted(code for code, _, _ in ref.OPS.values()) == list(range(15))


def test_edge_words_and_set_sizes():
    edges = ref.edge_words()
    for w in (0, 1, 2, ref.P - 2, ref.P - 1, ref.P, ref.P + 1, ref.M64, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 2 ** 63, 2 ** 63 - 1):
        assert w in edges
    assert all(1 << s in edges for s in range(64)) and len(edges) == len(set(edges)) and all(0 <= w <= ref.M64 for w in edges)
    for op in ref.OPS:
        a, b = ref.operands(op)
        in_set = set(zip(a, b))
        assert all((x, y) in in_set for x in edges for y in edges if ref.in_domain(op, x, y)), op  # the full cross product
        assert (1 << 16) < len(a) <= ref.MAX_PAIRS and len(a) % 2 and len(a) % 3, op             # coprime to 12
        assert all(0 <= x <= ref.M64 and 0 <= y <= ref.M64 and ref.in_domain(op, x, y) for x, y in in_set), op


@pytest.mark.parametrize("op", list(ref.OPS))
def test_expected_words_are_the_field_results(op):
    """congruent to the exact result, canonical where promised, within 64 bits, equal to the step-by-step model -- at every block position"""
    a, b, want0, want1, n = ref.uploaded(op)
    w = ref.width(op)
    for out, words in enumerate((want0, want1)[:ref.outputs(op)]):
        if op not in ref.TAIL_OPS:  # only the fold tails' words depend on the position: the repetitions hold the same words
            assert all(words[k * n:(k + 1) * n] == words[:n] for k in range(w))
        for j, (x, y, r) in enumerate(zip(a, b, words) if op in ref.TAIL_OPS else zip(a[:n], b[:n], words[:n])):
            pos = j % w
            assert 0 <= r <= ref.M64, (op, out, pos, x, y)
            assert r % ref.P == ref.exact(op, out, x, y), (op, out, pos, x, y)
            if ref.promises_canonical(op, out, pos, x, y):
                assert r < ref.P, (op, out, pos, x, y)
            assert ref.event(op, out, pos, x, y)[1] == r, (op, out, pos, x, y)


@pytest.mark.parametrize("op", list(ref.OPS))
def test_every_reachable_event_occurs_at_every_block_position(op):
    """each carry path of each output at least MIN_OCCURRENCES times in each chain; nothing outside the reachable list ever"""
    a, b, _, _, n = ref.uploaded(op)
    w = ref.width(op)
    assert len(a) == n * w
    for out in range(ref.outputs(op)):
        seen = [collections.Counter() for _ in range(w)]
        labels = None if op in ref.TAIL_OPS else [ref.event(op, out, 0, x, y)[0] for x, y in zip(a[:n], b[:n])]
        for j in range(n * w):
            seen[j % w][labels[j % n] if labels else ref.event(op, out, j % w, a[j], b[j])[0]] += 1
        for pos in range(w):
            expected = ref.reachable(op, out, pos)
            assert set(seen[pos]) == set(expected), (op, out, pos, set(seen[pos]) ^ set(expected))
            short = {e: seen[pos][e] for e in expected if seen[pos][e] < MIN_OCCURRENCES}
            assert not short, (op, out, pos, short)
            for label in seen[pos]:
                assert not any(label.startswith(bad) for bad in ref.impossible(op)), (op, out, pos, label)
            assert not set(expected) & set(ref.impossible(op))


def test_impossible_events_are_listed_with_a_reason():
    for op in ("ADD", "CANONICAL", "MONT_MUL", "MONT_MUL2", "MONT_MUL3", "MONT_MUL4", "MX_FOLD4_CANON", "MX_FOLD4_LAZY", "MX_FOLD2"):
        assert ref.impossible(op) and all(len(why) > 20 for why in ref.impossible(op).values()), op
    # the product's claim on a family that comes as close as any: both operands just above p, where x y is largest against x + y
    for x in range(2 ** 32 - 66, 2 ** 32 - 1):
        for y in (x, 2 ** 32 - 2, 2 ** 31, 1):
            assert ref.event("MONT_MUL", 0, 0, ref.P + x, ref.P + y)[0].endswith("none")


def test_uniform_operands_alone_would_not_do():
    """why the sets are built: among 2^16 uniform pairs no correction ever ripples"""
    import random

    rng = random.Random(1)
    for _ in range(1 << 16):
        a, b = rng.getrandbits(64), rng.getrandbits(64)
        assert "ripple" not in ref.event("MONT_MUL4", 0, 0, a, b)[0]
        assert "ripple" not in ref.event("ADD_SUB2", 0, 0, a % ref.P, b % ref.P)[0]


def test_argument_checks_need_no_device(tf):
    """an unknown op or an absurd count is an error before anything is launched; a count of 0 is nothing to do"""
    lib = tf.lib()
    assert lib.tf_debug_field_op_dev(15, None, None, None, None, 0, None) == 17  # TF_ERR_INVALID_ARGUMENT
    assert lib.tf_debug_field_op_dev(-1, None, None, None, None, 0, None) == 17
    assert lib.tf_debug_field_op_dev(15, None, None, None, None, 4, None) == 17
    assert lib.tf_debug_field_op_dev(0, None, None, None, None, (1 << 32) + 1, None) == 17
    for code, _, n_out in ref.OPS.values():
        assert lib.tf_debug_field_op_dev(code, None, None, None, None, 0, None) == 0
        assert lib.tf_debug_field_op_dev(code, None, None, None, None, 4, None) == 7  # TF_ERR_NULL_POINTER
    with pytest.raises(KeyError):
        tf.device.debug_field_op("NO_SUCH_OP", None, None, None)
