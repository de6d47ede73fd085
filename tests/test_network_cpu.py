"""CPU-side checks (no GPU) of tests/network_ref.py, the integer model behind tests/test_gpu_ntt_networks.py: reduced mod p the model is
the plain DFT on every block of every operand set; the operand sets reach every carry path of every butterfly of every form at least
eight times, and every condition (first operand >= p, second operand >= p, first operand >= p with a rippling carry) exactly where the
recursion over the network says an in-contract block can; the sets are deterministic; tf_debug_ntt_network_dev checks its arguments
before it looks for a device."""
import collections

import pytest

from tests import network_ref as nr

P = nr.P
FORMS = list(nr.FORMS)


def _tally(form, blocks):
    hits = collections.Counter()

    def trace(lvl, i, a, b, v, lazy):
        if lvl == 0:
            hits[(0, i, nr.glue_label(form, i, a, b))] += 1
            return
        labels, conds = nr.classify(lvl, a, b, v, lazy)
        for key in labels + conds:
            hits[(lvl, i, key)] += 1

    for block in blocks:
        assert nr.block_in_contract(form, block)
        out = nr.run(form, block, None, trace)
        assert [w % P for w in out] == nr.dft_reference(form, block), (form, block)
        if not nr.is_lazy(form):
            assert all(w < P for w in out)
    return hits


def _assert_reached(form, hits, canonical_inputs):
    reach, excluded = nr.reachable_conditions(form, canonical_inputs)
    for lvl, i in form.butterflies():
        for label in nr.labels_of(form):
            assert hits[(lvl, i, label)] >= 8, (form, lvl, i, label, hits[(lvl, i, label)])
        for cond in nr.CONDITIONS:
            if cond in reach.get((lvl, i), ()):
                assert hits[(lvl, i, cond)] >= 8, (form, lvl, i, cond, hits[(lvl, i, cond)])
            else:
                assert hits[(lvl, i, cond)] == 0, f"{form}: level {lvl} butterfly {i} reached {cond}, which the recursion excludes"
                assert cond.startswith("b>=p") and lvl == 1 or excluded[(lvl, i, cond)]  # (level 1 has no such conditions: tw_operand does not look)
    return excluded


def test_form_table_matches_the_package():
    from twenty_first_amd import device

    assert len(nr.FORMS) == nr.FORM_COUNT == len(device.NETWORK_FORMS)
    assert sorted(f.code for f in nr.FORMS.values()) == list(range(nr.FORM_COUNT))
    assert {n: (f.code, f.words) for n, f in nr.FORMS.items()} == device.NETWORK_FORMS


@pytest.mark.parametrize("name", FORMS)
def test_model_is_the_dft_and_every_reachable_event_is_reached(name):
    """model == plain DFT mod p on every block; >= 8 hits of every label at every butterfly and of every condition the recursion
    predicts, none of any it excludes; every aimed block sees the pair it was built for"""
    form = nr.FORMS[name]
    sets = nr.operand_sets(form)
    assert len(sets["uniform"]) == 1 << 10 and len(sets["edge"]) == 256
    hits = _tally(form, [b for blocks in sets.values() for b in blocks])
    excluded = _assert_reached(form, hits, False)
    if nr.is_lazy(form) and form.kind in ("NET32", "LEVELS", "C8") or (form.kind == "PRE2" and not form.half):
        assert not excluded or form.half, (form, len(excluded))  # the lazy contract (even slots any word) reaches everything
    if not nr.is_lazy(form):
        assert set(excluded.values()) == {nr.WHY_NOT["canonical"]}
    if form.kind in ("PRE2", "C8"):
        for q in range(32):
            for label in nr.glue_reachable(form, q):
                assert hits[(0, q, label)] >= 8, (form, q, label, hits[(0, q, label)])
        if not form.half:  # the pairs that would show an odd slot's sum left lazy
            pairs = collections.Counter((q, nr.glue_pair_label(form, b, q)) for b in sets["glue"] for q in range(1, 32, 2))
            assert all(pairs[(q, label)] >= 8 for q in range(1, 32, 2) for label in ("gep&borrow", "gep&a>=sum", "gep&carry")), (form, pairs)
    for canonical_inputs in ([False, True] if "constructed_canonical" in sets else [False]):
        for block, aims in nr.constructed(form, canonical_inputs):
            seen = {}
            nr.run(form, block, None, lambda lvl, i, a, b, v, lazy: seen.__setitem__((lvl, i), (a, b)))
            for lvl, i, kind, a, b in aims:
                assert seen[(lvl, i)] == (a, b), (form, lvl, i, kind)
            nonzero = sum(1 for w in block if w)
            assert nonzero <= 4 * len(aims) * (2 if form.words == 64 else 1)  # sparse: two to four words per aimed group


@pytest.mark.parametrize("logn", [1, 2, 3, 4, 5])
def test_canonical_inputs_reach_exactly_what_the_recursion_predicts(logn):
    """the blocks the short-transform kernels are steered with: canonical words in, lazy levels -- a word >= p appears only behind a sum"""
    form, blocks = nr.steered_rows(logn, True)
    assert all(w < P for b in blocks for w in b)
    excluded = _assert_reached(form, _tally(form, blocks), True)
    # level 1 sees the inputs themselves; in a sub-group of 2^m slots exactly one slot is reached through differences alone, so one
    # butterfly per group of level m + 1 has a first operand < p, and one a second operand < p
    for lvl in range(1, logn + 1):
        for cond in ("a>=p", "b>=p"):
            want = 16 if lvl == 1 else 16 >> (lvl - 1)
            assert sum(1 for key in excluded if key[0] == lvl and key[2] == cond) == (0 if (lvl, cond) == (1, "b>=p") else want)
    assert nr.WHY_NOT["canonical"] not in excluded.values() and set(excluded.values()) <= set(nr.WHY_NOT.values())
    fwd, fwd_blocks = nr.steered_rows(logn, False)
    assert not nr.is_lazy(fwd) and all(w < P for b in fwd_blocks for w in b)


def test_n64_dif_stage_hands_the_lanes_the_steered_blocks():
    """n = 64: the inputs solved backwards through rows64_dif_stage give the lane pair exactly the steered blocks, so the events of
    test_canonical_inputs_reach_exactly_what_the_recursion_predicts are reached behind the stage; and the whole is the 64-point DFT"""
    for inverse in (False, True):
        form, blocks = nr.steered_rows(6, inverse)
        for k in range(0, len(blocks), 7):
            even, odd = blocks[k], blocks[(k + 1) % len(blocks)]
            u = nr.rows64_elements(even, odd, inverse)
            assert all(w < P for w in u)
            assert nr.rows64_dif(u, inverse) == (list(even), list(odd))
            full = nr.dft(u, inverse)
            for half, block in ((0, even), (1, odd)):
                assert [w % P for w in nr.run(form, block)] == [full[2 * j + half] for j in range(32)]


def test_operand_sets_are_deterministic():
    for name in ("NET32_inv_lazy", "LEVELS3_inv_lazy", "TAIL5_fwd", "PRE2_fwd_half0", "C8_inv_half1"):
        first = nr.operand_sets(nr.FORMS[name])
        nr._operand_sets.cache_clear()
        again = nr.operand_sets(nr.FORMS[name])
        assert first == again and first is not again


def test_all_canonical_builds_get_a_canonical_model():
    """TF_LAZY = 0 or TF_ASM_BFLY = 0: every level canonical, every block of canonical words, the same DFT"""
    for config in ({"lazy": 0, "asm_bfly": 1, "asm_pow2": 1, "pow2_wide": 4}, {"lazy": 1, "asm_bfly": 0, "asm_pow2": 0, "pow2_wide": 2}):
        for name in ("NET32_fwd_lazy", "LEVELS4_inv_lazy", "PRE2_inv_half0", "C8_fwd_half0", "C8_inv_half1"):
            form = nr.FORMS[name]
            assert not nr.is_lazy(form, config)
            blocks, want = nr.expected(form, config)
            assert len(blocks) > 1000
            for b, w in zip(blocks[::17], want[::17]):
                assert all(x < P for x in nr.network_inputs(form, b, config)) and all(x < P for x in w)
                assert list(w) == nr.dft_reference(form, b)


def test_arguments_are_checked_without_a_device(tf):
    """an unknown form or a count that is not a whole number of blocks is an error before the library looks for a device; an empty
    call is fine (no launch)"""
    lib = tf.lib()
    invalid = 17  # TF_ERR_INVALID_ARGUMENT
    assert lib.tf_debug_ntt_network_dev(nr.FORM_COUNT, None, 0, None) == invalid
    assert lib.tf_debug_ntt_network_dev(-1, None, 0, None) == invalid
    for form in nr.FORMS.values():
        assert lib.tf_debug_ntt_network_dev(form.code, None, 0, None) == 0
        assert lib.tf_debug_ntt_network_dev(form.code, None, form.words - 1, None) == invalid
        assert lib.tf_debug_ntt_network_dev(form.code, None, form.words + 32 * (form.words == 64) + 1, None) == invalid
        assert lib.tf_debug_ntt_network_dev(form.code, None, form.words, None) == 7  # TF_ERR_NULL_POINTER
        assert lib.tf_debug_ntt_network_dev(form.code, None, (1 << 32) + 64, None) == invalid
    if nr.FORMS["PRE2_fwd_half0"].words == 64:
        assert lib.tf_debug_ntt_network_dev(nr.FORMS["PRE2_fwd_half0"].code, None, 96, None) == invalid  # a block and a half
    with pytest.raises(KeyError):
        tf.device.debug_ntt_network_("NO_SUCH_FORM", None)
    config = tf.device.debug_ntt_network_config()
    assert set(config) == {"lazy", "asm_bfly", "asm_pow2", "pow2_wide"} and all(v in (0, 1, 2, 4) for v in config.values())
