"""tests/tip5_steer.py checked without a GPU: the integer round is the oracle's, the steered inputs are canonical, both device models
end in the oracle's words, the bounds the kernel comments claim hold, and -- as a condition, not a measurement -- every form's model
takes every nameable event in every round at every output word for at least MIN_STATES states.  The uniform anchors alone do not.
tests/test_gpu_tip5_steer.py runs the kernels on these inputs."""
import collections
import functools

import numpy as np

from tests import field_ref as fr
from tests import tip5_steer as ts

P = ts.P
N_UNIFORM = 10 ** 4
FORMS = ("coop", "mx", "mx_trace")
FIXED_FORMS = ("coop", "mx")
# (the fold wraps -- ca -- about once in 2^13 words: a few of the 20 480 uniform word-rounds take it, far from MIN_STATES per cell)
RARE = {"coop": ("cb", "cb:p", "none:p-1"), "mx": ("gep", "gep:p", "none:p-1", "carry+ripple", "lazy carry+ripple", "lazy>=p"),
        "mx_trace": ("gep", "gep:p", "none:p-1", "carry+ripple")}


def _oracle_trace(oracle, state):
    tr, after = oracle.tip5_trace(np.array(state, dtype=np.uint64))
    tr = [[int(v) for v in row] for row in np.asarray(tr).reshape(6, 16)]
    assert [int(v) for v in after] == tr[5]
    return tr


@functools.lru_cache(maxsize=None)
def _classified():
    """(events of every state of S, final words of every model, the bounds record over S)"""
    states, _ = ts.steered_states()
    bounds = ts.Bounds()
    events, words = [], []
    for s in states:
        cw, ce, recs = ts.coop_run(s)
        assert all(rec["c"][1] == 0 and rec["c"][4] == 0 and not (rec["ca"] and rec["cb"]) for rows in recs for rec in rows)
        mx = ts.mx_run(s, bounds=bounds)
        events.append({"coop": ce, "mx": mx["lazy"][1], "mx_trace": mx["canon"][1]})
        words.append((cw, mx["lazy"][0], mx["canon"][0]))
    return events, words, bounds


@functools.lru_cache(maxsize=None)
def _classified_fixed(cap):
    inputs, _ = ts.fixed_inputs(cap)
    bounds = ts.Bounds()
    events, words = [], []
    for h in inputs:
        state = list(h) + [ts.ONE if cap else 0] * 6
        cw, ce, _ = ts.coop_run(state)
        mx = ts.mx_run(state, fixed0=1 if cap else 2, digest=bool(cap), bounds=bounds)
        events.append({"coop": ce, "mx": mx["lazy"][1]})
        words.append((cw, mx["lazy"][0]))
    return events, words, bounds


def _short_cells(seen, forms, rounds):
    return {(form, r, word, label): seen.get((form, r, word, label), 0) for form in forms for r in rounds for word in range(16)
            for label in ts.required(form, r, word) if seen.get((form, r, word, label), 0) < ts.MIN_STATES}


def _short_fixed(seen):
    short = _short_cells(seen, FIXED_FORMS, (0,))
    short.update({("mx", 1, word, "lazy>=p"): seen.get(("mx", 1, word, "lazy>=p"), 0) for word in range(4, 16)
                  if seen.get(("mx", 1, word, "lazy>=p"), 0) < ts.MIN_STATES})
    return short


def test_lookup_table_and_constants():
    assert sorted(ts.LUT) == list(range(256)) and ts.LUT[0] == 0 and ts.LUT[0xff] == 0xff  # what UNREACHABLE["lookup>=p"] rests on
    assert all(ts.ILUT[ts.LUT[x]] == x for x in range(256))
    assert 7 * ts.D7 % (P - 1) == 1
    inv = ts.mds_inverse()
    assert all(sum(ts.MROW[i][k] * inv[k][j] for k in range(16)) % P == int(i == j) for i in range(16) for j in range(16))
    assert all(0 <= c < P for row in ts.round_constants() for c in row) and len(set(sum(ts.round_constants(), ()))) == 80
    for key, starts in ts.mx_starts().items():
        assert all(ts.BIAS <= v < ts.BIAS + 256 for row in starts for v in row[:8]) and all(row[8:] == [ts.BIAS] * 2 for row in starts), key


def test_integer_round_is_the_oracles_and_inverts(oracle):
    """every state of the trace, on all of S and on 10^4 uniform states; unround(round(x)) == x on every round of S and of the first
    1000 uniform states"""
    states, _ = ts.steered_states()
    uniform = oracle.fill_random(16 * N_UNIFORM, 0x7374656572).reshape(N_UNIFORM, 16)
    for i, s in enumerate(list(states) + [[int(v) for v in row] for row in uniform]):
        tr = ts.trace(s)
        assert tr == _oracle_trace(oracle, s), i
        if i % 97 == 0:
            assert tr[5] == [int(v) for v in oracle.tip5_permutation(np.array(s, dtype=np.uint64))]
        if i < len(states) + 1000:
            for r in range(5):
                assert ts.unround(tr[r + 1], r) == tr[r], (i, r)


def test_inputs_are_canonical_and_distinct():
    states, classes = ts.steered_states()
    assert len(states) == len(classes) <= 4000 and len(set(states)) == len(states)
    assert all(len(s) == 16 and all(0 <= w < P for w in s) for s in states)
    assert sum(c == "e:uniform" for c in classes) == ts.N_UNIFORM
    for cap in (0, 1):
        inputs, labels = ts.fixed_inputs(cap)
        assert len(inputs) == len(labels) and len(set(inputs)) == len(inputs)
        assert all(len(h) == 10 and all(0 <= w < P for w in h) for h in inputs)


def test_both_models_end_in_the_oracles_words(oracle):
    states, classes = ts.steered_states()
    _, words, _ = _classified()
    for s, c, (cw, lw, tw) in zip(states, classes, words):
        want = [int(v) for v in oracle.tip5_permutation(np.array(s, dtype=np.uint64))]
        assert cw == want and lw == want and tw == want, c
    for cap in (0, 1):
        inputs, labels = ts.fixed_inputs(cap)
        _, words, _ = _classified_fixed(cap)
        for h, c, (cw, mw) in zip(inputs, labels, words):
            want = [int(v) for v in oracle.tip5_permutation(np.array(list(h) + [ts.ONE if cap else 0] * 6, dtype=np.uint64))]
            assert cw == want, c
            # the digest round (cap = 1) finishes words 0..7 only
            assert mw[:8] == want[:8] and (mw[8:] == [None] * 8 if cap else mw[8:] == want[8:]), c
            if cap:
                assert want[:5] == [int(v) for v in oracle.hash_10(np.array(h, dtype=np.uint64))]


def test_steered_folds_hold_their_targets():
    """class (b): the fold of the chosen (round, row) holds exactly the value it was steered to"""
    states, classes = ts.steered_states()
    events, _, _ = _classified()
    coop = {"p-1": "none:p-1", "p": "cb:p", "max": "cb", "gep": "cb", "wrap0": "ca", "wrap": "ca"}
    mx = {"p-1": "none:p-1", "p": "gep:p", "max": "gep", "gep": "gep", "carry0": "carry+ripple", "carry": "carry", "ripple": "carry+ripple"}
    n = 0
    for s, c, ev in zip(states, classes, events):
        if c.startswith("b:"):
            _, form, r, row, name = c.split(":")
            r, row = int(r[1:]), int(row[3:])
            assert (coop[name] in ev["coop"][r][row]) if form == "coop" else (mx[name] in ev["mx_trace"][r][row]), c
            post = []
            ts.trace(s, post)
            value, _ = ts._prefold(form, post[r], r, row, 16)
            exact = {"p-1": P - 1, "p": P, "max": ts.M64, "wrap0": 1 << 64, "carry0": 1 << 64}
            assert value == exact.get(name, value) and (name in exact or value > P), c
            n += 1
    assert n == 5 * 16 * (6 + 7)


def test_bounds_the_kernel_comments_claim(oracle):
    """|P_p| < 2^20, 0 <= Q_p < 2^22, hsum < 2^15 + 2^31, u < 2^64, t < T_BOUND, no 32-bit intermediate wraps: over S and H in the
    models, and over the 10^4 uniform states' five rounds in one numpy pass (u bounded by max hsum (2^32 - 1) + max L0)"""
    for b in (_classified()[2], _classified_fixed(0)[2], _classified_fixed(1)[2]):
        assert b.hold(), vars(b)
    uniform = oracle.fill_random(16 * N_UNIFORM, 0x7374656572).reshape(N_UNIFORM, 16)
    post = [[] for _ in range(N_UNIFORM)]
    for i, row in enumerate(uniform):
        ts.trace([int(v) for v in row], post[i])
    ma = np.stack(ts._MA)
    for r in range(5):
        t = np.array([post[i][r] for i in range(N_UNIFORM)], dtype=np.uint64)
        d = t.view(np.uint8).reshape(N_UNIFORM, 16, 8).astype(np.int64) - 128
        planes = np.zeros((N_UNIFORM, 16, 10), dtype=np.int64)
        for a in range(3):
            planes[:, :, a:a + 8] += np.einsum("rc,ncb->nrb", ma[a], d)
        assert np.array_equal(planes[7], ts.mx_planes(post[7][r]))
        q = planes + np.array(ts.mx_starts()[r], dtype=np.int64)[None]
        assert np.abs(planes).max() < 1 << 20 and q.min() >= 0 and q.max() < 1 << 22
        l0 = q[..., 0] + (q[..., 1] << 8) + (q[..., 2] << 16) + (q[..., 3] << 24)
        l1 = q[..., 4] + (q[..., 5] << 8) + (q[..., 6] << 16) + (q[..., 7] << 24)
        hsum = (l1 >> 32) + q[..., 8] + (q[..., 9] << 8)
        assert int(hsum.max()) < (1 << 15) + (1 << 31)
        assert int(hsum.max()) * ts.M32 + int(l0.max()) < fr.T_BOUND < 1 << 64


def test_plane_extremes_are_the_sign_rules(oracle):
    """class (d): the model's plane of the chosen (round, row) equals the value the sign rule gives, computed without the model; the
    largest of them is the largest |P_p| the whole set sees, and it is below 2^20"""
    states, classes = ts.steered_states()
    top = 0
    for s, c in zip(states, classes):
        if c.startswith("d:") and ":plane" in c:
            _, r, row, plane, which = c.split(":")
            r, row, plane, sign = int(r[1:]), int(row[3:]), int(plane[5:]), 1 if which == "max" else -1
            post = []
            ts.trace(s, post)
            got = int(ts.mx_planes(post[r])[row][plane])
            assert got == ts.plane_extreme_value(row, plane, sign), c
            top = max(top, abs(got))
    assert top == _classified()[2].abs_p < 1 << 20
    for cap in (0, 1):
        fixed = ts.ONE if cap else 0
        inputs, labels = ts.fixed_inputs(cap)
        for h, c in zip(inputs, labels):
            if c.startswith("d:"):
                _, _, row, plane, which = c.split(":")
                row, plane, sign = int(row[3:]), int(plane[5:]), 1 if which == "max" else -1
                t = ts.sbox(list(h) + [fixed] * 6)
                assert int(ts.mx_planes(t, 12)[row][plane]) == ts.plane_extreme_value(row, plane, sign, free=10, fixed=fixed, nw=12), c


def test_every_event_in_every_round_at_every_word():
    """the coverage condition on S: every form's model, every round, every output word, every label required() lists, at least
    MIN_STATES states each; nothing that UNREACHABLE lists ever occurs"""
    events, _, _ = _classified()
    seen = ts.coverage(events, FORMS, range(5))
    short = _short_cells(seen, FORMS, range(5))
    assert not short, short
    assert not any(key[3] in ts.UNREACHABLE for key in seen)
    allowed = set(ts.COOP_EVENTS) | set(ts.CANON_LABELS) | set(ts.LAZY_LABELS) | {"lazy>=p"}
    assert {key[3] for key in seen} <= allowed
    assert not any(label.startswith(bad) for label in allowed for bad in fr.impossible("MX_FOLD4_CANON"))
    # per form: the number of states that took each event at each round (any word)
    table = collections.defaultdict(lambda: [0] * 5)
    for ev in events:
        for form in FORMS:
            for r in range(5):
                for label in set().union(*ev[form][r]):
                    table[(form, label)][r] += 1
    for (form, label), counts in sorted(table.items()):
        print(f"S  {form:9s} {label:18s} states per round 0..4: {counts}")


def test_every_event_in_round_0_of_the_fixed_forms():
    for cap in (0, 1):
        events, _, _ = _classified_fixed(cap)
        seen = ts.coverage(events, FIXED_FORMS, range(2))
        short = _short_fixed(seen)
        assert not short, (cap, short)
        assert not any(key[3] in ts.UNREACHABLE for key in seen)
        table = collections.Counter((form, label) for ev in events for form in FIXED_FORMS for label in set().union(*ev[form][0]))
        table.update(("mx", "lazy>=p (round 1)") for ev in events if any("lazy>=p" in e for e in ev["mx"][1]))
        for (form, label), n in sorted(table.items()):
            print(f"H cap {cap}  {form:5s} {label:18s} states at round 0: {n}")


def test_uniform_states_alone_would_not_do():
    """the negative twin: the 256 uniform anchors fail the same condition in every form -- they take none of the rare labels at all"""
    states, classes = ts.steered_states()
    events, _, _ = _classified()
    uniform = [ev for ev, c in zip(events, classes) if c == "e:uniform"]
    assert len(uniform) == ts.N_UNIFORM
    seen = ts.coverage(uniform, FORMS, range(5))
    for form in FORMS:
        assert _short_cells(seen, (form,), range(5)), form
        assert not any(key[0] == form and key[3] in RARE[form] for key in seen), form
    for cap in (0, 1):  # and the fixed forms on 256 uniform inputs
        rng = __import__("random").Random(cap)
        evs = [ts.classify_fixed([rng.randrange(P) for _ in range(10)], cap)[0] for _ in range(ts.N_UNIFORM)]
        assert _short_fixed(ts.coverage(evs, FIXED_FORMS, range(2)))


def test_unreachable_events_are_listed_with_a_reason():
    assert all(len(why) > 20 for why in ts.UNREACHABLE.values())
    assert {"lookup>=p", "ca+cb", "c1", "c4", "tail gep+ripple", "tail lazy gep"} <= set(ts.UNREACHABLE)
    # the lookup argument, at the words that come closest: the largest canonical words and every word of equal bytes
    for w in [P - 1, P - 2, P - (1 << 32), 0xfffffffeffffffff] + [int.from_bytes(bytes([b] * 8), "little") % P for b in range(256)]:
        assert ts.lookup(w) < P and ts.lookup(w, ts.ILUT) < P
    for hi in range(255):  # a post-lookup word >= p has no canonical pre-image
        assert ts.lookup(P + hi * 0x01010101, ts.ILUT) >= P
