"""Word-exact integer model, operand sets and carry-path events for the register networks of the NTT kernels (csrc/ntt_network.h) and
the glue that hands words to their first level (csrc/ntt_kernels.h: pre2_combine8, pre2_shift, c8_combine8), as tf_debug_ntt_network_dev
runs them one composition ("form") at a time.  Python integers only: nothing here comes from the library or from the oracle.

The model is written from the comments of ntt_network.h and knows nothing of the order in which a level's butterflies run:
  Bf<INV, LVL, I>   butterfly I of level LVL pairs slots ia = (I / H) 2 H + I % H and ib = ia + H, H = 2^(LVL-1), with the twiddle
                    2^E, E = +-39 * 2^(6-LVL) * (I % H) mod 192; neg = the power-of-two product comes back negated
  twiddled operand  v = canonical(b) * 2^E mod p up to the sign neg -- a canonical word; E = 0 passes b through (level 1 and the
                    canonical networks, whose b is canonical by contract) or reduces it (lazy levels above the first)
  lazy level        s = field_ref.lazy_sum(a, v), d = field_ref.lazy_diff(a, v): a is any 64-bit word and so are s and d
  canonical level   s = (a + v) % p, d = (a - v) % p
  outputs           (x[ia], x[ib]) = (d, s) when neg, else (s, d)
class_fused / leftover_fused re-order the butterflies of a level by exponent class and promise "the same words as butterfly_pair":
that promise is what the GPU test checks, so the model runs the butterflies in index order and nothing else.

What pins the model: reduced mod p, its outputs are the n-point (i)DFT  sum_i x_i w^(+-ik)  with the reference's primitive roots
(dft_reference, which knows nothing of butterflies).  tests/test_network_cpu.py asserts that on every operand set.

Operand sets are BUILT, not searched.  A block leaves all but two to four slots of a group zero: a lone word passes first-operand
positions unchanged (a +- 0 = a as a word), so a word placed at the first slot of a sub-group of 2^m slots comes out of levels 1 .. m on
every slot of the sub-group, and the pair (a, b) a butterfly of level m + 1 sees is the pair of words placed in its two sub-groups.  A
word >= p that the input contract does not admit is made one level down as the sum of two canonical words (_make).
"""
import functools
import random

from tests import field_ref as fr
from tests import pyref

P, M64, M32, EPS = fr.P, fr.M64, fr.M32, fr.EPS
DEFAULT_CONFIG = {"lazy": 1, "asm_bfly": 1, "asm_pow2": 1, "pow2_wide": 4}
_POW2 = [pow(2, e, P) for e in range(192)]


# ------------------------------------------------------------------------------------------------------------- the network's pieces
def tw_exp(inv, lvl, j):  # TwExp<INV, LVL, J>::value
    fwd = ((39 << (6 - lvl)) * j) % 192
    return (192 - fwd) % 192 if inv else fwd


def pow2_neg(e):  # gl::Pow2Mul<E>::negate
    e %= 192
    return (e >= 96) != (e % 96 >= 32)


def pow2_apply(e, x):
    """gl::Pow2Mul<E>::apply: the canonical word v with x 2^E = (negate ? -v : v) for ANY 64-bit x; 2^0 and 2^96 pass x through"""
    e %= 192
    if e % 96 == 0:
        return x
    v = x % P * _POW2[e] % P
    return (P - v) % P if pow2_neg(e) else v


def brev(q, bits):
    return int(format(q, f"0{bits}b")[::-1], 2) if bits else 0


@functools.lru_cache(maxsize=None)
def bf(inv, lvl, i):
    """Bf<INV, LVL, I> -> (ia, ib, E, neg)"""
    h = 1 << (lvl - 1)
    j = i % h
    ia = (i // h) * 2 * h + j
    e = tw_exp(inv, lvl, j)
    return ia, ia + h, e, pow2_neg(e)


def tw_operand(e, lazy_in, b):
    if e % 192 == 0:
        return b % P if lazy_in else b  # b < 2^64 < 2 p:  b >= p ? b - p : b
    return pow2_apply(e, b)


def butterfly(x, inv, lvl, i, lazy, trace=None):
    ia, ib, e, neg = bf(inv, lvl, i)
    a, b = x[ia], x[ib]
    v = tw_operand(e, lazy and lvl > 1, b)
    if lazy:
        s, d = fr.lazy_sum(a, v), fr.lazy_diff(a, v)
    else:
        s, d = (a + v) % P, (a - v) % P
    if trace is not None:
        trace(lvl, i, a, b, v, lazy)
    x[ia], x[ib] = (d, s) if neg else (s, d)


# ------------------------------------------------------------------------------------------------------------- the glue
@functools.lru_cache(maxsize=None)
def pre2_slot(inv, q):
    """Pre2Slot<INV, Q> -> (E, neg): slot Q holds row brev5(Q) of the decimation-in-frequency stage, twiddle w_64^brev5(Q)"""
    e = tw_exp(inv, 6, brev(q, 5))
    return e, pow2_neg(e)


def pre2_combine(x, w, inv, odd, tf_lazy=1, trace=None):
    """the four pre2_combine8 calls: slots 0 .. 31 against their partner words"""
    for q in range(32):
        if trace is not None:
            trace(0, q, x[q], w[q], w[q], False)
        if odd:
            x[q] = (w[q] - x[q]) % P if pre2_slot(inv, q)[1] else (x[q] - w[q]) % P
        elif (q & 1) or not tf_lazy:
            x[q] = (x[q] + w[q]) % P
        else:
            s = (x[q] + w[q]) & M64
            x[q] = s + EPS if s < w[q] else s


def pre2_shift(x, inv, first=1, end=32):
    for q in range(first, end):
        x[q] = pow2_apply(pre2_slot(inv, q)[0], x[q])


def c8_combine(x, w, inv, odd, trace=None):
    """the four c8_combine8 calls: lazy differences with the slot's sign folded in (odd half); lazy sums on the even slots and
    canonical sums on the odd ones (even half)"""
    for q in range(32):
        if trace is not None:
            trace(0, q, x[q], w[q], w[q], False)
        if odd:
            a, v = (w[q], x[q]) if pre2_slot(inv, q)[1] else (x[q], w[q])
            x[q] = fr.lazy_diff(a, v)
        elif q & 1:
            x[q] = (x[q] + w[q]) % P
        else:
            x[q] = fr.lazy_sum(x[q], w[q])


# ------------------------------------------------------------------------------------------------------------- the forms
class Form:
    """one composition: name, code (include/tf_hip.h), words per block, direction, kind, the ranges (lvl, i0, end) of butterflies it
    runs in order, whether they are lazy, and for the glue forms which half"""

    def __init__(self, name, code, kind, inv, lazy, ranges, logn, half=None):
        self.name, self.code, self.kind, self.inv, self.lazy, self.ranges, self.logn, self.half = name, code, kind, inv, lazy, ranges, logn, half
        self.words = 64 if kind in ("PRE2", "C8") else 32
        self.slots = 8 if kind == "LAT" else 32  # slots the network touches

    def __repr__(self):
        return self.name

    def butterflies(self):
        return [(lvl, i) for lvl, i0, end in self.ranges for i in range(i0, end)]


def _half_ranges():
    return [(lvl, first // 2, first // 2 + 8) for first in (0, 16) for lvl in (1, 2, 3, 4)]


def _forms():
    out = {}
    for inv in (0, 1):
        d = "inv" if inv else "fwd"
        net32 = _half_ranges() + [(5, 0, 16)]
        for v, (name, lazy) in enumerate((("lazy", True), ("lazy_wide2", True), ("canonical", False))):
            out[f"NET32_{d}_{name}"] = Form(f"NET32_{d}_{name}", 2 * v + inv, "NET32", inv, lazy, net32, 5)
        for p2 in range(1, 6):
            for lazy in (0, 1):
                n = f"LEVELS{p2}_{d}_{'lazy' if lazy else 'canonical'}"
                out[n] = Form(n, 6 + 4 * (p2 - 1) + 2 * lazy + inv, "LEVELS", inv, bool(lazy), [(lvl, 0, 16) for lvl in range(1, p2 + 1)], p2)
        out[f"TAIL5_{d}"] = Form(f"TAIL5_{d}", 26 + inv, "TAIL5", inv, False, _half_ranges() + [(5, q0, q0 + 4) for q0 in (0, 4, 8, 12)], 5)
        for logr in (1, 2, 3):
            out[f"LAT{logr}_{d}"] = Form(f"LAT{logr}_{d}", 28 + 2 * (logr - 1) + inv, "LAT", inv, False, [(lvl, 0, 4) for lvl in range(1, logr + 1)], logr)
        for half in (0, 1):
            out[f"PRE2_{d}_half{half}"] = Form(f"PRE2_{d}_half{half}", 34 + 2 * half + inv, "PRE2", inv, True, net32, 5, half)
            out[f"C8_{d}_half{half}"] = Form(f"C8_{d}_half{half}", 38 + 2 * half + inv, "C8", inv, True, [(lvl, 0, 16) for lvl in range(1, 6)], 5, half)
    return out


FORMS = _forms()
FORM_COUNT = 42


def is_lazy(form, config=None):
    """do the form's levels run lazy in a library built with these switches?  (TF_LAZY = 0: every network canonical; TF_ASM_BFLY = 0:
    butterfly_pow2, canonical in and out)"""
    c = config or DEFAULT_CONFIG
    return bool(form.lazy and c["lazy"] and c["asm_bfly"])


def run(form, block, config=None, trace=None):
    """the 32 words the form leaves in place of block[:32]; trace(lvl, i, a, b, v, lazy) sees every butterfly (lvl = 0: the glue's
    slot i with its pair (x, w))"""
    c = config or DEFAULT_CONFIG
    lazy = is_lazy(form, c)
    x = list(block[:32])
    if form.kind == "PRE2":
        pre2_combine(x, block[32:], form.inv, form.half, c["lazy"], trace)
        if form.half:
            pre2_shift(x, form.inv)
    elif form.kind == "C8":
        c8_combine(x, block[32:], form.inv, form.half, trace)
        if form.half:
            pre2_shift(x, form.inv)
    for lvl, i0, end in form.ranges:
        for i in range(i0, end):
            butterfly(x, form.inv, lvl, i, lazy, trace)
    return x


def network_inputs(form, block, config=None):
    """the words the form's first level sees (= the block itself, or what the glue makes of it)"""
    c = config or DEFAULT_CONFIG
    x = list(block[:32])
    if form.kind == "PRE2":
        pre2_combine(x, block[32:], form.inv, form.half, c["lazy"])
    elif form.kind == "C8":
        c8_combine(x, block[32:], form.inv, form.half)
    if form.kind in ("PRE2", "C8") and form.half:
        pre2_shift(x, form.inv)
    return x


# ------------------------------------------------------------------------------------------------------------- the plain DFT
@functools.lru_cache(maxsize=None)
def _root_powers(n, inverse):
    w = pyref.root_of_unity(n)
    if inverse:
        w = pow(w, P - 2, P)
    return [pow(w, k, P) for k in range(n)]


def dft(vals, inverse=False):
    """sum_i x_i w_n^(+-ik) mod p, n = len(vals) a power of two up to 64, NO scaling by 1 / n; w_n = pyref.root_of_unity(n).  The words
    may be raw Montgomery words or values alike: the transform is linear, and a word stands for word * 2^-64."""
    n = len(vals)
    pw = _root_powers(n, bool(inverse))
    return [sum(x * pw[i * k % n] for i, x in enumerate(vals)) % P for k in range(n)]


def dft_reference(form, block):
    """the residues mod p the form's 32 outputs must have, from the plain DFT: groups of n = 2^logn slots are n-point transforms with
    bit-reversed inputs and natural outputs; the glue forms are the even (half 0) or odd (half 1) outputs of a 64-point transform of
    u[brev5(q)] = x[q], u[32 + brev5(q)] = w[q]"""
    if form.kind in ("PRE2", "C8"):
        u = [0] * 64
        for q in range(32):
            u[brev(q, 5)], u[32 + brev(q, 5)] = block[q], block[32 + q]
        full = dft(u, form.inv)
        return [full[2 * k + form.half] for k in range(32)]
    n = 1 << form.logn
    out = [w % P for w in block[:32]]
    for base in range(0, form.slots, n):
        out[base:base + n] = dft([block[base + brev(j, form.logn)] for j in range(n)], form.inv)
    return out


# ------------------------------------------------------------------------------------------------------------- contracts, events
def slot_admits(form, q, word, config=None):
    """the input contract: lazy forms take any word on even slots and words < p on odd ones (the second operands of level 1); canonical
    forms and both blocks of the glue forms take words < p"""
    if form.kind in ("PRE2", "C8") or not is_lazy(form, config):
        return word < P
    return word <= M64 if q % 2 == 0 else word < P


def block_in_contract(form, block, config=None):
    if not all(slot_admits(form, q % 32, w, config) for q, w in enumerate(block)):
        return False
    if form.kind in ("PRE2", "C8") and not is_lazy(form, config):  # a canonical network behind the glue takes canonical words only
        return all(w < P for w in network_inputs(form, block, config))
    return True


LAZY_LABELS = [(0, "none"), (0, "carry"), (0, "carry+ripple"), (1, "none"), (1, "borrow"), (1, "borrow+ripple")]
CANONICAL_LABELS = [(0, "none"), (0, "borrow"), (0, "borrow+ripple"), (1, "none"), (1, "borrow"), (1, "borrow+ripple")]
# the last three are where a second operand that stayed >= p would show: with v = b - p < 2^32 - 1 in place of b, the words of the sum and
# the difference change only if a < v, a >= b or a + v >= 2^64 -- any other pair hides a missing canonicalisation behind the lazy
# corrections (a + b wraps to a + v, a - b borrows to a - v)
# (the third, a + v >= 2^64, is the one pair on which an uncanonicalised b gives a word that is not even congruent: a + b wraps twice)
CONDITIONS = ("a>=p", "b>=p", "a>=p&carry+ripple", "b>=p&borrow", "b>=p&a>=b", "b>=p&carry")


def classify(lvl, a, b, v, lazy):
    """what the pair (a, v) of one butterfly takes: [(output, label)] for the sum and the difference (field_ref.event, labels of
    ADD_SUB_LAZY2 or ADD_SUB2), and the conditions that hold"""
    op = "ADD_SUB_LAZY2" if lazy else "ADD_SUB2"
    labels = [(0, fr.event(op, 0, 0, a, v)[0]), (1, fr.event(op, 1, 0, a, v)[0])]
    conds = []
    if a >= P:
        conds.append("a>=p")
        if labels[0][1] == "carry+ripple":
            conds.append("a>=p&carry+ripple")
    if b >= P and lvl > 1:
        conds.append("b>=p")
        if a < v:
            conds.append("b>=p&borrow")
        if a >= b:
            conds.append("b>=p&a>=b")
        if a + v > M64:
            conds.append("b>=p&carry")
    return labels, conds


def glue_label(form, q, x, w, config=None):
    """the path slot q's pair takes through the glue, in the labels of the field_ref op that does the same arithmetic"""
    c = config or DEFAULT_CONFIG
    if form.kind == "PRE2":
        if form.half:
            a, v = (w, x) if pre2_slot(form.inv, q)[1] else (x, w)
            return "SUB " + fr.event("SUB", 0, 0, a, v)[0]
        if (q & 1) or not c["lazy"]:
            return "ADD " + fr.event("ADD", 0, 0, x, w)[0]
        return "ADD_LAZY " + fr.event("ADD_LAZY4", 0, q // 2 % 4, x, w)[0]
    if form.half:
        a, v = (w, x) if pre2_slot(form.inv, q)[1] else (x, w)
        return "SUB_LAZY " + fr.event("SUB_LAZY4", 0, q % 4, a, v)[0]
    if q & 1:
        return "ADD " + fr.event("ADD", 0, 0, x, w)[0]
    return "ADD_LAZY " + fr.event("ADD_LAZY4", 0, q // 2 % 4, x, w)[0]


def glue_reachable(form, q, config=None):
    c = config or DEFAULT_CONFIG
    if form.half:
        return ["SUB" + ("_LAZY " if form.kind == "C8" else " ") + l for l in ("none", "borrow", "borrow+ripple")]
    if (q & 1) or (form.kind == "PRE2" and not c["lazy"]):
        return ["ADD " + l for l in ("none", "carry", "carry+ripple", "gep")]
    return ["ADD_LAZY " + l for l in ("none", "carry", "carry+ripple")]


# Which words >= p can a slot hold?  By recursion over the network, from what the first level is handed:
#   * a canonical level reduces both outputs: never;
#   * the SUM of a lazy level: always -- a + v lies in [p, 2^64) for suitable canonical a and v, whatever else a may be;
#   * the DIFFERENCE of a lazy level: only if its first operand can be >= p (then v = 0 passes it through).  A difference of canonical
#     words is canonical: a >= v gives a - v < p, and a < v gives a - v + 2^64 - (2^32 - 1) = a - v + p < p.
# So from canonical inputs a slot holds a word >= p after level l only if a sum lies upstream in its first-operand chain.
WHY_NOT = {
    "canonical": "every level of the form is canonical: its operands are < p by contract and its outputs are reduced",
    "a>=p": "the first operand is reached from words < p through differences only, and a difference of canonical words is canonical",
    "b>=p": "the second operand is reached from words < p through differences only, and a difference of canonical words is canonical",
    "a>=p&carry+ripple": "needs a first operand >= p, which this butterfly cannot see (see a>=p)",
    "b>=p&borrow": "needs a second operand >= p, which this butterfly cannot see (see b>=p)",
    "b>=p&a>=b": "needs both operands >= p, and this butterfly cannot see one of them so (see a>=p, b>=p)",
    "b>=p&carry": "aimed at with a first operand in [2^64 - v, 2^64) and b >= p, and this butterfly cannot see one of them so (see a>=p, b>=p)",
}


def first_level_can_exceed(form, config=None):
    """per slot: may the word the first level sees be >= p?"""
    if not is_lazy(form, config):
        return [False] * 32
    if form.kind in ("PRE2", "C8"):
        # even half: the lazy sum of two canonical words on the even slots is any word; odd half: pre2 takes canonical differences, c8
        # lazy differences of canonical words (canonical, above), and the shift reduces every slot but 0
        return [not form.half and q % 2 == 0 for q in range(32)]
    return [q % 2 == 0 for q in range(32)]


@functools.lru_cache(maxsize=None)
def _reach(name, canonical_inputs, config_key):
    form, config = FORMS[name], dict(config_key)
    lazy = is_lazy(form, config)
    can = [False] * 32 if canonical_inputs else first_level_can_exceed(form, config)
    reach, excluded = {}, {}
    for lvl, i in form.butterflies():
        ia, ib, _, neg = bf(form.inv, lvl, i)
        upper = lvl > 1
        for cond, ok in (("a>=p", can[ia]), ("b>=p", can[ib] if upper else None), ("a>=p&carry+ripple", can[ia]),
                         ("b>=p&borrow", can[ib] if upper else None), ("b>=p&a>=b", (can[ia] and can[ib]) if upper else None),
                         ("b>=p&carry", (can[ia] and can[ib]) if upper else None)):
            if ok is None:
                continue  # (level 1: its second operand is canonical by contract, and tw_operand does not look at it)
            if ok:
                reach.setdefault((lvl, i), set()).add(cond)
            else:
                excluded[(lvl, i, cond)] = WHY_NOT["canonical" if not lazy else cond]
        s, d = lazy, lazy and can[ia]
        can[ia], can[ib] = (d, s) if neg else (s, d)
    return reach, excluded


def reachable_conditions(form, canonical_inputs=False, config=None):
    """-> ({(lvl, i): set of conditions that some in-contract block produces}, {(lvl, i, condition): why none does})"""
    return _reach(form.name, bool(canonical_inputs), tuple(sorted((config or DEFAULT_CONFIG).items())))


def labels_of(form, config=None):
    return LAZY_LABELS if is_lazy(form, config) else CANONICAL_LABELS


# ------------------------------------------------------------------------------------------------------------- building blocks
def _multiplier(inv, lvl, i):
    """T with v = canonical(b) * T mod p at butterfly (lvl, i), and 1 / T"""
    _, _, e, neg = bf(inv, lvl, i)
    t = _POW2[e % 192]
    t = (P - t) % P if (neg and e % 96) else t  # (e = 0 passes b through: no sign)
    return t, pow(t, P - 2, P)


def _make(form, lazy, admits, s, m, word):
    """input words (slot -> word; the other inputs of the sub-group of 2^m slots around s are zero) that leave `word` on slot s after
    levels 1 .. m, or None if no in-contract inputs do"""
    if m == 0:
        return {s: word} if admits(s, word) else None
    base = s >> m << m
    if admits(base, word):  # a lone word on the sub-group's first slot comes out on every slot of the sub-group
        return {base: word}
    if not lazy:
        return None
    h = 1 << (m - 1)
    i = (base >> m) * h + (s - base) % h  # the butterfly of level m that writes slot s
    ia, ib, _, neg = bf(form.inv, m, i)
    assert s in (ia, ib)
    if (s == ia) != neg:  # slot s takes the sum: two canonical words c1 + c2 = word
        c2 = word - (P - 1) + (word * 0x9E3779B97F4A7C15 >> 7) % (2 * (P - 1) - word + 1)
        c1 = word - c2
        assert c1 < P and c2 < P
        return {base: c1, base + h: c2 * _multiplier(form.inv, m, i)[1] % P}
    return _make(form, lazy, admits, ia, m - 1, word)  # slot s takes the difference: the first operand as it is, minus 0


KINDS_LAZY = ("none", "carry", "carry+ripple", "borrow", "borrow+ripple") + CONDITIONS
KINDS_CANONICAL = ("none", "sum-none", "sum-borrow", "sum-borrow+ripple", "borrow", "borrow+ripple")


def _pair(rng, kind, a_max, b_lazy, t_inv, t=1):
    """(a, b) for one butterfly with multiplier T: a < a_max (p or 2^64), b canonical unless the kind asks otherwise"""
    for _ in range(64):
        v = rng.getrandbits(64) % P
        if kind == "none":  # no carry, no borrow
            v >>= 1 + rng.getrandbits(5)
            a = v + rng.getrandbits(64) % (min(a_max, M64 + 1 - v) - v)
        elif kind == "carry":
            v |= 1 << 63
            a = M64 + 1 - v + rng.getrandbits(62)
        elif kind == "carry+ripple":
            v |= 1 << 63
            a = M64 + 1 + (rng.getrandbits(30) << 32) - v
        elif kind == "borrow":
            a = rng.getrandbits(64) % (v or 1)
        elif kind == "borrow+ripple":
            v |= 1 << 62
            a = v - 1 - (rng.getrandbits(32) % (v >> 32) << 32)
        elif kind == "a>=p":
            a = P + rng.getrandbits(32) % EPS
        elif kind == "a>=p&carry+ripple":  # a = 2^64 - r, v = (h << 32) + r, 1 <= r <= 2^32 - 1
            r = 1 + rng.getrandbits(32) % EPS
            v = (rng.getrandbits(32) % (M32 - 1) << 32) + r
            a = M64 + 1 - r
        elif kind == "b>=p":
            b = P + rng.getrandbits(32) % EPS
            return rng.getrandbits(64) % a_max, b
        elif kind == "b>=p&borrow":  # a below the small canonical word b - p (times the twiddle)
            b = P + rng.getrandbits(32) % EPS
            v = (b - P) * t % P
            if v == 0:
                continue
            return rng.getrandbits(64) % v, b
        elif kind == "b>=p&carry":
            b = P + rng.getrandbits(32) % EPS
            v = (b - P) * t % P
            if v == 0:
                continue
            return M64 + 1 - v + rng.getrandbits(64) % v, b
        elif kind == "b>=p&a>=b":
            b = P + rng.getrandbits(32) % EPS
            return b + rng.getrandbits(32) % (M64 + 1 - b), b
        elif kind in ("sum-none", "gep"):  # a + v in [p, 2^64): no borrow in a - (p - v); gl::add corrects without a carry
            v |= 1 << 40
            a = P - v + rng.getrandbits(64) % min(EPS if kind == "gep" else v, v)
        elif kind == "sum-borrow":  # canonical levels: the sum is a - (p - v), + p on borrow
            a = rng.getrandbits(64) % (P - v)
        elif kind == "sum-borrow+ripple":
            v >>= 2
            n = P - v
            a = n - 1 - (rng.getrandbits(32) % (n >> 32) << 32)
        else:
            raise KeyError(kind)
        if 0 <= a < a_max and v < P:
            b = v * t_inv % P
            if b_lazy and b + P <= M64 and rng.getrandbits(1):
                b += P
            return a, b
    raise AssertionError(f"no operands for {kind}")


def _glue_inputs(form, net, rng):
    """(x, w) blocks of canonical words of which the glue (and the shift) makes the network inputs `net`"""
    x, w = [0] * 32, [0] * 32
    for q, word in net.items():
        if not form.half:
            if word < P and rng.getrandbits(1):
                x[q] = word
            else:  # word = c1 + c2 without a carry
                lo = max(0, word - (P - 1))
                x[q] = lo + rng.getrandbits(64) % (min(P - 1, word) - lo + 1)
                w[q] = word - x[q]
            continue
        assert word < P
        e, neg = pre2_slot(form.inv, q)
        t = 1 if q == 0 else _POW2[e] if not neg else (P - _POW2[e]) % P  # the shift's multiplier (slot 0 has none)
        u = word * pow(t, P - 2, P) % P  # the difference the shift must see:  neg ? w - x : x - w
        c = rng.getrandbits(64) % P if rng.getrandbits(1) else 0
        x[q], w[q] = ((c, (u + c) % P) if neg else ((u + c) % P, c))
    return x + w


def constructed(form, canonical_inputs=False, config=None, reps=8, seed=0x6E6574):
    """[(block, [(lvl, i, kind, a, b)])]: for every level of the form, every kind its butterflies can take, every butterfly index j
    within a group and `reps` draws, one block that aims butterfly j of EVERY group of that level at the kind."""
    lazy = is_lazy(form, config)
    rng = random.Random(seed + 977 * form.code + canonical_inputs)
    net_can = [False] * 32 if canonical_inputs else first_level_can_exceed(form, config)
    reach, _ = reachable_conditions(form, canonical_inputs, config)

    def admits(q, word):  # what the first level may be handed on slot q
        return word < P or (net_can[q] and word <= M64)

    present = {}
    for lvl, i in form.butterflies():
        present.setdefault(lvl, []).append(i)
    out = []
    for lvl, idx in sorted(present.items()):
        h = 1 << (lvl - 1)
        for kind in (KINDS_LAZY if lazy else KINDS_CANONICAL):
            for j in range(h):
                targets = [i for i in idx if i % h == j and (kind not in CONDITIONS or kind in reach.get((lvl, i), ()))]
                if not targets:
                    continue
                # ... and, where the level is not the form's last, two blocks that aim the butterfly of the FIRST group alone: with zeros
                # everywhere else its two output words ride first-operand positions to the end unchanged, whereas a dense block lets the
                # next level reduce or re-wrap them (a word that is congruent but not the documented one would go unseen)
                solo = 2 if lvl < max(present) and targets[0] == j else 0
                for rep in range(reps + solo):
                    net, aims = {}, []
                    for i in (targets if rep < reps else targets[:1]):
                        ia, ib, _, _ = bf(form.inv, lvl, i)
                        conds = reach.get((lvl, i), ())
                        t, t_inv = _multiplier(form.inv, lvl, i)
                        a, b = _pair(rng, kind, M64 + 1 if "a>=p" in conds else P, "b>=p" in conds, t_inv, t)
                        ma, mb = _make(form, lazy, admits, ia, lvl - 1, a), _make(form, lazy, admits, ib, lvl - 1, b)
                        assert ma is not None and mb is not None, (form, lvl, i, kind)
                        net.update(ma)
                        net.update(mb)
                        aims.append((lvl, i, kind, a, b))
                    if form.kind in ("PRE2", "C8"):
                        block = _glue_inputs(form, net, rng)
                    else:
                        block = [net.get(q, 0) for q in range(32)]
                    out.append((block, aims))
    return out


def glue_blocks(form, config=None, reps=8):
    """blocks of the glue forms that take every slot's sum or difference over each of its carry paths: block k aims slot q at label
    (k + q) mod the number of labels the slot can take"""
    rng = random.Random(0x676C7565 + form.code)
    kind_of = {"ADD none": "sum-borrow", "ADD carry": "carry", "ADD carry+ripple": "carry+ripple", "ADD gep": "gep",
               "ADD_LAZY none": "none", "ADD_LAZY carry": "carry", "ADD_LAZY carry+ripple": "carry+ripple"}
    out = []
    for k in range(reps * 4):
        x, w = [], []
        for q in range(32):
            labels = glue_reachable(form, q, config)
            label = labels[(k + q) % len(labels)]
            if form.half:
                a, v = _pair(rng, label.split(" ")[1], P, False, 1)
                a, v = (v, a) if pre2_slot(form.inv, q)[1] else (a, v)
            else:
                a, v = _pair(rng, kind_of[label], P, False, 1)
            x.append(a)
            w.append(v)
        out.append(x + w)
    for k in range(3 * reps + 6 if not form.half else 0):  # the even half's slot pairs (2 j, 2 j + 1), see glue_pair_label
        x, w = [0] * 32, [0] * 32
        for q in range(1, 32, 2):
            x[q], w[q] = _pair(rng, "gep", P, False, 1)
            r = x[q] + w[q] - P
            if r == 0:
                x[q] += 1
                r = 1
            if k >= 3 * reps and q > 1:  # the last blocks hold the first pair alone: nothing downstream re-wraps its words
                x[q], w[q] = 0, 0
            elif (k + q // 2) % 3 == 0:
                x[q - 1] = rng.getrandbits(64) % r
            elif (k + q // 2) % 3 == 1:  # a + r >= 2^64
                a = M64 + 1 - r + rng.getrandbits(64) % r
                x[q - 1] = a - (P - 1) + rng.getrandbits(64) % (2 * (P - 1) - a + 1)
                w[q - 1] = a - x[q - 1]
            else:  # p + r <= a < 2^64 - r, with a smaller r so that the range is not empty
                x[q] -= r - (r >> 2 or 1)
                r = r >> 2 or 1
                a = P + r + rng.getrandbits(32) % (EPS - 2 * r)
                x[q - 1] = a - (P - 1) + rng.getrandbits(64) % (2 * (P - 1) - a + 1)
                w[q - 1] = a - x[q - 1]
        out.append(x + w)
    return out


def glue_pair_label(form, block, q):
    """even half, odd slot q: its sum x + w lies in [p, 2^64) -- the one place where a canonical and a lazy sum differ -- AND the first
    operand a level 1 pairs it with (slot q - 1 after the glue) would show the difference: a < x + w - p ("gep&borrow"), a >= x + w
    ("gep&a>=sum") or a + (x + w - p) >= 2^64 ("gep&carry").  A sum left lazy on an odd slot is invisible to every other pair: see CONDITIONS."""
    s = block[q] + block[32 + q]
    if form.half or not P <= s <= M64:
        return None
    a = network_inputs(form, block)[q - 1]
    return "gep&borrow" if a < s - P else "gep&carry" if a + s - P > M64 else "gep&a>=sum" if a >= s else None


def _into_contract(form, q, word, config):
    return word if slot_admits(form, q % 32, word, config) else word % P


@functools.lru_cache(maxsize=None)
def _operand_sets(name, config_key):
    form, config = FORMS[name], dict(config_key)
    rng = random.Random(0x626C6F636B + form.code)
    sets = {"constructed": [b for b, _ in constructed(form, False, config)]}
    if is_lazy(form, config) and form.kind == "LEVELS" and form.inv:
        sets["constructed_canonical"] = [b for b, _ in constructed(form, True, config)]
    if form.kind in ("PRE2", "C8"):
        sets["glue"] = glue_blocks(form, config)
    edges = fr.edge_words()
    per_slot = [[w for w in edges if slot_admits(form, q % 32, w, config)] for q in range(form.words)]
    sets["edge"] = [[rng.choice(per_slot[q]) for q in range(form.words)] for _ in range(256)]
    sets["uniform"] = [[_into_contract(form, q, rng.getrandbits(64), config) for q in range(form.words)] for _ in range(1 << 10)]
    if form.kind in ("PRE2", "C8") and not is_lazy(form, config):
        sets = {k: [b for b in v if block_in_contract(form, b, config)] for k, v in sets.items()}
    return {k: tuple(tuple(b) for b in v) for k, v in sets.items()}


def operand_sets(form, config=None):
    """{set name: tuple of blocks (tuples of form.words words)}: 'constructed' (aimed at every butterfly under the form's own
    contract), 'constructed_canonical' (the same from canonical inputs only: the blocks the short-transform kernels are steered with),
    'glue', 'edge' (256 blocks of field_ref.edge_words(), per slot those the contract admits) and 'uniform' (2^10 blocks)"""
    return _operand_sets(form.name, tuple(sorted((config or DEFAULT_CONFIG).items())))


@functools.lru_cache(maxsize=None)
def _expected(name, config_key):
    form, config = FORMS[name], dict(config_key)
    blocks = [b for v in _operand_sets(name, config_key).values() for b in v]
    return tuple(blocks), tuple(tuple(run(form, b, config)) for b in blocks)


def expected(form, config=None):
    """(blocks, words): every block of every operand set of the form, and the 32 words the form must leave in place of its first 32"""
    return _expected(form.name, tuple(sorted((config or DEFAULT_CONFIG).items())))


def locate(form, block, got, config=None):
    """for a block whose output words differ from the model's: the first butterfly (in the model's order) one of whose outputs the
    wrong slots depend on -- (lvl, i, slot, label of the pair, a, b, v) -- found by running the model and looking, from the last level
    down, for the butterfly that wrote the first wrong slot"""
    want = run(form, block, config)
    wrong = [q for q in range(32) if got[q] != want[q]]
    if not wrong:
        return None
    seen = []
    run(form, block, config, lambda lvl, i, a, b, v, lazy: seen.append((lvl, i, a, b, v, lazy)))
    q = wrong[0]
    for lvl, i, a, b, v, lazy in reversed(seen):
        if lvl == 0:
            if i == q:
                return (0, i, q, glue_label(form, i, a, b, config), a, b, v)
            continue
        ia, ib, _, neg = bf(form.inv, lvl, i)
        if q in (ia, ib):
            labels, conds = classify(lvl, a, b, v, lazy)
            out = int((q == ib) != neg)  # 0: this slot took the sum
            return (lvl, i, q, f"{'difference' if out else 'sum'} {labels[out][1]}" + "".join(" " + c for c in conds), a, b, v)
    return (None, None, q, "slot not written by the form", block[q], 0, 0)


# ------------------------------------------------------------------------------------------------------------- the short transforms
def rows32_row(block, logn):
    """the lane's row of 32 elements that puts block[q] on slot q (rows32_src: slot q reads element (q / n) n + brev(q % n))"""
    n = 1 << logn
    row = [0] * 32
    for q in range(32):
        row[(q // n) * n + brev(q % n, logn)] = block[q]
    return row


def short_transform_row(row, logn, inverse):
    """the 32 / n transforms of n points a lane's row holds, by the plain DFT (the inverse scaled by 1 / n): canonical words"""
    n = 1 << logn
    scale = pow(n, P - 2, P) if inverse else 1
    out = []
    for base in range(0, 32, n):
        out += [y * scale % P for y in dft(row[base:base + n], inverse)]
    return out


def rows64_dif(elements, inv):
    """rows64_dif_stage on one 64-point transform: the even lane's slots hold u[e] + u[e + 32], the odd lane's (u[e] - u[e + 32]) w_64^e,
    e = brev5(slot), both canonical -> (even block, odd block) as the 32-slot networks see them"""
    even, odd = [], []
    for q in range(32):
        e = brev(q, 5)
        even.append((elements[e] + elements[e + 32]) % P)
        odd.append((elements[e] - elements[e + 32]) * _POW2[tw_exp(inv, 6, e)] % P)
    return even, odd


def rows64_elements(even, odd, inv):
    """the 64 canonical words of which rows64_dif makes the blocks (even, odd): per slot pair u0 + u1 = s and (u0 - u1) w = d"""
    half = pow(2, P - 2, P)
    u = [0] * 64
    for q in range(32):
        e = brev(q, 5)
        diff = odd[q] * pow(_POW2[tw_exp(inv, 6, e)], P - 2, P) % P
        u[e], u[e + 32] = (even[q] + diff) * half % P, (even[q] - diff) * half % P
    return u


def steered_rows(logn, inverse, config=None):
    """the canonical-input blocks of LEVELS<INV, INV, min(logn, 5)> the short-transform kernels are steered with"""
    form = FORMS[f"LEVELS{min(logn, 5)}_{'inv_lazy' if inverse else 'fwd_canonical'}"]
    sets = operand_sets(form, config)
    return form, sets.get("constructed_canonical", sets["constructed"])
