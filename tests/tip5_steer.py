"""Inputs that steer the Tip5 kernels of csrc/tip5_kernels.h onto the rare paths of their hand-written reductions, and step-by-step
models that say which path a state takes.  Python integers (numpy only to sum the byte planes); nothing here comes from the library.
The oracle is asked once, for one trace, from which the 80 round constants are derived.

Every Tip5 round ends in a reduction of the MDS sums whose corrective branches uniform states take about once in 2^32 words.  Tip5
is a permutation and every layer of a round can be inverted (the lookup table is a byte permutation, x^7 has the inverse exponent
7^-1 mod (p - 1), the circulant is invertible mod p, the round constants subtract), so any chosen post-S-box state or any chosen
OUTPUT of any round pulls back to a canonical input, which reaches the kernels through the public API.

  round_(s, r) / unround(x, r)   the round on raw Montgomery words and its inverse: lookup on lanes 0..3, raw^7 R^-6 on lanes 4..15,
                                 the integer sums S_r = sum_c M[(r - c) mod 16] w_c, the word (S_r + rc) mod p
  coop_run(state)                what tip5_permutation_coop / tip5_permutation_coop2 (and tip5_round) hold before the canonical
                                 word: slo, shi, the carries c0..c4, t, ca, cb
  mx_run(state, ...)             the i8 matrix-pipe round as the header of tip5_kernels.h and fill_tip5_mx define it: the planes P_p,
                                 the starts (c, cf, cz), Q_p, L0, L1, hsum, u, (tl, th, h0), the tail through tests/field_ref.event, and
                                 with the lazy tail the possibly non-canonical words 4..15 carried into the next round's x^7 chain
                                 (montyred on x x, sq sq, sq qu, x t -- the kernel's order)
The models classify; expected words always come from the integer round or from the oracle.

steered_states() is the set S of full 16-word canonical states, each class built for every round 0..4 and pulled back to round 0:
  (a) round outputs: all 16 words from the edge kinds (0, 1, a word below 2^32 - 1, 2^32 - 2, 2^32 - 1, 2^32, (h << 32) | 0xffffffff,
      p - 2, p - 1, a word just below p), and one such word among 15 random ones at every word position.  [A canonical word with the
      high dword 0xffffffff is p - 1 and nothing else.]
  (b) fold values: the pre-canonical value of the cooperative fold (t) and of the matrix-pipe tail ((th : tl) + h0 2^32) set to
      p - 1, p, 2^64 - 1, 2^64 (+ a little), 2^64 + (h << 32) on a chosen (round, row) by adjusting two x^7 lanes whose matrix entries
      are coprime (the sum is linear in the integer words)
  (c) the five byte patterns of test_tip5_degenerate_words_after_lookup.  A post-lookup word >= p has NO canonical pre-image (see
      UNREACHABLE), so there is nothing else to build in this class
  (d) byte-plane extremes: for every (round, row, plane) the post-S-box state that maximises P_p and the one that minimises it, and
      saturated words
  (e) the reference's degenerate known-answer state and 256 uniform states
fixed_inputs(cap) is the set H of 10-word inputs for the forms whose capacity is fixed on entry (cap = 1: hash_pair / hash_10, words
10..15 are ONE; cap = 0: the first permutation of hash_varlen, words 10..15 are 0).  Only round 0 can be steered there: classes (a)
-- ten output rows at a time, by solving the 10 x 10 linear system mod p --, (b) and (d) on the ten free words.  Rounds 1..4 of a
fixed-capacity call cannot be steered from outside -- that would mean inverting the hash -- and are not searched for; this includes the
DIGEST last round (mx_fold2_tail), which only the primitive probe of tests/test_gpu_field_primitives.py reaches on its rare paths.  The
generic last round is covered by S.
"""
import functools
import math
import operator
import random

import numpy as np

from tests import field_ref as fr

P, M64, M32, EPS = fr.P, fr.M64, fr.M32, fr.EPS
ONE = EPS  # the raw word of 1
COL = [61402, 1108, 28750, 33823, 7454, 43244, 53865, 12034, 56951, 27521, 41351, 40901, 12021, 59689, 26798, 17845]
MROW = [[COL[(r - c) & 15] for c in range(16)] for r in range(16)]
LUT = bytes(((x + 1) ** 3 % 257) - 1 for x in range(256))  # (x + 1)^3 mod 257 is never 0 for x < 256
ILUT = bytes(LUT.index(v) for v in range(256))
D7 = pow(7, -1, P - 1)
N_UNIFORM = 256
MIN_STATES = 4  # every coverage cell is reached by at least this many states


# ------------------------------------------------------------------------------------------------------ the round and its inverse
def lookup(w, table=LUT):
    return int.from_bytes(w.to_bytes(8, "little").translate(table), "little")


def pow7(raw):
    return pow(raw * fr.R_INV % P, 7, P) * EPS % P


def root7(raw):
    return pow(raw * fr.R_INV % P, D7, P) * EPS % P


def sbox(s):
    return [lookup(s[i]) if i < 4 else pow7(s[i]) for i in range(16)]


def mds(t):
    return [sum(map(operator.mul, row, t)) for row in MROW]


def solve_mod_p(a, b):
    """x with a x = b (mod p) for a square a, or None if a is singular"""
    n = len(a)
    m = [[v % P for v in row] + [b[i] % P] for i, row in enumerate(a)]
    for c in range(n):
        piv = next((r for r in range(c, n) if m[r][c]), None)
        if piv is None:
            return None
        m[c], m[piv] = m[piv], m[c]
        inv = pow(m[c][c], P - 2, P)
        m[c] = [v * inv % P for v in m[c]]
        for r in range(n):
            if r != c and m[r][c]:
                f = m[r][c]
                m[r] = [(v - f * w) % P for v, w in zip(m[r], m[c])]
    return [row[n] for row in m]


@functools.lru_cache(maxsize=None)
def mds_inverse():
    cols = [solve_mod_p(MROW, [int(i == j) for i in range(16)]) for j in range(16)]
    return [[cols[j][i] for j in range(16)] for i in range(16)]


@functools.lru_cache(maxsize=None)
def round_constants():
    """rc[r][j] as raw words, from ONE oracle trace: trace[r + 1] - MDS(Sbox(trace[r]))"""
    from oracle import tfo

    tr, _ = tfo.tip5_trace(tfo.fill_random(16, 1))
    tr = [[int(v) for v in row] for row in np.asarray(tr).reshape(6, 16)]
    return tuple(tuple((tr[r + 1][j] - m) % P for j, m in enumerate(mds(sbox(tr[r])))) for r in range(5))


def round_(s, r):
    rc = round_constants()[r]
    return [(m + rc[j]) % P for j, m in enumerate(mds(sbox(s)))]


def trace(s, post_sbox=None):
    """the six states of Tip5::trace; the five post-S-box states are appended to post_sbox if it is a list"""
    out = [list(s)]
    for r in range(5):
        t = sbox(out[-1])
        if post_sbox is not None:
            post_sbox.append(t)
        rc = round_constants()[r]
        out.append([(m + rc[j]) % P for j, m in enumerate(mds(t))])
    return out


def unsbox(t):
    """the canonical state whose S-box layer gives the words t (lanes 0..3 any 64-bit word, lanes 4..15 below p), or None"""
    s = []
    for i in range(16):
        if i < 4:
            w = lookup(t[i], ILUT)
            if w >= P:
                return None
            s.append(w)
        else:
            s.append(root7(t[i]))
    return s


def unround(x, r):
    """the canonical state that round r takes to x, or None.  For lanes 0..3 both representatives w and w + p of the post-lookup word
    are tried; UNREACHABLE says why only w ever has a canonical pre-image (and always has one)."""
    rc = round_constants()[r]
    y = [(x[j] - rc[j]) % P for j in range(16)]
    w = [sum(map(operator.mul, row, y)) % P for row in mds_inverse()]
    for i in range(4):
        for cand in (w[i], w[i] + P):
            if cand <= M64 and lookup(cand, ILUT) < P:
                w[i] = cand
                break
        else:
            return None
    return unsbox(w)


def pull_back_output(x, r):
    """the input state whose state after round r is x"""
    for rr in range(r, -1, -1):
        x = unround(x, rr)
        if x is None:
            return None
    return x


def pull_back_sbox(t, r):
    """the input state whose post-S-box words in round r are t"""
    x = unsbox(t)
    return x if x is None or r == 0 else pull_back_output(x, r - 1)


# ------------------------------------------------------------------------------------------------------ cooperative forms
COOP_EVENTS = ("none", "none:p-1", "cb", "cb:p", "ca")


def coop_fold(slo, shi, rc):
    """tip5_round / tip5_permutation_coop / tip5_permutation_coop2 after the (partner-row) sums, line for line"""
    w1 = ((slo >> 32) & M32) + (shi & M32)
    c0, w1 = w1 >> 32, w1 & M32
    w2 = ((shi >> 32) & M32) + c0
    c1, w2 = w2 >> 32, w2 & M32
    t0 = (slo & M32) + (rc & M32)
    c2, t0 = t0 >> 32, t0 & M32
    t1 = w1 + (rc >> 32) + c2
    c3, t1 = t1 >> 32, t1 & M32
    t2 = w2 + c3
    c4, t2 = t2 >> 32, t2 & M32
    l64 = (t1 << 32) | t0
    full = t2 * M32 + l64
    ca, t = full > M64, full & M64
    u = t + EPS
    cb = u > M64
    word = (u & M64) if (ca or cb) else t
    label = "ca" if ca else ("cb:p" if t == P else "cb") if cb else "none:p-1" if t == P - 1 else "none"
    return {"slo": slo, "shi": shi, "c": (c0, c1, c2, c3, c4), "t2": t2, "l64": l64, "full": full, "t": t, "ca": ca, "cb": cb,
            "word": word, "label": label}


def coop_row(t, r, row):
    return _coop_row([w & M32 for w in t], [w >> 32 for w in t], r, row)


def _coop_row(lo, hi, r, row):
    m = MROW[row]
    return coop_fold(sum(map(operator.mul, m, lo)), sum(map(operator.mul, m, hi)), round_constants()[r][row])


def coop_run(state):
    """-> (final words, events[round][word] as a set of labels, the fold records [round][word])"""
    s, events, recs = list(state), [], []
    for r in range(5):
        t = [lookup(s[i]) if i < 4 else pow7(s[i]) for i in range(16)]
        lo, hi = [w & M32 for w in t], [w >> 32 for w in t]
        rows = [_coop_row(lo, hi, r, row) for row in range(16)]
        events.append([{rows[j]["label"]} | ({"lookup>=p"} if j < 4 and t[j] >= P else set()) for j in range(16)])
        recs.append(rows)
        s = [x["word"] for x in rows]
    return s, events, recs


# ------------------------------------------------------------------------------------------------------ matrix-pipe form (i8)
def mds_digit(m, a):
    """signed base-256 digits of a matrix entry (mds_digit of tip5_kernels.h)"""
    def s8(v):
        return (v & 0xff) - 256 if v & 0x80 else v & 0xff
    m0 = s8(m)
    m1_ = (m - m0) >> 8
    m1 = s8(m1_)
    m2 = (m1_ - m1) >> 8
    return (m0, m1, m2)[a]


DIG = [[mds_digit(COL[k], a) for k in range(16)] for a in range(3)]
assert all(DIG[0][k] + 256 * DIG[1][k] + 65536 * DIG[2][k] == COL[k] and max(abs(DIG[a][k]) for a in range(3)) <= 128 for k in range(16))
_MA = [np.array([[DIG[a][(r - c) & 15] for c in range(16)] for r in range(16)], dtype=np.int64) for a in range(3)]
BIAS = 1 << 21


def _starts(rc16, skip, fixed_one):
    """fill_tip5_mx's `starts`: [row][plane]"""
    ones8 = 0x0101010101010101
    k2 = 0
    for _ in range(10):
        k2 = (k2 * 256 + BIAS) % P
    out = []
    for r in range(16):
        rowsum = sum(COL[(r - c) & 15] for c in range(12))
        tail = sum(COL[(r - c) & 15] for c in range(12, 16))
        if not skip:
            rowsum += tail
        adj = rc16[r] + (128 * rowsum) % P * (ones8 % P) % P + P - k2
        if skip and fixed_one:
            adj += tail * 0xffffffff
        x = adj % P
        out.append([BIAS + ((x >> (8 * p)) & 0xff if p < 8 else 0) for p in range(10)])
    return out


@functools.lru_cache(maxsize=None)
def mx_starts():
    rc = round_constants()
    return {**{r: _starts(rc[r], False, False) for r in range(5)}, "cf": _starts(rc[0], True, True), "cz": _starts(rc[0], True, False)}


def mx_planes(t, nw=16):
    """P_p[row] for the post-S-box words t (any 64-bit words); the bytes of words nw.. are left out of B.  -> int64 array [16][10]"""
    d = np.array(t, dtype=np.uint64).view(np.uint8).reshape(16, 8).astype(np.int64) - 128
    d[nw:] = 0
    planes = np.zeros((16, 10), dtype=np.int64)
    for a in range(3):
        planes[:, a:a + 8] += _MA[a] @ d
    return planes


def mx_recombine(q):
    """the ten accumulators of one word -> the record of the recombination (u32 / u64 arithmetic as the kernel writes it)"""
    lo32 = [(q[1] << 8) + q[0], (q[5] << 8) + q[4], (q[9] << 8) + q[8]]
    l0 = q[3] * (1 << 24) + (q[2] * (1 << 16) + lo32[0])
    l1 = q[7] * (1 << 24) + (q[6] * (1 << 16) + lo32[1])
    hsum = (l1 >> 32) + lo32[2]
    u = hsum * M32 + l0
    return {"q": q, "l0": l0, "l1": l1, "hsum": hsum, "u": u, "h0": l1 & M32, "value": u + ((l1 & M32) << 32),
            "u32_ok": max(lo32) <= M32 and hsum <= M32 and l0 <= M64 and l1 <= M64}


def mx_row(t, key, row, nw=16):
    """the recombination record of one output row (key: the round, or "cf" / "cz")"""
    planes = mx_planes(t, nw)[row]
    start = mx_starts()[key][row]
    rec = mx_recombine([int(planes[p]) + start[p] for p in range(10)])
    rec["planes"] = [int(v) for v in planes]
    return rec


def mont(a, b):
    t = a * b
    return fr.montyred(t & M64, t >> 64)


def x7_chain(x):
    """x^7 = x (x^2 x^4) as tip5_round_mx multiplies it: x x, sq sq, sq qu, x t, each a montyred of the 128-bit product"""
    sq = mont(x, x)
    qu = mont(sq, sq)
    return mont(x, mont(sq, qu))


class Bounds:
    """extremes of the quantities whose bounds the kernel's comments claim"""

    def __init__(self):
        self.abs_p = self.max_q = self.max_hsum = self.max_u = 0
        self.min_q = BIAS
        self.u32_ok = True

    def see(self, rec):
        self.abs_p = max(self.abs_p, max(abs(v) for v in rec["planes"]))
        self.min_q, self.max_q = min(self.min_q, min(rec["q"])), max(self.max_q, max(rec["q"]))
        self.max_hsum, self.max_u = max(self.max_hsum, rec["hsum"]), max(self.max_u, rec["u"])
        self.u32_ok = self.u32_ok and rec["u32_ok"]

    def hold(self):
        return (self.abs_p < 1 << 20 and 0 <= self.min_q and self.max_q < 1 << 22 and self.max_hsum < (1 << 15) + (1 << 31)
                and self.max_u < 1 << 64 and self.max_u < fr.T_BOUND and self.u32_ok)


def _mx_layer(s, key, nw, bounds):
    """S-box layer and planes of one round on the (possibly non-canonical) words s -> (flags[word], records[row])"""
    flags = [set() for _ in range(16)]
    t = [0] * 16
    for i in range(16):
        if i < 4:
            t[i] = lookup(s[i])
            if t[i] >= P:
                flags[i].add("lookup>=p")
        elif i >= nw:
            t[i] = s[i]  # FIXED0: a constant, neither multiplied nor part of B
        else:
            if s[i] >= P:
                flags[i].add("lazy>=p")
            t[i] = x7_chain(s[i])
    planes = mx_planes(t, nw).tolist()
    start = mx_starts()[key]
    recs = []
    for row in range(16):
        rec = mx_recombine(list(map(operator.add, planes[row], start[row])))
        rec["planes"] = planes[row]
        if bounds is not None:
            bounds.see(rec)
        recs.append(rec)
    return flags, recs


def mx_run(state, fixed0=0, digest=False, bounds=None):
    """The matrix-pipe permutation in both of its schedules at once.
    -> {"lazy": (words, events), "canon": (words, events)}: "lazy" is tip5_permutation_mx (mx_fold4_tail<false> in rounds 0..3, words
    4..15 carried over as they are; the last round canonical, or mx_fold2_tail on words 0..7 if digest), "canon" is the trace kernel
    (mx_fold4_tail<true> in every round).  fixed0 = 1 / 2: round 0 with the cf / cz starts and words 12..15 left out of B (both
    schedules).  events[round][word] is a set of labels: the tail's label from field_ref.event, "lazy>=p" if the word entered this
    round's x^7 chain non-canonical, "lookup>=p" if the post-lookup word is >= p.  A word the digest round leaves undefined is None."""
    out = {}
    s_lazy = s_canon = list(state)
    ev_lazy, ev_canon = [], []
    for r in range(5):
        key, nw = (("cf" if fixed0 == 1 else "cz"), 12) if (fixed0 and r == 0) else (r, 16)
        flags_c, recs_c = _mx_layer(s_canon, key, nw, bounds)
        flags_l, recs_l = (flags_c, recs_c) if s_lazy == s_canon else _mx_layer(s_lazy, key, nw, bounds)
        last = r == 4
        op_l = "MX_FOLD2" if (last and digest) else "MX_FOLD4_CANON" if last else "MX_FOLD4_LAZY"
        nxt_l, nxt_c, e_l, e_c = [], [], [], []
        for row in range(16):
            pos = row >> 2
            if last and digest and row >= 8:
                nxt_l.append(None)
                e_l.append(set())
            else:
                label, word = fr.event(op_l, 0, pos, recs_l[row]["u"], recs_l[row]["h0"])
                nxt_l.append(word)
                e_l.append({label} | flags_l[row])
            label, word = fr.event("MX_FOLD4_CANON", 0, pos, recs_c[row]["u"], recs_c[row]["h0"])
            nxt_c.append(word)
            e_c.append({label} | flags_c[row])
        s_lazy, s_canon = nxt_l, nxt_c
        ev_lazy.append(e_l)
        ev_canon.append(e_c)
    out["lazy"], out["canon"] = (s_lazy, ev_lazy), (s_canon, ev_canon)
    return out


CANON_LABELS = fr.reachable("MX_FOLD4_CANON", 0, 0)
LAZY_LABELS = fr.reachable("MX_FOLD4_LAZY", 0, 1)

# label -> why no canonical input state produces it (in every form, round and word it could be asked of)
UNREACHABLE = {
    "lookup>=p": "a post-lookup word >= p has the high bytes ff ff ff ff; LUT is a byte permutation with LUT[ff] = ff, so the input word "
                 "has them too, and the only canonical word with that high dword is p - 1 = ffffffff00000000, which looks up to itself "
                 "(LUT[0] = 0): < p",
    "ca+cb": "after the fold wrapped the word is below 2^54 (t2 < 2^22), far from p",
    "c1": "w2 = (shi >> 32) + c0 with shi < 2^52: no carry out of 32 bits",
    "c4": "t2 = w2 + c3 < 2^22: no carry out of 32 bits",
    **{"tail " + k: v for k, v in fr.impossible("MX_FOLD4_CANON").items()},
}


def required(form, r, word):
    """the labels that MIN_STATES states must reach in this cell"""
    if form.startswith("coop"):
        return COOP_EVENTS
    if form == "mx_trace" or r == 4 or word < 4:
        labels = CANON_LABELS
    else:
        labels = LAZY_LABELS
    if form != "mx_trace" and r >= 1 and word >= 4:
        labels = labels + ("lazy>=p",)
    return labels


def classify(state):
    """{form: events[round][word]} for a full state: "coop" (16 lanes and the row pair: the same fold), "mx" (tip5_permutation_mx),
    "mx_trace" (the trace kernel), and the final words of each model"""
    cw, ce, _ = coop_run(state)
    mx = mx_run(state)
    return {"coop": ce, "mx": mx["lazy"][1], "mx_trace": mx["canon"][1]}, {"coop": cw, "mx": mx["lazy"][0], "mx_trace": mx["canon"][0]}


def classify_fixed(inp, cap):
    """the same for a 10-word input of a fixed-capacity form: "coop" and "mx" (cf / cz starts; digest tail for cap = 1); only round 0
    and the lazy words entering round 1 are steered"""
    state = list(inp) + [ONE if cap else 0] * 6
    cw, ce, _ = coop_run(state)
    mx = mx_run(state, fixed0=1 if cap else 2, digest=bool(cap))
    return {"coop": ce, "mx": mx["lazy"][1]}, {"coop": cw, "mx": mx["lazy"][0]}


# ------------------------------------------------------------------------------------------------------ steering
KINDS = ("zero", "one", "small", "top32", "eps", "two32", "ripple", "pm2", "pm1", "nearp")


def kind_word(kind, rng):
    return {"zero": 0, "one": 1, "small": rng.randrange(2, M32 - 1), "top32": M32 - 1, "eps": M32, "two32": 1 << 32,
            "ripple": (rng.randrange(1, 1 << 12) << 32) | M32, "pm2": P - 2, "pm1": P - 1, "nearp": rng.randrange(P - (1 << 32), P - 2)}[kind]


def _adjust(t, row, delta, lanes, rng):
    """t with two of `lanes` changed so that the integer MDS sum of `row` moves by exactly delta, or None"""
    for _ in range(40):
        a, b = rng.sample(lanes, 2)
        ma, mb = MROW[row][a], MROW[row][b]
        if math.gcd(ma, mb) != 1:
            continue
        da = delta * pow(ma, -1, mb) % mb
        db = (delta - da * ma) // mb
        assert da * ma + db * mb == delta
        if 0 <= t[a] + da < P and 0 <= t[b] + db < P:
            out = list(t)
            out[a] += da
            out[b] += db
            return out
    return None


def _prefold(form, t, key, row, nw):
    """(pre-canonical value, the multiple of p the fold took off) of one row"""
    if form == "coop":
        rec = coop_row(t, key if isinstance(key, int) else 0, row)
        return rec["full"], rec["t2"]
    rec = mx_row(t, key, row, nw)
    return rec["value"], rec["hsum"]


def steer_fold(form, t, key, row, target, lanes, rng, nw=16):
    """post-S-box words near t whose fold of `row` holds exactly `target` before the canonical word is taken, or None"""
    for _ in range(5):
        value, _ = _prefold(form, t, key, row, nw)
        if value == target:
            return t
        t = _adjust(t, row, target - value, lanes, rng)
        if t is None:
            return None
    return None


def fold_targets(form, rng):
    """name -> pre-canonical value; the cooperative fold holds t (2^64 and above: ca), the matrix-pipe tail (th : tl) + h0 2^32"""
    small = rng.randrange(1, 1 << 31)
    common = {"p-1": P - 1, "p": P, "max": M64, "gep": P + small}
    if form == "coop":
        return {**common, "wrap0": 1 << 64, "wrap": (1 << 64) + small}
    return {**common, "carry0": 1 << 64, "carry": (1 << 64) + (rng.randrange(1, 1 << 20) << 32) + small,
            "ripple": (1 << 64) + (rng.randrange(1, 1 << 20) << 32)}


def plane_extreme(row, plane, sign, rng, free=16, fixed=None):
    """post-S-box words (all below p) that maximise (sign = 1) or minimise (-1) P_plane[row] over the words 0..free-1: byte
    plane - a of word c is 0xff or 0x00 by the sign of digit m_a[(row - c) mod 16], the other bytes random; words free.. are `fixed`"""
    t = []
    for c in range(16):
        if c >= free:
            t.append(fixed)
            continue
        while True:
            b = bytearray(rng.getrandbits(64).to_bytes(8, "little"))
            for a in range(3):
                m = DIG[a][(row - c) & 15] * sign
                if 0 <= plane - a < 8 and m:
                    b[plane - a] = 0xff if m > 0 else 0x00
            w = int.from_bytes(b, "little")
            if w < P:
                break
        t.append(w)
    return t


def plane_extreme_value(row, plane, sign, free=16, fixed=None, nw=16):
    """the sign rule's value, computed without the model: every free byte contributes |m| 127 or |m| 128, a fixed word its bytes"""
    total = 0
    for c in range(nw):
        for a in range(3):
            m = DIG[a][(row - c) & 15]
            if not 0 <= plane - a < 8:
                continue
            if c < free:
                total += m * (127 if m * sign > 0 else -128)
            else:
                total += m * (((fixed >> (8 * (plane - a))) & 0xff) - 128)
    return total


def _rand_state(rng):
    return [rng.randrange(P) for _ in range(16)]


@functools.lru_cache(maxsize=None)
def steered_states():
    """-> (states, classes): S as a tuple of 16-tuples and a class label for each"""
    from tests.test_oracle_kat import DEGENERATE_IN

    rng = random.Random(0x54697035)
    states, classes = [], []

    def add(state, label):
        assert state is not None, label
        states.append(tuple(state))
        classes.append(label)

    for r in range(5):
        # (a) round outputs
        for rep in range(MIN_STATES):
            for k in range(len(KINDS)):
                add(pull_back_output([kind_word(KINDS[(w + k) % len(KINDS)], rng) for w in range(16)], r), f"a:all16:r{r}:shift{k}")
        add(pull_back_output([rng.randrange(M32 - 1) for _ in range(16)], r), f"a:all16-small:r{r}")
        for w in range(16):
            for kind in ("zero", "small", "eps", "ripple", "pm1"):
                x = _rand_state(rng)
                x[w] = kind_word(kind, rng)
                add(pull_back_output(x, r), f"a:one:r{r}:word{w}:{kind}")
        # (b) fold values on every row
        for row in range(16):
            for form in ("coop", "mx"):
                for name, target in fold_targets(form, rng).items():
                    for _ in range(20):
                        t = steer_fold(form, _rand_state(rng), r, row, target, list(range(4, 16)), rng)
                        if t is not None:
                            break
                    add(pull_back_sbox(t, r), f"b:{form}:r{r}:row{row}:{name}")
        # (d) byte-plane extremes
        for row in range(16):
            for plane in range(10):
                for sign in (1, -1):
                    add(pull_back_sbox(plane_extreme(row, plane, sign, rng), r), f"d:r{r}:row{row}:plane{plane}:{'max' if sign > 0 else 'min'}")
        for name, w in (("p-1", P - 1), ("fffffffe_ffffffff", 0xfffffffeffffffff), ("00000000_ffffffff", 0xffffffff)):
            add(pull_back_sbox([w] * 16, r), f"d:r{r}:all-{name}")
    # (c) the byte patterns of test_tip5_degenerate_words_after_lookup (inputs, not post-lookup words: see UNREACHABLE)
    for b in (0x00, 0xFE, 0xFF, 0x01, 0x80):
        add([int.from_bytes(bytes([b] * 8), "little") % P] * 16, f"c:bytes-{b:02x}")
    # (e) anchors
    add([v * EPS % P for v in DEGENERATE_IN], "e:degenerate-kat")
    for _ in range(N_UNIFORM):
        add(_rand_state(rng), "e:uniform")
    return tuple(states), tuple(classes)


def fixed_round0(inp_t, cap):
    """post-S-box words of round 0 of a fixed-capacity state from its ten free post-S-box words"""
    return list(inp_t) + [ONE if cap else 0] * 6  # 1^7 = 1, 0^7 = 0 (raw words ONE and 0)


@functools.lru_cache(maxsize=None)
def fixed_inputs(cap):
    """-> (inputs, classes): H for capacity words `cap` (1 or 0) as a tuple of 10-tuples and a class label for each"""
    rng = random.Random(0x48000 + cap)
    inputs, classes = [], []
    fixed = ONE if cap else 0
    rc = round_constants()[0]

    def add(t, label):
        x = unsbox(t) if t is not None else None
        assert x is not None and x[10:] == [fixed] * 6, label
        inputs.append(tuple(x[:10]))
        classes.append(label)

    # (a) ten output rows of round 0 at a time
    for rep in range(MIN_STATES):
        for first in range(16):
            rows = [(first + i) & 15 for i in range(10)]
            while True:
                # a row is in ten of the sixteen windows, once at every position: every kind once per repetition
                want = [kind_word(KINDS[(i + rep) % len(KINDS)], rng) for i in range(10)]
                rhs = [want[i] - rc[row] - fixed * sum(MROW[row][10:]) for i, row in enumerate(rows)]
                free = solve_mod_p([MROW[row][:10] for row in rows], rhs)
                if free is not None:
                    break
                rows = rng.sample(range(16), 10)
            add(fixed_round0(free, cap), f"a:ten-rows:cap{cap}:first{first}:rep{rep}")
    # (b) fold values on every row, through the x^7 lanes that are free
    for row in range(16):
        for form in ("coop", "mx"):
            key, nw = (0, 16) if form == "coop" else ("cf" if cap else "cz", 12)
            for name, target in fold_targets(form, rng).items():
                for _ in range(20):
                    t = steer_fold(form, fixed_round0([rng.randrange(P) for _ in range(10)], cap), key, row, target, list(range(4, 10)), rng, nw)
                    if t is not None:
                        break
                add(t, f"b:{form}:cap{cap}:row{row}:{name}")
    # (d) byte-plane extremes over the free words
    for row in range(16):
        for plane in range(10):
            for sign in (1, -1):
                add(plane_extreme(row, plane, sign, rng, free=10, fixed=fixed), f"d:cap{cap}:row{row}:plane{plane}:{'max' if sign > 0 else 'min'}")
    return tuple(inputs), tuple(classes)


def coverage(events_list, forms, rounds):
    """{(form, round, word, label): number of states} over a list of classify() results"""
    seen = {}
    for ev in events_list:
        for form in forms:
            for r in rounds:
                for word in range(16):
                    for label in ev[form][r][word]:
                        key = (form, r, word, label)
                        seen[key] = seen.get(key, 0) + 1
    return seen
