"""Expected words, operand sets and carry-path events for the hand-scheduled field primitives (csrc/gl64.h, the fold tails of
csrc/tip5_kernels.h) that tf_debug_field_op_dev runs one at a time.  Python integers only: nothing here comes from the library or
from the oracle.

Every primitive ends in a correction by +-p or +-(2^32 - 1), done on 32-bit halves as "+-1 on the low word, -+1 on the high word
unless the low word rippled".  Uniform operands take the "rippled" half with probability 2^-32, so the sets below are built to take
it: the cross product of the edge words, 2^16 uniform pairs, and pairs solved backwards from a result whose low or high word is 0 or
0xffffffff.  want(op, a, b) is the word each output must hold; event(op, out, pos, a, b) names the path the pair takes through output
`out` at block position `pos` and returns the word a step-by-step model of the primitive produces, which the CPU tests pin to want().

  canonical ops        the value mod p
  lazy sum             (a + v) mod 2^64, + (2^32 - 1) iff a + v >= 2^64
  lazy difference      (a - v) mod 2^64, - (2^32 - 1) iff a < v
  Montgomery products  montyred (b_field_element.rs:357-370) on the 128-bit product, word for word
  fold tails           V = t + h0 2^32: V mod p on the canonical lanes (all lanes of MX_FOLD4_CANON and MX_FOLD2, lane 0 of
                       MX_FOLD4_LAZY), elsewhere V mod 2^64, + (2^32 - 1) iff V >= 2^64
"""
import functools
import math
import random

P = (1 << 64) - (1 << 32) + 1
M64 = (1 << 64) - 1
M32 = (1 << 32) - 1
EPS = M32  # 2^64 mod p
R_INV = pow(1 << 64, P - 2, P)
T_BOUND = (1 << 63) + (1 << 59)  # the fold tails' first operand t = (th : tl) is below this

# name -> (TF_FIELD_OP_* code, elements per block W, number of outputs); the same table as twenty_first_amd.device.FIELD_OPS
OPS = {
    "ADD": (0, 1, 1), "SUB": (1, 1, 1), "MONT_MUL": (2, 1, 1), "ADD_SUB": (3, 1, 2), "ADD_SUB2": (4, 2, 2), "ADD_SUB_LAZY2": (5, 2, 2),
    "ADD_LAZY4": (6, 4, 1), "SUB_LAZY4": (7, 4, 1), "MONT_MUL2": (8, 2, 1), "MONT_MUL3": (9, 3, 1), "MONT_MUL4": (10, 4, 1),
    "CANONICAL": (11, 1, 1), "MX_FOLD4_CANON": (12, 4, 1), "MX_FOLD4_LAZY": (13, 4, 1), "MX_FOLD2": (14, 2, 1),
}
CANONICAL_OPS = ("ADD", "SUB", "ADD_SUB", "ADD_SUB2")          # a, b < p
LAZY_OPS = ("ADD_SUB_LAZY2", "ADD_LAZY4", "SUB_LAZY4")         # a any word, b <= p
PRODUCT_OPS = ("MONT_MUL", "MONT_MUL2", "MONT_MUL3", "MONT_MUL4")  # any two words
TAIL_OPS = ("MX_FOLD4_CANON", "MX_FOLD4_LAZY", "MX_FOLD2")     # a < T_BOUND, h0 = low half of b
MAX_PAIRS = 1 << 18  # distinct pairs per op; the uploaded list repeats them W times


def width(op):
    return OPS[op][1]


def outputs(op):
    return OPS[op][2]


def in_domain(op, a, b):
    if op in CANONICAL_OPS:
        return a < P and b < P
    if op in LAZY_OPS:
        return b <= P
    if op in TAIL_OPS:
        return a < T_BOUND
    return True


def canonical_lane(op, pos):
    """fold tails: does block position pos hold a canonical word afterwards?"""
    return op != "MX_FOLD4_LAZY" or pos == 0


# ---------------------------------------------------------------------------------------------------------------- expected words
def montyred(lo, hi):
    """b_field_element.rs:357-370 on the words of x = hi 2^64 + lo"""
    a = (lo + (lo << 32)) & M64
    e = (lo + ((lo << 32) & M64)) >> 64
    b = (a - (a >> 32) - e) & M64
    r = (hi - b) & M64
    return (r - EPS) & M64 if hi < b else r


def lazy_sum(a, v):
    s = a + v
    return (s & M64) + EPS if s > M64 else s


def lazy_diff(a, v):
    return ((a - v) & M64) - EPS if a < v else a - v


def want(op, pos, a, b):
    """the words of the op's outputs (a tuple of one or two) for the pair (a, b) at block position pos"""
    if op == "ADD":
        return ((a + b) % P,)
    if op == "SUB":
        return ((a - b) % P,)
    if op in ("ADD_SUB", "ADD_SUB2"):
        return (a + b) % P, (a - b) % P
    if op == "ADD_SUB_LAZY2":
        return lazy_sum(a, b), lazy_diff(a, b)
    if op == "ADD_LAZY4":
        return (lazy_sum(a, b),)
    if op == "SUB_LAZY4":
        return (lazy_diff(a, b),)
    if op in PRODUCT_OPS:
        t = a * b
        return (montyred(t & M64, t >> 64),)
    if op == "CANONICAL":
        return (a % P,)
    v = a + ((b & M32) << 32)
    if canonical_lane(op, pos):
        return (v % P,)
    return ((v & M64) + EPS if v > M64 else v,)


def exact(op, out, a, b):
    """the field element output `out` must be congruent to, computed without any word formula"""
    if op in PRODUCT_OPS:
        return a * b * R_INV % P
    if op == "CANONICAL":
        return a % P
    if op in TAIL_OPS:
        return (a + ((b & M32) << 32)) % P
    if op in ("ADD", "ADD_LAZY4") or (op in ("ADD_SUB", "ADD_SUB2", "ADD_SUB_LAZY2") and out == 0):
        return (a + b) % P
    return (a - b) % P


def promises_canonical(op, out, pos, a, b):
    """does the primitive's contract promise a word < p for this pair?"""
    if op in CANONICAL_OPS or op == "CANONICAL":
        return True
    if op in PRODUCT_OPS:
        return a < P or b < P
    if op in TAIL_OPS:
        return canonical_lane(op, pos)
    return False


# ---------------------------------------------------------------------------------------------------------------- events
# A label is "<cause>" for no ripple and "<cause>+ripple" when the corrected low word wrapped (0 after +1, 0xffffffff after -1), so
# that the high word must NOT get its -+1.  event() returns (label, word of the step-by-step model).
def _plus_p(x, apply):
    """x + p on halves: lo += 1, hi -= 1 unless lo carried.  -> (word, rippled)"""
    if not apply:
        return x, False
    lo, hi = (x & M32) + 1, x >> 32
    ripple = lo > M32
    if not ripple:
        hi = (hi - 1) & M32
    return (hi << 32) | (lo & M32), ripple


def _plus_eps(x, apply):
    """x + (2^32 - 1) on halves: lo -= 1, hi += 1 unless lo borrowed.  -> (word, rippled)"""
    if not apply:
        return x, False
    lo, hi = (x & M32) - 1, x >> 32
    ripple = lo < 0
    if not ripple:
        hi = (hi + 1) & M32
    return (hi << 32) | (lo & M32), ripple


def _label(cause, ripple):
    return cause + "+ripple" if ripple else cause


def event(op, out, pos, a, b):
    if op == "ADD":  # gl::add: +(2^32 - 1) after a 64-bit carry, or when the sum is >= p without one
        s = a + b
        cause = "carry" if s > M64 else "gep" if s >= P else "none"
        r, ripple = _plus_eps(s & M64, cause != "none")
        return _label(cause, ripple), r
    if op == "SUB" or (op in ("ADD_SUB", "ADD_SUB2") and out == 1):  # a - b, + p on borrow
        r, ripple = _plus_p((a - b) & M64, a < b)
        return _label("borrow" if a < b else "none", ripple), r
    if op in ("ADD_SUB", "ADD_SUB2"):  # the sum as a - (p - v), + p on borrow
        n = P - b
        r, ripple = _plus_p((a - n) & M64, a < n)
        return _label("borrow" if a < n else "none", ripple), r
    if op == "ADD_LAZY4" or (op == "ADD_SUB_LAZY2" and out == 0):
        s = a + b
        r, ripple = _plus_eps(s & M64, s > M64)
        return _label("carry" if s > M64 else "none", ripple), r
    if op == "SUB_LAZY4" or op == "ADD_SUB_LAZY2":  # - (2^32 - 1) = + p (mod 2^64) on borrow
        r, ripple = _plus_p((a - b) & M64, a < b)
        return _label("borrow" if a < b else "none", ripple), r
    if op in PRODUCT_OPS:
        a0, a1, b0, b1 = a & M32, a >> 32, b & M32, b >> 32
        cm = (a0 * b1 + a1 * b0) >> 64  # carry of the middle term
        t = a * b
        lo, hi = t & M64, t >> 64
        l0, l1 = lo & M32, lo >> 32
        u = l1 + l0                                    # a1 = l1 + l0, carry e
        e, u = u >> 32, u & M32
        w = l0 - u - e                                 # b0 = l0 - a1 - e
        c, w = int(w < 0), w & M32
        u = (u - c) & M32                              # b1 = a1 - borrow  (never borrows: a1 = 0 and a borrow need l0 = 0 < e)
        r0 = (hi & M32) - w
        c, r0 = int(r0 < 0), r0 & M32
        r1 = (hi >> 32) - u - c
        borrow, r1 = r1 < 0, r1 & M32
        r, ripple = _plus_p((r1 << 32) | r0, borrow)
        return f"{'both>=p' if a >= P and b >= P else 'one<p'}|cm{cm}|{_label('borrow' if borrow else 'none', ripple)}", r
    if op == "CANONICAL":  # x >= p ? x + (2^32 - 1) : x
        r, ripple = _plus_eps(a, a >= P)
        cause = "gep" if a >= P else "none"
        return _label(cause, ripple) + (":p" if a == P else ":p-1" if a == P - 1 else ""), r
    # fold tails: th += h0 (carry k: the value is t + k 2^64); canonical lanes correct on k or t >= p, the others on k alone
    tl, th = a & M32, (a >> 32) + (b & M32)
    k, th = th >> 32, th & M32
    t = (th << 32) | tl
    if canonical_lane(op, pos):
        cause = "carry" if k else "gep" if t >= P else "none"
        r, ripple = _plus_eps(t, cause != "none")
        return _label(cause, ripple) + (":p" if (k, t) == (0, P) else ":p-1" if (k, t) == (0, P - 1) else ""), r
    r, ripple = _plus_eps(t, k)
    return "lazy " + _label("carry" if k else "none", ripple), r


_PRODUCT_REACHABLE = tuple(f"{g}|cm{c}|{e}" for g, c, e in
                           [("one<p", c, e) for c in (0, 1) for e in ("none", "borrow", "borrow+ripple")] + [("both>=p", 0, "none"), ("both>=p", 1, "none")])
_GE_P = ("none", "none:p-1", "gep", "gep:p")  # a comparison with p: both sides of it, and both words next to it


def reachable(op, out, pos):
    """the labels event() must produce at least 8 times for this output and block position"""
    if op == "ADD":
        return ("none", "carry", "carry+ripple", "gep")
    if op in CANONICAL_OPS or op in LAZY_OPS:
        cause = "carry" if op == "ADD_LAZY4" or (op == "ADD_SUB_LAZY2" and out == 0) else "borrow"
        return ("none", cause, cause + "+ripple")
    if op in PRODUCT_OPS:
        return _PRODUCT_REACHABLE
    if op == "CANONICAL":
        return _GE_P
    if canonical_lane(op, pos):
        return _GE_P + ("carry", "carry+ripple")
    return ("lazy none", "lazy carry", "lazy carry+ripple")


# label (or label prefix, for the products) -> why no operand pair of the op's domain produces it
IMPOSSIBLE = {
    "ADD": {
        "gep+ripple": "a ripple needs a sum with low word 0, but a sum >= p = 0xffffffff00000001 without a carry has a low word >= 1",
    },
    "CANONICAL": {
        "gep+ripple": "a word >= p = 0xffffffff00000001 has a low word >= 1, so the low word's -1 never borrows",
    },
    "PRODUCTS": {
        "both>=p|cm0|borrow": "with a = p + x, b = p + y the final borrow needs x y (2^32 + 1) mod 2^64 in [1, 2^32 - 2 - (x + y)], "
                              "so x y >= (x + y + 2) 2^32; but x y < 2^32 y",
        "both>=p|cm1|borrow": "as above: the argument does not look at the middle term",
    },
    "TAILS": {
        "gep+ripple": "t >= p without a carry is th = 0xffffffff and tl != 0 (the very test the tail makes), so tl - 1 never borrows",
        "lazy gep": "the lanes that may stay non-canonical correct on the carry alone: a word >= p is left as it is",
    },
}


def impossible(op):
    return IMPOSSIBLE["PRODUCTS" if op in PRODUCT_OPS else "TAILS" if op in TAIL_OPS else op] if (
        op in PRODUCT_OPS or op in TAIL_OPS or op in IMPOSSIBLE) else {}


# ---------------------------------------------------------------------------------------------------------------- operand sets
def edge_words():
    """the edge words of tests/test_gpu_pow2_products.py, plus 2, p - 2, 2^32 +- 1, 2^63, 2^63 - 1 and every single-bit word"""
    words = [0, 1, P - 1, P, P + 1, M64, 2 ** 32 - 1, 2 ** 32, 2 ** 64 - 2 ** 32 - 1, 2 ** 64 - 2 ** 32 + 1]
    words += [(M64 << s) & M64 for s in range(64)]
    words += [M64 >> s for s in range(64)]
    words += [2, P - 2, 2 ** 32 + 1, 2 ** 32 - 1, 2 ** 63, 2 ** 63 - 1]
    words += [1 << s for s in range(64)]
    return sorted(set(words))


def _targets(rng, canonical):
    """results that sit on a carry path: low word 0 / 0xffffffff, high word 0 / 0xffffffff, 0, p - 1 (and their neighbours)"""
    h, l = rng.getrandbits(32), rng.getrandbits(32)
    out = [h << 32, (h << 32) | M32, l, (M32 << 32) | l, 0, P - 1, 1, P - 2, M32, 1 << 32]
    if canonical:
        out = [r if r < P else r - P for r in out]  # (< 2p)
    return out


def _constructed(op, rng, rounds):
    pairs = []
    if op in CANONICAL_OPS:
        for _ in range(rounds):
            a = rng.getrandbits(64) % P
            for r in _targets(rng, True):
                pairs += [(a, (r - a) % P), (a, (a - r) % P), ((r - a) % P, a), (r, a), (a, r)]
    elif op in LAZY_OPS:
        for _ in range(rounds):
            v = rng.getrandbits(64) % (P + 1) if rng.getrandbits(3) else P
            for r in _targets(rng, False):
                pairs += [((r - v - EPS) & M64, v), ((r + v + EPS) & M64, v), ((r - v) & M64, v), ((r + v) & M64, v)]
    elif op in PRODUCT_OPS:
        for i in range(rounds):
            a = rng.getrandbits(64) % P or 1
            a_inv = pow(a, P - 2, P)
            for r in _targets(rng, True):
                b = (r << 64) * a_inv % P  # a b 2^-64 = r
                pairs += [(a, b), (b, a)]
                if b + P <= M64:
                    pairs.append((a, b + P))
            x, y = P + rng.getrandbits(32) % (M32 - 1), P + rng.getrandbits(32) % (M32 - 1)
            pairs += [(x, y), (x, x), (x, rng.getrandbits(64) % P), (rng.getrandbits(64) % P, y), (M64 - i % 64, y), (x, M64 - i % 64)]
    elif op == "CANONICAL":
        for i in range(rounds):
            pairs += [(P + rng.getrandbits(32) % (M32 - 1), rng.getrandbits(64)), (P - 1 - rng.getrandbits(32), rng.getrandbits(64)),
                      ((M32 << 32) | rng.getrandbits(32), i), ((P, P - 1, P + 1, M64)[i % 4], rng.getrandbits(64))]
    else:  # fold tails: h0 = 0xffffffff - th (the sum's high word is all ones, no carry) and 2^32 - th (it is 0, with a carry)
        for i in range(rounds):
            th = rng.getrandbits(32) % (T_BOUND >> 32) or 1
            junk = rng.getrandbits(32) << 32  # the high half of b is not an operand
            for tl in (0, 1, M32, M32 - 1, rng.getrandbits(32)):
                t = (th << 32) | tl
                pairs += [(t, junk | (M32 - th)), (t, junk | ((1 << 32) - th)), (t, junk | (M32 - 1 - th)), (t, junk | ((1 << 32) + 1 - th))]
    return [(a, b) for a, b in pairs if in_domain(op, a, b)]


def _into_domain(op, a, b):
    if op in CANONICAL_OPS:
        return a % P, b % P
    if op in LAZY_OPS:
        return a, b % (P + 1)
    if op in TAIL_OPS:
        return a % T_BOUND, b
    return a, b


@functools.lru_cache(maxsize=None)
def operands(op):
    """(a, b): the op's distinct operand pairs in upload order -- the edge words' cross product, 2^16 uniform pairs and the pairs built
    backwards from a result, each restricted to the op's domain, shuffled with a fixed seed (so the lanes of a wave take different
    branches), the length coprime to 12.  uploaded() repeats the list W times."""
    rng = random.Random(0x6669656C64 + OPS[op][0])
    edges = edge_words()
    pairs = [(a, b) for a in edges for b in edges if in_domain(op, a, b)]
    pairs += [_into_domain(op, rng.getrandbits(64), rng.getrandbits(64)) for _ in range(1 << 16)]
    pairs += _constructed(op, rng, 400)
    while math.gcd(len(pairs), 12) != 1:
        pairs.append(_into_domain(op, rng.getrandbits(64), rng.getrandbits(64)))
    rng.shuffle(pairs)
    assert len(pairs) <= MAX_PAIRS and all(in_domain(op, a, b) for a, b in pairs)
    return tuple(p[0] for p in pairs), tuple(p[1] for p in pairs)


@functools.lru_cache(maxsize=None)
def uploaded(op):
    """(a, b, want0, want1 or None, length of one repetition): operands(op) repeated W times.  The length L of one repetition is coprime
    to W, so pair i sits at the indices i, i + L, ..., i + (W - 1) L, whose residues mod W -- the block positions -- are all different:
    every pair rides every carry chain of the block."""
    a, b = operands(op)
    n, w = len(a), width(op)
    assert math.gcd(n, w) == 1
    a, b = a * w, b * w
    words = [want(op, j % w, a[j], b[j]) for j in range(n * w)]
    return a, b, tuple(x[0] for x in words), tuple(x[1] for x in words) if outputs(op) == 2 else None, n
