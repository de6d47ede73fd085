"""Expected values for the polynomial arithmetic entry points (include/tf_hip.h, "Polynomial arithmetic"), written independently of
the library and of the oracle: Python integers only.  A raw word r stands for the value r * R^-1 mod p (R = 2^64); every function
converts raw words to values, computes in the field, and converts back.  A BFieldElement is one value, an XFieldElement three
(c0 + c1 x + c2 x^2 in F_p[x] / (x^3 - x + 1), x_field_element.rs:512-536); a base-field element meets an extension-field one as
its lift (v, 0, 0) (x_field_element.rs:491-556).  tests/test_poly_algebra_cpu.py pins this builder against the oracle and tests/pyref.

All nine operations, all four width combinations:
    add, sub, neg, scalar_mul, scale, formal_derivative, degree, hadamard_xfe_bfe, linear_combination."""
import numpy as np

P = (1 << 64) - (1 << 32) + 1
R = (1 << 64) % P
R_INV = pow(R, P - 2, P)


def to_val(raw: int) -> int:
    return int(raw) * R_INV % P


def to_raw(val: int) -> int:
    return int(val) % P * R % P


# ------------------------------------------------------------------ field elements as tuples of values (length 1 or 3)
def lift(a, w):
    return a if len(a) == w else (a[0],) + (0,) * (w - 1)


def f_add(a, b):
    w = max(len(a), len(b))
    return tuple((x + y) % P for x, y in zip(lift(a, w), lift(b, w)))


def f_sub(a, b):
    w = max(len(a), len(b))
    return tuple((x - y) % P for x, y in zip(lift(a, w), lift(b, w)))


def f_neg(a):
    return tuple(-x % P for x in a)


def f_mul(a, b):
    if len(a) == 1 and len(b) == 1:
        return (a[0] * b[0] % P,)
    if len(a) == 1:
        return tuple(a[0] * y % P for y in b)
    if len(b) == 1:
        return tuple(x * b[0] % P for x in a)
    a0, a1, a2 = a
    b0, b1, b2 = b
    d0, d1, d2, d3, d4 = a0 * b0, a0 * b1 + a1 * b0, a0 * b2 + a1 * b1 + a2 * b0, a1 * b2 + a2 * b1, a2 * b2
    # x^3 = x - 1, x^4 = x^2 - x
    return ((d0 - d3) % P, (d1 + d3 - d4) % P, (d2 + d4) % P)


def f_one(w):
    return (1,) + (0,) * (w - 1)


def f_zero(w):
    return (0,) * w


def f_pow(a, e):
    r, s = f_one(len(a)), a
    while e:
        if e & 1:
            r = f_mul(r, s)
        s = f_mul(s, s)
        e >>= 1
    return r


# ------------------------------------------------------------------ raw arrays <-> lists of elements
def elements(raw, w):
    vals = [to_val(r) for r in np.asarray(raw, dtype=np.uint64).reshape(-1).tolist()]
    assert len(vals) % w == 0
    return [tuple(vals[i:i + w]) for i in range(0, len(vals), w)]


def words(elems, w):
    return np.array([to_raw(v) for e in elems for v in lift(e, w)], dtype=np.uint64)


def _rows(raw, n, w, batch):
    e = elements(raw, w)
    assert len(e) == n * batch
    return [e[r * n:(r + 1) * n] for r in range(batch)]


# ------------------------------------------------------------------ the nine operations on raw words
def _add_sub(a, na, b, nb, w, batch, op):
    ra, rb = _rows(a, na, w, batch), _rows(b, nb, w, batch)
    n = max(na, nb)
    z = f_zero(w)
    out = []
    for r in range(batch):
        x = ra[r] + [z] * (n - na)
        y = rb[r] + [z] * (n - nb)
        out += [op(p, q) for p, q in zip(x, y)]
    return words(out, w)


def add(a, na, b, nb, w=1, batch=1):
    """batch x max(na, nb) coefficients; the shorter operand reads as zero above its length (polynomial.rs:2526-2563)"""
    return _add_sub(a, na, b, nb, w, batch, f_add)


def sub(a, na, b, nb, w=1, batch=1):
    return _add_sub(a, na, b, nb, w, batch, f_sub)


def neg(a, w=1):
    return words([f_neg(e) for e in elements(a, w)], w)


def scalar_mul(a, wa, scalar, ws):
    """every coefficient times the scalar (polynomial.rs:498-532); out width max(wa, ws)"""
    s = elements(scalar, ws)[0]
    return words([f_mul(e, s) for e in elements(a, wa)], max(wa, ws))


def scale(a, na, wa, alpha, wal, batch=1):
    """out[j] = a[j] * alpha^j per row (polynomial.rs:760-773), the power carried as a running product"""
    al = elements(alpha, wal)[0]
    out = []
    for row in _rows(a, na, wa, batch):
        pw = f_one(wal)
        for e in row:
            out.append(f_mul(e, pw))
            pw = f_mul(pw, al)
    return words(out, max(wa, wal))


def formal_derivative(a, na, w=1, batch=1):
    """batch x (na - 1) coefficients: out[j] = (j + 1) * a[j + 1] (polynomial.rs:275-285)"""
    out = []
    for row in _rows(a, na, w, batch):
        out += [f_mul(((j + 1) % P,), row[j + 1]) for j in range(na - 1)]
    return words(out, w)


def degree(a, na, w=1, batch=1):
    """index of the highest non-zero coefficient per row, -1 for the zero polynomial (polynomial.rs:181)"""
    out = np.full(batch, -1, dtype=np.int64)
    for r, row in enumerate(_rows(a, na, w, batch)):
        for j in range(na - 1, -1, -1):
            if any(row[j]):
                out[r] = j
                break
    return out


def hadamard_xfe_bfe(a, b):
    """Mul<BFieldElement> for XFieldElement (x_field_element.rs:540-548), element by element"""
    return words([f_mul(x, y) for x, y in zip(elements(a, 3), elements(b, 1))], 3)


def linear_combination(cols, n, wp, stride, k, weights, ww):
    """out[i] = sum_{j<k} cols[j * stride + i] * weights[j]; the words between n * wp and stride of a column are not looked at"""
    cols = np.asarray(cols, dtype=np.uint64).reshape(-1)
    ws = elements(weights, ww)
    assert len(ws) == k
    wo = max(wp, ww)
    acc = [f_zero(wo)] * n
    for j in range(k):
        col = elements(cols[j * stride:j * stride + n * wp], wp)
        acc = [f_add(s, f_mul(c, ws[j])) for s, c in zip(acc, col)]
    return words(acc, wo)
