"""Expected values of the point, power and gather calls (tf_get_colinear_y, tf_are_colinear, tf_mod_pow, tf_powers,
tf_gather_elements_dev), as the reference states them (math/polynomial.rs:348-394, b_field_element.rs:340-353) -- pure Python
integers on top of tests/pyref (xfe_*, to_raw, to_val) and Python's pow: canonical values in, `% P` arithmetic, raw Montgomery
words only at the two ends.  Shares nothing with the kernels.  An XFieldElement is inverted by tests/inversion_ref's cofactor
formula (one base-field pow instead of pyref.xfe_inv's 192-bit exponent; the CPU tests pin the two to each other).
tests/test_field_points_cpu.py pins this model to the reference's doc examples, pyref and the oracle; the GPU tests compare with it
word for word."""
import numpy as np

from tests import inversion_ref, pyref

P = pyref.P
PAIRS = ((1, 1), (3, 3), (1, 3))


# ---- elements: an int (width 1) or a 3-tuple (width 3) of canonical values
def elements(raw, w):
    vals = [pyref.to_val(int(r)) for r in np.asarray(raw, dtype=np.uint64).reshape(-1)]
    return vals if w == 1 else [tuple(vals[3 * i:3 * i + 3]) for i in range(len(vals) // 3)]


def words(elems, w):
    flat = list(elems) if w == 1 else [c for e in elems for c in e]
    return np.array([pyref.to_raw(v) for v in flat], dtype=np.uint64)


def lift(a, w_from, w_to):
    return a if w_from == w_to else pyref.xfe(a)


def one(w):
    return 1 if w == 1 else (1, 0, 0)


def zero(w):
    return 0 if w == 1 else (0, 0, 0)


def f_sub(a, b, w):
    return (a - b) % P if w == 1 else pyref.xfe_sub(a, b)


def f_add(a, b, w):
    return (a + b) % P if w == 1 else pyref.xfe_add(a, b)


def f_mul(a, b, w):
    return a * b % P if w == 1 else pyref.xfe_mul(a, b)


def f_inv(a, w):
    return pow(a, P - 2, P) if w == 1 else inversion_ref.xfe_inv_values(a)


def f_pow(a, e, w):
    return pow(a, e, P) if w == 1 else pyref.xfe_pow(a, e)


# ---- the calls on elements
def colinear_y_elem(p0, p1, p2x, wx, wy):
    """polynomial.rs:386-394 with the x-coordinates lifted into the field of the y-coordinates; None where the reference panics"""
    x0, x1 = lift(p0[0], wx, wy), lift(p1[0], wx, wy)
    if x0 == x1:
        return None
    dy = f_sub(p0[1], p1[1], wy)
    dx = f_sub(x0, x1, wy)
    t = f_add(f_mul(dy, f_sub(p2x, x0, wy), wy), f_mul(dx, p0[1], wy), wy)
    return f_mul(t, f_inv(dx, wy), wy)


def are_colinear_elem(points, wx, wy):
    """polynomial.rs:348-364, step by step: the slope by a division, then a x + b == y"""
    if len(points) < 3:
        return False
    xs = [x for x, _ in points]
    if len(set(xs)) != len(xs):
        return False
    (x0, y0), (x1, y1) = [(lift(x, wx, wy), y) for x, y in points[:2]]
    a = f_mul(f_sub(y0, y1, wy), f_inv(f_sub(x0, x1, wy), wy), wy)
    b = f_sub(y0, f_mul(a, x0, wy), wy)
    return all(f_add(f_mul(a, lift(x, wx, wy), wy), b, wy) == y for x, y in points[2:])


# ---- the calls on raw words (numpy uint64 in and out), with the layouts of include/tf_hip.h
def get_colinear_y(x0, y0, x1, y1, p2x, wx, wy):
    """-> (out words, list of the offending triples); an offending triple's slot holds zeros"""
    ex0, ex1, ey0, ey1, ep = elements(x0, wx), elements(x1, wx), elements(y0, wy), elements(y1, wy), elements(p2x, wy)
    n = len(ex0)
    assert len(ep) in (1, n)
    out, bad = [], []
    for i in range(n):
        y = colinear_y_elem((ex0[i], ey0[i]), (ex1[i], ey1[i]), ep[i if len(ep) == n else 0], wx, wy)
        if y is None:
            bad.append(i)
            y = zero(wy)
        out.append(y)
    return words(out, wy), bad


def are_colinear(xs, ys, n_groups, k, wx, wy):
    ex, ey = elements(xs, wx), elements(ys, wy)
    assert len(ex) == n_groups * k and len(ey) == n_groups * k
    return np.array([int(are_colinear_elem(list(zip(ex[g * k:(g + 1) * k], ey[g * k:(g + 1) * k])), wx, wy)) for g in range(n_groups)],
                    dtype=np.int32)


def mod_pow(bases, exps, w, n):
    eb = elements(bases, w)
    ee = [int(e) for e in np.asarray(exps, dtype=np.uint64).reshape(-1)]
    assert len(eb) in (1, n) and len(ee) in (1, n)
    return words([f_pow(eb[i if len(eb) == n else 0], ee[i if len(ee) == n else 0], w) for i in range(n)], w)


def powers(first, ratio, w, n):
    acc, r = elements(first, w)[0], elements(ratio, w)[0]
    out = []
    for _ in range(n):
        out.append(acc)
        acc = f_mul(acc, r, w)
    return words(out, w)


def gather(src, width, indices):
    """-> (out words with the slots of out-of-range indices zeroed, list of those slots)"""
    src = np.asarray(src, dtype=np.uint64).reshape(-1, width)
    out = np.zeros((len(indices), width), dtype=np.uint64)
    bad = []
    for i, j in enumerate(indices):
        if int(j) < len(src):
            out[i] = src[int(j)]
        else:
            bad.append(i)
    return out.reshape(-1), bad
