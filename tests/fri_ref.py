"""Expected values of the FRI fold (tf_fri_fold): pure Python integers on top of tests/pyref (through the element helpers of
tests/points_ref), canonical values in, `% P` arithmetic, raw Montgomery words only at the two ends.  Shares nothing with the kernels.

One level on a codeword c of n elements over {g w_n^i} is the closed form of Polynomial::get_colinear_y through (x_i, c[i]) and
(-x_i, c[i + n/2]) at alpha (math/polynomial.rs:386-394),

    out[i] = 1/2 [(1 + alpha / x_i) c[i] + (1 - alpha / x_i) c[i + n/2]],   x_i = g w_n^i,

with x_i^-1 a base-field pow.  tests/test_fri_fold_cpu.py pins it to points_ref.get_colinear_y, to polynomials (p_even + alpha p_odd
on the squared coset) and to the oracle; the GPU tests compare with it word for word."""
import numpy as np

from tests import points_ref as pr
from tests import pyref

P = pyref.P
HALF = (P + 1) // 2


def f_scale(a, s, w):
    """the element a of w words times the base-field value s"""
    return a * s % P if w == 1 else tuple(c * s % P for c in a)


def domain(g, n):
    """[g w_n^i for i < n], canonical values"""
    w, x, out = pyref.root_of_unity(n), g % P, []
    for _ in range(n):
        out.append(x)
        x = x * w % P
    return out


def fold_level(c, n, wc, g, alpha, wa):
    """c: n elements of width wc on {g w_n^i}; -> n/2 elements of width wa on {g^2 w_{n/2}^i}"""
    xs = domain(g, n)
    one, h, out = pr.one(wa), n // 2, []
    for i in range(h):
        t = f_scale(alpha, pow(xs[i], P - 2, P), wa)  # alpha / x_i
        a, b = pr.lift(c[i], wc, wa), pr.lift(c[i + h], wc, wa)
        s = pr.f_add(pr.f_mul(pr.f_add(one, t, wa), a, wa), pr.f_mul(pr.f_sub(one, t, wa), b, wa), wa)
        out.append(f_scale(s, HALF, wa))
    return out


def fold_elements(c, n, wc, g, alphas, wa):
    """len(alphas) levels in a row: level j on the offset g^(2^(j-1)) and the length n / 2^(j-1)"""
    for alpha in alphas:
        c = fold_level(c, n, wc, g, alpha, wa)
        n, wc, g = n // 2, wa, g * g % P
    return c


def fold(words, n, batch, wc, g_raw, challenge_words, levels, n_sets, wa):
    """the layouts of include/tf_hip.h: raw words in (numpy uint64), raw words out"""
    cw, ch = pr.elements(words, wc), pr.elements(challenge_words, wa)
    assert len(cw) == batch * n and len(ch) == n_sets * levels and n_sets in (1, batch) and (1 << levels) <= n
    g = pyref.to_val(int(g_raw))
    out = []
    for b in range(batch):
        s = b if n_sets != 1 else 0
        out += fold_elements(cw[b * n:(b + 1) * n], n, wc, g, ch[s * levels:(s + 1) * levels], wa)
    return pr.words(out, wa)
