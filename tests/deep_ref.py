"""Expected values of the DEEP quotients (tf_deep_quotient_dev, tf_deep_quotient_rows_dev): the formula of include/tf_hip.h,

    out[i] = sum_p ( sum_c w[p][c] * (T_c[i] - v[p][c]) ) / (x_i - z_p),    x_i = offset * w_n^i,

evaluated literally, element by element and term by term, in Python integers on canonical values: tests/pyref for the extension
field (xfe_add, xfe_sub, xfe_mul, root_of_unity, to_raw, to_val) and tests/points_ref for the inverse.  Raw Montgomery words only at
the two ends; the layouts are those of the header.  Shares nothing with the kernels.

`codeword_by_sums` is the same value regrouped for the one test whose 65 535 columns the literal loop cannot walk in seconds:
sum_c w T_c[i] - sum_c w v, each sum one integer dot product.  tests/test_deep_cpu.py pins it to the literal model."""
import operator

import numpy as np

from tests import points_ref as pr
from tests import pyref

P = pyref.P
ZERO = (0, 0, 0)


def xfes(raw):
    """raw words, three per element -> list of triples of canonical values"""
    vals = [pyref.to_val(int(r)) for r in np.asarray(raw, dtype=np.uint64).reshape(-1)]
    return [tuple(vals[3 * i:3 * i + 3]) for i in range(len(vals) // 3)]


def words(elems):
    return np.array([pyref.to_raw(c) for e in elems for c in e], dtype=np.uint64)


def domain_point(n, offset_raw, i):
    """x_i = offset * w_n^i as a canonical value"""
    return pyref.to_val(int(offset_raw)) * pow(pyref.root_of_unity(n), int(i), P) % P


def column_row(main, k1, stride_main, aux, k3, stride_aux, i):
    """row i of the two column-major tables: k1 lifted BFieldElements, then k3 XFieldElements"""
    row = [pyref.xfe(pyref.to_val(int(main[c * stride_main + i]))) for c in range(k1)]
    for c in range(k3):
        at = c * stride_aux + 3 * i
        row.append(tuple(pyref.to_val(int(aux[at + m])) for m in range(3)))
    return row


def opened_row(main_rows, k1, row_stride_main, aux_rows, k3, row_stride_aux, r):
    """row r of the row-major rows that tf_table_gather_rows_dev wrote"""
    row = [pyref.xfe(pyref.to_val(int(main_rows[r * row_stride_main + c]))) for c in range(k1)]
    for c in range(k3):
        at = r * row_stride_aux + 3 * c
        row.append(tuple(pyref.to_val(int(aux_rows[at + m])) for m in range(3)))
    return row


def element(row, x, z, w, v):
    """the formula at one domain point x for one table row; None where a denominator is zero"""
    k = len(row)
    total = ZERO
    for p, zp in enumerate(z):
        s = ZERO
        for c in range(k):
            s = pyref.xfe_add(s, pyref.xfe_mul(w[p * k + c], pyref.xfe_sub(row[c], v[p * k + c])))
        den = pyref.xfe_sub(pyref.xfe(x), zp)
        if den == ZERO:
            return None
        total = pyref.xfe_add(total, pyref.xfe_mul(s, pr.f_inv(den, 3)))
    return total


def _operands(points, weights, values, k):
    z = xfes(points)
    w, v = (xfes(weights), xfes(values)) if k else ([], [])
    assert 1 <= len(z) <= 4 and len(w) == len(z) * k and len(v) == len(z) * k
    return z, w, v


def codeword(main, k1, stride_main, aux, k3, stride_aux, n, offset_raw, points, weights, values, at=None):
    """-> (3 words per position of `at` (default: every i < n), positions with a zero denominator; their slots hold zeros)"""
    z, w, v = _operands(points, weights, values, k1 + k3)
    out, bad = [], []
    for i in (range(n) if at is None else at):
        y = element(column_row(main, k1, stride_main, aux, k3, stride_aux, i), domain_point(n, offset_raw, i), z, w, v)
        if y is None:
            bad.append(int(i))
            y = ZERO
        out.append(y)
    return words(out), bad


def rows(main_rows, k1, row_stride_main, aux_rows, k3, row_stride_aux, n, offset_raw, indices, points, weights, values):
    """-> (3 words per index, rows with a zero denominator, rows whose index is >= n); the slots of both kinds hold zeros"""
    z, w, v = _operands(points, weights, values, k1 + k3)
    out, bad_zero, bad_index = [], [], []
    for r, i in enumerate(int(j) for j in np.asarray(indices).reshape(-1).astype(np.int64) & 0xFFFFFFFF):
        y = ZERO
        if i >= n:
            bad_index.append(r)
        else:
            y = element(opened_row(main_rows, k1, row_stride_main, aux_rows, k3, row_stride_aux, r), domain_point(n, offset_raw, i), z, w, v)
            if y is None:
                bad_zero.append(r)
                y = ZERO
        out.append(y)
    return words(out), bad_zero, bad_index


def _dot(a, b):
    return sum(map(operator.mul, a, b)) % P


def _dots(rows_raw, weights_val):
    """[sum_c rows_raw[i][c] * weights_val[c] mod p for every row i], exactly: both operands are cut into 16-bit limbs, whose
    products summed over fewer than 2^16 columns stay below 2^48 in numpy's 64-bit integers; Python integers put the sixteen partial
    sums back together.  rows_raw holds raw words, so the result is converted once (to_val is linear)."""
    a = np.asarray(rows_raw, dtype=np.uint64)
    b = np.array(weights_val, dtype=np.uint64)
    assert a.ndim == 2 and a.shape[1] == b.size and b.size < (1 << 16)
    total = [0] * a.shape[0]
    for la in range(4):
        al = (a >> np.uint64(16 * la)) & np.uint64(0xFFFF)
        for lb in range(4):
            part = al @ ((b >> np.uint64(16 * lb)) & np.uint64(0xFFFF))
            for i, x in enumerate(part.tolist()):
                total[i] += x << (16 * (la + lb))
    return [pyref.to_val(t % P) for t in total]


def codeword_by_sums(main, k1, stride_main, aux, k3, stride_aux, n, offset_raw, points, weights, values):
    """codeword() regrouped as (sum_c w T_c[i]) - (sum_c w v): one integer dot product per coefficient of the unreduced product, for
    all i at once, and x^3 = x - 1 once per sum.  No zero denominators (asserted)."""
    k = k1 + k3
    z, w, v = _operands(points, weights, values, k)
    main_rows = np.stack([main[c * stride_main:c * stride_main + n] for c in range(k1)], axis=1) if k1 else np.zeros((n, 0), np.uint64)
    aux_cols = np.stack([aux[c * stride_aux:c * stride_aux + 3 * n] for c in range(k3)]).reshape(k3, n, 3) if k3 else np.zeros((0, n, 3), np.uint64)

    def fold(d):
        return ((d[0] - d[3]) % P, (d[1] + d[3] - d[4]) % P, (d[2] + d[4]) % P)

    total = [ZERO] * n
    for p, zp in enumerate(z):
        wp, vp = w[p * k:(p + 1) * k], v[p * k:(p + 1) * k]
        wq = [[e[q] for e in wp] for q in range(3)]
        d = [[0] * 5 for _ in range(n)]                       # the unreduced coefficients of sum_c w T_c[i], per i
        for q in range(3):
            for i, x in enumerate(_dots(main_rows, wq[q][:k1])):
                d[i][q] += x
            for m in range(3):
                for i, x in enumerate(_dots(aux_cols[:, :, m].T, wq[q][k1:])):
                    d[i][m + q] += x
        c = [0] * 5
        for m in range(3):
            for q in range(3):
                c[m + q] += _dot([e[m] for e in vp], wq[q])
        c_p = fold(c)
        for i in range(n):
            den = pyref.xfe_sub(pyref.xfe(domain_point(n, offset_raw, i)), zp)
            assert den != ZERO
            total[i] = pyref.xfe_add(total[i], pyref.xfe_mul(pyref.xfe_sub(fold(d[i]), c_p), pr.f_inv(den, 3)))
    return words(total)


# ---- layouts
def strided(packed, lines, line_words, stride, fill):
    """`lines` lines of line_words words at `stride`, the padding between them (none behind the last) filled with `fill`"""
    packed = np.asarray(packed, dtype=np.uint64).reshape(-1)
    if lines == 0 or line_words == 0:
        return np.zeros(0, dtype=np.uint64)
    out = np.full((lines - 1) * stride + line_words, fill, dtype=np.uint64)
    for c in range(lines):
        out[c * stride:c * stride + line_words] = packed[c * line_words:(c + 1) * line_words]
    return out


def padding(lines, line_words, stride):
    """bool mask over strided(...): True on the padding words"""
    if lines == 0 or line_words == 0:
        return np.zeros(0, dtype=bool)
    mask = np.ones((lines - 1) * stride + line_words, dtype=bool)
    for c in range(lines):
        mask[c * stride:c * stride + line_words] = False
    return mask
