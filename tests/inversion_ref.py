"""Expected values for batch_inversion / inverse_or_zero (math/traits.rs:39-45, :93-121), written independently of the library and
of the oracle: Python integers, one inversion per element.  A BFieldElement's raw word is v * 2^64 mod p, so the raw word of v^-1
is 2^128 / raw mod p; an XFieldElement [c0, c1, c2] (canonical values) is inverted by the cofactors of its multiplication matrix in
F_p[x] / (x^3 - x + 1) (x_field_element.rs:512-536) over the determinant.  tests/test_batch_inversion_cpu.py pins this builder
against tests/pyref (Fermat in the field of p^3 elements) and against the oracle's bfe_inverse / xfe_inverse."""
import numpy as np

P = (1 << 64) - (1 << 32) + 1
R = (1 << 64) % P
R2 = R * R % P
R_INV = pow(R, P - 2, P)


def bfe_inv_raw(raw: int) -> int:
    """raw word of the inverse of the element with raw word `raw` (0 -> 0)."""
    return R2 * pow(int(raw), P - 2, P) % P


def xfe_inv_values(a):
    """inverse of the XFieldElement with canonical values a = (a0, a1, a2) != 0."""
    a0, a1, a2 = (int(v) for v in a)
    # multiplication by a: [[a0, -a2, -a1], [a1, a0 + a2, a1 - a2], [a2, a1, a0 + a2]]; a^-1 = its first column of the inverse
    s, d = a0 + a2, a1 - a2
    c0 = (s * s - d * a1) % P
    c1 = (d * a2 - a1 * s) % P
    c2 = (a1 * a1 - s * a2) % P
    det = (a0 * c0 - a2 * c1 - a1 * c2) % P
    di = pow(det, P - 2, P)
    return (c0 * di % P, c1 * di % P, c2 * di % P)


def xfe_inv_raw(raw3):
    vals = [int(r) * R_INV % P for r in raw3]
    return [v * R % P for v in xfe_inv_values(vals)]


def expected(x: np.ndarray, width: int, or_zero: bool = True) -> np.ndarray:
    """the words batch_inversion (no zero in x) / inverse_or_zero returns for the raw words x."""
    x = np.asarray(x, dtype=np.uint64).reshape(-1)
    out = np.zeros_like(x)
    if width == 1:
        for i, r in enumerate(x.tolist()):
            if r:
                out[i] = bfe_inv_raw(r)
            elif not or_zero:
                raise ZeroDivisionError(i)
        return out
    for i in range(x.size // 3):
        e = x[3 * i:3 * i + 3].tolist()
        if any(e):
            out[3 * i:3 * i + 3] = xfe_inv_raw(e)
        elif not or_zero:
            raise ZeroDivisionError(i)
    return out
