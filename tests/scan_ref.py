"""Expected values of the prefix scans (tf_scan_sum_dev, tf_scan_product_dev, tf_scan_affine_dev):

    y_-1 = init,   y_i = a_i y_(i-1) + b_i,   out[i] = y_i

`loop` is the sequential loop on elements -- canonical values, an int (width 1) or a 3-tuple (width 3), with the arithmetic of
tests/points_ref (f_mul, f_add, lift).  `blocked` is the model of what the kernels do instead: tile maps (aggregate), the value at
every tile's start from turns of tile maps (spine), every tile from its start value (apply), with the tile and turn sizes as
parameters; tests/test_scan_cpu.py proves it equal to the loop.  The functions on raw words take and return numpy uint64 arrays in the
layouts of include/tf_hip.h.  Shares nothing with the kernels."""
import numpy as np

from tests import points_ref as pr
from tests import pyref

P = pyref.P
SUM, PRODUCT, AFFINE = 0, 1, 2
PAIRS = ((1, 1), (3, 3), (3, 1))  # (width_a, width_b) of affine


# ---- on elements
def neutral(mode, w):
    return pr.one(w) if mode == PRODUCT else pr.zero(w)


def loop(a, b, init, w):
    """a, b: lists of n elements of width w (None: all one / all zero); -> [y_0 .. y_(n-1)]"""
    n = len(a) if a is not None else len(b)
    y, out = init, []
    for i in range(n):
        if a is not None:
            y = pr.f_mul(a[i], y, w)
        if b is not None:
            y = pr.f_add(y, b[i], w)
        out.append(y)
    return out


def then(f, g, w):
    """first the map f = (A, B), then g: (g.A f.A, g.A f.B + g.B)"""
    return pr.f_mul(g[0], f[0], w), pr.f_add(pr.f_mul(g[0], f[1], w), g[1], w)


def apply(m, y, w):
    return pr.f_add(pr.f_mul(m[0], y, w), m[1], w)


def blocked(a, b, init, w, tile, turn):
    """-> (out, maps, starts): the scan computed as the kernels do; maps[t] is the map of tile t (None for the last, which nobody
    needs), starts[t] the value at its start"""
    n = len(a) if a is not None else len(b)
    elem = lambda i: (a[i] if a is not None else pr.one(w), b[i] if b is not None else pr.zero(w))  # noqa: E731
    tiles = -(-n // tile)
    maps = []
    for t in range(tiles - 1):                                    # aggregate
        m = (pr.one(w), pr.zero(w))
        for i in range(t * tile, (t + 1) * tile):
            m = then(m, elem(i), w)
        maps.append(m)
    maps.append(None)
    starts, carry = [], init
    for t0 in range(0, tiles, turn):                              # spine: turns of `turn` maps, the carry handed on
        run = (pr.one(w), pr.zero(w))
        for t in range(t0, min(t0 + turn, tiles)):
            starts.append(apply(run, carry, w))
            if maps[t] is not None:
                run = then(run, maps[t], w)
        carry = apply(run, carry, w)
    out = []
    for t in range(tiles):                                        # apply
        y = starts[t]
        for i in range(t * tile, min((t + 1) * tile, n)):
            y = apply(elem(i), y, w)
            out.append(y)
    return out, maps, starts


# ---- on raw words
def column(words, c, n, w, stride):
    return pr.elements(np.asarray(words, dtype=np.uint64).reshape(-1)[c * stride:c * stride + n * w], w)


def scan(mode, n, batch, a=None, b=None, wa=1, wb=1, stride_a=None, stride_b=None, a_len=None, a_sets=1, init=None, tile=None, turn=None):
    """The scan of `batch` columns on raw words -> (batch x n elements of w = max(wa, wb) words, packed; per column (maps, starts) of
    the blocked model when `tile` is given, else None).  sum reads b, product reads a; affine both, a_len = 1: a holds a_sets packed
    multipliers (a_len None: a table, whatever n).  init: None, one element, or one per column."""
    w = wb if mode == SUM else wa
    packed = mode == AFFINE and a_len == 1   # given as 1: packed, also for n = 1 (the library is told by stride_a = 0 there)
    sa = n * w if stride_a is None else stride_a
    sb = n * wb if stride_b is None else stride_b
    inits = None if init is None else pr.elements(init, w)
    out, inner = [], []
    for c in range(batch):
        ea = eb = None
        if mode != SUM:
            ea = column(a, c, n, w, sa) if not packed else [pr.elements(a, w)[c if a_sets == batch else 0]] * n
        if mode != PRODUCT:
            eb = [pr.lift(x, wb, w) for x in column(b, c, n, wb, sb)]
        y0 = neutral(mode, w) if inits is None else inits[c if len(inits) == batch else 0]
        if tile is None:
            out += loop(ea, eb, y0, w)
        else:
            o, maps, starts = blocked(ea, eb, y0, w, tile, turn)
            out += o
            inner.append((maps, starts))
    return pr.words(out, w), (inner if tile is not None else None)


def strided(packed, n, batch, w, stride, fill=0):
    """batch columns of n * w packed words laid out at `stride`; the words in between hold `fill`"""
    out = np.full((batch - 1) * stride + n * w if batch else 0, fill, dtype=np.uint64)
    for c in range(batch):
        out[c * stride:c * stride + n * w] = np.asarray(packed, dtype=np.uint64).reshape(batch, n * w)[c]
    return out


def padding(n, batch, w, stride):
    """mask of the words between n * w and the stride"""
    m = np.ones((batch - 1) * stride + n * w if batch else 0, dtype=bool)
    for c in range(batch):
        m[c * stride:c * stride + n * w] = False
    return m


def work_words(mode, inner, w):
    """(words, mask of the words nobody writes) of the work space after a call of two tiles or more per column: tiles x batch tile
    maps (the words a mode carries, A before B; the slot of a column's last tile stays as it was), then tiles x batch start values"""
    m_words = 2 * w if mode == AFFINE else w
    tiles = len(inner[0][1])
    maps = np.zeros(len(inner) * tiles * m_words, dtype=np.uint64)
    kept = np.zeros(maps.size + len(inner) * tiles * w, dtype=bool)
    starts = []
    for c, (col_maps, col_starts) in enumerate(inner):
        for t, m in enumerate(col_maps):
            at = (c * tiles + t) * m_words
            if m is None:
                kept[at:at + m_words] = True
                continue
            carried = [m[0]] if mode == PRODUCT else [m[1]] if mode == SUM else [m[0], m[1]]
            maps[at:at + m_words] = pr.words(carried, w)
        starts += col_starts
    return np.concatenate([maps, pr.words(starts, w)]), kept
