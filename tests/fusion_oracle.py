"""NumPy restatement of the multi-descriptor fusion defined in include/dlc.h (dlc_fuse_rows): fp64, every operation rounded
on its own, every row sum in the TREE order, so that every comparison against the GPU is exact.

    TREE(v_0 .. v_{c-1}): P the smallest power of two >= c, v_j = -0.0 for c <= j < P,
        T(lo, 1) = v_lo;  T(lo, len) = T(lo, len / 2) + T(lo + len / 2, len / 2);  TREE = T(0, P)

    per source i and row r with c = lim(r) >= 1 offered cells x_j:
        none:    u_j = x_j, or -x_j if the source is lower-is-better
        zscore:  mean = TREE(x) / c;  d_j = x_j - mean;  sd = sqrt(TREE(d_j * d_j) / (c - 1))
                 u_j = 0.0 if c < 2 or sd == 0.0, else d_j / sd, or (mean - x_j) / sd if lower-is-better
        minmax:  lo, hi = the least / greatest offered cell (-0.0 below +0.0); a NaN among them: every u_j NaN
                 range = hi - lo;  u_j = 0.0 if range == 0.0, else (x_j - lo) / range, or (hi - x_j) / range
    out[r][j] = ((w_0 u_0j + w_1 u_1j) + ...) + w_{m-1} u_{m-1,j}, starting from the first term

tree_recursive is the definition word for word; tree_rows is the same tree level by level over whole rows
(a[:, 0::2] + a[:, 1::2]); NumPy's +, -, *, / and sqrt on float64 are the IEEE operations.
"""
import numpy as np

from sequence_oracle import limits, merit_keys

NORMS = ("none", "zscore", "minmax")


def _pow2(c):
    p = 1
    while p < c:
        p *= 2
    return p


def tree_recursive(v):
    """TREE of a 1-D fp64 array with at least one element, by the recursion itself."""
    v = np.asarray(v, np.float64)
    c = v.shape[0]

    def t(lo, length):
        if length == 1:
            return v[lo] if lo < c else np.float64(-0.0)
        with np.errstate(all="ignore"):
            return t(lo, length // 2) + t(lo + length // 2, length // 2)
    return np.float64(t(0, _pow2(c)))


def tree_rows(a, pad_to=None):
    """TREE of every row of a [rows, c >= 1] fp64 array, level by level; pad_to: a power of two >= c to pad to instead of
    the smallest (the result has the same bits)."""
    a = np.asarray(a, np.float64)
    rows, c = a.shape
    p = _pow2(c) if pad_to is None else pad_to
    assert p >= c and p & (p - 1) == 0
    x = np.full((rows, p), -0.0, np.float64)
    x[:, :c] = a
    with np.errstate(all="ignore"):
        while x.shape[1] > 1:
            x = x[:, 0::2] + x[:, 1::2]
    return x[:, 0]


def left_to_right(v):
    """The sum a sequential loop gives, starting from v_0: NOT the definition (test_fusion_cpu.py shows a row it differs on)."""
    s = np.float64(v[0])
    for x in v[1:]:
        s = s + np.float64(x)
    return s


def normalise_row(x, norm, lower_is_better):
    """u [c] of one source's offered cells x [c >= 1] (fp64 already)."""
    c = x.shape[0]
    with np.errstate(all="ignore"):
        if norm == "none":
            return -x if lower_is_better else x.copy()
        if norm == "zscore":
            mean = tree_rows(x[None, :])[0] / np.float64(c)
            d = x - mean
            sd = np.sqrt(tree_rows((d * d)[None, :])[0] / np.float64(c - 1))
            if c < 2 or sd == 0.0:
                return np.zeros(c, np.float64)
            return (mean - x) / sd if lower_is_better else d / sd
        if norm != "minmax":
            raise ValueError(norm)
        if np.isnan(x).any():
            return np.full(c, np.nan)
        key = merit_keys(x, False)                                 # unsigned order = the order of the numbers, -0.0 < +0.0
        lo, hi = x[np.argmin(key)], x[np.argmax(key)]
        rng = hi - lo
        if rng == 0.0:
            return np.zeros(c, np.float64)
        return (hi - x) / rng if lower_is_better else (x - lo) / rng


def fuse_rows(sources, weights=None, lower_is_better=False, norm="zscore", n=None, limit0=None, limit_step=0, out=None):
    """fp64 [rows, n]: the fused rows; cells that are not offered are NaN, or keep what `out` [rows, >= n] held (a copy of
    it is returned, whole)."""
    sources = [np.asarray(s) for s in sources]
    m = len(sources)
    rows = sources[0].shape[0]
    n = sources[0].shape[1] if n is None else n
    w = np.ones(m) if weights is None else np.asarray(weights, np.float64)
    lib = np.broadcast_to(np.asarray(lower_is_better, bool), (m,))
    lim = limits(rows, n, n if limit0 is None else limit0, limit_step)
    res = np.full((rows, n), np.nan) if out is None else np.array(out, np.float64)
    xs = [s[:, :n].astype(np.float64) for s in sources]            # fp32: exact; int64: round to nearest even
    with np.errstate(all="ignore"):
        for r in range(rows):
            c = int(lim[r])
            if c == 0:
                continue
            acc = None
            for i in range(m):
                t = np.float64(w[i]) * normalise_row(xs[i][r, :c], norm, bool(lib[i]))
                acc = t if acc is None else acc + t
            res[r, :c] = acc
    return res


def two_confusers_scene(rows=12, n=96, seed=3):
    """(scores fp64 [rows, n], distances int64 [rows, n], true column [rows]): two synthetic members of one place
    recognition problem.  Each member sees the true key-frame clearly, but a confuser of its OWN -- another column, not the
    other member's -- a little more clearly still: alone, each ranks its confuser first in every row.  The confusers are
    unremarkable to the other member, so the sum of the standardised rows ranks the true column first.  Background noise
    has sigma 1 (scores) and 1000 (distances); the true column stands 9 sigma out, a confuser 11."""
    rng = np.random.RandomState(seed)
    a = rng.randn(rows, n)
    d = np.rint(50000 + 1000 * rng.randn(rows, n)).astype(np.int64)
    true = (7 + 5 * np.arange(rows)) % n
    ca, cd = (true + 31) % n, (true + 57) % n
    r = np.arange(rows)
    a[r, true], a[r, ca] = 9.0, 11.0
    d[r, true], d[r, cd] = 50000 - 9000, 50000 - 11000
    return a, d, true
