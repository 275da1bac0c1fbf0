"""NumPy restatement of the elastic sequence search defined in include/dlc.h (dlc_sequence_elastic_topk): the recursion
itself, vectorised over columns and output rows, fp64 / int64, one addition per cell and level in the same order, so that
every comparison against the GPU is exact.  For an output row r with r - (L-1) >= 0 and rho(t) = r - (L-1) + t:

    A_0(c) = M[rho(0)][c]                           valid iff 0 <= c < lim(rho(0)) and the element is not NaN
    A_t(c) = P_t(c) + M[rho(t)][c]                  P_t(c) = the best valid A_{t-1}(c - d), d = d_min .. d_max, the
                                                    lowest d among equals; valid iff P_t exists, c < lim(rho(t)), not NaN
    E(r, j) = A_{L-1}(j),    span(r, j) = j - (the column the chosen chain started in)

"Best", the limits and the order of a row's list are sequence_oracle's (dlc_sequence_topk's).
"""
import numpy as np

from sequence_oracle import limits, merit_keys, same_bits   # noqa: F401  (same_bits: for the tests that import this module)


def elastic_scores(matrix, L, d_min, d_max, n=None, limit0=None, limit_step=0, lower_is_better=False, row0=0, only=None):
    """(E [rows - row0, n], span [rows - row0, n] int32).  E is fp64 (NaN where a cell is not offered) for float input and
    int64 (-1) for int64 input; span is -1 where the cell is not offered.  only: the rows of the matrix to work out (a cell
    is a function of the L rows behind it); the other rows of the result are then not meaningful."""
    m = np.asarray(matrix)
    is_int = m.dtype == np.int64
    if not is_int:
        m = m.astype(np.float64)                                   # fp32 -> fp64 is exact
    rows = m.shape[0]
    n = m.shape[1] if n is None else n
    m = m[:, :n]
    lim = limits(rows, n, n if limit0 is None else limit0, limit_step)
    inside = np.arange(n)[None, :] < lim[:, None]
    out = np.arange(L - 1, rows)                                   # the output rows that offer anything
    if only is not None:
        out = np.intersect1d(out, only)
    e_all = np.full((rows, n), -1 if is_int else np.nan, m.dtype)
    span_all = np.full((rows, n), -1, np.int32)
    if out.size:
        with np.errstate(invalid="ignore", over="ignore"):
            val = m[out - (L - 1)].copy()
            ok = inside[out - (L - 1)].copy()
            if not is_int:
                ok &= ~np.isnan(val)
            start = np.broadcast_to(np.arange(n, dtype=np.int32), val.shape).copy()   # the column a cell's chain began in
            for t in range(1, L):
                # what "best" compares: the integers themselves, or the fp64 values' ordered keys (-0.0 below +0.0)
                rank = val if is_int else merit_keys(val, False)
                none = np.ones(val.shape, bool)                    # no valid predecessor yet
                b_rank = np.zeros(val.shape, rank.dtype)
                b_val = b_rank if is_int else np.zeros(val.shape, m.dtype)
                b_start = np.zeros(val.shape, np.int32)
                for d in range(d_min, d_max + 1):                  # ascending d, strict compare: the lowest d among equals
                    if d >= n:
                        break
                    cand, best = rank[:, :n - d], b_rank[:, d:]    # column c takes column c - d
                    take = ok[:, :n - d] & (none[:, d:] | ((cand < best) if lower_is_better else (cand > best)))
                    np.copyto(best, cand, where=take)
                    if not is_int:
                        np.copyto(b_val[:, d:], val[:, :n - d], where=take)
                    np.copyto(b_start[:, d:], start[:, :n - d], where=take)
                    none[:, d:] &= ~take
                val = b_val + m[out - (L - 1) + t]
                ok = ~none & inside[out - (L - 1) + t]
                if not is_int:
                    ok &= ~np.isnan(val)
                start = b_start
            span = np.arange(n, dtype=np.int32)[None, :] - start
        e_all[out] = np.where(ok, val, e_all[out])
        span_all[out] = np.where(ok, span, -1)
    return e_all[row0:], span_all[row0:]


def elastic_topk(matrix, k, L, d_min, d_max, n=None, limit0=None, limit_step=0, lower_is_better=False, row0=0):
    """(scores [rows - row0, k], idx int64, span int32): the k best offered cells per row, best first, ties -> lower j;
    empty slots: index -1, span -1, score -inf (+inf when lower is better) or -1 for int64 input."""
    s, sp = elastic_scores(matrix, L, d_min, d_max, n, limit0, limit_step, lower_is_better, row0)
    return topk_of(s, sp, k, lower_is_better)


def topk_of(s, sp, k, lower_is_better):
    """The lists of dense scores s with spans sp (-1: not offered)."""
    is_int = s.dtype == np.int64
    rows = s.shape[0]
    empty = -1 if is_int else (np.inf if lower_is_better else -np.inf)
    out_s = np.full((rows, k), empty, s.dtype)
    out_i = np.full((rows, k), -1, np.int64)
    out_v = np.full((rows, k), -1, np.int32)
    for r in range(rows):
        cols = np.nonzero(sp[r] >= 0)[0]
        if not cols.size:
            continue
        worse = ~merit_keys(s[r, cols], lower_is_better)           # ascending = best first
        order = cols[np.lexsort((cols, worse))][:k]
        out_s[r, :order.size], out_i[r, :order.size], out_v[r, :order.size] = s[r, order], order, sp[r, order]
    return out_s, out_i, out_v


def planted_elastic_revisit():
    """int8 descriptors [300, 64] with a planted revisit at a CHANGING speed: frames 220 .. 279 revisit key-frames
    true[i] = 40 + (the sum of i steps drawn from {0, 1, 2}), each a copy with 24 bytes redrawn, and for every
    revisiting frame an alias -- a copy of it with only 6 bytes redrawn -- replaces an older frame away from the
    revisited stretch (sequence_oracle.planted_revisit with a step pattern; two random streams, drawn in this order).
    Returns (descriptors, true index per revisiting frame, alias index, first revisiting frame)."""
    dim, length, revisit = 64, 60, 220
    rng = np.random.RandomState(7)
    x = rng.randint(-128, 128, size=(300, dim)).astype(np.int8)
    steps = np.random.RandomState(3).randint(0, 3, size=length)
    true = 40 + np.concatenate([[0], np.cumsum(steps[:length - 1])])

    def redraw(row, count):
        row = row.copy()
        at = rng.permutation(dim)[:count]
        row[at] = (row[at].astype(np.int16) + rng.randint(1, 256, size=count)).astype(np.uint8).view(np.int8)   # never the old byte
        return row

    for i in range(length):
        x[revisit + i] = redraw(x[true[i]], 24)
    older = np.setdiff1d(np.arange(0, 190), np.arange(38, true.max() + 3))
    alias = rng.permutation(older)[:length]
    for i in range(length):
        x[alias[i]] = redraw(x[revisit + i], 6)
    return x, true, alias, revisit
