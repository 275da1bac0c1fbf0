"""NumPy restatement of the sequence search defined in include/dlc.h (dlc_sequence_topk): fp64 / int64, the same order of
additions, so that every comparison against the GPU is exact.

    Z_v(r, j) = M[r][j - off[v][0]] + M[r-1][j - off[v][1]] + ... + M[r-L+1][j - off[v][L-1]]     (left to right)

valid when r - (L-1) >= 0, j < lim(r), every element read lies in 0 <= column < lim(its row), and the sum is not NaN;
lim(r) = clamp(limit0 + r * limit_step, 0, n).  S(r, j) is the best valid Z_v (the lowest v on a tie), a row's list its k
best cells (ties -> the lower j).  fp64 values are ordered as dlc_topk_rows_f64 orders them: by the number, -0.0 below +0.0.
"""
import numpy as np

SIGN = np.uint64(1 << 63)


def merit_keys(values, lower_is_better):
    """uint64 keys whose unsigned order is the order of merit (larger = better) of fp64 / int64 values."""
    v = np.ascontiguousarray(values)
    if v.dtype == np.int64:
        key = v.view(np.uint64) ^ SIGN
    else:
        u = v.astype(np.float64).view(np.uint64)
        key = np.where(u >> np.uint64(63) != 0, ~u, u | SIGN)
    return ~key if lower_is_better else key


def limits(rows, n, limit0, limit_step):
    return np.clip(limit0 + np.arange(rows, dtype=np.int64) * limit_step, 0, n)


def sequence_scores(matrix, L, offsets, n=None, limit0=None, limit_step=0, lower_is_better=False, row0=0):
    """(S [rows - row0, n], slope [rows - row0, n] int32).  S is fp64 (NaN where a cell is not offered) for float input and
    int64 (-1) for int64 input; slope is -1 where the cell is not offered."""
    m = np.asarray(matrix)
    is_int = m.dtype == np.int64
    if not is_int:
        m = m.astype(np.float64)                                   # fp32 -> fp64 is exact
    rows = m.shape[0]
    n = m.shape[1] if n is None else n
    m = m[:, :n]
    offsets = np.asarray(offsets, dtype=np.int64).reshape(-1, L)
    lim = limits(rows, n, n if limit0 is None else limit0, limit_step)
    inside = np.arange(n)[None, :] < lim[:, None]                  # [rows, n] what each row offers
    best_key = np.zeros((rows, n), np.uint64)
    best_val = np.zeros((rows, n), m.dtype)
    slope = np.full((rows, n), -1, np.int32)
    with np.errstate(invalid="ignore", over="ignore"):
        for v, off in enumerate(offsets):
            acc = np.zeros((rows, n), m.dtype)
            ok = np.ones((rows, n), bool)
            for s in range(L):
                o = int(off[s])
                el = np.zeros((rows, n), m.dtype)
                el_ok = np.zeros((rows, n), bool)
                if s < rows and o < n:
                    el[s:, o:] = m[:rows - s, :n - o]
                    el_ok[s:, o:] = inside[:rows - s, :n - o]
                acc = el.copy() if s == 0 else acc + el             # (0 + x would turn -0.0 into +0.0)
                ok &= el_ok
            if not is_int:
                ok &= ~np.isnan(acc)
            key = merit_keys(acc, lower_is_better)
            take = ok & ((slope < 0) | (key > best_key))
            best_key[take], best_val[take], slope[take] = key[take], acc[take], v
    s_out = best_val.copy()
    s_out[slope < 0] = -1 if is_int else np.nan
    return s_out[row0:], slope[row0:]


def sequence_topk(matrix, k, L, offsets, n=None, limit0=None, limit_step=0, lower_is_better=False, row0=0):
    """(scores [rows - row0, k], idx int64, slope int32): the k best offered cells per row, best first, ties -> lower j;
    empty slots: index -1, slope -1, score -inf (+inf when lower is better) or -1 for int64 input."""
    s, sl = sequence_scores(matrix, L, offsets, n, limit0, limit_step, lower_is_better, row0)
    is_int = s.dtype == np.int64
    rows = s.shape[0]
    empty = -1 if is_int else (np.inf if lower_is_better else -np.inf)
    out_s = np.full((rows, k), empty, s.dtype)
    out_i = np.full((rows, k), -1, np.int64)
    out_v = np.full((rows, k), -1, np.int32)
    for r in range(rows):
        cols = np.nonzero(sl[r] >= 0)[0]
        if not cols.size:
            continue
        worse = ~merit_keys(s[r, cols], lower_is_better)           # ascending = best first
        order = cols[np.lexsort((cols, worse))][:k]
        out_s[r, :order.size], out_i[r, :order.size], out_v[r, :order.size] = s[r, order], order, sl[r, order]
    return out_s, out_i, out_v


def same_bits(a, b):
    """Exact equality of two result arrays: fp64 by bit pattern except that any NaN equals any NaN (compared by position)."""
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype != np.float64:
        return np.array_equal(a, b)
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint64), b[~nb].view(np.uint64))


def planted_revisit(frames=260, dim=64, first=50, length=60, revisit=200, seed=7, true_changes=24, alias_changes=6):
    """int8 descriptors with a planted revisit: frames revisit .. revisit + length - 1 are copies of frames first .. with
    `true_changes` bytes redrawn, and for every revisiting frame an ALIAS -- a copy of it with only `alias_changes` bytes
    redrawn -- replaces an older frame at a seeded permutation of the indices outside the revisited stretch (scattered,
    so no line through the score matrix follows them).  Returns (descriptors, true index per revisiting frame, alias index)."""
    rng = np.random.RandomState(seed)
    x = rng.randint(-128, 128, size=(frames, dim)).astype(np.int8)

    def redraw(row, count):
        row = row.copy()
        at = rng.permutation(dim)[:count]
        row[at] = (row[at].astype(np.int16) + rng.randint(1, 256, size=count)).astype(np.uint8).view(np.int8)   # never the old byte
        return row

    for i in range(length):
        x[revisit + i] = redraw(x[first + i], true_changes)
    older = np.concatenate([np.arange(0, first), np.arange(first + length, revisit - 30)])
    alias = rng.permutation(older)[:length]
    for i in range(length):
        x[alias[i]] = redraw(x[revisit + i], alias_changes)
    return x, first + np.arange(length), alias
