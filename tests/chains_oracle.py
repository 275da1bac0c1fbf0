"""NumPy restatement of the chains defined in include/dlc.h (dlc_sequence_elastic_chains, dlc_sequence_chains): for a
candidate cell (r, j) the column each of the L frames of its chain was matched to, oldest frame first, and the matrix cells
along them.

Elastic: the recursion of elastic_oracle.elastic_scores, which additionally keeps the step d every (level, column) chose
(-1: the cell is not valid), then the walk back from j: chain[L-1] = j, chain[t-1] = chain[t] - d_t(chain[t]).
Lines: sequence_oracle.sequence_scores gives the winning slope v* of the cell; chain[t] = j - off[v*][L-1-t].

A slot that is no chain (idx outside 0 .. lim(r)-1, a cell that is not valid) holds -1 in all L places, slope -1, and NaN
(-1 for int64 matrices) in cells.
"""
import numpy as np

from sequence_oracle import limits, merit_keys, sequence_scores


def elastic_steps(matrix, L, d_min, d_max, n=None, limit0=None, limit_step=0, lower_is_better=False):
    """(E [rows, n], steps [rows, L, n] int8): E as elastic_oracle.elastic_scores gives it, and for output row r the step
    chosen at level t in column c, steps[r, t, c] (level 0: 0), -1 where A_t(c) is not valid."""
    m = np.asarray(matrix)
    is_int = m.dtype == np.int64
    if not is_int:
        m = m.astype(np.float64)
    rows = m.shape[0]
    n = m.shape[1] if n is None else n
    m = m[:, :n]
    lim = limits(rows, n, n if limit0 is None else limit0, limit_step)
    inside = np.arange(n)[None, :] < lim[:, None]
    e_all = np.full((rows, n), -1 if is_int else np.nan, m.dtype)
    steps = np.full((rows, L, n), -1, np.int8)
    out = np.arange(L - 1, rows)
    if not out.size:
        return e_all, steps
    with np.errstate(invalid="ignore", over="ignore"):
        val = m[out - (L - 1)].copy()
        ok = inside[out - (L - 1)].copy()
        if not is_int:
            ok &= ~np.isnan(val)
        steps[out, 0] = np.where(ok, 0, -1)
        for t in range(1, L):
            rank = val if is_int else merit_keys(val, False)
            none = np.ones(val.shape, bool)
            b_rank = np.zeros(val.shape, rank.dtype)
            b_val = np.zeros(val.shape, m.dtype)
            b_d = np.full(val.shape, -1, np.int8)
            for d in range(d_min, d_max + 1):                      # ascending d, strict compare: the lowest d among equals
                if d >= n:
                    break
                cand, best = rank[:, :n - d], b_rank[:, d:]
                take = ok[:, :n - d] & (none[:, d:] | ((cand < best) if lower_is_better else (cand > best)))
                np.copyto(best, cand, where=take)
                np.copyto(b_val[:, d:], val[:, :n - d], where=take)
                np.copyto(b_d[:, d:], np.int8(d), where=take)
                none[:, d:] &= ~take
            val = b_val + m[out - (L - 1) + t]
            ok = ~none & inside[out - (L - 1) + t]
            if not is_int:
                ok &= ~np.isnan(val)
            steps[out, t] = np.where(ok, b_d, -1)
    e_all[out] = np.where(ok, val, e_all[out])
    return e_all, steps


def _fill(m, idx, L):
    is_int = np.asarray(m).dtype == np.int64
    idx = np.asarray(idx, dtype=np.int64)
    chain = np.full(idx.shape + (L,), -1, np.int32)
    cells = np.full(idx.shape + (L,), -1 if is_int else np.nan, np.int64 if is_int else np.float64)
    return idx, chain, cells


def elastic_chains(matrix, idx, L, d_min, d_max, n=None, limit0=None, limit_step=0, lower_is_better=False, row0=0):
    """(chain [rows - row0, k, L] int32, cells [rows - row0, k, L]) of the candidates idx [rows - row0, k]."""
    m = np.asarray(matrix)
    rows = m.shape[0]
    n = m.shape[1] if n is None else n
    lim = limits(rows, n, n if limit0 is None else limit0, limit_step)
    _, steps = elastic_steps(m, L, d_min, d_max, n, limit0, limit_step, lower_is_better)
    idx, chain, cells = _fill(m, idx, L)
    for q in range(idx.shape[0]):
        r = row0 + q
        for i in range(idx.shape[1]):
            j = int(idx[q, i])
            if not 0 <= j < lim[r] or steps[r, L - 1, j] < 0:
                continue
            c = j
            for t in range(L - 1, -1, -1):
                assert steps[r, t, c] >= 0                         # a chosen predecessor is valid
                chain[q, i, t] = c
                cells[q, i, t] = m[r - (L - 1) + t, c]
                c -= int(steps[r, t, c])
    return chain, cells


def line_chains(matrix, idx, L, offsets, n=None, limit0=None, limit_step=0, lower_is_better=False, row0=0):
    """(chain [rows - row0, k, L] int32, cells, slope [rows - row0, k] int32) of the candidates idx [rows - row0, k]."""
    m = np.asarray(matrix)
    offsets = np.asarray(offsets, dtype=np.int64).reshape(-1, L)
    _, slope_of = sequence_scores(m, L, offsets, n, limit0, limit_step, lower_is_better)
    idx, chain, cells = _fill(m, idx, L)
    slope = np.full(idx.shape, -1, np.int32)
    for q in range(idx.shape[0]):
        r = row0 + q
        for i in range(idx.shape[1]):
            j = int(idx[q, i])
            if not 0 <= j < slope_of.shape[1] or slope_of[r, j] < 0:
                continue
            v = slope[q, i] = slope_of[r, j]
            for t in range(L):
                chain[q, i, t] = j - offsets[v, L - 1 - t]
                cells[q, i, t] = m[r - (L - 1) + t, chain[q, i, t]]
    return chain, cells, slope


def sum_oldest_first(cells):
    """((cells[0] + cells[1]) + ...) + cells[L-1] along the last axis, in the cells' own arithmetic (int64 wraps)."""
    with np.errstate(invalid="ignore", over="ignore"):
        acc = cells[..., 0].copy()
        for t in range(1, cells.shape[-1]):
            acc = acc + cells[..., t]
    return acc


def sum_newest_first(cells):
    """cells[L-1] + cells[L-2] + ... + cells[0], left to right, as Z_v is defined."""
    return sum_oldest_first(cells[..., ::-1])
