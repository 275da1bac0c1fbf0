"""NumPy restatement of the windowed peak top-k defined in include/dlc.h (dlc_peak_topk_rows), so that every comparison
against the GPU is exact.

Row r offers the cells j < lim(r) = clamp(limit0 + r * limit_step, 0, n) that are present (not NaN; not the `absent`
value of an int64 row).  The offered cells are sorted by (merit, column) -- the order of dlc_topk_rows_f64 and
dlc_sequence_topk: by the number, -0.0 below +0.0, descending (ascending with lower_is_better), ties -> the lower column
-- and taken greedily: a cell is a pick when it lies more than `suppress` columns from every pick before it.
"""
import numpy as np

from sequence_oracle import limits, merit_keys


def best_first(values, cols, lower_is_better):
    """cols, sorted by the merit of values (one per column of cols), best first, ties -> the lower column."""
    worse = ~merit_keys(values, lower_is_better)                   # ascending = best first
    return cols[np.lexsort((cols, worse))]


def offered_columns(row, lim, absent=None):
    """The columns row offers among its first lim."""
    cols = np.arange(lim)
    if row.dtype == np.int64:
        return cols if absent is None else cols[row[:lim] != absent]
    return cols[~np.isnan(row[:lim])]


def peak_topk_rows(matrix, k, suppress, n=None, limit0=None, limit_step=0, lower_is_better=False, absent=None):
    """(scores [rows, k], idx [rows, k] int64): fp64 scores (int64 for int64 input); empty slots hold index -1 and the
    score -inf (+inf when lower is better), or -1 for int64 input."""
    m = np.asarray(matrix)
    is_int = m.dtype == np.int64
    if not is_int:
        m = m.astype(np.float64)                                   # fp32 -> fp64 is exact
    rows = m.shape[0]
    n = m.shape[1] if n is None else n
    lim = limits(rows, n, n if limit0 is None else limit0, limit_step)
    out_s = np.full((rows, k), -1 if is_int else (np.inf if lower_is_better else -np.inf), m.dtype)
    out_i = np.full((rows, k), -1, np.int64)
    for r in range(rows):
        cols = offered_columns(m[r], int(lim[r]), absent)
        order = best_first(m[r, cols], cols, lower_is_better)
        alive = np.ones(order.size, bool)                          # sorted cells no pick has suppressed yet
        for t in range(k):
            if not alive.any():
                break
            j = int(order[np.argmax(alive)])                       # the first of them: the next pick
            out_s[r, t], out_i[r, t] = m[r, j], j
            alive &= np.abs(order - j) > suppress
    return out_s, out_i


def hand_worked_row(reach_b=6):
    """fp64 [400], all cells 0.5; cells 100 +- d are 10 - d for d <= 6 and cells 300 +- d are 8 - d for d <= reach_b: two
    places of different strength, each with its shoulders."""
    row = np.full(400, 0.5)
    for d in range(7):
        row[100 - d] = row[100 + d] = 10.0 - d
    for d in range(reach_b + 1):
        row[300 - d] = row[300 + d] = 8.0 - d
    return row


def two_place_scene(seed, draw, units, frames=120, first=90, place_a=20, place_b=55, share_a=0.65, redrawn=0.3):
    """A route whose frames first .. frames - 1 revisit TWO places at once, one strongly and one weakly -- the hand-worked
    row's two peaks with their shoulders, as descriptors.  A frame is `units` units (bytes, columns, patches) drawn by
    draw(rng, count) -> [count, ...]; every frame copies the one before it and redraws a random `redrawn` of its units, so
    a frame resembles its neighbours less and less with their distance (the shoulders).  Revisiting frame first + i takes
    a fixed share_a of its units from frame place_a + i and the others from frame place_b + i.
    Returns descriptors [frames, units, ...]."""
    rng = np.random.RandomState(seed)
    x = [draw(rng, units)]
    for _ in range(1, first):
        nxt = x[-1].copy()
        at = rng.permutation(units)[:int(round(redrawn * units))]
        nxt[at] = draw(rng, at.size)
        x.append(nxt)
    from_a = rng.permutation(units)[:int(round(share_a * units))]
    for i in range(frames - first):
        nxt = x[place_b + i].copy()
        nxt[from_a] = x[place_a + i][from_a]
        x.append(nxt)
    return np.stack(x)
