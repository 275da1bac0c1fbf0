"""NumPy restatement of the ground-truth evaluation defined in include/dlc.h (dlc_pr_cell_counts, dlc_positive_rank_rows)
and of the formulas of deeploopcloser_amd/evaluate.py, so that every comparison against the GPU is exact.  Written from
the header's text, one definition at a time; test_evaluate_cpu.py pins it against brute-force loops.

Row r offers the cells j < lim(r) = clamp(limit0 + r * limit_step, 0, n) that are present (not NaN; not the `absent`
value of an int64 row).  The order is the order of the numbers with -0.0 below +0.0: `order_keys` maps a value to a
uint64 whose unsigned order is that order.
"""
import numpy as np

SIGN = np.uint64(1 << 63)


def order_keys(values):
    """uint64 keys, ascending as the numbers are (fp32 / fp64: through fp64, -0.0 below +0.0; int64: biased)."""
    v = np.ascontiguousarray(values)
    if v.dtype == np.int64:
        return v.view(np.uint64) ^ SIGN
    u = v.astype(np.float64).view(np.uint64)
    return np.where(u >> np.uint64(63) != 0, ~u, u | SIGN)


def limits(rows, n, limit0, limit_step):
    return np.clip((n if limit0 is None else limit0) + np.arange(rows, dtype=np.int64) * limit_step, 0, n)


def offered_mask(m, n, limit0, limit_step, absent):
    """bool [rows, n]: the cells the rows offer."""
    lim = limits(m.shape[0], n, limit0, limit_step)
    off = np.arange(n)[None, :] < lim[:, None]
    if m.dtype == np.int64:
        return off if absent is None else off & (m[:, :n] != absent)
    return off & ~np.isnan(m[:, :n])


def sort_thresholds(thresholds, is_int):
    """The table the Python wrapper hands over: ascending and distinct BY KEY (so -0.0 and +0.0 are two thresholds)."""
    t = np.asarray(thresholds, dtype=np.int64 if is_int else np.float64).reshape(-1)
    keys, first = np.unique(order_keys(t), return_index=True)
    return t[first]


def pr_cell_counts(matrix, truth, thresholds, n=None, limit0=None, limit_step=0, lower_is_better=False, absent=None):
    """(pos [T + 1], neg [T + 1]) int64 for an ASCENDING table: the bin of x is #{i : t_i <= x} (#{i : t_i < x} when lower
    is better), by key."""
    m = np.asarray(matrix)
    n = m.shape[1] if n is None else n
    t = np.asarray(thresholds, dtype=np.int64 if m.dtype == np.int64 else np.float64)
    off = offered_mask(m, n, limit0, limit_step, absent)
    bins = np.searchsorted(order_keys(t), order_keys(m[:, :n]), side="left" if lower_is_better else "right")
    positive = np.asarray(truth)[:, :n] != 0
    size = t.size + 1
    return (np.bincount(bins[off & positive], minlength=size).astype(np.int64),
            np.bincount(bins[off & ~positive], minlength=size).astype(np.int64))


def positive_rank_rows(matrix, truth, n=None, limit0=None, limit_step=0, lower_is_better=False, absent=None):
    """(rank [rows], idx [rows], npos [rows]) int64; a row without an offered positive: (-1, -1, 0)."""
    m = np.asarray(matrix)
    n = m.shape[1] if n is None else n
    off = offered_mask(m, n, limit0, limit_step, absent)
    positive = np.asarray(truth)[:, :n] != 0
    rank, idx, npos = (np.full(m.shape[0], v, np.int64) for v in (-1, -1, 0))
    for r in range(m.shape[0]):
        cols = np.flatnonzero(off[r])
        keys = order_keys(m[r, cols])
        merit = ~keys if lower_is_better else keys                 # larger = better
        pcols = positive[r, cols]
        npos[r] = pcols.sum()
        if npos[r] == 0:
            continue
        best = merit[pcols].max()
        p = cols[pcols & (merit == best)][0]                       # ties -> the lower column
        idx[r] = p
        rank[r] = np.sum((merit > best) | ((merit == best) & (cols < p)))
    return rank, idx, npos


# ---- the derived numbers --------------------------------------------------------------------------------------------------
def curve_from_counts(pos, neg, thresholds, lower_is_better):
    """(thresholds, tp, fp, positives), strictest threshold first: at t_i the cells x >= t_i (bin > i), or with
    lower_is_better x <= t_i (bin <= i), are reported."""
    t = np.asarray(thresholds)
    tp = np.array([pos[:i + 1].sum() if lower_is_better else pos[i + 1:].sum() for i in range(t.size)], np.int64)
    fp = np.array([neg[:i + 1].sum() if lower_is_better else neg[i + 1:].sum() for i in range(t.size)], np.int64)
    if not lower_is_better:
        t, tp, fp = t[::-1], tp[::-1], fp[::-1]
    return t, tp, fp, int(pos.sum())


def precision_recall(tp, fp, positives):
    precision = np.array([a / (a + b) if a + b else 1.0 for a, b in zip(tp.tolist(), fp.tolist())], np.float64)
    recall = np.array([a / positives if positives else 0.0 for a in tp.tolist()], np.float64)
    return precision, recall


def average_precision(tp, fp, positives):
    """sum_i (R_i - R_{i-1}) * P_i, strictest first, R_{-1} = 0 (the terms formed one by one, then summed by NumPy)."""
    p, r = precision_recall(tp, fp, positives)
    terms, before = [], 0.0
    for pi, ri in zip(p, r):
        terms.append((ri - before) * pi)
        before = ri
    return float(np.sum(np.array(terms, np.float64)))


def recall_at_full_precision(tp, fp, positives):
    _, r = precision_recall(tp, fp, positives)
    return float(max([ri for ri, b in zip(r, fp.tolist()) if b == 0], default=0.0))


def best_f1(tp, fp, positives, thresholds):
    """(the largest 2 tp / (2 tp + fp + positives - tp), its threshold -- the strictest on a tie); (0.0, None) without any."""
    best, at = 0.0, None
    for a, b, t in zip(tp.tolist(), fp.tolist(), np.asarray(thresholds).tolist()):
        den = 2 * a + b + positives - a
        f = 2 * a / den if den else 0.0
        if at is None or f > best:
            best, at = f, t
    return best, at


def queries_curve(scores, ids, hit, has_positive, lower_is_better):
    """(thresholds, tp, fp, positives) of the detector protocol: every distinct score of a row with id >= 0, strictest
    first; a row passes when score >= t (<= t when lower is better)."""
    s, i = np.asarray(scores), np.asarray(ids)
    rows = [r for r in range(s.size) if i[r] >= 0 and s[r] == s[r]]
    t = sorted({s[r].item() for r in rows}, reverse=not lower_is_better)
    tp, fp = [], []
    for v in t:
        passing = [r for r in rows if (s[r] <= v if lower_is_better else s[r] >= v)]
        tp.append(sum(1 for r in passing if hit[r]))
        fp.append(sum(1 for r in passing if not hit[r]))
    return np.array(t, s.dtype), np.array(tp, np.int64), np.array(fp, np.int64), int(np.sum(np.asarray(has_positive) != 0))


def within(a, b, radius):
    """Python integers: is position b within radius of position a (positions: an int or a pair)?"""
    a, b = np.atleast_1d(a).tolist(), np.atleast_1d(b).tolist()
    return sum((int(x) - int(y)) ** 2 for x, y in zip(a, b)) <= int(radius) ** 2


def detector_flags(positions, radius, exclusion, first_id, ids):
    """(hit, any_hit, has_positive) per row of ids [B, k] for the frames first_id .. first_id + B - 1."""
    ids = np.asarray(ids)
    hit, any_hit, has = [], [], []
    for r in range(ids.shape[0]):
        t = first_id + r
        good = [c >= 0 and c < t - exclusion and within(positions[t], positions[c], radius) for c in ids[r].tolist()]
        hit.append(good[0])
        any_hit.append(any(good))
        has.append(any(within(positions[t], positions[j], radius) for j in range(max(0, t - exclusion))))
    return np.array(hit), np.array(any_hit), np.array(has)


def pr_line(queries, tp, fp, positives, thresholds):
    f1, at = best_f1(tp, fp, positives, thresholds)
    at = "-" if at is None else ("%d" % at if isinstance(at, int) else "%.6g" % at)
    return "pr\tqueries\t%d\tloops\t%d\tap\t%.6f\trecall_at_p1\t%.6f\tbest_f1\t%.6f\tthreshold\t%s" % (
        queries, positives, average_precision(tp, fp, positives), recall_at_full_precision(tp, fp, positives), f1, at)
