"""Ground-truth evaluation: what a place-recognition front-end is judged by -- the precision-recall curve with its average
precision, the recall at 100 % precision, the best F1 and recall@K -- for any of the detectors and any score matrix.

Two protocols, as in the literature:

  cells     every offered cell of a score matrix is a decision (pr_curve_cells, at caller thresholds), and recall@K asks
            where a row's best true match stands in its ranking (recall_at).  The counting is the library's, one pass over
            the matrix next to a truth mask: dlc_pr_cell_counts and dlc_positive_rank_rows (include/dlc.h).
  queries   a detector reports one candidate per frame; sweeping the acceptance threshold over every score it gave is the
            curve (pr_curve_queries, exact at every score; LoopClosureEvaluator feeds it from a stream).

ground_truth() makes the truth mask from positions (or frame indices) and a radius.  All counts are integers; the derived
numbers come from them on the host, one formula each (PRCurve).
"""
import numpy as np
import torch

MAX_COORDINATE = 1 << 30       # |coordinate| of a position: squared distances then stay within int64 (ground_truth)
_ALL_WITHIN = 3037000500       # the smallest radius whose square is >= 2^63: beyond every squared distance there is


class PRCurve:
    """A precision-recall curve as integer counts, STRICTEST threshold first (descending thresholds, ascending with
    lower_is_better): thresholds [T], tp [T] and fp [T] int64 (what is reported at threshold i and is / is not a true
    match), positives (the true matches there are to find), and from them
        precision[i] = tp / (tp + fp), 1.0 where nothing is reported;   recall[i] = tp / positives, 0.0 if positives == 0."""

    def __init__(self, thresholds, tp, fp, positives, lower_is_better=False):
        self.thresholds = np.asarray(thresholds)
        self.tp = np.asarray(tp, dtype=np.int64)
        self.fp = np.asarray(fp, dtype=np.int64)
        if not self.thresholds.shape == self.tp.shape == self.fp.shape or self.tp.ndim != 1:
            raise ValueError("PRCurve: thresholds, tp and fp must be three vectors of one length")
        self.positives = int(positives)
        self.lower_is_better = bool(lower_is_better)
        reported = self.tp + self.fp
        self.precision = np.where(reported > 0, self.tp / np.maximum(reported, 1), 1.0)
        self.recall = self.tp / self.positives if self.positives > 0 else np.zeros(self.tp.shape)

    def __len__(self):
        return self.tp.shape[0]

    @property
    def average_precision(self):
        """sum_i (R_i - R_{i-1}) * P_i, strictest first, R_{-1} = 0."""
        return float(np.sum(np.diff(self.recall, prepend=0.0) * self.precision))

    @property
    def recall_at_full_precision(self):
        """max R_i over the thresholds with fp_i == 0 (0.0 when there is none)."""
        clean = self.fp == 0
        return float(self.recall[clean].max()) if clean.any() else 0.0

    @property
    def best_f1(self):
        """(max_i 2 tp / (2 tp + fp + positives - tp), the threshold it is reached at -- the strictest one on a tie);
        (0.0, None) for a curve without thresholds."""
        if len(self) == 0:
            return 0.0, None
        den = self.tp + self.fp + self.positives                  # = 2 tp + fp + (positives - tp)
        f1 = np.where(den > 0, 2.0 * self.tp / np.maximum(den, 1), 0.0)
        at = int(np.argmax(f1))
        return float(f1[at]), self.thresholds[at].item()

    def rows(self):
        """[(threshold, tp, fp, precision, recall)], strictest first: the lines of the CLI's --pr-curve file."""
        return [(self.thresholds[i].item(), int(self.tp[i]), int(self.fp[i]), float(self.precision[i]), float(self.recall[i]))
                for i in range(len(self))]


def _positions(p, what):
    t = p if isinstance(p, torch.Tensor) else torch.as_tensor(np.asarray(p))
    if t.is_floating_point() or t.dtype == torch.bool or t.dim() not in (1, 2) or (t.dim() == 2 and t.shape[1] != 2):
        raise ValueError("ground_truth: %s must be integers [*, 2] or [*]" % what)
    t = t.to(torch.int64)
    if t.numel() and int(t.abs().max()) > MAX_COORDINATE:
        raise ValueError("ground_truth: a coordinate of %s lies outside +-2^30" % what)
    return t


def ground_truth(query_pos, key_pos, radius):
    """uint8 [Q, N] on the positions' device: cell (q, j) is 1 iff key-frame j lies within `radius` of query q --
    dx^2 + dy^2 <= radius^2, exactly, in int64.  Positions are integers [*, 2] (x, y) or [*] (one coordinate: a frame index
    or a distance along the route; both arguments the same form), |coordinate| <= 2^30; radius an integer >= 0.  Computed
    with torch a tile of rows at a time, so it runs on CPU tensors too."""
    q, k = _positions(query_pos, "query_pos"), _positions(key_pos, "key_pos")
    if q.dim() != k.dim() or q.device != k.device:
        raise ValueError("ground_truth: query_pos and key_pos must have one form and one device")
    if int(radius) != radius or radius < 0:
        raise ValueError("ground_truth: radius=%r must be an integer >= 0" % (radius,))
    radius = int(radius)
    nq, nk = q.shape[0], k.shape[0]
    out = torch.empty((nq, nk), dtype=torch.uint8, device=q.device)
    if radius >= _ALL_WITHIN:                                     # (radius^2 no longer fits; every pair is within it)
        return out.fill_(1)
    r2 = radius * radius
    tile = max(1, (1 << 22) // max(1, nk))
    for lo in range(0, nq, tile):
        qt = q[lo:lo + tile]
        if q.dim() == 1:
            dx = qt[:, None] - k[None, :]
            near = dx * dx <= r2
        else:
            dx = qt[:, None, 0] - k[None, :, 0]
            dy = qt[:, None, 1] - k[None, :, 1]
            # |d| <= 2^31: each square fits, their sum need not -- so dx^2 against r^2 - dy^2 (never below -2^62)
            near = dx * dx <= r2 - dy * dy
        out[lo:lo + tile] = near
    return out


def _operands(scores, truth):
    from .engine import default_engine
    from .sequence import _on_device
    e = default_engine()
    scores, _ = _on_device(e, scores)
    if not isinstance(truth, torch.Tensor):
        truth = torch.as_tensor(np.ascontiguousarray(np.asarray(truth)))
    if truth.dtype not in (torch.uint8, torch.bool):
        truth = truth != 0
    return e, scores, truth.to(e.device)


def _even_thresholds(scores, count, n, limit0, limit_step, absent):
    """`count` evenly spaced values from the smallest to the largest finite offered cell of scores (integers for int64)."""
    rows = scores.shape[0]
    n = scores.shape[1] if n is None else int(n)
    lim = (n if limit0 is None else int(limit0)) + int(limit_step) * torch.arange(rows, device=scores.device)
    offered = torch.arange(n, device=scores.device)[None, :] < lim.clamp(0, n)[:, None]
    cells = scores[:, :n]
    if scores.dtype == torch.int64:
        if absent is not None:
            offered &= cells != int(absent)
    else:
        offered &= torch.isfinite(cells)
    if not bool(offered.any()):
        raise ValueError("pr_curve_cells: no finite offered cell to space %d thresholds over" % count)
    lo, hi = cells[offered].min().item(), cells[offered].max().item()
    if scores.dtype == torch.int64:
        return sorted({lo + (i * (hi - lo)) // max(1, count - 1) for i in range(count)})
    return np.linspace(float(lo), float(hi), count)


def pr_curve_cells(scores, truth, thresholds, n=None, limit0=None, limit_step=0, lower_is_better=False, absent=None):
    """The cell-level PRCurve of a score matrix [rows, >= n] (fp64, fp32 or int64; NumPy or a device tensor) against
    truth [rows, >= n] (non-zero = a true match): at threshold t every offered cell x >= t (x <= t with lower_is_better)
    is reported.  Offered: row r's first clamp(limit0 + r * limit_step, 0, n) cells (limit0 None: all), never a NaN, nor
    `absent` in int64 rows.  thresholds: up to 4096 numbers in any order (sorted and de-duplicated; a NaN is refused), or
    an int T: T evenly spaced values over the range of the finite offered cells.  positives = the offered true matches.
    One pass over the matrix on the GPU (Engine.pr_cell_counts)."""
    e, scores, truth = _operands(scores, truth)
    if isinstance(thresholds, (int, np.integer)) and not isinstance(thresholds, bool):
        if not 1 <= int(thresholds) <= 4096:
            raise ValueError("pr_curve_cells: T=%d thresholds outside 1..4096" % int(thresholds))
        thresholds = _even_thresholds(scores, int(thresholds), n, limit0, limit_step, absent)
    t = e.sorted_thresholds(thresholds, scores.dtype == torch.int64)
    pos, neg = e.pr_cell_counts(scores, truth, t, n=n, limit0=limit0, limit_step=limit_step, lower_is_better=lower_is_better,
                                absent=absent)
    pos, neg, t = pos.cpu().numpy(), neg.cpu().numpy(), t.cpu().numpy()
    if lower_is_better:       # x <= t_i  <=>  bin <= i: running sums from the lowest bin; ascending thresholds are strictest first
        tp, fp = np.cumsum(pos)[:-1], np.cumsum(neg)[:-1]
    else:                     # x >= t_i  <=>  bin > i: running sums from the highest bin; the strictest threshold is the last
        tp, fp = np.cumsum(pos[::-1])[:-1], np.cumsum(neg[::-1])[:-1]
        t = t[::-1]
    return PRCurve(t, tp, fp, int(pos.sum()), lower_is_better)


def recall_at(scores, truth, ks=(1, 5, 10, 20), n=None, limit0=None, limit_step=0, lower_is_better=False, absent=None):
    """({K: recall@K}, rank): recall@K = #{rows whose best true match is among the row's K best offered cells} /
    #{rows that offer a true match} (0.0 when no row does); rank [rows] int64 on the device is the slot of that best true
    match in the row's ranking, -1 for a row without one (Engine.positive_rank_rows).  Operands as in pr_curve_cells."""
    e, scores, truth = _operands(scores, truth)
    rank, _, npos = e.positive_rank_rows(scores, truth, n=n, limit0=limit0, limit_step=limit_step,
                                         lower_is_better=lower_is_better, absent=absent)
    have = int((npos > 0).sum())
    return {int(k): (int(((rank >= 0) & (rank < int(k))).sum()) / have if have else 0.0) for k in ks}, rank


def pr_curve_queries(scores, ids, hit, has_positive, lower_is_better=False):
    """The detector protocol on one candidate per query: scores [Q], ids [Q] (>= 0: a candidate was reported), hit [Q]
    (the candidate is a true match), has_positive [Q] (the query has a true match to find).  The thresholds are every
    distinct score of a row with id >= 0 (a NaN score is no candidate), strictest first; at threshold t a row with
    id >= 0 passes when score >= t (score <= t with lower_is_better); tp counts the passing rows with hit, fp those
    without; positives = #{has_positive}.  Exact at every score; host NumPy."""
    s, i = np.asarray(scores), np.asarray(ids)
    hit, has_positive = np.asarray(hit).astype(bool), np.asarray(has_positive).astype(bool)
    if not s.shape == i.shape == hit.shape == has_positive.shape or s.ndim != 1:
        raise ValueError("pr_curve_queries: scores, ids, hit and has_positive must be four vectors of one length")
    there = i >= 0
    if s.dtype.kind == "f":
        there &= ~np.isnan(s)
    t = np.unique(s[there])                                       # ascending, distinct
    order = np.argsort(s[there], kind="stable")
    ss, hh = s[there][order], hit[there][order]
    chit = np.concatenate([[0], np.cumsum(hh)])                   # hits among the i lowest scores
    if lower_is_better:
        upto = np.searchsorted(ss, t, side="right")               # rows with score <= t
        tp, fp = chit[upto], upto - chit[upto]
    else:
        t = t[::-1]
        frm = np.searchsorted(ss, t, side="left")                 # rows with score >= t: those from here on
        tp = chit[-1] - chit[frm]
        fp = (len(ss) - frm) - tp
    return PRCurve(t, tp, fp, int(has_positive.sum()), lower_is_better)


class LoopClosureEvaluator:
    """Ground-truth evaluation of a streaming detector -- any of the five: LoopClosureDetector (with or without
    sequence=L), SdavLoopClosureDetector, CnnVtlLoopClosureDetector, SeqSlamLoopClosureDetector, LdbLoopClosureDetector.

    positions: the position of every frame of the run, integers [F, 2] or [F] (ground_truth); radius: how near a key-frame
    must lie to be the same place; exclusion: the detector's; lower_is_better: True for the distance, SAD and Hamming detectors.
    add(scores, ids, first_id) takes what query_and_insert returned for the frames first_id .. first_id + B - 1.  For
    frame t:  has_positive = some key-frame j < t - exclusion is within the radius;  hit = the candidate at slot 0 is
    within the radius and j < t - exclusion;  any_hit = the same of any of the k candidates.  result() -> (PRCurve of
    pr_curve_queries over slot 0, candidates_recall = #{any_hit} / #{has_positive}, 0.0 when no frame has one)."""

    def __init__(self, positions, radius, exclusion, lower_is_better=False):
        self.positions = _positions(positions, "positions").cpu()
        if int(radius) != radius or radius < 0:
            raise ValueError("LoopClosureEvaluator: radius=%r must be an integer >= 0" % (radius,))
        if exclusion < 0:
            raise ValueError("LoopClosureEvaluator: exclusion must be >= 0")
        self.radius, self.exclusion, self.lower_is_better = int(radius), int(exclusion), bool(lower_is_better)
        self._scores, self._ids, self._hit, self._any, self._has = [], [], [], [], []

    @property
    def queries(self):
        return sum(len(i) for i in self._ids)

    def add(self, scores, ids, first_id):
        s = scores.cpu().numpy() if isinstance(scores, torch.Tensor) else np.asarray(scores)
        i = ids.cpu().numpy() if isinstance(ids, torch.Tensor) else np.asarray(ids)
        if s.ndim != 2 or s.shape != i.shape or s.shape[1] < 1:
            raise ValueError("LoopClosureEvaluator.add: scores and ids must be [B, k >= 1]")
        b, frames = s.shape[0], self.positions.shape[0]
        if first_id < 0 or first_id + b > frames or i.max(initial=-1) >= frames:
            raise ValueError("LoopClosureEvaluator.add: frames %d..%d or a candidate lie outside the %d positions"
                             % (first_id, first_id + b - 1, frames))
        near = ground_truth(self.positions[first_id:first_id + b], self.positions, self.radius).numpy().astype(bool)
        older = np.arange(frames)[None, :] < (first_id + np.arange(b) - self.exclusion)[:, None]
        match = near & older
        at = np.where(i >= 0, i, 0)
        hits = (i >= 0) & np.take_along_axis(match, at, axis=1)
        self._scores.append(s[:, 0])
        self._ids.append(i[:, 0])
        self._hit.append(hits[:, 0])
        self._any.append(hits.any(axis=1))
        self._has.append(match.any(axis=1))

    def result(self):
        if not self._ids:
            return PRCurve([], [], [], 0, self.lower_is_better), 0.0
        has = np.concatenate(self._has)
        curve = pr_curve_queries(np.concatenate(self._scores), np.concatenate(self._ids), np.concatenate(self._hit), has,
                                 self.lower_is_better)
        return curve, (int(np.concatenate(self._any).sum()) / int(has.sum()) if has.any() else 0.0)


def read_positions(path):
    """int64 [F] or [F, 2] from a text file: one line per frame, one or two integers on each (the same number on all)."""
    with open(path) as f:
        lines = [ln.split() for ln in f.read().splitlines() if ln.strip()]
    if not lines or len(lines[0]) not in (1, 2) or any(len(ln) != len(lines[0]) for ln in lines):
        raise ValueError("%s: every line must hold one or two integers, the same number on all" % path)
    try:
        p = np.array([[int(v) for v in ln] for ln in lines], dtype=np.int64)
    except (ValueError, OverflowError):
        raise ValueError("%s: every line must hold one or two integers" % path)
    if np.abs(p).max() > MAX_COORDINATE:
        raise ValueError("%s: a coordinate lies outside +-2^30" % path)
    return p[:, 0] if p.shape[1] == 1 else p


def pr_line(queries, curve):
    """The CLI's summary line: `pr`, then tab-separated names and values -- queries, loops (the frames with a true match
    to find), ap, recall_at_p1, best_f1 and the threshold it is reached at (`-` for a curve without thresholds)."""
    f1, at = curve.best_f1
    at = "-" if at is None else ("%d" % at if isinstance(at, int) else "%.6g" % at)
    return "pr\tqueries\t%d\tloops\t%d\tap\t%.6f\trecall_at_p1\t%.6f\tbest_f1\t%.6f\tthreshold\t%s" % (
        queries, curve.positives, curve.average_precision, curve.recall_at_full_precision, f1, at)
