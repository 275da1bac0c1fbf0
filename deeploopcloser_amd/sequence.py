"""Sequence-consistent loop search over a score matrix (the trajectory search of SeqSLAM, Milford & Wyeth, ICRA 2012; not
in the reference): a pair (query frame t, key-frame j) is scored by the sum of the frame scores along a short line through
(t, j) of the matrix, the best of a few slopes, and the k best pairs of every query frame are the candidates
(dlc_sequence_topk, include/dlc.h: the definition, the order of the additions and the tie rules).  A single-frame nearest
neighbour is fooled by a place that merely looks alike; a run of L frames that all look alike in order is not.

The matrices are the reference's as they come: SimilarityCalculator.similarity_matrix (int64 or fp64, higher is better)
and DistanceCalculator.distance_matrix (int64, lower_is_better=True).  NumPy in -> NumPy out, device tensors in -> device
tensors out.

Elastic search.  A straight line is a revisit at one speed.  steps = (d_min, d_max) on sequence_topk, sequence_scores and
sequence_peaks replaces the lines by chains: from frame to frame the chain steps back any d_min .. d_max key-frames (a
stop, a slow corner, unevenly spaced key-frames), the best chain found by dynamic programming, one addition per cell and
level, oldest row first (dlc_sequence_elastic_topk, include/dlc.h: the recursion is the definition; the lowest step wins
ties).  In place of the winning slope the lists carry the chain's span, the key-frames it covers.  contrast runs in front
of it and suppress behind it as with the lines; steps=None is every path as it was.

Chains.  A candidate's score is a sum over L frames; sequence_chains (and chains=True on sequence_topk / sequence_peaks)
returns the alignment behind it: for each of the L frames, oldest first, the column it was matched to, and on request
the matrix cells along them (dlc_sequence_elastic_chains / dlc_sequence_chains, include/dlc.h) -- L frame-to-key-frame
pairs per loop closure, the weakest frame's score, per-frame correspondences.  With steps it is the chain the recursion
chose, otherwise the winning line.

Distinct places.  The k best cells of a row are mostly ONE place: a revisit of key-frame j scores almost as well against
j - 1, j + 1, ...  peak_topk / sequence_peaks pick the best cell, then the best one more than `suppress` key-frames from
it, and so on (dlc_peak_topk_rows, include/dlc.h) -- SeqSLAM's "best trajectory, then the best one outside a window
around it" -- and uniqueness_ratio is the quotient of the first two.

contrast = R (None: off) first scores every cell against its neighbourhood within its row, (x - local mean) / local std
over the R key-frames on either side -- SeqSLAM's local contrast normalisation (III-B of the paper; dlc_contrast_rows,
include/dlc.h) -- so that a stretch of key-frames that resembles everything goes flat before the lines are summed.
"""
import numpy as np
import torch

from ._lib import DLC_MAX_K
from .engine import check_steps, default_engine


def slope_offsets(L, v_min=0.8, v_max=1.2, v_step=0.1):
    """int32 [V, L] column offsets of the lines searched: row i is floor(v_i * s + 0.5), s = 0 .. L-1, for the velocities
    v_i = v_min + i * v_step up to v_max -- how many key-frames the line steps back while the query steps back s frames.
    Duplicate rows are dropped (the first is kept).  Host NumPy."""
    L = int(L)
    if L < 1:
        raise ValueError("slope_offsets: L must be >= 1")
    if v_step <= 0 or v_min < 0 or v_max < v_min:
        raise ValueError("slope_offsets: need 0 <= v_min <= v_max and v_step > 0")
    count = int(np.floor((v_max - v_min) / v_step + 1e-9)) + 1
    s = np.arange(L, dtype=np.float64)
    rows, seen = [], set()
    for i in range(count):
        row = np.floor((v_min + i * v_step) * s + 0.5).astype(np.int32)
        if row.tobytes() not in seen:
            seen.add(row.tobytes())
            rows.append(row)
    return np.stack(rows)


def _on_device(e, matrix):
    """(the matrix as a device tensor of a type the kernels take, whether it came as NumPy)"""
    as_numpy = not isinstance(matrix, torch.Tensor)
    if as_numpy:
        a = np.asarray(matrix)
        if a.dtype not in (np.float64, np.float32, np.int64):
            a = a.astype(np.int64 if np.issubdtype(a.dtype, np.integer) else np.float64)
        matrix = e.to_device(a)
    if matrix.dim() != 2:
        raise ValueError("sequence search: the score matrix must be [rows, n]")
    return matrix, as_numpy


def contrast_normalize(matrix, radius, limit0=None, limit_step=0):
    """fp64 [rows, n]: SeqSLAM's local contrast normalisation of matrix [rows, n] (fp64, fp32 or int64), every cell
    (x - mean) / sample std over the cells within `radius` (1..32) of it in its row, clipped to the row's first
    clamp(limit0 + r * limit_step, 0, n) cells (limit0 None: all); 0.0 where that window holds fewer than two cells or is
    constant (dlc_contrast_rows, include/dlc.h: the order of the additions, bit for bit).  Cells that are not offered are
    NaN.  The order of merit is kept: what was lower-is-better still is."""
    e = default_engine()
    matrix, as_numpy = _on_device(e, matrix)
    out = torch.full(tuple(matrix.shape), float("nan"), dtype=torch.float64, device=e.device)
    if matrix.shape[0] and matrix.shape[1]:
        e.contrast_rows(matrix, radius, limit0=limit0, limit_step=limit_step, out=out)
    elif not 1 <= int(radius) <= 32:
        raise ValueError("contrast_normalize: radius=%d outside 1..32" % int(radius))
    return out.cpu().numpy() if as_numpy else out


def _search(e, matrix, L, offsets, k, dense, limit0, limit_step, lower_is_better, contrast, poison=None, steps=None):
    """Engine.sequence_topk -- with steps, Engine.sequence_elastic_topk -- of a device matrix behind the optional contrast
    normalisation: device tensors."""
    if steps is not None:
        if offsets is not None:
            raise ValueError("sequence search: steps and offsets exclude each other")
        steps = check_steps(steps)
    if contrast is not None:
        matrix = contrast_normalize(matrix, contrast, limit0, limit_step)
    if steps is not None:
        return e.sequence_elastic_topk(matrix, L, steps, k=k, limit0=limit0, limit_step=limit_step,
                                       lower_is_better=lower_is_better, dense=dense, poison=poison)
    offsets = slope_offsets(L) if offsets is None else offsets
    return e.sequence_topk(matrix, L, offsets, k=k, limit0=limit0, limit_step=limit_step, lower_is_better=lower_is_better,
                           dense=dense, poison=poison)


def _run(matrix, L, offsets, k, dense, limit0, limit_step, lower_is_better, contrast=None, steps=None):
    e = default_engine()
    matrix, as_numpy = _on_device(e, matrix)
    out = _search(e, matrix, L, offsets, k, dense, limit0, limit_step, lower_is_better, contrast, steps=steps)
    return tuple(None if t is None else (t.cpu().numpy() if as_numpy else t) for t in out)


def _chains(e, matrix, idx, L, offsets, steps, limit0, limit_step, lower_is_better, cells):
    """(chain, cells or None) of a device matrix that the search saw (behind the contrast front already) and a device idx."""
    if steps is not None:
        if offsets is not None:
            raise ValueError("sequence search: steps and offsets exclude each other")
        return e.sequence_elastic_chains(matrix, L, check_steps(steps), idx, limit0=limit0, limit_step=limit_step,
                                         lower_is_better=lower_is_better, cells=cells)
    return e.sequence_chains(matrix, L, slope_offsets(L) if offsets is None else offsets, idx, limit0=limit0,
                             limit_step=limit_step, lower_is_better=lower_is_better, cells=cells)[:2]


def sequence_chains(matrix, idx, L, offsets=None, steps=None, limit0=None, limit_step=0, lower_is_better=False, contrast=None,
                    cells=False):
    """chain int32 [rows, k, L] -- with cells=True (chain, cells [rows, k, L]) -- of the candidates idx [rows, k] (int64
    end columns from sequence_topk or sequence_peaks with the same L, offsets or steps, limits, order and contrast; -1: an
    empty slot): the column each of the L frames of the candidate's chain was matched to, oldest frame first, chain[...,
    L-1] = idx.  With steps the chain the elastic recursion chose (its cells summed oldest first are the candidate's score
    bit for bit), otherwise the winning line (summed newest first).  A slot that is no candidate of its row holds -1, and
    NaN / -1 in cells.  contrast = R: of contrast_normalize(matrix, R, limit0, limit_step), the matrix the search saw."""
    e = default_engine()
    matrix, as_numpy = _on_device(e, matrix)
    idx = e.to_device(np.ascontiguousarray(idx, dtype=np.int64)) if not isinstance(idx, torch.Tensor) else idx
    if contrast is not None:
        matrix = contrast_normalize(matrix, contrast, limit0, limit_step)
    out = _chains(e, matrix, idx, L, offsets, steps, limit0, limit_step, lower_is_better, cells)
    out = tuple(t.cpu().numpy() if as_numpy else t for t in out if t is not None)
    return out if cells else out[0]


def sequence_topk(matrix, k, L, offsets=None, limit0=None, limit_step=0, lower_is_better=False, contrast=None, steps=None,
                  chains=False):
    """(scores [rows, k], idx [rows, k] int64, slope [rows, k] int32): per row r of matrix [rows, n] the k best cells by the
    sequence score over L rows, among the row's first clamp(limit0 + r * limit_step, 0, n) columns (limit0 None: all),
    best first, ties -> the lower column.  offsets: an int32 table [V, L] (default slope_offsets(L)); slope: the row of it
    that won.  Empty slots: (-inf or +inf, -1, -1) in fp64, (-1, -1, -1) for int64 matrices; the first L - 1 rows are empty.
    contrast = R: the search runs on contrast_normalize(matrix, R, limit0, limit_step); scores are then fp64 for int64
    matrices too.
    steps = (d_min, d_max) (None: the lines above; with offsets: ValueError): the ELASTIC search -- the best chain of L
    cells that ends in (r, j) and steps back d_min .. d_max columns per row (dlc_sequence_elastic_topk); the third
    result is then span [rows, k] int32, the columns the chosen chain covers.
    chains=True: a fourth result, chain [rows, k, L] int32 -- the column each of the L frames of a candidate was matched
    to, oldest first (sequence_chains)."""
    if not chains:
        return _run(matrix, L, offsets, int(k), False, limit0, limit_step, lower_is_better, contrast, steps)[:3]
    e = default_engine()
    matrix, as_numpy = _on_device(e, matrix)
    if contrast is not None:
        matrix = contrast_normalize(matrix, contrast, limit0, limit_step)
    out = _search(e, matrix, L, offsets, int(k), False, limit0, limit_step, lower_is_better, None, steps=steps)[:3]
    out += (_chains(e, matrix, out[1], L, offsets, steps, limit0, limit_step, lower_is_better, False)[0],)
    return tuple(t.cpu().numpy() if as_numpy else t for t in out)


def sequence_scores(matrix, L, offsets=None, limit0=None, limit_step=0, lower_is_better=False, contrast=None, steps=None):
    """The dense [rows, n] sequence scores themselves (fp64, or int64 for int64 matrices): NaN / -1 where a cell has no
    valid line.  contrast = R: of contrast_normalize(matrix, R, limit0, limit_step), fp64.  steps = (d_min, d_max): the
    elastic search's (no valid chain), as in sequence_topk."""
    return _run(matrix, L, offsets, None, True, limit0, limit_step, lower_is_better, contrast, steps)[3]


def _peaks(e, matrix, k, suppress, limit0, limit_step, lower_is_better, absent):
    """Engine.peak_topk_rows of a device matrix; a matrix without rows or columns gives the empty lists."""
    if matrix.shape[0] and matrix.shape[1]:
        return e.peak_topk_rows(matrix, k, suppress, limit0=limit0, limit_step=limit_step, lower_is_better=lower_is_better,
                                absent=absent)
    if not 1 <= int(k) <= DLC_MAX_K or int(suppress) < 0:
        raise ValueError("peak_topk: k=%d outside 1..%d or suppress=%d negative" % (int(k), DLC_MAX_K, int(suppress)))
    is_int = matrix.dtype == torch.int64
    fill = -1 if is_int else float("inf" if lower_is_better else "-inf")
    shape = (matrix.shape[0], int(k))
    return (torch.full(shape, fill, dtype=torch.int64 if is_int else torch.float64, device=e.device),
            torch.full(shape, -1, dtype=torch.int64, device=e.device))


def peak_topk(matrix, k, suppress, limit0=None, limit_step=0, lower_is_better=False, absent=None):
    """(scores [rows, k], idx [rows, k] int64): distinct-place candidates of any score matrix [rows, n] (fp64, fp32 or
    int64).  Per row the best cell among its first clamp(limit0 + r * limit_step, 0, n) columns (limit0 None: all), then
    the best one more than `suppress` columns from it, then the best one more than `suppress` from both, ...: k picks,
    best first, ties -> the lower column (dlc_peak_topk_rows, include/dlc.h).  A NaN is never picked; absent: for int64
    matrices, a value that marks a cell as not there.  Scores are fp64 (int64 for int64 matrices); empty slots are
    (-inf or +inf, -1), or (-1, -1) for int64.  suppress = 0 is the plain top-k."""
    e = default_engine()
    matrix, as_numpy = _on_device(e, matrix)
    out = _peaks(e, matrix, k, suppress, limit0, limit_step, lower_is_better, absent)
    return tuple(t.cpu().numpy() if as_numpy else t for t in out)


def sequence_peaks(matrix, k, L, suppress, offsets=None, limit0=None, limit_step=0, lower_is_better=False, contrast=None,
                   steps=None, chains=False):
    """(scores [rows, k], idx [rows, k] int64): the distinct-place candidates by the sequence score -- sequence_scores
    (same L, offsets or steps, limits and contrast), then peak_topk over those dense scores with the same limits: the best
    trajectory, then the best one whose end lies more than `suppress` key-frames from it, ...  With k = 2,
    lower_is_better and suppress = R_window / 2 the two slots are OpenSeqSLAM's min_value and min_value_2nd
    (uniqueness_ratio).  int64 matrices: the dense scores mark "no valid line" with -1, which is passed on as the absent
    value, so a genuine sequence sum of -1 is not offered either -- the convention (and the collision) of
    dlc_sequence_topk's int64 seq_out.
    chains=True: a third result, chain [rows, k, L] int32, the picks' chains over the same input (sequence_chains)."""
    e = default_engine()
    matrix, as_numpy = _on_device(e, matrix)
    if contrast is not None:
        matrix = contrast_normalize(matrix, contrast, limit0, limit_step)
    dense = _search(e, matrix, L, offsets, None, True, limit0, limit_step, lower_is_better, None, steps=steps)[3]
    out = _peaks(e, dense, k, suppress, limit0, limit_step, lower_is_better, -1 if dense.dtype == torch.int64 else None)
    if chains:
        out += (_chains(e, matrix, out[1], L, offsets, steps, limit0, limit_step, lower_is_better, False)[0],)
    return tuple(t.cpu().numpy() if as_numpy else t for t in out)


def uniqueness_ratio(scores):
    """float64 [rows]: scores[:, 0] / scores[:, 1] of lists with k >= 2 from peak_topk / sequence_peaks -- SeqSLAM's
    uniqueness ratio, the best score over the best score outside the window around it.  It is meaningful for positive
    lower-is-better scores (sums of distances): near 0 for a match that stands alone, near 1 for one that does not.  NaN
    where slot 1 is empty (an infinity, or -1 in int64 lists).  NumPy in -> NumPy out, tensors in -> tensors out."""
    as_numpy = not isinstance(scores, torch.Tensor)
    s = torch.as_tensor(np.asarray(scores)) if as_numpy else scores
    if s.dim() != 2 or s.shape[1] < 2:
        raise ValueError("uniqueness_ratio: scores must be [rows, k >= 2]")
    empty = (s[:, 1] == -1) if not s.dtype.is_floating_point else torch.isinf(s[:, 1])
    ratio = s[:, 0].to(torch.float64) / s[:, 1].to(torch.float64)
    ratio = torch.where(empty, torch.full_like(ratio, float("nan")), ratio)
    return ratio.numpy() if as_numpy else ratio
