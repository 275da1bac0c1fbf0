"""Sequence-consistent loop search over a score matrix (the trajectory search of SeqSLAM, Milford & Wyeth, ICRA 2012; not
in the reference): a pair (query frame t, key-frame j) is scored by the sum of the frame scores along a short line through
(t, j) of the matrix, the best of a few slopes, and the k best pairs of every query frame are the candidates
(dlc_sequence_topk, include/dlc.h: the definition, the order of the additions and the tie rules).  A single-frame nearest
neighbour is fooled by a place that merely looks alike; a run of L frames that all look alike in order is not.

The matrices are the reference's as they come: SimilarityCalculator.similarity_matrix (int64 or fp64, higher is better)
and DistanceCalculator.distance_matrix (int64, lower_is_better=True).  NumPy in -> NumPy out, device tensors in -> device
tensors out.

contrast = R (None: off) first scores every cell against its neighbourhood within its row, (x - local mean) / local std
over the R key-frames on either side -- SeqSLAM's local contrast normalisation (III-B of the paper; dlc_contrast_rows,
include/dlc.h) -- so that a stretch of key-frames that resembles everything goes flat before the lines are summed.
"""
import numpy as np
import torch

from .engine import default_engine


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


def _run(matrix, L, offsets, k, dense, limit0, limit_step, lower_is_better, contrast=None):
    e = default_engine()
    matrix, as_numpy = _on_device(e, matrix)
    if contrast is not None:
        matrix = contrast_normalize(matrix, contrast, limit0, limit_step)
    offsets = slope_offsets(L) if offsets is None else offsets
    out = e.sequence_topk(matrix, L, offsets, k=k, limit0=limit0, limit_step=limit_step, lower_is_better=lower_is_better,
                          dense=dense)
    return tuple(None if t is None else (t.cpu().numpy() if as_numpy else t) for t in out)


def sequence_topk(matrix, k, L, offsets=None, limit0=None, limit_step=0, lower_is_better=False, contrast=None):
    """(scores [rows, k], idx [rows, k] int64, slope [rows, k] int32): per row r of matrix [rows, n] the k best cells by the
    sequence score over L rows, among the row's first clamp(limit0 + r * limit_step, 0, n) columns (limit0 None: all),
    best first, ties -> the lower column.  offsets: an int32 table [V, L] (default slope_offsets(L)); slope: the row of it
    that won.  Empty slots: (-inf or +inf, -1, -1) in fp64, (-1, -1, -1) for int64 matrices; the first L - 1 rows are empty.
    contrast = R: the search runs on contrast_normalize(matrix, R, limit0, limit_step); scores are then fp64 for int64
    matrices too."""
    return _run(matrix, L, offsets, int(k), False, limit0, limit_step, lower_is_better, contrast)[:3]


def sequence_scores(matrix, L, offsets=None, limit0=None, limit_step=0, lower_is_better=False, contrast=None):
    """The dense [rows, n] sequence scores themselves (fp64, or int64 for int64 matrices): NaN / -1 where a cell has no
    valid line.  contrast = R: of contrast_normalize(matrix, R, limit0, limit_step), fp64."""
    return _run(matrix, L, offsets, None, True, limit0, limit_step, lower_is_better, contrast)[3]
