"""Multi-descriptor fusion of score matrices (not in the reference): several matrices that compare the same frames with
the same key-frames -- the SDAV similarity matrix, drivers.create_distance_matrix's cnn_vtl distances, SeqSLAM's
create_difference_matrix, cosine scores -- have different units, ranges and signs.  fuse_scores normalises each within
its own row, turns the sign of what is lower-is-better, weights and sums: one fp64, higher-is-better matrix that
sequence_topk / sequence_peaks / peak_topk / pr_curve_cells take as any other (dlc_fuse_rows, include/dlc.h: the
normalisations, the TREE order of every row sum, the rounding -- a row does not depend on its batch).  The sum of
per-query standardised similarities is a standard remedy in place recognition (Schubert et al.; Hausler et al.,
Multi-Process Fusion): a hand-crafted descriptor and a deep one fail in different places.

NumPy in -> NumPy out, device tensors in -> device tensors out.
"""
import torch

from .engine import default_engine
from .sequence import _on_device

NORMS = ("zscore", "minmax", "none")


def fuse_scores(matrices, weights=None, lower_is_better=False, norm="zscore", limit0=None, limit_step=0):
    """fp64 [rows, n], higher is better: cell (r, j) = sum_i weights[i] * norm_i(matrices[i][r, j]), every matrix
    normalised within its own row r over the row's first clamp(limit0 + r * limit_step, 0, n) cells (limit0 None: all) --
    norm "zscore": (x - mean) / sample std (0.0 for a constant row or a single cell), "minmax": (x - min) / (max - min),
    "none": x itself -- and negated where it is lower-is-better (a bool, or one per matrix).  matrices: 1..8 arrays or
    tensors [rows, n] of one shape (fp64, fp32 or int64; other types are converted as the sequence search converts
    them); weights: None (all 1) or one finite number per matrix.  Cells that are not offered are NaN."""
    matrices = list(matrices)
    if not matrices:
        raise ValueError("fuse_scores: no matrix")
    e = default_engine()
    pairs = [_on_device(e, m) for m in matrices]
    as_numpy = all(p[1] for p in pairs)
    if not as_numpy and any(p[1] for p in pairs):
        raise ValueError("fuse_scores: NumPy arrays and device tensors mixed")
    mats = [p[0] for p in pairs]
    if any(tuple(m.shape) != tuple(mats[0].shape) for m in mats):
        raise ValueError("fuse_scores: the matrices must have one shape")
    out = torch.full(tuple(mats[0].shape), float("nan"), dtype=torch.float64, device=e.device)
    if out.shape[0] and out.shape[1]:
        e.fuse_rows(mats, weights=weights, lower_is_better=lower_is_better, norm=norm, limit0=limit0, limit_step=limit_step,
                    out=out)
    elif norm not in NORMS:
        raise ValueError("fuse_scores: norm=%r is none of %s" % (norm, ", ".join(NORMS)))
    return out.cpu().numpy() if as_numpy else out
