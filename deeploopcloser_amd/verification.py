"""Geometric verification of loop candidates: the last stage of a loop closer.

Every detector of this package reports a candidate on appearance alone, and two frames that look alike but are different
places (perceptual aliasing) pass all of them.  A SLAM back-end does not add a pose-graph constraint on that: it matches
the local features of the query frame to those of the candidate, fits a 2-D transform to the matched positions and keeps
the candidate only if enough matches agree with it.  Here the local features are what the SDAV front-end already has --
the P patch descriptors of a frame (SDAV.transform, [N, P, H] fp64) and the integer key-points the patches were cut at
(CvInputParser.parse_batch(..., return_key_points=True)) -- and the stage is Engine.verify_pairs (dlc_verify_pairs,
include/dlc.h): nearest-neighbour patch matching by the stated serial-chain distance, cross-checked, then an EXHAUSTIVE
search over every two-match similarity (or one-match translation) in integer arithmetic.  No random sampling, no floating
point in the geometry: the inlier count of a pair is a function of that pair's descriptors and points alone.

THE POINTS.  The verifier is defined on the points it is given, (x, y) int32 with 0 <= x, y <= 8191; any other point
(the Harris pass writes (-1, -1) past a frame's point count) is absent and its match is dropped.  The library's Harris
stand-in returns (x = column, y = row) while dlc_extract_patches, like the reference, walks pt[0] along image dimension
0 and shifts windows to stay inside the image; a caller with its own key-points passes the verifier the SAME array it
gave the extractor, whatever its convention -- the geometry only needs both frames to use one convention.
"""
import numpy as np
import torch

from . import _lib as L

MODELS = ("similarity", "translation")


def keep_accepted(accept, scores, ids, fill, *others):
    """Rows of candidate lists [B, k] with the rejected slots turned into (fill, -1) and moved, stably, behind the
    accepted ones -> (scores, ids, *others); `others` ([B, k] tensors: inlier counts, ...) are moved along as they are.
    Plain tensor indexing on whatever device the tensors live on."""
    accept = accept & (ids >= 0)
    order = torch.argsort((~accept).to(torch.int8), dim=1, stable=True)
    acc = accept.gather(1, order)
    s, i = scores.gather(1, order), ids.gather(1, order)
    s = torch.where(acc, s, torch.full_like(s, fill))
    i = torch.where(acc, i, torch.full_like(i, -1))
    return (s, i) + tuple(o.gather(1, order) for o in others)


class GeometricVerifier:
    """Resident stores of every frame's patch descriptors [capacity, P, H] fp64 and key-points [capacity, P, 2] int32,
    growable as KeyframeDatabase is (doubling; ids never change), and the verification of candidate lists against them.

        first = verifier.append(desc, points)            # the batch's frames become resident: ids first .. first + B - 1
        inliers, n_matches = verifier.verify(first, ids) # frame first + r against the key-frames ids[r, :]
        scores, ids = verifier.apply(scores, ids, fill, first_id=first)

    Append first, then verify: a candidate from the same batch is then legal.  A candidate is ACCEPTED iff its inlier
    count reaches min_inliers.  model, tol, max_scale and mutual are Engine.verify_pairs'."""

    def __init__(self, patches=30, width=2500, capacity=1024, min_inliers=6, model="similarity", tol=3, max_scale=2.0,
                 mutual=True, device=None):
        if not 1 <= patches <= L.DLC_VERIFY_MAX_PATCHES:
            raise ValueError("patches=%d outside 1..%d" % (patches, L.DLC_VERIFY_MAX_PATCHES))
        if width < 1 or capacity < 1:
            raise ValueError("width and capacity must be positive")
        if min_inliers < 0:
            raise ValueError("min_inliers must be >= 0")
        if model not in MODELS:
            raise ValueError("model=%r is none of %s" % (model, ", ".join(MODELS)))
        if int(tol) != tol or not 0 <= tol <= 255:
            raise ValueError("tol=%r outside 0..255" % (tol,))
        if max_scale is not None and not 16 <= int(round(16 * float(max_scale))) <= 256:
            raise ValueError("max_scale=%r outside 1..16" % (max_scale,))
        self.p, self.h, self.capacity, self.min_inliers = int(patches), int(width), int(capacity), int(min_inliers)
        self.model, self.tol, self.max_scale, self.mutual = model, int(tol), max_scale, bool(mutual)
        self._device, self._engine = device, None
        self.desc = self.points = None                       # allocated by the first append
        self.n = 0

    def __len__(self):
        return self.n

    @property
    def engine(self):
        if self._engine is None:
            from .engine import default_engine
            self._engine = default_engine(self._device)
        return self._engine

    def _reserve(self, n):
        """Room for n frames: the stores are re-laid at twice the capacity (at least n) and the frames copied."""
        if self.desc is not None and n <= self.capacity:
            return
        cap = self.capacity
        while cap < n:
            cap *= 2
        dev = self.engine.device
        desc = torch.empty((cap, self.p, self.h), dtype=torch.float64, device=dev)
        points = torch.full((cap, self.p, 2), -1, dtype=torch.int32, device=dev)
        if self.desc is not None and self.n:
            desc[:self.n] = self.desc[:self.n]
            points[:self.n] = self.points[:self.n]
        self.desc, self.points, self.capacity = desc, points, cap

    def append(self, desc, points):
        """desc [B, P, H] (or [B * P, H]) fp64 and points int32 [B, P, 2], tensors or arrays -> the first id; the frames
        are resident afterwards."""
        e = self.engine
        x = e.to_device(desc, torch.float64)
        pts = e.to_device(points)
        if pts.dtype != torch.int32:
            pts = pts.to(torch.int32)
        if x.dim() == 2:
            x = x.view(-1, self.p, x.shape[1]) if x.shape[0] % self.p == 0 else x
        if x.dim() != 3 or x.shape[1] != self.p or x.shape[2] != self.h:
            raise ValueError("descriptors must be [B, %d, %d], not %s" % (self.p, self.h, tuple(x.shape)))
        if pts.dim() == 2:
            pts = pts.unsqueeze(0)
        if tuple(pts.shape) != (x.shape[0], self.p, 2):
            raise ValueError("points must be [%d, %d, 2], not %s" % (x.shape[0], self.p, tuple(pts.shape)))
        first, b = self.n, x.shape[0]
        self._reserve(first + b)
        self.desc[first:first + b] = x
        self.points[first:first + b] = pts
        self.n = first + b
        return first

    def verify(self, first_id, ids, with_mask=False, with_match=False):
        """Frames first_id .. first_id + B - 1 of the store against the key-frames ids [B, k] (int64; -1 or any id outside
        the store: 0 inliers) -> (inliers int32 [B, k], n_matches int32 [B, k]) on the device, + Engine.verify_pairs'
        optional results."""
        e = self.engine
        ids = e.to_device(ids, torch.int64)
        if ids.dim() != 2:
            raise ValueError("ids must be [B, k]")
        b = ids.shape[0]
        if not 0 <= first_id <= first_id + b <= self.n:
            raise ValueError("frames %d .. %d are not in the store of %d" % (first_id, first_id + b - 1, self.n))
        if b == 0:
            empty = torch.empty((0, ids.shape[1]), dtype=torch.int32, device=e.device)
            return empty, empty.clone()
        return e.verify_pairs(self.desc[first_id:first_id + b], self.points[first_id:first_id + b], self.desc[:self.n],
                              self.points[:self.n], ids, model=self.model, tol=self.tol, max_scale=self.max_scale,
                              mutual=self.mutual, with_mask=with_mask, with_match=with_match)

    def accept(self, first_id, ids):
        """bool [B, k]: the candidate exists and its inlier count reaches min_inliers."""
        ids = self.engine.to_device(ids, torch.int64)
        inliers, _ = self.verify(first_id, ids)
        return (inliers >= self.min_inliers) & (ids >= 0)

    def apply(self, scores, ids, fill=float("-inf"), first_id=None, accept=None):
        """A detector's lists (scores [B, k], ids [B, k]) with the rejected slots turned into (fill, -1) and moved, stably,
        behind the accepted ones.  accept: a bool [B, k] to go by; None: self.accept(first_id, ids)."""
        if accept is None:
            if first_id is None:
                raise ValueError("apply needs first_id (the store id of the lists' first frame) or accept")
            accept = self.accept(first_id, ids)
        return keep_accepted(accept, scores, ids, fill)


def verify_candidates(q_desc, q_pts, db_desc, db_pts, cand, model="similarity", tol=3, max_scale=2.0, mutual=True, device=None):
    """One call over arrays or tensors: q_desc [Q, P, H], q_pts [Q, P, 2], db_desc [N, P, H], db_pts [N, P, 2], cand
    [Q, k] -> (inliers, n_matches) int32 [Q, k]; NumPy arrays if q_desc is one, else device tensors."""
    from .engine import default_engine
    e = default_engine(device)
    as_numpy = isinstance(q_desc, np.ndarray)
    pts = lambda t: e.to_device(t).to(torch.int32)
    out = e.verify_pairs(e.to_device(q_desc, torch.float64), pts(q_pts), e.to_device(db_desc, torch.float64), pts(db_pts),
                         e.to_device(cand, torch.int64), model=model, tol=tol, max_scale=max_scale, mutual=mutual)
    return tuple(t.cpu().numpy() for t in out) if as_numpy else out
