"""SeqSLAM's front-end (Milford & Wyeth, ICRA 2012, III-A) on MI355X: the image descriptor the sequence matcher of this
package was designed for, and its difference matrix.

    SeqSlam                 frames -> patch-normalised grey thumbnails, uint8 [B, h * w] (dlc_seqslam_describe_u8); no weights
    DifferenceCalculator    sum of absolute differences of descriptors: the full matrix, or a rectangular set of pairs
    SadKeyframeDatabase     the descriptors resident in HBM, a batch's difference rows against them (dlc_sad_u8_rows)

shift = S with width = w on any of the three compares over the lateral shifts -S .. S of the thumbnail's columns and keeps
the best, rescaled to the plain SAD's scale (dlc_sad_u8_shift_rows): a place revisited a little to the side still matches.

The rows are int64 and lower is better, as the cnn_vtl distance rows are: sequence_topk / contrast_normalize /
sequence_peaks / sequence_chains take them as they are, and SeqSlamLoopClosureDetector (loop_closure.py) is the streaming
form.  Both definitions are exact and stated in include/dlc.h.
"""
import numpy as np
import torch

from .distance import _ByteRowStore
from .engine import default_engine


class SeqSlam:
    """The descriptor 'network' of SeqSLAM, with the call surface of SDAV / CnnVtl: transform() NumPy in, NumPy out;
    transform_tensor() device tensors in and out.  size = (h, w) of the thumbnail, patch: the side of the normalisation
    tiles, strength: the descriptor's byte is 128 + strength * (T - tile mean) / tile sample std, clamped to 0..255 (32
    keeps +-4 standard deviations inside the byte)."""

    def __init__(self, size=(32, 64), patch=8, strength=32, device=None):
        h, w = (int(v) for v in size)
        if h < 1 or w < 1 or h * w > 65536:
            raise ValueError("SeqSlam: size=%r must be positive with at most 65536 cells" % (size,))
        if not 1 <= int(patch) <= 64:
            raise ValueError("SeqSlam: patch=%r outside 1..64" % (patch,))
        if not 1 <= int(strength) <= 127:
            raise ValueError("SeqSlam: strength=%r outside 1..127" % (strength,))
        self.size, self.patch, self.strength = (h, w), int(patch), int(strength)
        self.engine = default_engine(device)

    @property
    def dim(self):
        """Bytes of a descriptor: h * w."""
        return self.size[0] * self.size[1]

    def transform_tensor(self, frames, out=None):
        """frames: uint8 [B, H, W, 3] RGB or [B, H, W] grey, a device tensor -> uint8 [B, h * w] on the device (grey by
        Engine.rgb_to_gray, then Engine.seqslam_describe).  out: a caller-kept uint8 [B, >= h * w] tensor or row view."""
        e = self.engine
        x = e.to_device(frames)
        if x.dtype != torch.uint8 or x.dim() not in (3, 4) or (x.dim() == 4 and x.shape[-1] != 3):
            raise ValueError("SeqSlam: frames must be uint8 [B, H, W, 3] (RGB) or [B, H, W] (grey)")
        gray = e.rgb_to_gray(x) if x.dim() == 4 else x
        return e.seqslam_describe(gray, self.size, self.patch, self.strength, out=out)

    def transform(self, frames):
        """frames: uint8 [B, H, W, 3] RGB or [B, H, W] grey (anything np.asarray takes) -> numpy uint8 [B, h * w]."""
        a = np.asarray(frames)
        if a.dtype != np.uint8:
            raise ValueError("SeqSlam: frames must be uint8")
        return self.transform_tensor(self.engine.to_device(np.ascontiguousarray(a))).cpu().numpy()


class DifferenceCalculator:
    """The counterpart of DistanceCalculator for SeqSLAM descriptors: sum_p |a[p] - b[p]| on unsigned bytes."""

    @staticmethod
    def _rows(engine, x, what):
        """x, a NumPy array (or anything np.asarray takes) or a tensor, as uint8 [N, D] on the device -- checked."""
        if not isinstance(x, torch.Tensor):
            x = np.ascontiguousarray(np.asarray(x))
        if x.dtype != (torch.uint8 if isinstance(x, torch.Tensor) else np.uint8) or x.ndim != 2:
            raise ValueError("%s must be [N, D] uint8" % what)
        return engine.to_device(x)

    @staticmethod
    def _host(res):
        """A sad_rows result, one tensor or (out, shift_out), as NumPy."""
        return tuple(t.cpu().numpy() for t in res) if isinstance(res, tuple) else res.cpu().numpy()

    @staticmethod
    def difference_matrix(descriptors, shift=None, width=None, return_shift=False):
        """Full N x N matrix incl. the diagonal (zeros), numpy int64: difference_rows(descriptors, descriptors).
        descriptors: uint8 [N, D], NumPy or a tensor.  shift, width, return_shift: as difference_rows takes them (the
        shifted values are symmetric too -- shift s of (i, j) is shift -s of (j, i) -- the shifts are not)."""
        e = default_engine()
        d = DifferenceCalculator._rows(e, descriptors, "descriptors")
        return DifferenceCalculator._host(e.sad_rows(d, d, shift=shift, width=width, shift_out=True if return_shift else None))

    @staticmethod
    def difference_rows(queries, descriptors, shift=None, width=None, return_shift=False):
        """numpy int64 [Q, N]: every query against every descriptor as one call (dlc_sad_u8_rows).  queries [Q, D] and
        descriptors [N, D]: uint8, NumPy or tensors.  shift = S with width = w (the thumbnail's columns): the best of the
        lateral shifts -S .. S instead (dlc_sad_u8_shift_rows); return_shift: (rows, numpy int8 [Q, N] of the winning
        shifts)."""
        e = default_engine()
        q = DifferenceCalculator._rows(e, queries, "queries")
        x = DifferenceCalculator._rows(e, descriptors, "descriptors")
        if q.shape[1] != x.shape[1]:
            raise ValueError("difference_rows: queries [Q, D] and descriptors [N, D] with one D")
        return DifferenceCalculator._host(e.sad_rows(q, x, shift=shift, width=width, shift_out=True if return_shift else None))


class SadKeyframeDatabase(_ByteRowStore):
    """SeqSLAM key-frame descriptors (uint8 [n, dim]) resident in HBM, compared by the sum of absolute differences.

    Rows are stored zero-padded to a multiple of 16 bytes in a capacity-reserved buffer that doubles when an append()
    outgrows it (the store of CnnVtlKeyframeDatabase); `rows` is the view of the first len(db) rows.  differences() is
    dlc_sad_u8_rows: the [Q, len(db)] difference rows, for the sequence search and the peak selection to rank."""

    DTYPE, KIND = torch.uint8, "SeqSLAM"

    def differences(self, queries, limit0=None, limit_step=0, out=None, shift=None, width=None, return_shift=False):
        """int64 [Q, len(self)] on the device: the SAD of each query row to every stored key-frame.  queries: [Q, dim]
        uint8, or stored rows [Q, stored_width(dim)] such as a slice of `rows` (the padding is ignored).  limit0 /
        limit_step: query r is written in its first limit0 + r * limit_step cells only (default: all); the others keep
        what `out` held (a caller-kept int64 [Q, len(self)] tensor or row-strided view), or hold -1 when the result is
        allocated here.  shift = S with width = w (the thumbnail's columns, dim a multiple of it): the best of the lateral
        shifts -S .. S (dlc_sad_u8_shift_rows); return_shift: (rows, int8 [Q, len(self)] of the winning shifts, 0 where a
        cell was not offered) -- the lateral offset of the revisit in thumbnail columns."""
        q = self._queries("differences", queries)
        return self.engine.sad_rows(q, self.rows, d=self.dim, limit0=limit0, limit_step=limit_step, out=out, shift=shift,
                                    width=width, shift_out=True if return_shift else None)
