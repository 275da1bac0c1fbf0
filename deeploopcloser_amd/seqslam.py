"""SeqSLAM's front-end (Milford & Wyeth, ICRA 2012, III-A) on MI355X: the image descriptor the sequence matcher of this
package was designed for, and its difference matrix.

    SeqSlam                 frames -> patch-normalised grey thumbnails, uint8 [B, h * w] (dlc_seqslam_describe_u8); no weights
    DifferenceCalculator    sum of absolute differences of descriptors: the full matrix, or a rectangular set of pairs
    SadKeyframeDatabase     the descriptors resident in HBM, a batch's difference rows against them (dlc_sad_u8_rows)

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
    def difference_matrix(descriptors):
        """Full N x N matrix incl. the diagonal (zeros), numpy int64: difference_rows(descriptors, descriptors).
        descriptors: uint8 [N, D], NumPy or a tensor."""
        e = default_engine()
        d = DifferenceCalculator._rows(e, descriptors, "descriptors")
        return e.sad_rows(d, d).cpu().numpy()

    @staticmethod
    def difference_rows(queries, descriptors):
        """numpy int64 [Q, N]: every query against every descriptor as one call (dlc_sad_u8_rows).  queries [Q, D] and
        descriptors [N, D]: uint8, NumPy or tensors."""
        e = default_engine()
        q = DifferenceCalculator._rows(e, queries, "queries")
        x = DifferenceCalculator._rows(e, descriptors, "descriptors")
        if q.shape[1] != x.shape[1]:
            raise ValueError("difference_rows: queries [Q, D] and descriptors [N, D] with one D")
        return e.sad_rows(q, x).cpu().numpy()


class SadKeyframeDatabase(_ByteRowStore):
    """SeqSLAM key-frame descriptors (uint8 [n, dim]) resident in HBM, compared by the sum of absolute differences.

    Rows are stored zero-padded to a multiple of 16 bytes in a capacity-reserved buffer that doubles when an append()
    outgrows it (the store of CnnVtlKeyframeDatabase); `rows` is the view of the first len(db) rows.  differences() is
    dlc_sad_u8_rows: the [Q, len(db)] difference rows, for the sequence search and the peak selection to rank."""

    DTYPE, KIND = torch.uint8, "SeqSLAM"

    def differences(self, queries, limit0=None, limit_step=0, out=None):
        """int64 [Q, len(self)] on the device: the SAD of each query row to every stored key-frame.  queries: [Q, dim]
        uint8, or stored rows [Q, stored_width(dim)] such as a slice of `rows` (the padding is ignored).  limit0 /
        limit_step: query r is written in its first limit0 + r * limit_step cells only (default: all); the others keep
        what `out` held (a caller-kept int64 [Q, len(self)] tensor or row-strided view), or hold -1 when the result is
        allocated here."""
        q = self._queries("differences", queries)
        return self.engine.sad_rows(q, self.rows, d=self.dim, limit0=limit0, limit_step=limit_step, out=out)
