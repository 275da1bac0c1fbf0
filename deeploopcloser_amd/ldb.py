"""A binary place descriptor on MI355X: the global LDB code of a frame ("Local Difference Binary", Yang & Cheng, ISMAR
2012; taken over the whole down-sampled frame as ABLE-M does, Arroyo et al., IROS 2015) and its Hamming distance.

    Ldb                        frames -> packed bits, uint8 [B, row bytes] (dlc_ldb_describe_u8); no weights
    HammingCalculator          Hamming distance of packed descriptors: the full matrix, or a rectangular set of pairs
    HammingKeyframeDatabase    the descriptors resident in HBM, a batch's Hamming rows against them (dlc_hamming_rows)

A frame is a few hundred bits -- comparisons of the sums and the two gradients of the grid cells of a grey thumbnail --
so a million key-frames are 64 MB, and every bit is unchanged by a gain and an offset of the image.  The code does not
tolerate lateral shifts beyond a few pixels (docs/LAB.md 34).

The rows are int64 and lower is better, as the SAD rows are: sequence_topk / contrast_normalize / sequence_peaks /
sequence_chains take them as they are, and LdbLoopClosureDetector (loop_closure.py) is the streaming form.  Both
definitions are exact and stated in include/dlc.h.
"""
import numpy as np
import torch

from .distance import _ByteRowStore
from .engine import default_engine


def ldb_bits(levels):
    """Bits of the code for `levels`, 3 * sum g^2 (g^2 - 1) / 2; ValueError for a list that is not 1 to 4 grid sizes,
    strictly ascending, each 2..8 (what dlc_ldb_row_bytes answers with 0)."""
    try:
        lv = tuple(levels)
        ok = 1 <= len(lv) <= 4 and all(int(g) == g and 2 <= g <= 8 for g in lv) and all(a < b for a, b in zip(lv, lv[1:]))
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError("Ldb: levels=%r must be 1 to 4 grid sizes, strictly ascending, each 2..8" % (levels,))
    return 3 * sum(int(g) ** 2 * (int(g) ** 2 - 1) // 2 for g in lv)


class Ldb:
    """The descriptor 'network' of the binary route, with the call surface of SeqSlam: transform() NumPy in, NumPy out;
    transform_tensor() device tensors in and out.  size = (h, w) of the thumbnail; levels: the grid sizes g, each cutting
    the thumbnail into g x g cells (2 g must divide h and w)."""

    def __init__(self, size=(48, 48), levels=(2, 3, 4), device=None):
        h, w = (int(v) for v in size)
        if h < 1 or w < 1 or h * w > 65536:
            raise ValueError("Ldb: size=%r must be positive with at most 65536 cells" % (size,))
        self.n_bits = ldb_bits(levels)
        self.levels = tuple(int(g) for g in levels)
        for g in self.levels:
            if h % (2 * g) or w % (2 * g):
                raise ValueError("Ldb: 2 x %d does not divide size=%r" % (g, (h, w)))
        self.size = (h, w)
        self.engine = default_engine(device)

    @property
    def dim(self):
        """Bytes of a descriptor row: 16 * ceil(n_bits / 128)."""
        return 16 * ((self.n_bits + 127) // 128)

    def transform_tensor(self, frames, out=None):
        """frames: uint8 [B, H, W, 3] RGB or [B, H, W] grey, a device tensor -> uint8 [B, dim] on the device (grey by
        Engine.rgb_to_gray, then Engine.ldb_describe).  out: a caller-kept uint8 [B, >= dim] tensor or row view."""
        e = self.engine
        x = e.to_device(frames)
        if x.dtype != torch.uint8 or x.dim() not in (3, 4) or (x.dim() == 4 and x.shape[-1] != 3):
            raise ValueError("Ldb: frames must be uint8 [B, H, W, 3] (RGB) or [B, H, W] (grey)")
        gray = e.rgb_to_gray(x) if x.dim() == 4 else x
        return e.ldb_describe(gray, self.size, self.levels, out=out)

    def transform(self, frames):
        """frames: uint8 [B, H, W, 3] RGB or [B, H, W] grey (anything np.asarray takes) -> numpy uint8 [B, dim]."""
        a = np.asarray(frames)
        if a.dtype != np.uint8:
            raise ValueError("Ldb: frames must be uint8")
        return self.transform_tensor(self.engine.to_device(np.ascontiguousarray(a))).cpu().numpy()


class HammingCalculator:
    """The counterpart of DifferenceCalculator for packed binary descriptors: sum_p popcount(a[p] ^ b[p]) on bytes."""

    @staticmethod
    def _rows(x, what):
        """x, a NumPy array (or anything np.asarray takes) or a tensor, as uint8 [N, D] -- checked, then on the device."""
        if not isinstance(x, torch.Tensor):
            x = np.ascontiguousarray(np.asarray(x))
        if x.dtype != (torch.uint8 if isinstance(x, torch.Tensor) else np.uint8) or x.ndim != 2:
            raise ValueError("%s must be [N, D] uint8" % what)
        return default_engine().to_device(x)

    @staticmethod
    def hamming_matrix(descriptors):
        """Full N x N matrix incl. the diagonal (zeros), numpy int64: hamming_rows(descriptors, descriptors)."""
        d = HammingCalculator._rows(descriptors, "descriptors")
        return default_engine().hamming_rows(d, d).cpu().numpy()

    @staticmethod
    def hamming_rows(queries, descriptors):
        """numpy int64 [Q, N]: every query against every descriptor as one call (dlc_hamming_rows).  queries [Q, D] and
        descriptors [N, D]: uint8, NumPy or tensors."""
        if np.ndim(queries) == 2 and np.ndim(descriptors) == 2 and np.shape(queries)[1] != np.shape(descriptors)[1]:
            raise ValueError("hamming_rows: queries [Q, D] and descriptors [N, D] with one D")
        q = HammingCalculator._rows(queries, "queries")
        x = HammingCalculator._rows(descriptors, "descriptors")
        return default_engine().hamming_rows(q, x).cpu().numpy()


class HammingKeyframeDatabase(_ByteRowStore):
    """Binary key-frame descriptors (uint8 [n, dim], packed bits) resident in HBM, compared by Hamming distance.

    Rows are stored zero-padded to a multiple of 16 bytes in a capacity-reserved buffer that doubles when an append()
    outgrows it (the store of CnnVtlKeyframeDatabase); `rows` is the view of the first len(db) rows.  distances() is
    dlc_hamming_rows: the [Q, len(db)] Hamming rows, for the sequence search and the peak selection to rank."""

    DTYPE, KIND = torch.uint8, "binary"

    def distances(self, queries, limit0=None, limit_step=0, out=None):
        """int64 [Q, len(self)] on the device: the Hamming distance of each query row to every stored key-frame.
        queries: [Q, dim] uint8, or stored rows [Q, stored_width(dim)] such as a slice of `rows` (the padding is
        ignored).  limit0 / limit_step: query r is written in its first limit0 + r * limit_step cells only (default:
        all); the others keep what `out` held (a caller-kept int64 [Q, len(self)] tensor or row-strided view), or hold
        -1 when the result is allocated here."""
        q = self._queries("distances", queries)
        return self.engine.hamming_rows(q, self.rows, d=self.dim, limit0=limit0, limit_step=limit_step, out=out)
