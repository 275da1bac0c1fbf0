"""Orderless place descriptors: a k-means codebook of patch descriptors and VLAD pooling (Jegou et al., CVPR 2010).

A frame's SDAV patch descriptors come in key-point response order, which a viewpoint change permutes; their
concatenation (flatten_frame_descriptors) then compares unrelated patches.  Vlad describes the frame by the per-word
sums of residuals instead -- [K * H], independent of the order of the patches -- and that row goes into
KeyframeDatabase and the certified cosine top-k as it is.  With SDAV(hidden_units=[.., 256]) and 16 words it is the
4096-d row of the headline benchmark.

Every number is defined in include/dlc.h (dlc_vlad_assign, dlc_vlad_encode, dlc_kmeans_step) and computed by the HIP
kernels behind it; fit() is a function of the rows in their order and of the seed.  The descriptor depends on the
codebook: rows of two codebooks do not compare.
"""
import numpy as np
import torch

from .engine import default_engine

NORMS = ("intra", "none")


class Vlad:
    """Vlad(n_words=16, norm="intra", seed=0): fit() a codebook, transform() frames' patch descriptors."""

    def __init__(self, n_words=16, norm="intra", seed=0, device=None):
        from . import _lib as L
        if int(n_words) != n_words or not 1 <= n_words <= L.DLC_VLAD_MAX_WORDS:
            raise ValueError("Vlad: n_words=%r outside 1..%d" % (n_words, L.DLC_VLAD_MAX_WORDS))
        if norm not in NORMS:
            raise ValueError("Vlad: norm=%r is none of %s" % (norm, ", ".join(NORMS)))
        self.n_words, self.norm, self.seed = int(n_words), norm, int(seed)
        self.engine = default_engine(device)
        self.centroids = None                  # fp64 [K, H] on the device
        self.inertia_ = []                     # per Lloyd step of the last fit()
        self.n_iter_ = 0

    # ---- operands ------------------------------------------------------------
    def _rows(self, who, h):
        """[rows, H] or [N, P, H], NumPy or tensor -> fp64 [rows, H] on the device."""
        t = h if isinstance(h, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(h, dtype=np.float64)))
        if t.dim() == 3:
            t = t.reshape(-1, t.shape[2])
        if t.dim() != 2 or t.shape[0] < 1 or t.shape[1] < 1:
            raise ValueError("%s: descriptors must be [rows, H] or [N, P, H]" % who)
        t = t.to(self.engine.device)
        return t if t.dtype == torch.float64 else t.to(torch.float64)

    def _need_codebook(self, who, width):
        if self.centroids is None:
            raise ValueError("%s: no codebook -- fit(), load() or set_codebook() first" % who)
        if width != self.centroids.shape[1]:
            raise ValueError("%s: the descriptors are %d wide, the codebook %d" % (who, width, self.centroids.shape[1]))

    @property
    def width(self):
        """Columns of a patch descriptor the codebook takes (None before there is one)."""
        return None if self.centroids is None else int(self.centroids.shape[1])

    @property
    def dim(self):
        """Columns of a VLAD row, K * H (None before there is a codebook)."""
        return None if self.centroids is None else int(self.centroids.shape[0] * self.centroids.shape[1])

    # ---- codebook ------------------------------------------------------------
    def set_codebook(self, c):
        c = self._rows("Vlad.set_codebook", c).contiguous().clone()
        if c.shape[0] != self.n_words:
            raise ValueError("Vlad.set_codebook: %d centres for n_words=%d" % (c.shape[0], self.n_words))
        self.centroids = c
        return self

    def fit(self, descriptors, iters=20):
        """Lloyd's k-means on the rows of `descriptors` ([rows, H] or [N, P, H]).  The initial centres are the rows at
        sorted(RandomState(seed).choice(rows, K, replace=False)); steps run until no row changes its word or `iters` is
        reached.  The changed counter is read once per step (this is a training routine); inertia_ keeps the summed
        squared distance each step started from."""
        x = self._rows("Vlad.fit", descriptors)
        rows = x.shape[0]
        if rows < self.n_words:
            raise ValueError("Vlad.fit: %d rows for %d words" % (rows, self.n_words))
        if int(iters) < 1:
            raise ValueError("Vlad.fit: iters must be >= 1")
        first = np.sort(np.random.RandomState(self.seed).choice(rows, self.n_words, replace=False))
        c = x[torch.from_numpy(first).to(self.engine.device)].contiguous()
        prev, inertia, steps = None, [], 0
        for _ in range(int(iters)):
            c, prev, _, s, changed = self.engine.kmeans_step(x, c, prev)
            inertia.append(s)
            steps += 1
            if int(changed.item()) == 0:
                break
        self.centroids = c
        self.inertia_ = torch.cat(inertia).cpu().tolist()
        self.n_iter_ = steps
        return self

    # ---- use -----------------------------------------------------------------
    def assign(self, h):
        """The word of every patch descriptor: int32 [rows] on the device (-1: every distance NaN)."""
        x = self._rows("Vlad.assign", h)
        self._need_codebook("Vlad.assign", x.shape[1])
        return self.engine.vlad_assign(x, self.centroids)

    def transform_tensor(self, h, patches=30, out=None):
        """[frames * patches, H] or [frames, patches, H] -> the frames' VLAD rows fp64 [frames, K * H] on the device."""
        if isinstance(h, torch.Tensor) and h.dim() == 3:
            patches = h.shape[1]
        x = self._rows("Vlad.transform", h)
        self._need_codebook("Vlad.transform", x.shape[1])
        return self.engine.vlad_encode(x, self.centroids, patches=patches, norm=self.norm, out=out)

    def transform(self, h, patches=30):
        """As transform_tensor; a NumPy input gives a NumPy result."""
        if not isinstance(h, torch.Tensor):
            a = np.asarray(h)
            if a.ndim == 3:
                patches = a.shape[1]
            return self.transform_tensor(a, patches).cpu().numpy()
        return self.transform_tensor(h, patches)

    # ---- persistence ---------------------------------------------------------
    def save(self, path):
        if self.centroids is None:
            raise ValueError("Vlad.save: no codebook")
        with open(path, "wb") as f:              # (np.savez would append .npz to a bare name)
            np.savez(f, centroids=self.centroids.cpu().numpy(), norm=np.array(self.norm), seed=np.array(self.seed),
                     inertia=np.asarray(self.inertia_, dtype=np.float64))

    @classmethod
    def load(cls, path, device=None):
        with np.load(path, allow_pickle=False) as z:
            missing = [k for k in ("centroids", "norm", "seed", "inertia") if k not in z.files]
            if missing:
                raise ValueError("Vlad.load: %s lacks %s" % (path, ", ".join(missing)))
            c = np.asarray(z["centroids"], dtype=np.float64)
            if c.ndim != 2 or c.shape[0] < 1 or c.shape[1] < 1:
                raise ValueError("Vlad.load: centroids of %s must be [K, H]" % path)
            v = cls(n_words=c.shape[0], norm=str(z["norm"]), seed=int(z["seed"]), device=device)
            v.inertia_ = z["inertia"].tolist()
        return v.set_codebook(c)
