"""Compact place descriptors: PCA and whitening of a pooled row (Jegou & Chum, ECCV 2012).

A VLAD row of the reference's SDAV (H = 2500, 16 words) is 40 000 wide and the concatenation of its 30 patch descriptors
75 000; the certified cosine top-k stores rows of up to 4096.  Pca projects either onto the leading principal directions
of a training set -- out = ((x - mean) . basis) * scale -- and that row goes into KeyframeDatabase as it is (the L2
normalisation and the bf16 store stay the database's).

transform() is dlc_pca_project (include/dlc.h) and nothing else: its sum order is stated, so a frame projected alone
while streaming has the bits it had in the batch that built the database.  fit() is a training routine: the GPU forms
the mean (dlc_kmeans_step with one word) and the products (dlc_gemm_bias_act, fp64), the host solves the eigenproblem.
The descriptor depends on the fitted model: rows of two models do not compare.
"""
import numpy as np
import torch

from . import _lib as L
from .engine import default_engine

BASES = ("f64", "f32")
FIELDS = ("mean", "basis", "variance", "scale", "whiten", "eps", "n_rows")


class Pca:
    """Pca(n_components, whiten=True, eps=0.0, basis="f64", max_rows=4096, seed=0): fit() rows, transform() rows."""

    def __init__(self, n_components, whiten=True, eps=0.0, basis="f64", max_rows=4096, seed=0, device=None):
        if int(n_components) != n_components or not 1 <= n_components <= L.DLC_PCA_MAX_COMPONENTS:
            raise ValueError("Pca: n_components=%r outside 1..%d" % (n_components, L.DLC_PCA_MAX_COMPONENTS))
        if basis not in BASES:
            raise ValueError("Pca: basis=%r is none of %s" % (basis, ", ".join(BASES)))
        if not float(eps) >= 0.0 or not np.isfinite(float(eps)):
            raise ValueError("Pca: eps=%r must be finite and >= 0" % (eps,))
        if int(max_rows) != max_rows or max_rows < 2:
            raise ValueError("Pca: max_rows=%r must be >= 2" % (max_rows,))
        self.n_components, self.whiten, self.eps = int(n_components), bool(whiten), float(eps)
        self.basis_dtype, self.max_rows, self.seed = basis, int(max_rows), int(seed)
        self.engine = default_engine(device)
        self.mean = self.basis = self.variance = self.scale = None     # device tensors once fitted or loaded
        self.n_rows = 0
        self.total_variance_ = None            # of the rows the last fit() took (not stored by save())

    # ---- operands ------------------------------------------------------------
    def _rows(self, who, x):
        """[rows, D], NumPy or tensor -> fp64 [rows, D] on the device (a tensor's strides are kept)."""
        t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=np.float64)))
        if t.dim() != 2 or t.shape[0] < 1 or t.shape[1] < 1:
            raise ValueError("%s: rows must be [rows, D]" % who)
        t = t.to(self.engine.device)
        return t if t.dtype == torch.float64 else t.to(torch.float64)

    @property
    def width(self):
        """Columns of a row the model takes, D (None before there is one)."""
        return None if self.basis is None else int(self.basis.shape[0])

    @property
    def dim(self):
        """Columns of a projected row, M (None before there is a model)."""
        return None if self.basis is None else int(self.basis.shape[1])

    @property
    def explained_variance_(self):
        """The kept components' variances lambda_c / (N - 1), descending, as a NumPy array."""
        return None if self.variance is None else self.variance.cpu().numpy()

    # ---- training ------------------------------------------------------------
    def fit(self, rows):
        """Principal directions of `rows` [N, D].  More than max_rows rows: those at sorted(RandomState(seed).choice(N,
        max_rows, replace=False)).  mu = dlc_kmeans_step's mean with one word; Xc = X - mu.  N <= D: the eigenvectors U
        of (G + G^T) / 2, G = Xc Xc^T, taken back as B = Xc^T U lam^-1/2 with columns rescaled to unit 2-norm; N > D:
        the eigenvectors of Xc^T Xc.  variance = lam / (N - 1); every column's largest entry (the lowest index among
        equals) is made positive; scale = 1 / sqrt(variance + eps) when whitening.  n_components above the numerical
        rank (numpy.linalg.matrix_rank's rule on sqrt(lam), and never more than min(N - 1, D)) is refused."""
        eng = self.engine
        x = self._rows("Pca.fit", rows)
        if not bool(torch.isfinite(x).all().item()):
            raise ValueError("Pca.fit: the rows hold a NaN or an infinity")
        if x.shape[0] > self.max_rows:
            take = np.sort(np.random.RandomState(self.seed).choice(x.shape[0], self.max_rows, replace=False))
            x = x[torch.from_numpy(take).to(eng.device)]
        x = x.contiguous()
        n, d = x.shape
        if n < 2:
            raise ValueError("Pca.fit: %d row: no variance to fit" % n)
        mu = eng.kmeans_step(x, torch.zeros((1, d), dtype=torch.float64, device=eng.device))[0][0].contiguous()
        xc = x - mu
        self.total_variance_ = float((xc * xc).sum().item()) / (n - 1)  # the trace of the fitted rows' covariance
        xct = xc.t().contiguous()
        g = eng.gemm_bias_act(xc, xc, blayout=L.DLC_B_NK) if n <= d else eng.gemm_bias_act(xct, xct, blayout=L.DLC_B_NK)
        g = g.cpu().numpy()
        lam, u = np.linalg.eigh((g + g.T) / 2)
        lam, u = lam[::-1], u[:, ::-1]
        s = np.sqrt(np.clip(lam, 0.0, None))
        rank = min(int((s > s.max() * max(n, d) * np.finfo(np.float64).eps).sum()), n - 1, d)
        m = self.n_components
        if m > rank:
            raise ValueError("Pca.fit: n_components=%d above the numerical rank %d of %d rows x %d" % (m, rank, n, d))
        if n <= d:
            w = torch.from_numpy(np.ascontiguousarray(u[:, :m] / np.sqrt(lam[:m]))).to(eng.device)
            b = eng.gemm_bias_act(xct, w)
            b = (b / torch.linalg.vector_norm(b, dim=0)).cpu().numpy()
        else:
            b = np.ascontiguousarray(u[:, :m])
        top = np.argmax(np.abs(b), axis=0)                             # (the first of equals)
        flip = b[top, np.arange(m)] < 0
        b[:, flip] = -b[:, flip]
        var = np.ascontiguousarray(lam[:m]) / (n - 1)
        self._set(mu, b, var, 1.0 / np.sqrt(var + self.eps) if self.whiten else None, n)
        return self

    def _set(self, mean, basis, variance, scale, n_rows):
        dev = self.engine.device
        def up(a, dt=torch.float64):
            t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
            return t.to(dev).to(dt).contiguous()
        self.mean = up(mean)
        self.basis = up(basis, torch.float32 if self.basis_dtype == "f32" else torch.float64)      # rounded once, here
        self.variance = up(variance)
        self.scale = up(scale) if scale is not None else None
        self.n_rows = int(n_rows)

    # ---- use -----------------------------------------------------------------
    def transform_tensor(self, x, out=None, plan="auto"):
        """[rows, D] -> the projected rows fp64 [rows, M] on the device."""
        x = self._rows("Pca.transform", x)
        if self.basis is None:
            raise ValueError("Pca.transform: no model -- fit() or load() first")
        if x.shape[1] != self.width:
            raise ValueError("Pca.transform: the rows are %d wide, the model %d" % (x.shape[1], self.width))
        return self.engine.pca_project(x, self.basis, self.mean, self.scale, out=out, plan=plan)

    def transform(self, x, plan="auto"):
        """As transform_tensor; a NumPy input gives a NumPy result."""
        if not isinstance(x, torch.Tensor):
            return self.transform_tensor(np.asarray(x), plan=plan).cpu().numpy()
        return self.transform_tensor(x, plan=plan)

    # ---- persistence ---------------------------------------------------------
    def save(self, path):
        if self.basis is None:
            raise ValueError("Pca.save: no model")
        with open(path, "wb") as f:              # (np.savez would append .npz to a bare name)
            np.savez(f, mean=self.mean.cpu().numpy(), basis=self.basis.cpu().numpy(), variance=self.variance.cpu().numpy(),
                     scale=self.scale.cpu().numpy() if self.scale is not None else np.zeros(0), whiten=np.array(self.whiten),
                     eps=np.array(self.eps), n_rows=np.array(self.n_rows, dtype=np.int64))

    @classmethod
    def load(cls, path, device=None):
        with np.load(path, allow_pickle=False) as z:
            missing = [k for k in FIELDS if k not in z.files]
            if missing:
                raise ValueError("Pca.load: %s lacks %s" % (path, ", ".join(missing)))
            b = np.asarray(z["basis"])
            if b.ndim != 2 or b.shape[0] < 1 or b.shape[1] < 1 or b.dtype not in (np.float64, np.float32):
                raise ValueError("Pca.load: basis of %s must be a float64 or float32 [D, M]" % path)
            whiten = bool(z["whiten"])
            mean, var = np.asarray(z["mean"], dtype=np.float64), np.asarray(z["variance"], dtype=np.float64)
            scale = np.asarray(z["scale"], dtype=np.float64)
            if mean.shape != (b.shape[0],) or var.shape != (b.shape[1],) or scale.shape != ((b.shape[1],) if whiten else (0,)):
                raise ValueError("Pca.load: mean, variance or scale of %s do not fit a basis [%d, %d]" % ((path,) + b.shape))
            p = cls(b.shape[1], whiten=whiten, eps=float(z["eps"]), basis="f32" if b.dtype == np.float32 else "f64", device=device)
            p._set(mean, b, var, scale if whiten else None, int(z["n_rows"]))
        return p
