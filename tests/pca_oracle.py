"""NumPy restatement of the PCA definitions: the projection of include/dlc.h (dlc_pca_project) -- a loop over d inside a
chunk, vectorised over (row, component), and a serial loop over the chunks -- and Pca.fit's recipe by two routes, the
SVD of the centred rows and the Gram matrix followed by back-projection, with the sign rule.  fp64, every operation
rounded on its own (NumPy never contracts).  Test infrastructure only."""
import numpy as np

import vlad_oracle

CHUNK = 1024

# How far the two fit routes below differ on yardstick_rows(N, D, seed=0), 12 components: (delta_var, delta_vec) --
# the largest relative variance difference and the largest basis entry difference after the sign rule.  Both routes
# are exact up to rounding, so this is the summation-order error of the fit at that shape; the device fit is held to
# 64 x these (tests/test_gpu_pca.py).  Recorded from test_pca_cpu.py::test_fit_routes_agree (which prints them).
RECORDED_DELTA = {(48, 200): (3.6e-11, 1.7e-11), (200, 48): (4.3e-12, 1.2e-10)}
DELTA_CEILING = 1e-8


def project(x, basis, mean=None, scale=None):
    """out [rows, M] of x [rows, D], basis [D, M] (fp64 or fp32), mean [D] or None, scale [M] or None."""
    x = np.asarray(x, dtype=np.float64)
    b = np.asarray(basis).astype(np.float64)                           # exact for fp32
    rows, D = x.shape
    with np.errstate(all="ignore"):
        t = x - np.asarray(mean, dtype=np.float64)[None, :] if mean is not None else x
        y = None
        for d0 in range(0, D, CHUNK):
            s = np.zeros((rows, b.shape[1]))
            for d in range(d0, min(D, d0 + CHUNK)):
                q = t[:, d, None] * b[None, d, :]
                s = s + q
            y = s if y is None else y + s
        return y * np.asarray(scale, dtype=np.float64)[None, :] if scale is not None else y


def project_one_chain(x, basis, mean=None, scale=None):
    """What the definition is NOT: one unbroken serial chain over all of D."""
    x = np.asarray(x, dtype=np.float64)
    b = np.asarray(basis).astype(np.float64)
    with np.errstate(all="ignore"):
        t = x - np.asarray(mean, dtype=np.float64)[None, :] if mean is not None else x
        s = np.zeros((x.shape[0], b.shape[1]))
        for d in range(x.shape[1]):
            s = s + t[:, d, None] * b[None, d, :]
        return s * np.asarray(scale, dtype=np.float64)[None, :] if scale is not None else s


def column_mean(x):
    """The training mean: dlc_kmeans_step with one word -- block sums of 1024 rows, TREE over the blocks, / count."""
    x = np.asarray(x, dtype=np.float64)
    return vlad_oracle.kmeans_step(x, np.zeros((1, x.shape[1])))[0][0]


def sign_rule(B):
    """Every column's entry of largest magnitude made positive; on a tie the lowest index decides."""
    B = np.array(B, dtype=np.float64)
    top = np.argmax(np.abs(B), axis=0)                                 # (argmax takes the first of equals)
    flip = B[top, np.arange(B.shape[1])] < 0
    B[:, flip] = -B[:, flip]
    return B


def numerical_rank(lam, n, d):
    """numpy.linalg.matrix_rank's rule on the singular values sqrt(lam), and never more than min(n - 1, d)."""
    s = np.sqrt(np.clip(lam, 0.0, None))
    return min(int((s > s.max() * max(n, d) * np.finfo(np.float64).eps).sum()), n - 1, d)


def _finish(mu, B, lam, n, d, m, whiten, eps):
    if m > numerical_rank(lam, n, d):
        raise ValueError("n_components=%d above the numerical rank" % m)
    var = lam[:m] / (n - 1)
    scale = 1.0 / np.sqrt(var + eps) if whiten else None
    return mu, sign_rule(B[:, :m]), var, scale


def fit_svd(x, m, whiten=True, eps=0.0):
    """(mean [D], basis [D, m], variance [m], scale [m] or None) from the SVD of the centred rows."""
    x = np.asarray(x, dtype=np.float64)
    n, d = x.shape
    mu = column_mean(x)
    _, s, vt = np.linalg.svd(x - mu, full_matrices=False)
    return _finish(mu, vt.T, s * s, n, d, m, whiten, eps)


def fit_gram(x, m, whiten=True, eps=0.0):
    """The same by Pca.fit's recipe: N <= D: eigh of (G + G^T) / 2, G = Xc Xc^T, and B = Xc^T U lam^-1/2 with columns
    rescaled to unit 2-norm; N > D: eigh of Xc^T Xc."""
    x = np.asarray(x, dtype=np.float64)
    n, d = x.shape
    mu = column_mean(x)
    xc = x - mu
    g = xc @ xc.T if n <= d else xc.T @ xc
    lam, u = np.linalg.eigh((g + g.T) / 2)
    lam, u = lam[::-1], u[:, ::-1]
    k = min(m, len(lam))
    if n <= d:
        with np.errstate(all="ignore"):
            B = xc.T @ (u[:, :k] / np.sqrt(lam[:k]))
            B = B / np.linalg.norm(B, axis=0)
    else:
        B = u[:, :k]
    return _finish(mu, B, lam, n, d, m, whiten, eps)


def yardstick_rows(n, d, seed=0):
    """Rows whose spectrum falls by about 2 x per component in sigma (4 x in variance): well separated directions, so
    the basis is well conditioned and route differences measure rounding alone."""
    rng = np.random.RandomState(seed)
    r = min(n, d)
    q, _ = np.linalg.qr(rng.standard_normal((d, r)))
    z, _ = np.linalg.qr(rng.standard_normal((n, r)))                   # orthogonal latent columns: clean ratios
    return (z * 2.0 ** -np.arange(r)) @ q.T + rng.standard_normal(d)[None, :]


def route_delta(a, b):
    """(delta_var, delta_vec) between two fits (mean, basis, variance, scale)."""
    return float(np.max(np.abs(a[2] - b[2]) / np.abs(b[2]))), float(np.max(np.abs(a[1] - b[1])))
