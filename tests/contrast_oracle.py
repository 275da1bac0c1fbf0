"""NumPy restatement of the local contrast normalisation defined in include/dlc.h (dlc_contrast_rows): fp64, every
operation rounded on its own, each cell's window summed left to right starting FROM its first element, so that every
comparison against the GPU is exact.

    a = max(0, j - radius), b = min(lim(r), j + radius + 1), cnt = b - a
    s = x_a + x_{a+1} + ... + x_{b-1};  mean = s / cnt
    q = (x_a - mean)^2 + ... + (x_{b-1} - mean)^2;  sd = sqrt(q / (cnt - 1))
    out[r][j] = 0.0 if cnt < 2 or sd == 0.0 else (x_j - mean) / sd

Vectorised over the cells: the loop runs over the window offset t = -radius .. radius, initialises every cell from its
first valid element and adds the later ones in order (NumPy's +, -, *, / and sqrt on float64 are the IEEE operations).
"""
import numpy as np

from sequence_oracle import limits


def window_sums(x, lim, radius, term=None):
    """(sum [rows, n], cnt [rows, n]) over every cell's window of term(x_c) (default x_c itself): left to right,
    initialised from the window's first element -- not from 0, which would turn a sum of -0.0 into +0.0.  x: fp64
    [rows, n]; lim: [rows] columns each row offers; cells at or past their row's limit have cnt 0."""
    rows, n = x.shape
    lim = np.asarray(lim, np.int64)[:, None]
    j = np.arange(n)[None, :]
    offered = j < lim
    acc = np.zeros((rows, n), np.float64)
    cnt = np.zeros((rows, n), np.int64)
    with np.errstate(all="ignore"):
        for t in range(-radius, radius + 1):
            c = j + t
            valid = offered & (c >= 0) & (c < lim)
            xc = np.zeros((rows, n), np.float64)
            lo, hi = max(0, -t), min(n, n - t)                     # cells whose column j + t exists at all
            if lo < hi:
                xc[:, lo:hi] = x[:, lo + t:hi + t]
            v = xc if term is None else term(xc)
            acc = np.where(valid, np.where(cnt == 0, v, acc + v), acc)
            cnt += valid
    return acc, cnt


def contrast_rows(matrix, radius, n=None, limit0=None, limit_step=0):
    """fp64 [rows, n]: the normalised rows; NaN where a cell is not offered (j >= lim(r))."""
    m = np.asarray(matrix)
    rows = m.shape[0]
    n = m.shape[1] if n is None else n
    x = m[:, :n].astype(np.float64)                                # fp32: exact; int64: round to nearest even
    lim = limits(rows, n, n if limit0 is None else limit0, limit_step)
    with np.errstate(all="ignore"):
        s, cnt = window_sums(x, lim, radius)
        mean = s / cnt.astype(np.float64)
        q, _ = window_sums(x, lim, radius, lambda xc: (xc - mean) * (xc - mean))
        sd = np.sqrt(q / (cnt - 1).astype(np.float64))
        out = np.where((cnt < 2) | (sd == 0.0), 0.0, (x - mean) / sd)
    out[cnt == 0] = np.nan
    return out


def confuser_band_scene(seed=0, frames=200, dim=64):
    """int8 descriptors [frames, dim] of a route with a planted revisit behind a confuser band: frames 150..179 are copies
    of frames 20..49 with 28 bytes redrawn (the revisit), and 40 columns -- the same 40 everywhere -- of frames 70..109 (the
    band: a stretch that resembles whoever shares those columns) and of frames 150..179 hold one template row's bytes.
    Every revisiting frame is then nearer to EVERY band frame than to the frame it revisits.  Returns (descriptors, the
    frame each of 150..179 revisits)."""
    rng = np.random.RandomState(seed)
    x = rng.randint(-128, 128, size=(frames, dim)).astype(np.int8)
    for i in range(30):
        at = rng.permutation(dim)[:28]
        x[150 + i] = x[20 + i]
        x[150 + i, at] = rng.randint(-128, 128, size=28).astype(np.int8)
    template = rng.randint(-128, 128, size=dim).astype(np.int8)
    cols = rng.permutation(dim)[:40]
    for f in list(range(70, 110)) + list(range(150, 180)):
        x[f, cols] = template[cols]
    return x, np.arange(20, 50)
