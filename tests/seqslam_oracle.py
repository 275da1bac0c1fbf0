"""NumPy restatement of the two SeqSLAM front-end definitions of include/dlc.h: dlc_seqslam_describe_u8 (integer area
resize as two weight matrices, patch normalisation as a loop over the tiles) and dlc_sad_u8_rows (np.abs of an int64
difference, summed).  Written from the header's text, not from the kernels: no tiling, no lane groups, no shortcuts."""
import numpy as np


def area_weights(n_out, n_in):
    """int64 [n_out, n_in]: w(y, i) = max(0, min((i + 1) n_out, (y + 1) n_in) - max(i n_out, y n_in))."""
    y = np.arange(n_out, dtype=np.int64)[:, None]
    i = np.arange(n_in, dtype=np.int64)[None, :]
    return np.maximum(0, np.minimum((i + 1) * n_out, (y + 1) * n_in) - np.maximum(i * n_out, y * n_in))


def resize(gray, h, w):
    """gray uint8 [..., H, W] -> int64 [..., h, w]: floor((2 sum wy wx gray + H W) / (2 H W))."""
    gray = np.asarray(gray)
    hh, ww = gray.shape[-2:]
    wy, wx = area_weights(h, hh), area_weights(w, ww)
    total = wy @ gray.astype(np.int64) @ wx.T
    return (2 * total + hh * ww) // (2 * hh * ww)


def normalise(thumb, patch, strength):
    """thumb int64 [h, w] (values 0..255) -> uint8 [h, w]: per tile 128 + strength (T - mean) / sample std, the header's
    three fp64 operations per cell, rint to nearest even, clamped."""
    h, w = thumb.shape
    out = np.empty((h, w), dtype=np.uint8)
    for y0 in range(0, h, patch):
        for x0 in range(0, w, patch):
            tile = thumb[y0:y0 + patch, x0:x0 + patch].astype(np.int64)
            c = tile.size
            s, t = int(tile.sum()), int((tile * tile).sum())
            qv = c * t - s * s
            if c < 2 or qv == 0:
                out[y0:y0 + patch, x0:x0 + patch] = 128
                continue
            u = (c * tile - s).astype(np.float64)
            v = np.sqrt(np.float64(c - 1) / (np.float64(c) * np.float64(qv)))
            z = np.rint((np.float64(strength) * u) * v)
            out[y0:y0 + patch, x0:x0 + patch] = np.clip(128.0 + z, 0.0, 255.0).astype(np.uint8)
    return out


def describe(gray, size, patch, strength):
    """gray uint8 [F, H, W] -> uint8 [F, h * w]."""
    gray = np.asarray(gray)
    assert gray.dtype == np.uint8 and gray.ndim == 3
    h, w = size
    thumbs = resize(gray, h, w)
    return np.stack([normalise(t, patch, strength).reshape(-1) for t in thumbs]) if len(thumbs) else \
        np.empty((0, h * w), np.uint8)


def sad_rows(q, db):
    """int64 [Q, N]: sum_p |q_r[p] - db_j[p]| on unsigned bytes."""
    q, db = np.asarray(q), np.asarray(db)
    assert q.dtype == np.uint8 and db.dtype == np.uint8
    out = np.empty((q.shape[0], db.shape[0]), dtype=np.int64)
    for r in range(q.shape[0]):
        out[r] = np.abs(q[r].astype(np.int64)[None, :] - db.astype(np.int64)).sum(axis=1)
    return out


def offered(q, n, limit0, limit_step):
    """bool [q, n]: j < clamp(limit0 + r * limit_step, 0, n)."""
    lim = np.clip(limit0 + limit_step * np.arange(q, dtype=np.int64), 0, n)
    return np.arange(n)[None, :] < lim[:, None]
