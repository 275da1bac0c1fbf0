"""Plain NumPy models of the exact kernels around the fp64 CnnVtl GEMMs (csrc/cnnvtl.hip): im2col, space-to-depth and
the quantise + gather, written from the definitions in include/dlc.h with explicit loops, and the shapes and rows the
CPU and GPU tests share.  Test infrastructure only; tests/test_cnn_pieces_cpu.py ties the models to oracle.cnn_vtl."""
import numpy as np

from oracle import cnn_vtl as ocnn


# ---- models ---------------------------------------------------------------------------------------------------------
def im2col(x, kh, kw, stride, pad_top, pad_left, oh, ow):
    """x [n, h, w, c] -> cols [n*oh*ow, kh*kw*c], column order (ky, kx, ch), zeros outside the image."""
    x = np.asarray(x, dtype=np.float64)
    n, h, w, c = x.shape
    cols = np.zeros((n, oh, ow, kh, kw, c), dtype=np.float64)
    for oy in range(oh):
        for ox in range(ow):
            for ky in range(kh):
                iy = oy * stride - pad_top + ky
                if iy < 0 or iy >= h:
                    continue
                for kx in range(kw):
                    ix = ox * stride - pad_left + kx
                    if ix < 0 or ix >= w:
                        continue
                    cols[:, oy, ox, ky, kx, :] = x[:, iy, ix, :]
    return cols.reshape(n * oh * ow, kh * kw * c)


def space_to_depth(x, s):
    """y[n, Y, X, (dy*s + dx)*c + ch] = x[n, Y*s + dy, X*s + dx, ch] (include/dlc.h, dlc_space_to_depth_nhwc_f64)."""
    x = np.asarray(x)
    n, h, w, c = x.shape
    assert h % s == 0 and w % s == 0
    y = np.empty((n, h // s, w // s, s * s * c), dtype=x.dtype)
    for dy in range(s):
        for dx in range(s):
            for ch in range(c):
                y[:, :, :, (dy * s + dx) * c + ch] = x[:, dy::s, dx::s, ch]
    return y


def quantize_gather(segs, cols):
    """dlc_minmax_quant_gather_i8: segs is a list of [n, width_g] fp64 arrays, cols int64 indices into the concatenated
    row -> int8 [n, len(cols)].  Min and max over the non-NaN cells; (d - min) * (255 / (max - min)); byte 0 where that is
    NaN or |.| >= 9e18, else truncated toward zero and wrapped modulo 256; byte 0 for an index outside [0, width)."""
    d = np.concatenate([np.asarray(s, dtype=np.float64).reshape(len(segs[0]), -1) for s in segs], axis=1)
    cols = np.asarray(cols, dtype=np.int64)
    n, width = d.shape
    out = np.zeros((n, len(cols)), dtype=np.uint8)
    inside = (cols >= 0) & (cols < width)
    with np.errstate(all="ignore"):
        for r in range(n):
            mn = np.fmin.reduce(d[r])
            mx = np.fmax.reduce(d[r])
            scale = np.float64(255) / (mx - mn)
            for j in np.flatnonzero(inside):
                scaled = (d[r, cols[j]] - mn) * scale
                if np.isnan(scaled) or abs(scaled) >= 9e18:
                    continue
                out[r, j] = int(np.trunc(scaled)) & 0xFF
    return out.view(np.int8)


def max_cell_byte(row):
    """The byte of a finite row's own maximum cell, as an unsigned value (255, or 254 when the product rounds below)."""
    row = np.asarray(row, dtype=np.float64)
    return int(quantize_gather([row[None, :]], [int(np.argmax(row))])[0, 0]) & 0xFF


# ---- shared shapes --------------------------------------------------------------------------------------------------
# (n, h, w, c, kh, kw, stride, padding): K = kh*kw*c below 256, exactly 256, 261 and 363; kh != kw both ways; h != w;
# strides 1, 2, 3, 4 and one larger than the kernel; SAME with pad_top != pad_left and the extra pad after; VALID; n 1 / 3
IM2COL_CASES = (
    (1, 9, 14, 3, 1, 5, 1, "SAME"),          # K 15: pads 0 / 2
    (3, 13, 8, 5, 5, 1, 2, "SAME"),          # K 25: 5x1, stride 2
    (1, 17, 21, 4, 3, 7, 1, "SAME"),         # K 84: pads 1 / 3
    (1, 18, 21, 6, 3, 7, 2, "SAME"),         # K 126: pad 1 along h goes after (top 0), 3 left
    (3, 13, 14, 7, 2, 3, 4, "SAME"),         # K 42: stride one larger than the kernel, extra pad after on both axes
    (3, 16, 11, 16, 2, 8, 1, "VALID"),       # K 256 exactly
    (1, 14, 12, 29, 3, 3, 3, "SAME"),        # K 261, stride 3
    (1, 11, 10, 29, 1, 9, 1, "SAME"),        # K 261, 1x9: pads 0 / 4
    (3, 35, 43, 3, 11, 11, 4, "VALID"),      # K 363 (conv1's kernel), stride 4
    (1, 10, 13, 2, 2, 3, 1, "VALID"),
    (3, 9, 12, 5, 5, 1, 1, "VALID"),
    (1, 20, 17, 3, 2, 3, 2, "SAME"),         # pads 0 / 1
    (3, 15, 10, 3, 1, 5, 6, "SAME"),         # stride one larger than 1x5
    (1, 12, 16, 3, 4, 2, 1, "SAME"),         # pads 3 / 1: 1 above and 2 below, 0 left and 1 right
    (3, 40, 33, 3, 3, 7, 1, "SAME"),         # 3960 output pixels
)


def conv_geometry(h, w, kh, kw, stride, padding):
    """(oh, ow, pad_top, pad_left) by TensorFlow's rule (oracle.cnn_vtl._out_size)."""
    oh, ph = ocnn._out_size(h, kh, stride, padding)
    ow, pw = ocnn._out_size(w, kw, stride, padding)
    return oh, ow, ph, pw


def case_id(case):
    return "x".join(str(v) for v in case)


# ---- shared rows for the quantiser ----------------------------------------------------------------------------------
QUANT_SEED = 20
QUANT_ROWS = 24
QUANT_WIDTHS = ((300,), (1, 130), (5, 1, 17, 40, 3, 64, 2, 9))     # 1, 2 and 8 segments of unequal width


def quant_rows(widths, n=QUANT_ROWS, seed=QUANT_SEED):
    """n seeded finite rows with max > min, cut into segments of the given widths: a list of [n, width_g] arrays.
    Spread and offset differ from row to row, so that the top byte is 254 for some rows and 255 for others."""
    rng = np.random.RandomState(seed)
    total = int(np.sum(widths))
    d = rng.standard_normal((n, total)) * rng.uniform(0.01, 300.0, size=(n, 1)) + rng.uniform(-50.0, 50.0, size=(n, 1))
    edges = np.concatenate([[0], np.cumsum(widths)])
    return [np.ascontiguousarray(d[:, edges[g]:edges[g + 1]]) for g in range(len(widths))]


def edge_columns(segs, n_cols, seed=QUANT_SEED):
    """n_cols indices, unsorted, with duplicates: every row's argmin and argmax, the first and last column of every
    segment, then seeded draws and one repeat of the first.  (Rows with NaN: the extremes of their non-NaN cells.)"""
    d = np.concatenate(segs, axis=1)
    rng = np.random.RandomState(seed + 1)
    must = []
    for row in d:
        if not np.isnan(row).all():
            must += [int(np.nanargmin(row)), int(np.nanargmax(row))]
    start = 0
    for s in segs:
        must += [start, start + s.shape[1] - 1]
        start += s.shape[1]
    must = list(dict.fromkeys(must))
    assert n_cols > len(must), "n_cols %d cannot hold the %d mandatory columns and a duplicate" % (n_cols, len(must))
    fill = rng.randint(0, d.shape[1], size=n_cols - len(must))
    cols = np.concatenate([np.array(must, dtype=np.int64), fill.astype(np.int64)])
    cols[-1] = cols[0]
    return cols[rng.permutation(n_cols)]
