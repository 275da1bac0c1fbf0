"""The NumPy models of tests/cnn_pieces_oracle.py against what the project already trusts (oracle.cnn_vtl), on the CPU:
the GPU tests of csrc/cnnvtl.hip compare bits with these models, so the models are checked first."""
import numpy as np
import pytest

import cnn_pieces_oracle as P
from oracle import cnn_vtl as ocnn


@pytest.mark.parametrize("case", P.IM2COL_CASES, ids=[P.case_id(c) for c in P.IM2COL_CASES])
def test_im2col_model_times_kernel_is_the_oracle_convolution(case):
    """im2col(x) @ w.reshape(K, cout) + b == oracle.cnn_vtl.conv2d_nhwc, non-square kernels included (which also shows
    that the oracle's convolution handles kh != kw)."""
    n, h, w, c, kh, kw, stride, padding = case
    rng = np.random.RandomState(kh * 100 + kw * 10 + c)
    x = rng.standard_normal((n, h, w, c))
    cout = 4
    wk = rng.standard_normal((kh, kw, c, cout)) / np.sqrt(kh * kw * c)
    b = rng.standard_normal(cout)
    oh, ow, ph, pw = P.conv_geometry(h, w, kh, kw, stride, padding)
    cols = P.im2col(x, kh, kw, stride, ph, pw, oh, ow)
    assert cols.shape == (n * oh * ow, kh * kw * c)
    for relu in (False, True):
        y = cols @ wk.reshape(-1, cout) + b
        if relu:
            y = np.maximum(y, 0.0)
        ref = ocnn.conv2d_nhwc(x, wk, b, stride, padding, relu)
        assert ref.shape == (n, oh, ow, cout)
        assert np.abs(y.reshape(ref.shape) - ref).max() < 1e-10


def test_im2col_model_places_every_tap():
    """A 2x3 kernel over an image whose cell values name their own coordinates: every column is read off by hand."""
    h, w, c = 4, 5, 2
    x = np.zeros((1, h, w, c))
    for iy in range(h):
        for ix in range(w):
            for ch in range(c):
                x[0, iy, ix, ch] = 100 * iy + 10 * ix + ch + 1000
    cols = P.im2col(x, 2, 3, 2, 0, 1, 2, 3).reshape(2, 3, 2, 3, 2)
    for oy in range(2):
        for ox in range(3):
            for ky in range(2):
                for kx in range(3):
                    iy, ix = oy * 2 + ky, ox * 2 - 1 + kx
                    for ch in range(c):
                        want = 1000 + 100 * iy + 10 * ix + ch if 0 <= iy < h and 0 <= ix < w else 0.0
                        assert cols[oy, ox, ky, kx, ch] == want


def test_space_to_depth_model_is_the_definition():
    rng = np.random.RandomState(1)
    for (n, h, w, c, s) in ((2, 6, 9, 3, 3), (1, 8, 4, 5, 4), (3, 4, 6, 1, 2), (1, 3, 5, 2, 1)):
        x = rng.standard_normal((n, h, w, c))
        y = P.space_to_depth(x, s)
        assert y.shape == (n, h // s, w // s, s * s * c)
        for _ in range(50):
            i, yy, xx = rng.randint(n), rng.randint(h // s), rng.randint(w // s)
            dy, dx, ch = rng.randint(s), rng.randint(s), rng.randint(c)
            assert y[i, yy, xx, (dy * s + dx) * c + ch] == x[i, yy * s + dy, xx * s + dx, ch]
        if s == 1:
            assert np.array_equal(y, x)


@pytest.mark.parametrize("widths", [(300,), (1, 130), (5, 1, 17, 40, 3, 64, 2, 9)])
def test_quantize_gather_model_equals_the_oracle_on_finite_rows(widths):
    segs = P.quant_rows(widths)
    d = np.concatenate(segs, axis=1)
    assert np.isfinite(d).all() and (d.max(axis=1) > d.min(axis=1)).all()
    cols = P.edge_columns(segs, 100)
    assert np.array_equal(P.quantize_gather(segs, cols), ocnn.quantize_int8(d)[:, cols])
    every = np.arange(d.shape[1])                                    # every column, three rows
    assert np.array_equal(P.quantize_gather([s[:3] for s in segs], every), ocnn.quantize_int8(d[:3]))


def test_quantize_gather_model_edges():
    """What include/dlc.h states for the inputs the oracle leaves undefined."""
    row = np.array([[3.0, 1.0, 2.0, 1.0]])
    assert P.quantize_gather([row], [0, 1, 2, -1, 4, 3]).view(np.uint8).tolist() == [[255, 0, 127, 0, 0, 0]]
    assert P.quantize_gather([np.full((1, 5), 7.5)], [0, 4]).tolist() == [[0, 0]]                       # constant row
    assert P.quantize_gather([np.array([[np.nan, 0.0, 4.0, 1.0]])], [0, 1, 2, 3]).view(np.uint8).tolist() == [[0, 0, 255, 63]]
    assert P.quantize_gather([np.full((1, 3), np.nan)], [0, 1, 2]).tolist() == [[0, 0, 0]]
    assert P.quantize_gather([np.array([[-1e308, 0.0, 1e308]])], [0, 1, 2]).tolist() == [[0, 0, 0]]    # spread overflows
    assert P.quantize_gather([np.array([[0.0, 5e-324, 1e-323]])], [0, 1, 2]).tolist() == [[0, 0, 0]]    # 255 / spread = inf
    assert P.quantize_gather([np.array([[1.0, np.inf, 2.0]])], [0, 1, 2]).tolist() == [[0, 0, 0]]
    assert P.quantize_gather([np.array([[-0.0, 0.0, 2.0]])], [0, 1, 2]).view(np.uint8).tolist() == [[0, 0, 255]]


def test_seeded_rows_reach_both_top_bytes():
    """(max - min) * (255 / (max - min)) is 255 for some (min, max) and rounds below it -- byte 254 -- for others: the
    rows of the GPU test hold both, so the operation order of the kernel decides bytes that the test compares."""
    for widths, n in [(w, P.QUANT_ROWS) for w in P.QUANT_WIDTHS] + [((1, 70001), 5), ((1, 36), 2049)]:
        tops = [P.max_cell_byte(row) for row in np.concatenate(P.quant_rows(widths, n=n), axis=1)]
        assert set(tops) <= {254, 255}
        assert tops.count(254) >= 1 and tops.count(255) >= 1, widths
    tops = [P.max_cell_byte(row) for row in np.concatenate(P.quant_rows((1, 130)), axis=1)]
    # and the other operation order, (d - min) * 255 / (max - min), disagrees on those rows
    d = np.concatenate(P.quant_rows((1, 130)), axis=1)
    mn, mx = d.min(axis=1), d.max(axis=1)
    other = np.trunc((mx - mn) * 255.0 / (mx - mn)).astype(np.int64)
    assert (other != np.array(tops)).any()


def test_fp32_patch_table_has_one_value_per_byte():
    """v / 255 in fp32 == the fp64 quotient rounded to fp32, for every byte: the fp32 output of dlc_extract_patches has
    one possible value per pixel whichever way the table is computed."""
    for v in range(256):
        assert np.float32(v) / np.float32(255) == np.float32(v / 255.0)
