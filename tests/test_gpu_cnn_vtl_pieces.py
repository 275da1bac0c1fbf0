"""The exact kernels around the GEMMs of the fp64 CnnVtl route (csrc/cnnvtl.hip; the implicit-GEMM gather of
dlc_conv2d_nhwc_f64 in csrc/gemm_dense.hip and csrc/gemm_dma_f64.hip), at the edges no other test enters: non-square
kernels on every loader route, grid-stride launches past their workgroup cap, the quantiser's top byte, segment
boundaries, out-of-range columns and non-finite rows.

im2col, max-pool, space-to-depth and the quantise + gather are copies, order-independent min / max or one rounding per
element: they are compared with == against the plain NumPy models of tests/cnn_pieces_oracle.py (tied to oracle.cnn_vtl
by tests/test_cnn_pieces_cpu.py) and oracle.cnn_vtl.maxpool3x3s2.  Only the convolution against the NumPy oracle keeps
the project's 1e-10; against im2col + GEMM on the GPU it is torch.equal."""
import ctypes as C

import numpy as np
import pytest
import torch

import cnn_pieces_oracle as P
from oracle import cnn_vtl as ocnn

pytestmark = pytest.mark.gpu

OK, BAD_ARG, BAD_SHAPE = 0, -1, -2


@pytest.fixture(scope="module")
def eng():
    import deeploopcloser_amd as d
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return d.default_engine()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda")


def same(what, got, want):
    """got == want, elementwise and in shape; the message says where they part."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, "%s: shape %s, expected %s" % (what, got.shape, want.shape)
    bad = ~((got == want) | ((got != got) & (want != want)))
    if bad.any():
        at = tuple(int(v) for v in np.argwhere(bad)[0])
        raise AssertionError("%s: %d of %d differ, first at %s: got %r, expected %r" % (what, int(bad.sum()), bad.size, at, got[at], want[at]))


# ---- im2col ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", P.IM2COL_CASES, ids=[P.case_id(c) for c in P.IM2COL_CASES])
def test_im2col_equals_the_model(eng, case):
    n, h, w, c, kh, kw, stride, padding = case
    rng = np.random.RandomState(kh * 100 + kw * 10 + c)
    x = rng.standard_normal((n, h, w, c))
    oh, ow, ph, pw = P.conv_geometry(h, w, kh, kw, stride, padding)
    got = eng.im2col(dev(x), kh, kw, stride, ph, pw, oh, ow)
    same("im2col %s" % (case,), got.cpu().numpy(), P.im2col(x, kh, kw, stride, ph, pw, oh, ow))


# ---- conv2d with non-square kernels on each loader route (the rule of include/dlc.h, dlc_conv2d_nhwc_f64) ------------
# (route, n, h, w, c, kh, kw, cout, stride, padding, relu)
CONV_CASES = (
    ("lds-dma", 8, 24, 23, 16, 3, 5, 40, 1, "SAME", True),            # c % 16 == 0, 4416 output pixels: 18 tiles of 256 x 96
    ("lds-dma", 20, 31, 33, 32, 5, 2, 130, 2, "VALID", False),        # 4480 output pixels, two column tiles
    ("registers", 2, 11, 13, 8, 2, 3, 6, 1, "SAME", True),            # c % 8 == 0, c % 16 != 0
    ("registers", 3, 17, 12, 24, 5, 1, 10, 2, "VALID", False),
    ("registers", 1, 9, 10, 16, 1, 5, 12, 1, "SAME", False),          # c % 16 == 0 but one tile: too small for the DMA form
    ("element-wise", 2, 15, 19, 3, 3, 7, 9, 2, "SAME", True),
    ("element-wise", 3, 12, 9, 5, 5, 1, 7, 1, "VALID", False),
    ("element-wise", 1, 14, 11, 5, 2, 3, 4, 1, "SAME", True),
)


@pytest.mark.parametrize("case", CONV_CASES, ids=["%s-%s" % (c[0], P.case_id(c[1:])) for c in CONV_CASES])
def test_conv2d_non_square_kernels(eng, case):
    _, n, h, w, c, kh, kw, cout, stride, padding, relu = case
    rng = np.random.RandomState(n * 1000 + c * 10 + kh)
    x = rng.standard_normal((n, h, w, c))
    wk = rng.standard_normal((kh, kw, c, cout)) / np.sqrt(kh * kw * c)
    b = rng.standard_normal(cout)
    oh, ow, ph, pw = P.conv_geometry(h, w, kh, kw, stride, padding)
    act = 2 if relu else 0
    xd, wd, bd = dev(x), dev(wk.reshape(-1, cout)), dev(b)
    got = eng.conv2d(xd, wd, bd, kh, kw, stride, ph, pw, oh, ow, act)
    ref = ocnn.conv2d_nhwc(x, wk, b, stride, padding, relu)
    assert tuple(got.shape) == ref.shape
    err = float(np.abs(got.cpu().numpy() - ref).max())
    print("conv2d %s: max |gpu - oracle| = %.3g" % (case, err))
    assert err < 1e-10
    cols = eng.im2col(xd, kh, kw, stride, ph, pw, oh, ow)
    alt = eng.gemm_bias_act(cols, wd, bd, act=act).reshape(got.shape)
    assert torch.equal(alt, got)
    # the per-frame range folded on the way == the range of the output
    keys = eng.frame_minmax_keys(n)
    again = eng.conv2d(xd, wd, bd, kh, kw, stride, ph, pw, oh, ow, act, frame_keys=keys)
    assert torch.equal(again, got)
    pick = torch.from_numpy(np.random.RandomState(3).permutation(got[0].numel())[:200].astype(np.int64)).to(eng.device)
    from_keys = eng.quant_gather([got], pick, keys)
    assert torch.equal(from_keys, eng.minmax_quant_gather([got], pick))
    same("bytes of conv2d %s" % (case,), from_keys.cpu().numpy(), P.quantize_gather([got.reshape(n, -1).cpu().numpy()], pick.cpu().numpy()))


# ---- max-pool -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [1, 5, 64])
@pytest.mark.parametrize("hw", [(3, 3), (4, 4), (8, 6), (7, 10), (23, 31)], ids=lambda v: "%dx%d" % v)
def test_maxpool_equals_the_oracle(eng, hw, c):
    h, w = hw
    rng = np.random.RandomState(h * 100 + w + c)
    negative = -rng.uniform(1.0, 255.0, size=(2, h, w, c))
    mixed = rng.standard_normal((2, h, w, c))
    holes = rng.standard_normal((2, h, w, c))
    holes[rng.uniform(size=holes.shape) < 0.3] = -np.inf
    holes[0, 0:3, 0:3, :] = -np.inf                                  # a whole window of -inf
    for name, x in (("negative", negative), ("mixed", mixed), ("-inf cells", holes)):
        want = ocnn.maxpool3x3s2(x)
        assert want.shape == (2, (h - 3) // 2 + 1, (w - 3) // 2 + 1, c)
        same("maxpool %s %s c %d" % (name, hw, c), eng.maxpool3x3s2(dev(x)).cpu().numpy(), want)
    assert np.isneginf(ocnn.maxpool3x3s2(holes)[0, 0, 0]).all() and (ocnn.maxpool3x3s2(negative) < 0).all()


def test_maxpool_past_the_workgroup_cap(eng):
    """More outputs than 16384 workgroups x 256 threads hold: the grid-stride loop goes round."""
    shape = (9, 131, 131, 112)
    g = torch.Generator(device=eng.device)
    g.manual_seed(5)
    x = torch.randint(-1000, 1000, shape, generator=g, device=eng.device).to(torch.float64)
    got = eng.maxpool3x3s2(x)
    assert got.numel() > 16384 * 256
    want = ocnn.maxpool3x3s2(x.cpu().numpy())
    assert np.array_equal(got.cpu().numpy(), want)


# ---- space-to-depth -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", [1, 3, 5])
@pytest.mark.parametrize("s", [1, 2, 3, 4])
def test_space_to_depth_equals_the_model(eng, s, c):
    rng = np.random.RandomState(10 * s + c)
    for (n, h, w) in ((2, 3 * s, 5 * s), (1, 7 * s, 2 * s), (3, s, s)):
        x = rng.standard_normal((n, h, w, c))
        same("space_to_depth %s" % ((n, h, w, c, s),), eng.space_to_depth(dev(x), s).cpu().numpy(), P.space_to_depth(x, s))


def test_space_to_depth_past_the_workgroup_cap(eng):
    shape, s = (1, 1024, 1032, 4), 4
    assert int(np.prod(shape)) > 16384 * 256
    x = np.arange(int(np.prod(shape)), dtype=np.float64).reshape(shape)          # every cell names itself
    got = eng.space_to_depth(dev(x), s)
    assert np.array_equal(got.cpu().numpy(), P.space_to_depth(x, s))


# ---- quantise + gather ----------------------------------------------------------------------------------------------
def fold_keys(eng, segs):
    """Per-row keys as the encoder gets them: initialised, then every segment folded in by the convolution that made
    it -- here a 1x1 convolution with kernel 1 and bias 0 over the segment as a [n, 1, width, 1] image.  Returns the keys
    and the convolutions' outputs (the segments themselves, up to the sign of a zero)."""
    n = segs[0].shape[0]
    keys = eng.frame_minmax_keys(n)
    one = torch.ones((1, 1), dtype=torch.float64, device=eng.device)
    zero = torch.zeros((1,), dtype=torch.float64, device=eng.device)
    outs = []
    for s in segs:
        width = s.shape[1]
        y = eng.conv2d(s.reshape(n, 1, width, 1), one, zero, 1, 1, 1, 0, 0, 1, width, 0, frame_keys=keys)
        outs.append(y.reshape(n, width))
    return keys, outs


def check_both_forms(eng, what, segs_np, cols_np):
    """minmax_quant_gather and init-keys / fold / quant_gather against the model; returns the bytes."""
    segs = [dev(s) for s in segs_np]
    cols = dev(np.asarray(cols_np, dtype=np.int64))
    want = P.quantize_gather(segs_np, cols_np)
    one_call = eng.minmax_quant_gather(segs, cols).cpu().numpy()
    same("%s, minmax_quant_gather" % what, one_call, want)
    keys, outs = fold_keys(eng, segs)
    from_keys = eng.quant_gather(outs, cols, keys).cpu().numpy()
    same("%s, quant_gather from folded keys" % what, from_keys, P.quantize_gather([o.cpu().numpy() for o in outs], cols_np))
    same("%s, the two forms" % what, from_keys, one_call)
    return one_call


@pytest.mark.parametrize("n_cols", [256, 257])
@pytest.mark.parametrize("widths", P.QUANT_WIDTHS, ids=lambda w: "%d-segments" % len(w))
def test_quantiser_top_byte_and_segment_boundaries(eng, widths, n_cols):
    segs = P.quant_rows(widths)
    d = np.concatenate(segs, axis=1)
    tops = [P.max_cell_byte(row) for row in d]
    assert 254 in tops and 255 in tops                               # the operation order decides bytes compared below
    cols = P.edge_columns(segs, n_cols)
    assert len(cols) == n_cols and len(set(cols.tolist())) < n_cols and (np.diff(cols) < 0).any()
    for row in d:
        assert int(np.argmin(row)) in cols and int(np.argmax(row)) in cols
    got = check_both_forms(eng, "%d segments, %d columns" % (len(widths), n_cols), segs, cols)
    for r, row in enumerate(d):                                       # the bytes of the extremes, read off the result
        assert got[r, cols.tolist().index(int(np.argmin(row)))] == 0
        assert int(got[r, cols.tolist().index(int(np.argmax(row)))]) & 0xFF == tops[r]
    # the identity convolution that folds the keys returns the segment
    keys, outs = fold_keys(eng, [dev(s) for s in segs])
    for s, o in zip(segs, outs):
        assert np.array_equal(o.cpu().numpy(), s)


def test_quantiser_one_row_one_column(eng):
    segs = [s[:1] for s in P.quant_rows((1, 130))]
    row = np.concatenate(segs, axis=1)[0]
    for col in (int(np.argmax(row)), int(np.argmin(row)), 0, 130):
        check_both_forms(eng, "one row, column %d" % col, segs, np.array([col], dtype=np.int64))


def test_quantiser_few_very_wide_rows(eng):
    """5 rows of more than 16 x 4096 cells: every row is cut into slices that meet in the key atomics."""
    widths = (1, 70001)
    assert sum(widths) > 16 * 4096
    segs = P.quant_rows(widths, n=5)
    tops = [P.max_cell_byte(row) for row in np.concatenate(segs, axis=1)]
    assert 254 in tops and 255 in tops
    check_both_forms(eng, "5 wide rows", segs, P.edge_columns(segs, 257))


def test_quantiser_many_rows_one_slice(eng):
    """2049 rows: above 2048 rows a row is one slice."""
    segs = P.quant_rows((1, 36), n=2049)
    every = np.arange(37, dtype=np.int64)
    cols = np.concatenate([every, every[:11]])[np.random.RandomState(2).permutation(48)]      # every column, duplicates
    check_both_forms(eng, "2049 rows", segs, cols)


def special_rows(widths):
    rng = np.random.RandomState(77)
    width = int(np.sum(widths))
    base = lambda: rng.standard_normal(width) * 3.0
    rows = {}
    rows["constant"] = np.full(width, 7.5)
    r = rng.uniform(-1.0, 1.0, width) * 1e308; r[3], r[width - 2] = -1e308, 1e308
    rows["spread overflows"] = r
    rows["subnormal spread"] = rng.permutation(width).astype(np.float64) * 5e-324
    rows["tiny normal spread"] = rng.uniform(0.0, 1.0, width) * 2.0 ** -1000
    r = base(); r[5] = np.inf
    rows["+inf"] = r
    r = base(); r[width - 1] = -np.inf
    rows["-inf"] = r
    r = base(); r[0], r[9] = np.inf, -np.inf
    rows["both infinities"] = r
    r = base(); r[[1, 7, 8, width - 1]] = np.nan
    rows["some NaN"] = r
    rows["all NaN"] = np.full(width, np.nan)
    r = np.abs(base()); r[[2, 11]] = -0.0; r[[4, 12]] = 0.0
    rows["-0.0 and +0.0 minimum"] = r
    r = base(); r[6], r[10] = np.nan, np.inf
    rows["NaN and +inf"] = r
    rows["plain"] = base()
    names = list(rows)
    d = np.stack([rows[k] for k in names])
    edges = np.concatenate([[0], np.cumsum(widths)])
    return names, [np.ascontiguousarray(d[:, edges[g]:edges[g + 1]]) for g in range(len(widths))]


def test_quantiser_constant_overflowing_and_non_finite_rows(eng):
    """What include/dlc.h states: min and max over the non-NaN cells; a cell whose scaled value is NaN or beyond
    +-9e18 writes 0, so constant rows, rows with an infinity and rows whose spread overflows 255 / (max - min) or its
    product are all zeros."""
    widths = (7, 1, 92)
    names, segs = special_rows(widths)
    every = np.arange(100, dtype=np.int64)
    cols = np.concatenate([every, every[::4]])[np.random.RandomState(4).permutation(125)]
    got = check_both_forms(eng, "special rows", segs, cols).view(np.uint8)
    for name in ("constant", "spread overflows", "subnormal spread", "+inf", "-inf", "both infinities", "all NaN", "NaN and +inf"):
        assert not got[names.index(name)].any(), name
    d = np.concatenate(segs, axis=1)
    for name in ("tiny normal spread", "some NaN", "-0.0 and +0.0 minimum", "plain"):
        r = names.index(name)
        assert got[r].max() >= 254 and got[r].min() == 0, name
        assert not got[r, np.isnan(d[r, cols])].any()


def raw_quant(eng, ptrs, sizes, n_segs, n, cols, n_cols, minmax, out_ptr, keys=None):
    p = (C.c_void_p * len(ptrs))(*ptrs)
    z = (C.c_int64 * len(sizes))(*sizes)
    if keys is None:
        return eng.lib.dlc_minmax_quant_gather_i8(eng.ctx, p, z, n_segs, n, C.c_void_p(cols.data_ptr()), n_cols,
                                                  C.c_void_p(minmax.data_ptr()), C.c_void_p(out_ptr), eng._stream())
    return eng.lib.dlc_quant_gather_i8(eng.ctx, p, z, n_segs, n, C.c_void_p(cols.data_ptr()), n_cols, C.c_void_p(keys.data_ptr()),
                                       C.c_void_p(minmax.data_ptr()), C.c_void_p(out_ptr), eng._stream())


def test_quantiser_out_of_range_columns_write_zero(eng):
    """Column indices -1 and width give byte 0; every other byte is the model's and nothing outside the [n, n_cols]
    view of a larger, sentinel-filled buffer is touched."""
    segs_np = [s[:6] for s in P.quant_rows((5, 1, 17))]
    width, n = 23, 6
    cols_np = np.array([4, -1, 5, 22, width, 0, -1, 21, width, 6, 2 ** 40, -2 ** 40], dtype=np.int64)
    want = P.quantize_gather(segs_np, cols_np)
    assert not want[:, [1, 4, 6, 8, 10, 11]].any() and want[:, [0, 2, 3, 5, 7, 9]].any(axis=0).all()
    segs, cols = [dev(s) for s in segs_np], dev(cols_np)
    guard, nbytes = 64, n * len(cols_np)
    for use_keys in (False, True):
        buf = torch.full((guard + nbytes + guard,), 0x55, dtype=torch.int8, device=eng.device)
        minmax = torch.empty((n, 2), dtype=torch.float64, device=eng.device)
        keys = fold_keys(eng, segs)[0] if use_keys else None
        rc = raw_quant(eng, [s.data_ptr() for s in segs], [s.shape[1] for s in segs], 3, n, cols, len(cols_np), minmax,
                       buf.data_ptr() + guard, keys)
        assert rc == OK
        host = buf.cpu().numpy()
        assert (host[:guard] == 0x55).all() and (host[guard + nbytes:] == 0x55).all()
        same("out-of-range columns", host[guard:guard + nbytes].reshape(n, -1), want)


def test_quantiser_refusals_write_nothing(eng):
    n, w = 4, 10
    seg = dev(np.random.RandomState(1).standard_normal((65536, w)))
    cols = dev(np.arange(w, dtype=np.int64))
    keys = eng.frame_minmax_keys(65536)
    keys_before = keys.clone()
    p = seg.data_ptr()
    cases = (
        ("9 segments", [p] * 9, [1] * 9, 9, n, BAD_ARG),
        ("a NULL segment", [p, None], [5, 5], 2, n, BAD_ARG),
        ("an empty segment", [p, p], [5, 0], 2, n, BAD_ARG),
        ("no segment", [p], [w], 0, n, BAD_ARG),
        ("65536 rows", [p], [w], 1, 65536, BAD_SHAPE),
    )
    for use_keys in (False, True):
        for what, ptrs, sizes, n_segs, rows, status in cases:
            out = torch.full((65536 * w,), 0x55, dtype=torch.int8, device=eng.device)
            minmax = torch.full((65536, 2), -7.0, dtype=torch.float64, device=eng.device)
            rc = raw_quant(eng, ptrs, sizes, n_segs, rows, cols, w, minmax, out.data_ptr(), keys if use_keys else None)
            assert rc == status, what
            assert eng.lib.dlc_last_error(eng.ctx).decode() != "", what
            torch.cuda.synchronize()
            assert bool((out == 0x55).all()) and bool((minmax == -7.0).all()), what
    assert torch.equal(keys, keys_before)
    # the limits themselves are accepted: 8 segments, 65535 rows
    out = torch.empty((65535 * 2,), dtype=torch.int8, device=eng.device)
    minmax = torch.empty((65535, 2), dtype=torch.float64, device=eng.device)
    two = dev(np.array([0, 7], dtype=np.int64))
    assert raw_quant(eng, [p + 8 * g for g in range(8)], [1] * 8, 8, 65535, two, 2, minmax, out.data_ptr()) == OK
    flat = seg.cpu().numpy().reshape(-1)                              # segment g of row r is flat[g + r]
    got = out.cpu().numpy().reshape(65535, 2)
    for r in (0, 1, 40000, 65534):
        same("row %d of 65535" % r, got[r:r + 1], P.quantize_gather([flat[g + r].reshape(1, 1) for g in range(8)], [0, 7]))
