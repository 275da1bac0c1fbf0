"""What runs BETWEEN the GEMMs of CnnVtl(dtype="f16x2") (dlc_cnnvtl_encode_split, csrc/gemm_split_f16.hip), pinned exactly.
tests/test_gpu_cnn_vtl_f16x2.py holds one layer to its derived bound and the whole chain to a window; the stages in
between -- cs_input_kernel, cs_maxpool_kernel, the per-frame min / max fold of the SP_CONV epilogue,
cs_quant_gather_kernel, conv_run_layers' bookkeeping over several layers, the status word -- are exact operations on
fp32 values and are held here with NO tolerance:

  A  copy networks (tests/cnn_chain_oracle.py: one-hot tap x identity kernels on integer frames, exact in this mode by
     construction and checked so on the CPU by tests/test_cnn_vtl_chain_cpu.py): features and bytes compared with ==;
     A1 input conversion and space-to-depth, A2 max-pool, A3 the key fold and the quantiser, A4 constant frames and
     batch independence, A5 the non-finite-output flag;
  B  real weights, each layer conditioned on the GPU's OWN previous output: the one-layer bound
     (conv_precision_bounds.conv_split_layer_bound) with no slack, bytes == the quantiser's formula on the returned
     features, dlc_cnnvtl_layers_split bit-identical to the full run;
  C  the fp64 twins in csrc/cnnvtl.hip (maxpool_kernel, row_minmax_kernel, quant_gather_kernel) over the same tables.

Nothing here is fitted: every assertion is an equality or the derived bound."""
import numpy as np
import pytest
import torch

import cnn_chain_oracle as O
import conv_precision_bounds as CB
from oracle import cnn_vtl as ocnn
from precision_bounds import ratio

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dlc():
    import deeploopcloser_amd as d
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    d.default_engine()
    return d


@pytest.fixture(scope="module")
def eng(dlc):
    return dlc.default_engine()


def dev(a, dtype=None):
    t = torch.from_numpy(np.array(a, order="C")).to("cuda")            # (a copy: the shared case arrays are read-only)
    return t if dtype is None else t.to(dtype)


def same(what, got, want):
    """got == want, elementwise and in shape; the message says where they part."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, "%s: shape %s, expected %s" % (what, got.shape, want.shape)
    bad = got != want
    if bad.any():
        at = tuple(int(v) for v in np.argwhere(bad)[0])
        raise AssertionError("%s: %d of %d differ, first at %s: got %r, expected %r" % (what, int(bad.sum()), bad.size, at, got[at], want[at]))


def run_network(eng, x, geom, weights, biases, cols, s2d=1):
    """x: host frames [n, h, w, c] of the dtype the kernel is to read -> (bytes int8, fp64 copies of the layers' fp32
    outputs, the status word, the prepared panels)."""
    panels = eng.cnnvtl_split_panels(geom, [dev(w.reshape(-1, w.shape[-1]), torch.float64) for w in weights])
    status = torch.zeros(1, dtype=torch.int32, device=eng.device)
    b = [dev(v, torch.float64) for v in biases]
    out, fs = eng.cnnvtl_encode_split(dev(x), geom, s2d, panels, b, dev(cols, torch.int64), status, feats=True)
    return out.cpu().numpy(), [f.to(torch.float64).cpu().numpy() for f in fs], int(status.item()), panels


def run_copy(eng, x, layers, cols, s2d=1):
    h, w = x.shape[1] // s2d, x.shape[2] // s2d
    return run_network(eng, x, O.layer_geometry(layers, h, w), O.layer_weights(layers), [L.bias for L in layers], cols, s2d)[:3]


def every_column(feats, seed=0):
    return O.all_columns(np.random.RandomState(seed), O.concat_features(feats).shape[1])


# ---- A1: input conversion and space-to-depth ----------------------------------------------------------------------
@pytest.mark.parametrize("case", O.A1_CASES, ids=["%dx%dx%dx%d s2d %d %s" % c for c in O.A1_CASES])
def test_a1_input_conversion_and_space_to_depth(eng, case):
    n, h, w, c, s, dt = case
    x, layers = O.a1_case(case)
    assert x.dtype == np.dtype(dt) and (dt == "uint8" or x.min() < 0)
    want = x.astype(np.float64).reshape(n, h // s, s, w // s, s, c).transpose(0, 1, 3, 2, 4, 5).reshape(n, h // s, w // s, s * s * c) \
        + layers[0].bias
    cols = every_column([want], 1)
    got, feats, status = run_copy(eng, x, layers, cols, s2d=s)
    assert status == 0
    same("A1 %s features" % (case,), feats[0], want)
    same("A1 %s bytes" % (case,), got, O.expected_bytes([want], cols))


def test_a1_frames_that_are_no_whole_number_of_blocks_are_refused(eng):
    x = np.zeros((2, 6, 8, 3), dtype=np.float32)
    layers = [O.identity_layer(np.zeros(48))]
    with pytest.raises(ValueError):
        run_copy(eng, x, layers, np.arange(4), s2d=4)                   # h % s2d != 0
    with pytest.raises(ValueError):
        run_copy(eng, x.transpose(0, 2, 1, 3), layers, np.arange(4), s2d=4)      # w % s2d != 0


# ---- A2: max-pool --------------------------------------------------------------------------------------------------
def check_pool(eng, what, x, layers):
    want = O.expected_features(x, layers)
    cols = every_column(want, 2)
    got, feats, status = run_copy(eng, x.astype(np.float32), layers, cols)
    assert status == 0
    same(what + " layer 0", feats[0], want[0])
    same(what + " layer 1 against the pool of the GPU's own layer 0", feats[1], ocnn.maxpool3x3s2(feats[0]) + layers[1].bias)
    same(what + " layer 1", feats[1], want[1])
    same(what + " bytes", got, O.expected_bytes(want, cols))
    return got, feats


@pytest.mark.parametrize("kind", O.A2_KINDS)
def test_a2_maxpool(eng, kind):
    for (h, w) in O.A2_SHAPES:
        for c in O.A2_CHANNELS:
            x, layers = O.a2_case(kind, h, w, c)
            if kind == "negative":
                assert O.expected_features(x, layers)[0].max() < 0
            check_pool(eng, "A2 %s %dx%dx%d" % (kind, h, w, c), x, layers)


def test_a2_maxpool_grid_wraps(eng):
    n, h, w, c = O.A2_BIG
    x, layers = O.a2_case("any", h, w, c, n=n)
    want = O.expected_features(x, layers)
    assert want[1].size > O.GRID_WRAP_F32
    cols = np.array([0, want[0][0].size - 1, want[0][0].size, want[0][0].size + want[1][0].size - 1, -1], dtype=np.int64)
    got, feats, status = run_copy(eng, x.astype(np.float32), layers, cols)
    assert status == 0
    same("A2 big layer 0", feats[0], want[0])
    same("A2 big layer 1", feats[1], want[1])
    same("A2 big bytes", got, O.expected_bytes(want, cols))


def test_a2_pool_on_the_last_layer_changes_nothing(eng):
    x, with_pool = O.a2_case("any", 23, 31, 16, last_pool=1)
    no_pool = [with_pool[0], with_pool[1]._replace(pool=0)]
    b1, f1 = check_pool(eng, "A2 last layer pools", x, with_pool)
    b0, f0 = check_pool(eng, "A2 last layer does not pool", x, no_pool)
    assert f1[1].shape == (3, 11, 15, 16)                               # the last segment keeps its unpooled width
    same("bytes with / without the last pool", b1, b0)
    for l in range(2):
        same("layer %d with / without the last pool" % l, f1[l], f0[l])


# ---- A3: the key fold and the quantiser ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", O.A3_NAMES)
def test_a3_key_fold_and_quantiser(eng, name):
    O.assert_a3_coverage()                  # from the expected features alone: every branch, every plant (the whole list)
    print("A3 " + O.a3_summary(name))
    x, layers, cols, want = O.a3_case(name)
    got, feats, status = run_copy(eng, x.astype(np.float32), layers, cols)
    assert status == 0
    for l in range(len(layers)):
        same("A3 %s layer %d" % (name, l), feats[l], want[l])
    same("A3 %s bytes" % name, got, O.expected_bytes(want, cols))


# ---- A4: constant frames and independence --------------------------------------------------------------------------
def test_a4_a_constant_frame_gives_zero_bytes(eng):
    x, layers = O.a4_zero_frame_case()
    want = O.expected_features(x, layers)
    cols = every_column(want, 4)
    got, feats, status = run_copy(eng, x, layers, cols)                 # (fp64 frames)
    assert status == 0
    same("A4 features", feats[0], want[0])
    assert not got[2].any() and all(got[f].any() for f in (0, 1, 3, 4))
    same("A4 bytes", got, O.expected_bytes(want, cols))


@pytest.mark.parametrize("case", O.A4_INDEPENDENCE, ids=["%d rows per frame" % (c[1] * c[2]) for c in O.A4_INDEPENDENCE])
def test_a4_a_frame_does_not_depend_on_its_batch(eng, case):
    x, layers = O.a4_case(*case)
    want = O.expected_features(x, layers)
    cols = every_column(want, 5)
    got, feats, status = run_copy(eng, x.astype(np.float32), layers, cols)
    assert status == 0
    same("A4 batch bytes", got, O.expected_bytes(want, cols))
    for f in range(x.shape[0]):                                          # its neighbours share its wave in the batch
        g1, f1, s1 = run_copy(eng, x[f:f + 1].astype(np.float32), layers, cols)
        assert s1 == 0
        same("A4 frame %d alone, bytes" % f, g1, got[f:f + 1])
        same("A4 frame %d alone, features" % f, f1[0], feats[0][f:f + 1])


# ---- A5: the non-finite-output flag --------------------------------------------------------------------------------
def test_a5_an_overflowing_layer_output_sets_the_output_flag(dlc, eng):
    """Finite frames and finite weights whose product leaves fp32: plain arithmetic, flag value 2 (a layer's output) and
    not 1 (a layer's input).  dlc_cnnvtl_layers_split reports inputs only (include/dlc.h): the output flag rides on the
    key fold, which that entry does not run."""
    x = np.full((2, 3, 3, 5), 1.0e9, dtype=np.float32)
    geom = [(1, 1, 5, 5, 1, 0, 0, 3, 3, CB.ACT_NONE, 0)]
    w, b = [np.eye(5).reshape(1, 1, 5, 5) * 1.0e30], [np.zeros(5)]
    _, feats, status, panels = run_network(eng, x, geom, w, b, np.arange(45))
    assert np.isinf(feats[0]).any()
    assert status & 2 and not status & 1
    st = torch.zeros(1, dtype=torch.int32, device=eng.device)
    ys = eng.cnnvtl_layers_split(dev(x), (3, 3, 5), geom, 0, 0, panels, [dev(b[0])], st)
    assert torch.isinf(ys[0]).any() and not int(st.item()) & 1
    # through the class: only conv5 overflows (its input, conv4's output, is finite), so no layer INPUT is flagged
    ws = [np.full((kh, kw, cin, cout), 1.0 / (kh * kw * cin)) for _, kh, kw, cin, cout, *_ in ocnn.LAYERS]
    ws[4] = np.full_like(ws[4], 1.0e30)
    net = dlc.CnnVtl(input_shape=[1, 35, 39, 3], seed=1, mask_seed=2, dtype="f16x2", compress_factor=50.0)
    net.set_weights(ws, [np.zeros(w_.shape[-1]) for w_ in ws])
    frames = torch.full((1, 35, 39, 3), 1.0e9, dtype=torch.float32, device=eng.device)
    with pytest.raises(ValueError, match="a layer's output"):
        net.transform_tensor(frames)
    net.set_weights(ws[:4] + [np.full_like(ws[4], 1.0e-3)], [np.zeros(w_.shape[-1]) for w_ in ws])
    assert net.transform_tensor(frames).shape[0] == 1                   # the same frames, finite outputs: accepted


# ---- B: real weights, each layer conditioned on the GPU's own input ----------------------------------------------
def check_conditioned_layers(what, x0, feats, convs):
    """convs: per layer (W [kh, kw, c, cout], b, CB geometry, CB act, pool).  Layer l's kernel output feats[l] against the
    fp64 convolution of input_l = the (host-pooled) GPU output of layer l - 1: the one-layer bound, no slack.
    -> the inputs."""
    inputs = [x0]
    for l, (w, b, geom, act, pool) in enumerate(convs):
        xin = dev(inputs[l], torch.float64)
        got = dev(feats[l], torch.float64)
        ref = CB.conv_reference(xin, dev(w), dev(b), geom, act)
        bound = CB.conv_split_layer_bound(xin, dev(w), dev(b), geom, act)
        assert got.shape == ref.shape == bound.shape
        r = ratio(got - ref, bound)
        print("%s layer %d: kernel error / bound = %.3f (max error %.3e, max bound %.3e, max |y| %.3e)"
              % (what, l, r, float((got - ref).abs().max()), float(bound.max()), float(ref.abs().max())))
        assert torch.isfinite(got).all()
        assert r <= 1.0, "%s layer %d" % (what, l)
        inputs.append(ocnn.maxpool3x3s2(feats[l]) if pool else feats[l])        # exact on fp32 values
    return inputs


def test_b_three_layers_conditioned_on_the_gpus_own_outputs(eng):
    rng = np.random.RandomState(61)
    n, h, w = 4, 27, 31
    x = rng.randint(0, 256, size=(n, h, w, 8)).astype(np.float64)
    spec = [(5, 8, 24, CB.ACT_RELU, 1), (3, 24, 40, CB.ACT_RELU, 1), (3, 40, 33, CB.ACT_NONE, 0)]
    geom, convs, ws, bs = [], [], [], []
    for k, cin, cout, act, pool in spec:
        g = CB.same_geometry(h, w, k, 1)
        wt = rng.standard_normal((k, k, cin, cout)) / np.sqrt(k * k * cin)
        b = rng.standard_normal(cout) * 0.1
        geom.append((k, k, cin, cout, 1, g[3], g[4], g[5], g[6], act, pool))
        convs.append((wt, b, g, act, pool))
        ws.append(wt)
        bs.append(b)
        if pool:
            h, w = (h - 3) // 2 + 1, (w - 3) // 2 + 1
    assert [g[7] * g[8] for g in geom] == [27 * 31, 13 * 15, 6 * 7]
    width = sum(g[7] * g[8] * g[3] for g in geom)
    cols = O.all_columns(np.random.RandomState(62), width)
    got, feats, status, panels = run_network(eng, x.astype(np.float32), geom, ws, bs, cols)
    assert status == 0
    inputs = check_conditioned_layers("three layers", x, feats, convs)
    same("three layers: bytes", got, O.expected_bytes(feats, cols))
    bias_t = [dev(b) for b in bs]
    for a, b in ((1, 1), (1, 2), (2, 2)):
        st = torch.zeros(1, dtype=torch.int32, device=eng.device)
        ys = eng.cnnvtl_layers_split(dev(inputs[a], torch.float32), (27, 31, 8), geom, a, b, panels, bias_t, st)
        assert int(st.item()) == 0 and len(ys) == b - a + 1
        for l in range(a, b + 1):
            same("layers %d..%d alone, layer %d" % (a, b, l), ys[l - a].to(torch.float64).cpu().numpy(), feats[l])


@pytest.mark.parametrize("hw", [(36, 40), (35, 39)], ids=["space-to-depth conv1", "element-wise conv1"])
def test_b_five_layers_conditioned_on_the_gpus_own_outputs(dlc, hw):
    """The real conv1..conv5 at the smallest frames that survive both pools (test_encoders_fuzz: 35 x 39; 36 x 40 is the
    smallest whose H and W are multiples of 4)."""
    from deeploopcloser_amd.cnn_vtl import space_to_depth_kernel
    h, w = hw
    n = 3
    x = np.random.RandomState(63).randint(0, 256, size=(n, h, w, 3)).astype(np.float64)
    net = dlc.CnnVtl(input_shape=[n, h, w, 3], seed=11, mask_seed=12, dtype="f16x2", compress_factor=50.0)
    assert bool(net._s2d) == (h % 4 == 0 and w % 4 == 0)
    ws, bs = ocnn.init_weights(11)
    got, fs = net.features_split(dev(x))
    feats = [f.to(torch.float64).cpu().numpy() for f in fs]
    convs, x0 = [], x
    for l, ((name, k, _, cin, cout, s, pad, relu), wt, b) in enumerate(zip(ocnn.LAYERS, ws, bs)):
        ih, iw = (h, w) if l == 0 else convs_in
        act = CB.ACT_RELU if relu else CB.ACT_NONE
        if l == 0 and net._s2d:
            x0, wt = O.space_to_depth(x, 4), space_to_depth_kernel(wt, 4)
            g = CB.valid_geometry(ih // 4, iw // 4, 3, 1)
        else:
            g = CB.same_geometry(ih, iw, k, s) if pad == "SAME" else CB.valid_geometry(ih, iw, k, s)
        pool = name in ocnn.POOL_AFTER
        convs.append((wt, b, g, act, pool))
        convs_in = ((g[5] - 3) // 2 + 1, (g[6] - 3) // 2 + 1) if pool else (g[5], g[6])
    assert [f[0].size for f in feats] == ocnn.layer_sizes((h, w))
    check_conditioned_layers("conv1..5 at %dx%d" % hw, x0, feats, convs)
    same("conv1..5 at %dx%d: bytes" % hw, got.cpu().numpy(), O.expected_bytes(feats, net.columns))


# ---- C: the fp64 siblings ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", O.A2_KINDS)
def test_c_fp64_maxpool(eng, kind):
    for (h, w) in O.A2_SHAPES:
        for c in O.A2_CHANNELS:
            x = O.a2_frames(kind, 3, h, w, c, 7000 + h + w + c) * 1.0e-3 + 1.0e-9        # values fp32 does not hold
            same("fp64 pool %s %dx%dx%d" % (kind, h, w, c), eng.maxpool3x3s2(dev(x)).cpu().numpy(), ocnn.maxpool3x3s2(x))


def test_c_fp64_maxpool_grid_wraps(eng):
    n, h, w, c = 64, 47, 47, 128
    assert n * 23 * 23 * c > O.GRID_WRAP_F64
    x = np.random.RandomState(71).randint(-30000, 0, size=(n, h, w, c)).astype(np.float64)      # all negative
    same("fp64 pool, grid wraps", eng.maxpool3x3s2(dev(x)).cpu().numpy(), ocnn.maxpool3x3s2(x))


@pytest.mark.parametrize("case", O.C_CASES, ids=["%d segments %d rows from width %d" % (c[0], c[1], O.C_WIDTHS[c[2]]) for c in O.C_CASES])
def test_c_fp64_minmax_and_quantiser(eng, case):
    segs, cols = O.c_case(*case)
    want = O.expected_bytes(segs, cols)
    st, ct = [dev(s) for s in segs], dev(cols, torch.int64)
    same("minmax_quant_gather %s" % (case,), eng.minmax_quant_gather(st, ct).cpu().numpy(), want)
    # quant_gather reads its range from keys (frame_minmax_keys): folded here by the one entry that folds into them, the
    # convolution -- a 1x1 identity over the rows' concatenation, exact in fp64 -- at the widths that keeps small
    rows = segs[0].shape[0]
    d = np.concatenate(segs, axis=1)
    if d.shape[1] <= 1024:
        k = d.shape[1]
        keys = eng.frame_minmax_keys(rows)
        y = eng.conv2d(dev(d.reshape(rows, 1, 1, k)), dev(np.eye(k)), dev(np.zeros(k)), 1, 1, 1, 0, 0, 1, 1, CB.ACT_NONE, frame_keys=keys)
        same("the identity convolution", y.cpu().numpy().reshape(rows, k), d)
        same("quant_gather %s" % (case,), eng.quant_gather(st, ct, keys).cpu().numpy(), want)
