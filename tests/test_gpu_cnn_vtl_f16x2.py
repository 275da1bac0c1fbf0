"""CnnVtl(dtype="f16x2"): the tolerance-mode encoder on the fp16 matrix cores (dlc_cnnvtl_encode_split,
csrc/gemm_split_f16.hip) held to

  1. the elementwise bound of ONE layer (tests/conv_precision_bounds.py: derived, nothing fitted), at every element;
  2. the fp64 oracle end to end through a WINDOW on the scaled values: a gathered byte whose fp64 scaled value s lies
     farther than W quantisation steps from an integer equals the oracle's byte, every other byte equals it or differs by
     one step modulo 256;
  3. batch independence, 4. weights that follow set_weights, 5. an untouched fp64 mode, 6. the pipeline and the CLI,
  7. the full 1063-frame size.

The window.  W cannot be derived (no saturating activation damps the chain: a rigorous bound through five layers grows
by ~40 per layer), so it is measured -- NOT against the code under test: W = 8 x the largest |s_emulated - s| that the CPU
emulation scripts/emul_cnn_split.py shows against the fp64 oracle on the six frames of test 2 (three golden frames,
RandomState(2) pixels; seed = 5, mask_seed = 9).  The factor 8 covers the summation order inside a 32-deep slice, which
the emulation (BLAS) does not reproduce.
    emulated largest |s_emulated - s|   EMULATED_MAX_SCALED_ERR = 1.989e-4 steps (per frame 0.90e-4 .. 1.99e-4)
    W = 8 x that                        1.59e-3 steps
    the GPU's own largest |s_gpu - s|   2.89e-4 steps on an MI355X (per frame 2.20e-4 .. 2.89e-4; printed by test 2 from
                                        the layers' fp32 outputs, CnnVtl.features_split): 1.45 x the emulation's, 0.18 W
The condition that keeps the window from hiding a failure is asserted first, by the oracle alone: at most 2 % of each
frame's gathered bytes lie inside W, no frame's zero class (the ~47 % of the features that are exact ReLU zeros and share
ONE scaled value) does, and W stays below 1e-2.
"""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import conv_precision_bounds as CB
import real_frames
from conftest import GOLDEN, ROOT
from precision_bounds import ratio

pytestmark = pytest.mark.gpu

EMULATED_MAX_SCALED_ERR = 1.989e-4           # scripts/emul_cnn_split.py, quantisation steps
W = 8 * EMULATED_MAX_SCALED_ERR


@pytest.fixture(scope="module")
def dlc():
    import deeploopcloser_amd as d
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    d.default_engine()
    return d


@pytest.fixture(scope="module")
def eng(dlc):
    return dlc.default_engine()


def dev(a, dtype=torch.float64):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda", dtype)


# ---- 1. one layer against its bound -----------------------------------------------------------------------------------
def run_layer(eng, x, w, b, geom, act):
    """x [n, h, w, c] fp64 (fp32-representable) on the device -> the kernel's fp32 output of the one-layer network."""
    from deeploopcloser_amd import _lib as L
    kh, kw, s, pt, pl, oh, ow = geom
    c, cout = x.shape[3], w.shape[-1]
    g = [(kh, kw, c, cout, s, pt, pl, oh, ow, L.DLC_ACT_RELU if act == CB.ACT_RELU else L.DLC_ACT_NONE, 0)]
    w2 = w.reshape(-1, cout).contiguous()
    panels = eng.cnnvtl_split_panels(g, [w2])
    status = torch.zeros(1, dtype=torch.int32, device=eng.device)
    y = eng.cnnvtl_layers_split(x.to(torch.float32), tuple(x.shape[1:]), g, 0, 0, panels, [b], status)[0]
    assert int(status.item()) == 0
    return y.to(torch.float64)


def layer_case(seed, n, h, w, c, cout, k, s, same, wscale, act, pixels=False):
    rng = np.random.RandomState(seed)
    if pixels:
        x = rng.randint(0, 256, size=(n, h, w, c)).astype(np.float64)
    else:
        x = (np.abs(rng.standard_normal((n, h, w, c))) * 100.0).astype(np.float32).astype(np.float64)
    wt = rng.standard_normal((k, k, c, cout))
    if wscale == "fan_in":
        wt = wt / np.sqrt(k * k * c)
    b = rng.standard_normal(cout) * 0.1
    geom = CB.same_geometry(h, w, k, s) if same else CB.valid_geometry(h, w, k, s)
    return dev(x), dev(wt), dev(b), geom


def check_layer(eng, what, x, w, b, geom, act):
    got = run_layer(eng, x, w, b, geom, act)
    ref = CB.conv_reference(x, w, b, geom, act)
    bound = CB.conv_split_layer_bound(x, w, b, geom, act)
    assert got.shape == ref.shape == bound.shape
    r = ratio(got - ref, bound)
    print("%s: kernel error / bound = %.3f (max error %.3e, max bound %.3e, max |y| %.3e)"
          % (what, r, float((got - ref).abs().max()), float(bound.max()), float(ref.abs().max())))
    assert torch.isfinite(got).all()
    assert r <= 1.0, what


CNNVTL_LAYERS = [
    # name, n, h, w, c, cout, k, s, same, act        (the five GEMMs of a 192 x 240 frame)
    ("conv2", 2, 23, 29, 96, 256, 5, 1, True, CB.ACT_RELU),
    ("conv3", 5, 10, 13, 256, 384, 3, 1, True, CB.ACT_RELU),
    ("conv4", 5, 10, 13, 384, 384, 3, 1, True, CB.ACT_RELU),
    ("conv5", 5, 10, 13, 384, 256, 3, 1, True, CB.ACT_NONE),
]


@pytest.mark.parametrize("wscale", ["fan_in", "n01"])
@pytest.mark.parametrize("layer", CNNVTL_LAYERS, ids=[l[0] for l in CNNVTL_LAYERS])
def test_layer_bound_cnnvtl_shapes(eng, layer, wscale):
    name, n, h, w, c, cout, k, s, same, act = layer
    x, wt, b, geom = layer_case(11, n, h, w, c, cout, k, s, same, wscale, act)
    check_layer(eng, "%s %s" % (name, wscale), x, wt, b, geom, act)


@pytest.mark.parametrize("wscale", ["fan_in", "n01"])
def test_layer_bound_conv1_both_forms(dlc, eng, wscale):
    """conv1 on integer pixels: over the space-to-depth input (3 x 3 x 48, K = 432, what a 192 x 240 frame runs) and
    element by element (11 x 11 x 3 stride 4, K = 363 with a k-tail)."""
    from deeploopcloser_amd.cnn_vtl import space_to_depth_kernel
    rng = np.random.RandomState(12)
    px = rng.randint(0, 256, size=(2, 192, 240, 3)).astype(np.float64)
    wt = rng.standard_normal((11, 11, 3, 96)) / (np.sqrt(363.0) if wscale == "fan_in" else 1.0)
    b = dev(rng.standard_normal(96) * 0.1)
    check_layer(eng, "conv1 element-wise " + wscale, dev(px), dev(wt), b, CB.valid_geometry(192, 240, 11, 4), CB.ACT_RELU)
    s2d = px.reshape(2, 48, 4, 60, 4, 3).transpose(0, 1, 3, 2, 4, 5).reshape(2, 48, 60, 48)
    check_layer(eng, "conv1 space-to-depth " + wscale, dev(s2d), dev(space_to_depth_kernel(wt, 4)), b,
                CB.valid_geometry(48, 60, 3, 1), CB.ACT_RELU)


def test_layer_bound_odd_shapes(eng):
    # stride 2 SAME, channels and outputs that are no multiple of anything
    x, w, b, geom = layer_case(21, 3, 11, 9, 5, 7, 3, 2, True, "fan_in", CB.ACT_RELU)
    check_layer(eng, "stride 2 SAME c=5", x, w, b, geom, CB.ACT_RELU)
    x, w, b, geom = layer_case(22, 2, 13, 12, 20, 33, 3, 1, True, "n01", CB.ACT_NONE)
    check_layer(eng, "c=20 cout=33", x, w, b, geom, CB.ACT_NONE)
    # 90 rows per frame: a 256-row tile spans three frames, each with its own exponent (maxima 3, 40, 700, 9)
    x, w, b, geom = layer_case(23, 4, 9, 10, 16, 24, 3, 1, True, "fan_in", CB.ACT_NONE)
    for f, m in enumerate((3.0, 40.0, 700.0, 9.0)):
        x[f] *= m / float(x[f].abs().max())
    x = x.to(torch.float32).to(torch.float64)
    assert len(set(CB.frame_exponents(x))) == 4
    check_layer(eng, "tile over three frames", x, w, b, geom, CB.ACT_NONE)
    # a frame of exact zeros beside a frame whose maximum is 1e4
    x, w, b, geom = layer_case(24, 3, 9, 10, 16, 24, 3, 1, True, "fan_in", CB.ACT_RELU)
    x[1] = 0.0
    x[2] *= 1.0e4 / float(x[2].abs().max())
    x = x.to(torch.float32).to(torch.float64)
    check_layer(eng, "zero frame beside 1e4", x, w, b, geom, CB.ACT_RELU)


# ---- 2. end to end against the fp64 oracle ---------------------------------------------------------------------------
def scaled(d):
    mx = d.max(axis=1).reshape(-1, 1)
    mn = d.min(axis=1).reshape(-1, 1)
    return (d - mn) * (np.float64(255) / (mx - mn)), mn, mx


def near(s):
    f = s - np.floor(s)
    return np.minimum(f, 1 - f)


def window_rule(what, got, x, ws, bs, cols, feats=None):
    """The rule of the file header for frames x (numpy fp64) whose f16x2 bytes are `got` [n, cols.size]."""
    from oracle import cnn_vtl as ocnn
    assert W <= 1e-2, "the window may not grow past 1e-2 quantisation steps"
    ref_d = ocnn.features(x, ws, bs)
    s, mn, mx = scaled(ref_d)
    ref = ocnn.quantize_int8(ref_d)[:, cols]
    d = near(s[:, cols])
    zero = near((0.0 - mn) * (np.float64(255) / (mx - mn))).ravel()
    for f in range(x.shape[0]):
        inside = float((d[f] <= W).mean())
        print("%s frame %d: %.2f %% of the gathered bytes inside W = %.2e; zero class %.4f steps from an integer"
              % (what, f, 100 * inside, W, zero[f]))
        assert inside <= 0.02, "the window would cover more than 2 % of frame " + str(f)
        assert zero[f] > W, "frame %d's zero class lies inside the window" % f
    if feats is not None:
        s_gpu, _, _ = scaled(feats)
        e = np.abs(s_gpu - s).max(axis=1)
        print("%s: largest |s_gpu - s| per frame (steps): %s  -- emulated %.2e, W %.2e" % (what, e, EMULATED_MAX_SCALED_ERR, W))
    step = (got.astype(np.int16) - ref.astype(np.int16)) & 0xFF
    differ = step != 0
    print("%s: %d of %d gathered bytes differ from the oracle's" % (what, int(differ.sum()), differ.size))
    assert not (differ & (d > W)).any(), "%s: a byte outside the window differs from the oracle" % what
    assert np.isin(step[differ], (1, 255)).all(), "%s: a byte differs by more than one step" % what


def six_frames(dlc):
    paths = sorted(p for p in real_frames.frame_paths() if os.sep + "frames" + os.sep in p)
    golden = np.stack([dlc.read_ppm(p)[:, :, ::-1] for p in paths]).astype(np.float64)
    rnd = np.random.RandomState(2).randint(0, 256, size=(3, 192, 240, 3)).astype(np.float64)
    return golden, rnd


def test_end_to_end_vs_oracle_window(dlc):
    from oracle import cnn_vtl as ocnn
    ws, bs = ocnn.init_weights(5)
    net = dlc.CnnVtl(input_shape=[3, 192, 240, 3], seed=5, mask_seed=9, dtype="f16x2")
    cols = ocnn.column_indices(net.layer_sizes, 99.59, seed=9)
    assert np.array_equal(net.columns, cols)
    for what, x in zip(("golden", "random"), six_frames(dlc)):
        got = net.transform(x)
        assert got.dtype == np.int8 and got.shape == (3, cols.size)
        b2, fs = net.features_split(dev(x))
        assert np.array_equal(b2.cpu().numpy(), got)
        feats = np.concatenate([f.reshape(3, -1).to(torch.float64).cpu().numpy() for f in fs], axis=1)
        window_rule(what, got, x, ws, bs, cols, feats)


# ---- 3. batch independence --------------------------------------------------------------------------------------------
def test_batch_independence_and_input_dtypes(dlc):
    x = real_frames.tiled_bgr_frames(dlc, 40)
    net = dlc.CnnVtl(input_shape=[40, 192, 240, 3], seed=5, mask_seed=9, dtype="f16x2")
    all40 = net.transform_tensor(x)
    alone = net.transform_tensor(x[7:8])
    assert torch.equal(all40[7:8], alone)
    net16 = dlc.CnnVtl(input_shape=[40, 192, 240, 3], seed=5, mask_seed=9, dtype="f16x2", frame_chunk=16)
    assert torch.equal(net16.transform_tensor(x), all40)
    assert torch.equal(net.transform_tensor(x.to(torch.uint8)), all40)              # uint8 pixels, not widened
    assert torch.equal(net.transform_tensor(x.to(torch.float32)), all40)
    host = net.transform(x.to(torch.uint8).cpu().numpy(), chunk_frames=7)            # the chunked host path
    assert np.array_equal(host, all40.cpu().numpy())


def test_non_finite_frames_are_refused(dlc):
    net = dlc.CnnVtl(input_shape=[2, 192, 240, 3], seed=5, mask_seed=9, dtype="f16x2")
    x = real_frames.tiled_bgr_frames(dlc, 2).clone()
    x[1, 5, 5, 1] = float("nan")
    with pytest.raises(ValueError):
        net.transform_tensor(x)
    x[1, 5, 5, 1] = float("inf")
    with pytest.raises(ValueError):
        net.transform_tensor(x)
    x[1, 5, 5, 1] = 1.0e6                                                             # large but finite: accepted
    assert net.transform_tensor(x).shape[0] == 2


# ---- 4. weights follow ------------------------------------------------------------------------------------------------
def test_weights_follow_set_weights(dlc, tmp_path):
    from oracle import cnn_vtl as ocnn
    x = real_frames.tiled_bgr_frames(dlc, 3)
    net = dlc.CnnVtl(input_shape=[3, 192, 240, 3], seed=5, mask_seed=9, dtype="f16x2")
    before = net.transform_tensor(x)
    ws, bs = ocnn.init_weights(6)
    net.set_weights(ws, bs)
    after = net.transform_tensor(x)
    fresh = dlc.CnnVtl(input_shape=[3, 192, 240, 3], seed=6, mask_seed=9, dtype="f16x2")
    assert torch.equal(after, fresh.transform_tensor(x)) and not torch.equal(after, before)
    blob = {name: [w, b] for (name, *_), w, b in zip(ocnn.LAYERS, *ocnn.init_weights(7))}
    path = str(tmp_path / "alexnet.npy")
    np.save(path, np.array(blob, dtype=object), allow_pickle=True)
    net.load_alexnet_npy(path)
    fresh7 = dlc.CnnVtl(input_shape=[3, 192, 240, 3], seed=7, mask_seed=9, dtype="f16x2")
    assert torch.equal(net.transform_tensor(x), fresh7.transform_tensor(x))


# ---- 5. the fp64 mode is untouched ------------------------------------------------------------------------------------
def test_fp64_mode_untouched(dlc):
    from oracle import cnn_vtl as ocnn
    x = np.random.RandomState(2).randint(0, 256, size=(3, 192, 240, 3)).astype(np.float64)
    a = dlc.CnnVtl(input_shape=[3, 192, 240, 3], seed=5, mask_seed=9)
    b = dlc.CnnVtl(input_shape=[3, 192, 240, 3], seed=5, mask_seed=9, dtype="float64")
    assert a.dtype == b.dtype == "float64"
    ws, bs = ocnn.init_weights(5)
    ref = ocnn.transform(x, ws, bs, ocnn.column_indices(a.layer_sizes, 99.59, seed=9))
    got = a.transform(x)
    assert np.array_equal(got, b.transform(x)) and np.array_equal(got, ref)


# ---- 6. pipeline and CLI ----------------------------------------------------------------------------------------------
def test_pipeline_and_cli(dlc):
    from deeploopcloser_amd import pipeline
    x = real_frames.tiled_bgr_frames(dlc, 24)
    net = dlc.CnnVtl(input_shape=[24, 192, 240, 3], seed=5, mask_seed=9, dtype="f16x2")
    dm = pipeline.cnn_vtl_distance_matrix_from_frames(x.to(torch.uint8).cpu().numpy(), net)
    own = net.engine.cnnvtl_distance_matrix(net.transform_tensor(x)).cpu().numpy()
    assert np.array_equal(dm, own)
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-m", "deeploopcloser_amd.loop_closure", os.path.join(GOLDEN, "datasets_test"),
                        "--network", "cnn_vtl", "--encoder-dtype", "f16x2", "--k", "2", "--exclusion", "0", "--threshold", "-1",
                        "--batch", "4"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [l for l in r.stdout.splitlines() if l.startswith("loop\t")]
    assert len(lines) >= 10, r.stdout + r.stderr
    r = subprocess.run([sys.executable, "-m", "deeploopcloser_amd.loop_closure", os.path.join(GOLDEN, "frames"),
                        "--network", "sdav", "--encoder-dtype", "f16x2", "--k", "1", "--exclusion", "0", "--threshold", "-1",
                        "--batch", "3"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and len([l for l in r.stdout.splitlines() if l.startswith("loop\t")]) == 2, r.stdout + r.stderr


# ---- 7. full size -----------------------------------------------------------------------------------------------------
def test_full_size_1063_frames(dlc):
    from oracle import cnn_vtl as ocnn
    n = 1063
    x = real_frames.tiled_bgr_frames(dlc, n).to(torch.uint8)
    net = dlc.CnnVtl(input_shape=[n, 192, 240, 3], seed=5, mask_seed=9, dtype="f16x2", frame_chunk=300)
    got = net.transform_tensor(x)                               # four chunks of 266 (the last 265)
    assert got.shape == (n, net.columns.size) and got.dtype == torch.int8
    for f in (0, 265, 266, 531, 532, 797, 798, n - 1):         # either side of every chunk seam
        assert torch.equal(got[f:f + 1], net.transform_tensor(x[f:f + 1])), f
    ws, bs = ocnn.init_weights(5)
    cols = ocnn.column_indices(net.layer_sizes, 99.59, seed=9)
    x20 = x[:20].to(torch.float64).cpu().numpy()                # the 20 distinct real frames
    g20 = got[:20].cpu().numpy()
    for lo in range(0, 20, 5):
        window_rule("real frames %d..%d" % (lo, lo + 4), g20[lo:lo + 5], x20[lo:lo + 5], ws, bs, cols)
    f64 = dlc.CnnVtl(input_shape=[n, 192, 240, 3], seed=5, mask_seed=9, frame_chunk=300).transform_tensor(x.to(torch.float64))
    print("1063 frames: %.4f %% of the bytes differ from the fp64 mode's" % (100.0 * float((f64 != got).float().mean())))
