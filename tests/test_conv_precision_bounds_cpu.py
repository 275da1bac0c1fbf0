"""CPU checks of the CnnVtl tolerance mode (CnnVtl(dtype="f16x2"), dlc_cnnvtl_encode_split) that need no GPU:
  * conv_precision_bounds.conv_split_layer_bound holds for the emulation of the kernel (ratio <= 1 at every element)
    and every modelled defect exceeds it -- a bound that nothing can break would hold the GPU kernel to nothing;
  * the new C symbols resolve with their signatures, the panel / workspace sizes are pure host arithmetic;
  * CnnVtl(dtype=...) validates its argument before any engine is made."""
import ctypes as C

import numpy as np
import pytest
import torch

import conv_precision_bounds as CB
from precision_bounds import ratio


def _case(seed, n, h, w, c, cout, k, s, same, wscale, act, zero_frame=None, big_frame=None):
    rng = np.random.RandomState(seed)
    x = torch.from_numpy(rng.standard_normal((n, h, w, c)).astype(np.float32).astype(np.float64))
    if act == CB.ACT_RELU:
        x = x.abs()
    if zero_frame is not None:
        x[zero_frame] = 0.0
    if big_frame is not None:
        x[big_frame] *= 1.0e4 / float(x[big_frame].abs().max())
        x = x.to(torch.float32).to(torch.float64)
    wt = rng.standard_normal((k, k, c, cout))
    if wscale == "fan_in":
        wt = wt / np.sqrt(k * k * c)
    b = torch.from_numpy(rng.standard_normal(cout) * 0.1)
    geom = CB.same_geometry(h, w, k, s) if same else CB.valid_geometry(h, w, k, s)
    return x, torch.from_numpy(wt), b, geom


CASES = [
    # seed, n, h, w, c, cout, k, s, same, weights, act
    (1, 2, 9, 10, 16, 24, 3, 1, True, "fan_in", CB.ACT_RELU),
    (2, 2, 9, 10, 16, 24, 3, 1, True, "n01", CB.ACT_NONE),
    (3, 3, 11, 9, 5, 7, 3, 2, True, "fan_in", CB.ACT_RELU),          # stride 2 SAME, C no multiple of anything
    (4, 2, 23, 19, 3, 12, 11, 4, False, "fan_in", CB.ACT_RELU),      # conv1's form
]


@pytest.mark.parametrize("case", CASES)
def test_emulation_stays_under_the_bound(case):
    x, w, b, geom = _case(*case)
    act = case[-1]
    ref = CB.conv_reference(x, w, b, geom, act)
    bound = CB.conv_split_layer_bound(x, w, b, geom, act)
    got = CB.emulate_conv_split(x, w, b, geom, act)
    r = ratio(got - ref, bound)
    print("emulation / bound: %.3f  (max bound %.3e, max |ref| %.3e)" % (r, float(bound.max()), float(ref.abs().max())))
    assert r <= 1.0
    # the bound is a bound on THIS mode, not a loose tolerance: far below fp16's own 2^-11
    assert float((bound / (ref.abs().max() + 1e-300)).max()) < 2.0 ** -14


def test_zero_frame_beside_a_large_one():
    """A frame of exact zeros beside a frame whose maximum is 1e4: per-frame exponents keep both exact to their own scale;
    the zero frame's outputs are the biases, within 2 u |b| (fp32(b), one fma rounding)."""
    x, w, b, geom = _case(7, 2, 9, 10, 16, 24, 3, 1, True, "fan_in", CB.ACT_NONE, zero_frame=0, big_frame=1)
    assert CB.frame_exponents(x) == [0, -3]                                 # 1e4 = 0.61 2^14
    ref = CB.conv_reference(x, w, b, geom, CB.ACT_NONE)
    bound = CB.conv_split_layer_bound(x, w, b, geom, CB.ACT_NONE)
    got = CB.emulate_conv_split(x, w, b, geom, CB.ACT_NONE)
    assert ratio(got - ref, bound) <= 1.0
    assert float(bound[0].max()) <= 2 * 2.0 ** -24 * float(b.abs().max()) * 1.01 + 2.0 ** -120


@pytest.mark.parametrize("defect", ["slice", "x2w1", "exponent"])
def test_modelled_defects_exceed_the_bound(defect):
    # two frames whose exponents differ (maxima 3 and 40), 90 rows each: a 256-row tile spans both
    x, w, b, geom = _case(5, 2, 9, 10, 16, 24, 3, 1, True, "fan_in", CB.ACT_NONE)
    x[0] *= 3.0 / float(x[0].abs().max())
    x[1] *= 40.0 / float(x[1].abs().max())
    x = x.to(torch.float32).to(torch.float64)
    assert len(set(CB.frame_exponents(x))) == 2
    ref = CB.conv_reference(x, w, b, geom, CB.ACT_NONE)
    bound = CB.conv_split_layer_bound(x, w, b, geom, CB.ACT_NONE)
    assert ratio(CB.emulate_conv_split(x, w, b, geom, CB.ACT_NONE) - ref, bound) <= 1.0
    kw = {"slice": dict(drop_slice=2), "x2w1": dict(drop_x2w1=True), "exponent": dict(frame_exponent_of={1: 0})}[defect]
    bad = CB.emulate_conv_split(x, w, b, geom, CB.ACT_NONE, **kw)
    r = ratio(bad - ref, bound)
    print("%s: defect / bound = %.1f" % (defect, r))
    assert r > 1.0


# ---- the surface, without a GPU ---------------------------------------------------------------------------------------
def _geom_192x240():
    from deeploopcloser_amd import _lib as L
    rows = [(3, 3, 48, 96, 1, 0, 0, 46, 58, L.DLC_ACT_RELU, 1), (5, 5, 96, 256, 1, 2, 2, 22, 28, L.DLC_ACT_RELU, 1),
            (3, 3, 256, 384, 1, 1, 1, 10, 13, L.DLC_ACT_RELU, 0), (3, 3, 384, 384, 1, 1, 1, 10, 13, L.DLC_ACT_RELU, 0),
            (3, 3, 384, 256, 1, 1, 1, 10, 13, L.DLC_ACT_NONE, 0)]
    flat = [v for r in rows for v in r]
    return (C.c_int32 * len(flat))(*flat)


def test_new_symbols_and_host_arithmetic():
    from deeploopcloser_amd import _lib
    lib = _lib.load()
    for name in ("dlc_cnnvtl_split_panels_bytes", "dlc_cnnvtl_split_prepare", "dlc_cnnvtl_encode_split_workspace_bytes",
                 "dlc_cnnvtl_encode_split", "dlc_cnnvtl_layers_split"):
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
    g = _geom_192x240()
    panels = lib.dlc_cnnvtl_split_panels_bytes(5, g)
    # two fp16 pieces of every kernel, columns padded to the 256-column tile: at least 2 x 2 bytes per weight
    weights = 432 * 96 + 2400 * 256 + 2304 * 384 + 3456 * 384 + 3456 * 256
    assert panels >= 4 * weights and panels % 256 == 0
    w1 = lib.dlc_cnnvtl_encode_split_workspace_bytes(1, 48, 60, 48, 5, g)
    w8 = lib.dlc_cnnvtl_encode_split_workspace_bytes(8, 48, 60, 48, 5, g)
    w64 = lib.dlc_cnnvtl_encode_split_workspace_bytes(64, 48, 60, 48, 5, g)
    assert 0 < w1 < w8 < w64 and w64 % 256 == 0
    assert w64 >= 64 * 546944 * 4                                          # the five fp32 layer outputs of 64 frames
    assert lib.dlc_cnnvtl_encode_split_workspace_bytes(0, 48, 60, 48, 5, g) == 0
    assert lib.dlc_cnnvtl_encode_split_workspace_bytes(8, 48, 60, 47, 5, g) == 0      # channels do not match layer 0
    assert lib.dlc_cnnvtl_split_panels_bytes(0, g) == 0


def test_cnn_vtl_dtype_is_validated_before_an_engine_exists():
    import deeploopcloser_amd as dlc
    with pytest.raises(ValueError):
        dlc.CnnVtl(input_shape=(1, 192, 240, 3), dtype="bogus")
    if not torch.cuda.is_available():
        for dt in ("float64", "f16x2"):
            with pytest.raises(RuntimeError):
                dlc.CnnVtl(input_shape=(1, 192, 240, 3), dtype=dt)
