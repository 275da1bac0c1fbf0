#!/usr/bin/env python3
"""CPU emulation of CnnVtl(dtype="f16x2") (dlc_cnnvtl_encode_split) against the fp64 oracle: what the arithmetic of the
tolerance mode -- two fp16 pieces per operand, ONE ACTIVATION EXPONENT PER FRAME AND LAYER, three fp32 products per
32-deep k-slice added in slice order, fp32 bias / ReLU / max-pool, the reference's fp64 quantiser -- does to the features
and to the bytes.  The emulated layer is tests/conv_precision_bounds.emulate_conv_split (BLAS sums the 32 products of a
slice in another order than the MFMA does: an indication, not the kernel).

The largest |s_emulated - s| over the six frames below (s = the scaled value (d - min) * 255 / (max - min), in quantisation
steps) is the constant EMULATED_MAX_SCALED_ERR of tests/test_gpu_cnn_vtl_f16x2.py, whose window is W = 8 x it.

usage: emul_cnn_split.py [--frames20]     (--frames20: the window condition on all 20 real frames instead)"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import conv_precision_bounds as CB                       # noqa: E402
from oracle import cnn_vtl as ocnn                       # noqa: E402
from deeploopcloser_amd.input import read_ppm            # noqa: E402
import real_frames                                       # noqa: E402


def emul_features(x, ws, bs):
    """[n, sum(sizes)] fp64: the emulated fp32 layer outputs, flattened and concatenated like oracle.cnn_vtl.features."""
    n = x.shape[0]
    h = torch.from_numpy(np.asarray(x, dtype=np.float64))
    outs = []
    for (name, kh, kw, _, cout, s, pad, relu), w, b in zip(ocnn.LAYERS, ws, bs):
        hh, ww = h.shape[1], h.shape[2]
        geom = CB.same_geometry(hh, ww, kh, s) if pad == "SAME" else CB.valid_geometry(hh, ww, kh, s)
        y = CB.emulate_conv_split(h, torch.from_numpy(w), torch.from_numpy(b), geom, CB.ACT_RELU if relu else CB.ACT_NONE)
        outs.append(y.reshape(n, -1).numpy())
        h = y
        if name in ocnn.POOL_AFTER:
            h = torch.from_numpy(ocnn.maxpool3x3s2(y.numpy()))
    return np.concatenate(outs, axis=1)


def scaled(d):
    mx = d.max(axis=1).reshape(-1, 1)
    mn = d.min(axis=1).reshape(-1, 1)
    return (d - mn) * (np.float64(255) / (mx - mn)), mn, mx


def near(s):
    f = s - np.floor(s)
    return np.minimum(f, 1 - f)


def report(tag, x, ws, bs, cols):
    ref = ocnn.features(x, ws, bs)
    emu = emul_features(x, ws, bs)
    s_ref, mn, mx = scaled(ref)
    s_emu, _, _ = scaled(emu)
    err = np.abs(s_emu - s_ref).max(axis=1)
    q_ref, q_emu = ocnn.quantize_int8(ref), ocnn.quantize_int8(emu)
    mism = q_ref != q_emu
    step = ((q_emu.astype(np.int16) - q_ref.astype(np.int16)) & 0xFF)
    zero = near((0.0 - mn) * (255.0 / (mx - mn))).ravel()
    for f in range(x.shape[0]):
        print("%s frame %d: max feature err / range %.2e  max |s_emu - s| %.3e steps  bytes differing %d of %d (gathered %d of %d)  "
              "zero class %.3f steps from an integer (%.1f %% of the features)"
              % (tag, f, np.abs(emu[f] - ref[f]).max() / float(mx[f, 0] - mn[f, 0]), err[f], mism[f].sum(), ref.shape[1],
                 mism[f, cols].sum(), cols.size, zero[f], 100.0 * (ref[f] == 0).mean()), flush=True)
    print("%s: every differing byte is one step modulo 256: %s" % (tag, bool(np.all(np.isin(step[mism], (1, 255))))))
    return float(err.max())


def main():
    ws, bs = ocnn.init_weights(5)
    cols = ocnn.column_indices(ocnn.layer_sizes((192, 240)), 99.59, seed=9)
    if "--frames20" in sys.argv:
        x = np.stack([read_ppm(p)[:, :, ::-1] for p in real_frames.frame_paths()]).astype(np.float64)
        for i in range(0, 20, 5):
            s, mn, mx = scaled(ocnn.features(x[i:i + 5], ws, bs))
            d = near(s[:, cols])
            z = near((0.0 - mn) * (255.0 / (mx - mn))).ravel()
            for f in range(5):
                print("frame %2d: zero class %.4f steps from an integer; gathered bytes within 1.6e-3: %.2f %%, within 1e-2: %.2f %%"
                      % (i + f, z[f], 100 * (d[f] <= 1.6e-3).mean(), 100 * (d[f] <= 1e-2).mean()), flush=True)
        return
    paths = sorted(p for p in real_frames.frame_paths() if os.sep + "frames" + os.sep in p)
    golden = np.stack([read_ppm(p)[:, :, ::-1] for p in paths]).astype(np.float64)
    rnd = np.random.RandomState(2).randint(0, 256, size=(3, 192, 240, 3)).astype(np.float64)
    worst = max(report("golden", golden, ws, bs, cols), report("random", rnd, ws, bs, cols))
    print("largest |s_emulated - s| over the six frames: %.3e steps; W = 8 x that = %.3e" % (worst, 8 * worst))


if __name__ == "__main__":
    main()
