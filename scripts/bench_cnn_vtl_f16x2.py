"""CnnVtl.transform_tensor in the fp64 mode and in the f16x2 tolerance mode, ALTERNATING in one process on one device (GPU
box only; the boxes of a pool differ by several per cent, so only a ratio taken inside one run means anything).

1063 tiled real frames of 192 x 240 resident on the device, HIP events, 3 warm-ups, median of 20.  One JSON line each for
  * transform_tensor, both modes, and their ratio (the bar for the mode is 2 x);
  * BASELINE configs[2] end to end through pipeline.cnn_vtl_distance_matrix_from_frames (device-resident), both modes;
  * the f16x2 mode's per-layer split: dlc_cnnvtl_layers_split on one layer at a time, fed that layer's real input (the
    frame exponents, im2col + piece split and the split GEMM; not the max-pool behind it, not the min / max fold).

    python scripts/bench_cnn_vtl_f16x2.py [--frames 1063] [--reps 20] [--once f16x2|float64]   (--once: one call, for a profiler)
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch  # noqa: E402

import deeploopcloser_amd as dlc  # noqa: E402
from deeploopcloser_amd import pipeline  # noqa: E402
import real_frames  # noqa: E402


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def alternating(fns, warmup, reps):
    """{name: median ms} with the candidates taking turns inside every repetition."""
    for _ in range(warmup):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            out[k].append(timed(f))
    return {k: sorted(v)[len(v) // 2] for k, v in out.items()}, {k: min(v) for k, v in out.items()}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1063)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--once", choices=["f16x2", "float64"], default=None)
    args = ap.parse_args(argv)
    n = args.frames
    x8 = real_frames.tiled_bgr_frames(dlc, n).to(torch.uint8)
    x64 = x8.to(torch.float64)
    nets = {"float64": dlc.CnnVtl(input_shape=[n, 192, 240, 3], seed=5, mask_seed=9),
            "f16x2": dlc.CnnVtl(input_shape=[n, 192, 240, 3], seed=5, mask_seed=9, dtype="f16x2")}
    if args.once:
        net = nets[args.once]
        for _ in range(2):
            net.transform_tensor(x64)
        torch.cuda.synchronize()
        return 0
    base = {"frames": n, "frame": "192x240", "device": torch.cuda.get_device_name(0), "warmup": 3, "reps": args.reps}
    med, best = alternating({"float64": lambda: nets["float64"].transform_tensor(x64),
                             "f16x2": lambda: nets["f16x2"].transform_tensor(x64),
                             "f16x2_uint8_in": lambda: nets["f16x2"].transform_tensor(x8)}, 3, args.reps)
    print(json.dumps(dict(base, what="transform_tensor", ms_median={k: round(v, 3) for k, v in med.items()},
                          ms_best={k: round(v, 3) for k, v in best.items()},
                          speedup_f16x2=round(med["float64"] / med["f16x2"], 3))), flush=True)
    med, best = alternating({k: (lambda net=net: pipeline.cnn_vtl_distance_matrix_from_frames(x64, net, device_result=True))
                             for k, net in nets.items()}, 3, args.reps)
    print(json.dumps(dict(base, what="configs[2] end to end, device-resident", ms_median={k: round(v, 3) for k, v in med.items()},
                          ms_best={k: round(v, 3) for k, v in best.items()},
                          speedup_f16x2=round(med["float64"] / med["f16x2"], 3))), flush=True)
    # per-layer split of the tolerance mode
    net = nets["f16x2"]
    eng = net.engine
    geom, s2d, panels = net._split_plan()
    _, feats = net.features_split(x8)
    xin = x8.to(torch.float32).reshape(n, 192 // s2d, s2d, 240 // s2d, s2d, 3).permute(0, 1, 3, 2, 4, 5).reshape(n, 192 // s2d, 240 // s2d, -1)
    in_shape = tuple(xin.shape[1:])
    layers = {}
    for l, g in enumerate(geom):
        xin = xin.contiguous()
        m, b = alternating({"l": lambda: eng.cnnvtl_layers_split(xin, in_shape, geom, l, l, panels, net._b)}, 3, args.reps)
        M, K, N = n * g[7] * g[8], g[0] * g[1] * g[2], g[3]
        layers["conv%d" % (l + 1)] = {"ms_median": round(m["l"], 3), "M": M, "K": K, "N": N,
                                      "tflops_3_products": round(3 * 2.0 * M * K * N / m["l"] / 1e9, 1)}
        xin = feats[l]
        if g[10]:
            xin = torch.nn.functional.max_pool2d(xin.permute(0, 3, 1, 2), 3, 2).permute(0, 2, 3, 1)
    print(json.dumps(dict(base, what="f16x2 per layer (exponents + im2col/split + GEMM)", layers=layers,
                          ms_sum=round(sum(v["ms_median"] for v in layers.values()), 3))), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
