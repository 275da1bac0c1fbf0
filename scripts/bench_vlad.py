"""Timing of the VLAD / k-means entry points (dlc_vlad_assign, dlc_vlad_encode, dlc_kmeans_step) beside the same
quantities composed from torch ops on the device -- what a caller would write without them (GPU box only).  One JSON
line per (shape, call), all in one process: device events, median of 10 calls after 3 warm-ups, the kernel and the torch
composition timed ALTERNATELY so that a drift of the clock falls on both.

  shapes   1063 frames x 30 patches x 2500 (the reference's data set through the reference's SDAV) with 16 and 64 words;
           one streamed frame of the same; 1063 x 30 x 256 with 16 words (the 4096-d row of the headline benchmark)
  torch    torch.cdist in fp64 + argmin; residuals by index_add_ into [frames * K, H] and a per-word norm; the Lloyd
           step by index_add_ + bincount.  Its distances are not DIST's serial chain, so its assignments may differ at
           near-ties and its sums are atomics: it is a clock, not a check.  `vs_torch` = torch's median over the
           kernel's (above 1: the kernel is faster).
  floor    the fp64 vector issue floor of the assignment, rows * K * H * 3 operations (a subtraction, a product, a sum,
           none fused) at half the 78.6 TFLOP/s the data sheet gives for fp64 fma; `floor_share` = floor / median.

After the timings, unless --skip-frames: one line `real_frames` -- the 20 real frames, each against its copy translated
4 px horizontally with the edge pixels replicated, default (untrained) SDAV weights, 16 words fitted on the 20 frames'
600 patches: top-1 hits of the concatenation and of VLAD through KeyframeDatabase, plain and centred.

    python scripts/bench_vlad.py [--quick] [--skip-frames]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import deeploopcloser_amd as dlc  # noqa: E402

SHAPES = [(1063, 30, 2500, 16), (1063, 30, 2500, 64), (1, 30, 2500, 16), (1, 30, 2500, 64), (1063, 30, 256, 16)]
FP64_OPS_PER_S = 78.6e12 / 2


def time_alternately_ms(fns, warmup, reps):
    """{name: (median, best)} of the calls in fns, one of each per round: device events around every call."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    out = {name: [] for name in fns}
    for _ in range(reps):
        for name, fn in fns.items():
            a.record()
            fn()
            b.record()
            b.synchronize()
            out[name].append(a.elapsed_time(b))
    return {name: (sorted(v)[len(v) // 2], min(v)) for name, v in out.items()}


def torch_assign(x, c):
    return torch.cdist(x, c).argmin(dim=1)


def torch_encode(x, c, frames, patches):
    k, h = c.shape
    a = torch_assign(x, c)
    slot = torch.arange(frames, device=x.device).repeat_interleave(patches) * k + a
    out = torch.zeros((frames * k, h), dtype=torch.float64, device=x.device).index_add_(0, slot, x - c[a])
    n = out.norm(dim=1, keepdim=True)
    return (out / torch.where(n == 0, torch.ones_like(n), n)).view(frames, k * h)


def torch_step(x, c):
    k, h = c.shape
    a = torch_assign(x, c)
    sums = torch.zeros((k, h), dtype=torch.float64, device=x.device).index_add_(0, a, x)
    counts = torch.bincount(a, minlength=k)
    return torch.where(counts[:, None] > 0, sums / counts.clamp(min=1)[:, None], c), a


def real_frames_line():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import real_frames
    from deeploopcloser_amd import pipeline
    frames = np.stack([dlc.read_ppm(p) for p in real_frames.frame_paths()])                  # [20, 192, 240, 3] RGB
    shift = 4
    moved = np.concatenate([np.repeat(frames[:, :, :1], shift, axis=2), frames[:, :, :-shift]], axis=2)
    net = dlc.SDAV()
    keys = pipeline.sdav_descriptors_from_frames(frames, net)                                # [20, 30, 2500] on the device
    queries = pipeline.sdav_descriptors_from_frames(np.ascontiguousarray(moved), net)
    vlad = dlc.Vlad(n_words=16, seed=0).fit(keys, iters=20)
    n = frames.shape[0]
    truth = torch.arange(n)

    def hits(d_rows, q_rows, center):
        db = dlc.KeyframeDatabase(d_rows.to(torch.float32), center=center)
        _, i = db.match_topk(db.prepare_queries(q_rows.to(torch.float32)), 1)
        return int((i[:, 0].cpu() == truth).sum())
    res = {}
    for center in (False, True):
        tag = "_centred" if center else ""
        res["concatenation" + tag] = hits(keys.view(n, -1), queries.view(n, -1), center)
        res["vlad" + tag] = hits(vlad.transform_tensor(keys), vlad.transform_tensor(queries), center)
    return {"what": "real_frames", "queries": n, "shift_px": shift, "words": 16, "lloyd_steps": vlad.n_iter_,
            "inertia_first_last": [vlad.inertia_[0], vlad.inertia_[-1]], "top1_hits": res}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="fewer repetitions")
    ap.add_argument("--skip-frames", action="store_true", help="timings only")
    args = ap.parse_args(argv)
    eng = dlc.default_engine()
    dev = eng.device
    g = torch.Generator(device=dev).manual_seed(0)
    reps = 4 if args.quick else 10
    print(json.dumps({"what": "device", "name": torch.cuda.get_device_name(dev),
                      "compute_units": torch.cuda.get_device_properties(dev).multi_processor_count}), flush=True)
    for frames, patches, h, k in SHAPES:
        rows = frames * patches
        x = torch.rand((rows, h), dtype=torch.float64, device=dev, generator=g)              # (sigmoid outputs lie in 0..1)
        c = x[torch.randperm(rows, device=dev, generator=g)[:k]].contiguous() if rows >= k else \
            torch.rand((k, h), dtype=torch.float64, device=dev, generator=g)
        floor_ms = rows * k * h * 3 / FP64_OPS_PER_S * 1e3
        calls = {
            "vlad_assign": (lambda: eng.vlad_assign(x, c), lambda: torch_assign(x, c)),
            "vlad_encode": (lambda: eng.vlad_encode(x, c, patches=patches), lambda: torch_encode(x, c, frames, patches)),
            "kmeans_step": (lambda: eng.kmeans_step(x, c), lambda: torch_step(x, c)),
        }
        for name, (ours, theirs) in calls.items():
            t = time_alternately_ms({"dlc": ours, "torch": theirs}, 3, reps)
            med, best = t["dlc"]
            print(json.dumps({"what": name, "frames": frames, "patches": patches, "H": h, "K": k, "calls": reps,
                              "ms_median": round(med, 4), "ms_best": round(best, 4), "torch_ms_median": round(t["torch"][0], 4),
                              "vs_torch": round(t["torch"][0] / med, 2), "assign_floor_ms": round(floor_ms, 4),
                              "floor_share": round(floor_ms / med, 3)}), flush=True)
        del x, c
        torch.cuda.empty_cache()
    if not args.skip_frames:
        print(json.dumps(real_frames_line()), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
