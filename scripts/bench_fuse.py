"""Timing of the multi-descriptor fusion of score rows (dlc_fuse_rows) beside the same quantity composed from torch ops on
the device -- what a caller would write without it (GPU box only).  One JSON line per (shape, m, norm, plan), all in one
process: the time from device events, median of 20 calls after 3 warm-ups, the plans and the torch composition timed
ALTERNATELY (row, slab, auto, torch, row, ...) so that a drift of the clock falls on all of them.

  shapes   1063 x 1063 (an all-vs-all matrix of the reference's data set), 32 x 100 000 (a streamed batch against a large
           map) and 1 x 1 000 000 (one frame against a very large one)
  sources  m = 2: fp64 scores + int64 distances (lower is better); m = 3: one more int64 source
  bytes    the algorithm's: every source read ONCE, m * rows * n * 8, plus rows * n * 8 written; `gbps` is that over the
           median time, `hbm_share` its share of the 8 TB/s of HBM3E (the kernel's roofline: it reads the sources two or
           three times, the re-reads meant for L2)
  torch    none: the weighted sum; zscore: (x - mean) / std(unbiased) per row; minmax: (x - min) / (max - min) per row;
           fp64 throughout.  It does not sum in the TREE order, so its bits depend on torch's reduction; it is the yardstick
           for time only.  `vs_torch` = torch's median over the plan's (above 1: the kernel is faster).

After the timings, on the 20 real frames with the revisit an eighth of the width to the side (columns 0..191 as key-frames,
24..215 as queries -- the scene of the lateral-shift SAD), one line `real_frames`: of 20 queries, how many have the true
key-frame as nearest neighbour by each member alone (plain SAD, cnn_vtl distance, cosine) and by their z-score fusion.

--crossover times ROW against SLAB (zscore, m = 2) over rows in 16 .. 2048 and n in 4096 .. 262144 instead: the grid the
AUTO rule of dlc_fuse_rows (include/dlc.h) is read from, one line `crossover` per cell.

    python scripts/bench_fuse.py [--quick] [--skip-frames] [--crossover]
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

SHAPES = [(1063, 1063), (32, 100_000), (1, 1_000_000)]
NORMS = ("zscore", "minmax", "none")
PLANS = ("row", "slab", "auto")
HBM_BYTES_PER_S = 8.0e12


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


def torch_fusion(sources, weights, lower, norm):
    """The composition a caller would write: fp64, per-row statistics by torch's own reductions."""
    acc = None
    for s, w, low in zip(sources, weights, lower):
        x = s.to(torch.float64)
        if norm == "zscore":
            u = (x - x.mean(dim=1, keepdim=True)) / x.std(dim=1, keepdim=True)
        elif norm == "minmax":
            lo, hi = x.amin(dim=1, keepdim=True), x.amax(dim=1, keepdim=True)
            u = (x - lo) / (hi - lo)
            if low:
                u = 1.0 - u
        else:
            u = x
        if low and norm != "minmax":
            u = -u
        acc = w * u if acc is None else acc + w * u
    return acc


def real_frames_line():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import real_frames
    from deeploopcloser_amd import pipeline
    frames = np.stack([dlc.read_ppm(p) for p in real_frames.frame_paths()])                  # [20, 192, 240, 3] RGB
    keys, queries = np.ascontiguousarray(frames[:, :, :192]), np.ascontiguousarray(frames[:, :, 24:216])
    thumbs = dlc.SeqSlam(size=(32, 64), patch=8, strength=32)
    cnn = dlc.CnnVtl(input_shape=[20] + list(keys.shape[1:]))
    sad = [pipeline.seqslam_descriptors_from_frames(x, thumbs) for x in (keys, queries)]
    deep = [pipeline.cnn_vtl_descriptors_from_frames(np.ascontiguousarray(x[..., ::-1]), cnn) for x in (keys, queries)]
    rows = {"sad": dlc.default_engine().sad_rows(sad[1], sad[0]),
            "distance": dlc.default_engine().cnnvtl_distance_rows(deep[1], deep[0])}
    db = dlc.KeyframeDatabase(deep[0].to(torch.float32), center=True)
    rows["cosine"] = db.scores_f64(deep[1].to(torch.float32))
    truth = torch.arange(20, device=rows["sad"].device)
    hits = {"sad": int((rows["sad"].argmin(1) == truth).sum()), "distance": int((rows["distance"].argmin(1) == truth).sum()),
            "cosine": int((rows["cosine"].argmax(1) == truth).sum())}
    for members in (("sad", "distance"), ("sad", "cosine"), ("sad", "distance", "cosine")):
        fused = dlc.fuse_scores([rows[m] for m in members], lower_is_better=[m != "cosine" for m in members])
        hits["+".join(members)] = int((fused.argmax(1) == truth).sum())
    return {"what": "real_frames", "queries": 20, "shift_px": 24, "nearest_neighbour_hits": hits}


def crossover(eng, reps):
    dev = eng.device
    g = torch.Generator(device=dev).manual_seed(1)
    for n in (4096, 8192, 16384, 65536, 262144):
        for rows in (16, 64, 256, 512, 1024, 2048):
            if rows * n > 1 << 28:
                continue
            srcs = [torch.randn((rows, n), dtype=torch.float64, device=dev, generator=g),
                    torch.randint(0, 1 << 20, (rows, n), dtype=torch.int64, device=dev, generator=g)]
            out = torch.empty((rows, n), dtype=torch.float64, device=dev)
            fns = {p: (lambda p=p: eng.fuse_rows(srcs, None, [False, True], "zscore", out=out, plan=p)) for p in PLANS}
            t = time_alternately_ms(fns, 3, reps)
            print(json.dumps({"what": "crossover", "rows": rows, "n": n, "row_ms": round(t["row"][0], 4),
                              "slab_ms": round(t["slab"][0], 4), "auto_ms": round(t["auto"][0], 4),
                              "faster": "row" if t["row"][0] <= t["slab"][0] else "slab"}), flush=True)
            del srcs, out
            torch.cuda.empty_cache()


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="fewer repetitions")
    ap.add_argument("--skip-frames", action="store_true", help="timings only")
    ap.add_argument("--crossover", action="store_true", help="the ROW / SLAB grid behind the AUTO rule instead")
    args = ap.parse_args(argv)
    eng = dlc.default_engine()
    dev = eng.device
    g = torch.Generator(device=dev).manual_seed(0)
    reps = 5 if args.quick else 20
    print(json.dumps({"what": "device", "name": torch.cuda.get_device_name(dev),
                      "compute_units": torch.cuda.get_device_properties(dev).multi_processor_count}), flush=True)
    if args.crossover:
        crossover(eng, reps)
        return 0
    for rows, n in SHAPES:
        srcs = [torch.randn((rows, n), dtype=torch.float64, device=dev, generator=g),
                torch.randint(0, 1 << 20, (rows, n), dtype=torch.int64, device=dev, generator=g),
                torch.randint(0, 1 << 14, (rows, n), dtype=torch.int64, device=dev, generator=g)]
        out = torch.empty((rows, n), dtype=torch.float64, device=dev)
        for m in (2, 3):
            sources, weights, lower = srcs[:m], [1.0, 0.5, 2.0][:m], [False, True, True][:m]
            nbytes = (m + 1) * rows * n * 8
            for norm in NORMS:
                fns = {p: (lambda p=p: eng.fuse_rows(sources, weights, lower, norm, out=out, plan=p)) for p in PLANS}
                fns["torch"] = lambda: torch_fusion(sources, weights, lower, norm)
                t = time_alternately_ms(fns, 3, reps)
                for p in PLANS:
                    med, best = t[p]
                    print(json.dumps({"what": "fuse_rows", "rows": rows, "n": n, "m": m, "norm": norm, "plan": p, "calls": reps,
                                      "ms_median": round(med, 4), "ms_best": round(best, 4), "bytes": nbytes,
                                      "gbps": round(nbytes / med / 1e6, 1), "hbm_share": round(nbytes / (med * 1e-3) / HBM_BYTES_PER_S, 3),
                                      "torch_ms_median": round(t["torch"][0], 4), "vs_torch": round(t["torch"][0] / med, 2)}),
                          flush=True)
        del srcs, out
        torch.cuda.empty_cache()
    if not args.skip_frames:
        print(json.dumps(real_frames_line()), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
