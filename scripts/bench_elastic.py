#!/usr/bin/env python3
"""Timing of the elastic sequence search (dlc_sequence_elastic_topk) on an MI355X against its yardstick, the linear search
(dlc_sequence_topk) at the same L with V = d_max - d_min + 1 slopes (velocities d_min .. d_max) on the same matrix: the
two alternate call by call in one process, median of 20 calls each after 3 warm-ups, HIP events.

Shapes -- 1063 x 1063 fp64 (the reference's dataset) and (32 + L - 1) x 100 000 fp64 and int64 with row0 = L - 1 and
limit_step 1 (a streamed batch against a long map), each at L = 10 with steps (0, 2); 1063 x 1063 fp64 once more at L = 64
with steps (0, 8).  k = 5.  Then every detector's 32-frame step over 1063 frames with sequence=10 against sequence=10,
steps=(0, 2), alternating.      usage: python scripts/bench_elastic.py [--json OUT] [--no-detector]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import deeploopcloser_amd as dlc                                                          # noqa: E402

WARMUP, REPEATS, K = 3, 20, 5


def timed_pair(fa, fb):
    """Median milliseconds of fa() and of fb(), called in turn, each between two events on the current stream."""
    for _ in range(WARMUP):
        fa()
        fb()
    torch.cuda.synchronize()
    ms = ([], [])
    for _ in range(REPEATS):
        for fn, acc in ((fa, ms[0]), (fb, ms[1])):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            acc.append(a.elapsed_time(b))
    return statistics.median(ms[0]), statistics.median(ms[1])


def bench_shapes(eng):
    out = []
    g = torch.Generator(device=eng.device)
    g.manual_seed(1)
    cases = [("1063x1063 fp64", 1063, 1063, torch.float64, 10, (0, 2)),
             ("(32+L-1)x100000 fp64, limit_step 1", None, 100000, torch.float64, 10, (0, 2)),
             ("(32+L-1)x100000 int64, limit_step 1", None, 100000, torch.int64, 10, (0, 2)),
             ("1063x1063 fp64", 1063, 1063, torch.float64, 64, (0, 8))]
    for name, rows, n, dtype, L, steps in cases:
        r = rows if rows is not None else 32 + L - 1
        kw = dict(limit0=-30, limit_step=1) if rows is not None else dict(limit0=n - r - 30, limit_step=1)
        row0 = 0 if rows is not None else L - 1
        lower = dtype == torch.int64
        if dtype == torch.int64:
            m = torch.randint(0, 20000, (r, n), generator=g, device=eng.device, dtype=dtype)
        else:
            m = torch.randn((r, n), generator=g, device=eng.device, dtype=dtype)
        off = dlc.slope_offsets(L, float(steps[0]), float(steps[1]), 1.0)
        assert off.shape[0] == steps[1] - steps[0] + 1
        el, lin = timed_pair(lambda: eng.sequence_elastic_topk(m, L, steps, k=K, row0=row0, lower_is_better=lower, **kw),
                             lambda: eng.sequence_topk(m, L, off, k=K, row0=row0, lower_is_better=lower, **kw))
        out.append({"shape": name, "rows": r, "n": n, "L": L, "steps": list(steps), "slopes": int(off.shape[0]), "k": K,
                    "elastic_ms": el, "linear_ms": lin, "ratio": el / lin})
        del m
    return out


def detectors(eng, frames):
    """name -> (make(**kw) -> detector, the frames' descriptors)"""
    g = torch.Generator(device=eng.device)
    g.manual_seed(2)
    p, h = 30, 2500
    ds = torch.sigmoid(4.0 * torch.randn((frames, p, h), generator=g, device=eng.device, dtype=torch.float64))
    score = eng.distinctive_score(ds, 0.5, 0.2)
    x8 = torch.randint(-128, 128, (frames, 4096), generator=g, device=eng.device, dtype=torch.int8)
    xf = torch.randn((frames, 256), generator=g, device=eng.device, dtype=torch.float32)
    return {
        "SdavLoopClosureDetector": (lambda **kw: dlc.SdavLoopClosureDetector(score, patches=p, width=h, k=K, exclusion=30,
                                                                             capacity=frames, **kw), ds),
        "CnnVtlLoopClosureDetector": (lambda **kw: dlc.CnnVtlLoopClosureDetector(4096, k=K, exclusion=30, capacity=frames, **kw), x8),
        "LoopClosureDetector": (lambda **kw: dlc.LoopClosureDetector(256, k=K, exclusion=30, capacity=frames, **kw), xf),
    }


def bench_detectors(eng, frames=1063, batch=32, rounds=5):
    """Milliseconds per 32-frame step (the time of `frames` frames through query_and_insert in batches of `batch`, over the
    number of batches) with sequence=10 and with sequence=10, steps=(0, 2), alternating; the median over `rounds` after
    one warm-up round of each."""
    out = []
    for name, (make, x) in detectors(eng, frames).items():
        def one(**kw):
            det = make(sequence=10, **kw)
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for lo in range(0, frames, batch):
                det.query_and_insert(x[lo:lo + batch])
            b.record()
            b.synchronize()
            return a.elapsed_time(b) / ((frames + batch - 1) // batch)

        ms = ([], [])
        for r in range(rounds + 1):
            for kw, acc in ((dict(), ms[0]), (dict(steps=(0, 2)), ms[1])):
                t = one(**kw)
                if r:
                    acc.append(t)
        lin, el = statistics.median(ms[0]), statistics.median(ms[1])
        out.append({"detector": name, "frames": frames, "batch": batch, "linear_step_ms": lin, "elastic_step_ms": el,
                    "ratio": el / lin})
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--json", help="also write the results to this file")
    ap.add_argument("--no-detector", action="store_true")
    args = ap.parse_args()
    eng = dlc.default_engine()
    res = {"device": torch.cuda.get_device_name(eng.device), "shapes": bench_shapes(eng)}
    if not args.no_detector:
        res["detectors"] = bench_detectors(eng)
    for r in res["shapes"]:
        print("%-40s L=%-2d steps=(%d, %d)  elastic %.3f ms   linear, %d slopes %.3f ms   x %.2f"
              % (r["shape"], r["L"], r["steps"][0], r["steps"][1], r["elastic_ms"], r["slopes"], r["linear_ms"], r["ratio"]))
    for d in res.get("detectors", []):
        print("%-26s %d-frame step over %d frames, sequence=10: %.3f ms with the lines, %.3f ms with steps=(0, 2)   x %.2f"
              % (d["detector"], d["batch"], d["frames"], d["linear_step_ms"], d["elastic_step_ms"], d["ratio"]))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
