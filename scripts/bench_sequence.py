#!/usr/bin/env python3
"""Timing of the sequence search (dlc_sequence_topk) on an MI355X: the median of 20 calls after 3 warm-ups, HIP events.

Three shapes -- 1063 x 1063 fp64 (the reference's dataset), (32 + L - 1) x 100 000 fp64 with limit_step 1 (a streamed batch
against a long map) and 20 000 x 20 000 int64 (a cnn_vtl distance matrix) -- each at L = 10 with the default slopes and at
L = 1 with one slope, each against two yardsticks measured in the same process: Engine.topk_rows_f64 on the same rows (the
existing ranking; fp64 only: at L = 1 the difference is what the fusion costs) and the time to read the matrix once at the
device-copy rate the script measures itself.  Then SdavLoopClosureDetector.query_and_insert per 1063 frames in batches of
32, with and without sequence=10, alternating.      usage: python scripts/bench_sequence.py [--json OUT]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import deeploopcloser_amd as dlc                                                          # noqa: E402

WARMUP, REPEATS, K = 3, 20, 5


def timed(fn, warmup=None, repeats=None):
    """Median milliseconds of fn() between two events on the current stream."""
    warmup, repeats = WARMUP if warmup is None else warmup, REPEATS if repeats is None else repeats
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms)


def copy_rate(eng):
    """Bytes read per second by a device-to-device copy of 1 GiB (it reads and writes: the read side is half its traffic)."""
    src = torch.empty(1 << 30, dtype=torch.uint8, device=eng.device)
    dst = torch.empty_like(src)
    ms = timed(lambda: dst.copy_(src))
    return src.numel() / (ms * 1e-3)


def bench_shapes(eng, rate):
    out = []
    g = torch.Generator(device=eng.device)
    g.manual_seed(1)
    shapes = [("1063x1063 fp64", 1063, 1063, torch.float64, dict(limit0=-30, limit_step=1), False),
              ("(32+L-1)x100000 fp64, limit_step 1", None, 100000, torch.float64, None, False),
              ("20000x20000 int64", 20000, 20000, torch.int64, dict(), True)]
    for name, rows, n, dtype, limits, lower in shapes:
        for L in (10, 1):
            r = rows if rows is not None else 32 + L - 1
            kw = limits if limits is not None else dict(limit0=n - r - 30, limit_step=1)
            row0 = 0 if rows is not None else L - 1
            if dtype == torch.int64:
                m = torch.randint(0, 20000, (r, n), generator=g, device=eng.device, dtype=dtype)
            else:
                m = torch.randn((r, n), generator=g, device=eng.device, dtype=dtype)
            off = dlc.slope_offsets(L)
            seq = timed(lambda: eng.sequence_topk(m, L, off, k=K, row0=row0, lower_is_better=lower, **kw))
            rec = {"shape": name, "rows": r, "n": n, "L": L, "slopes": int(off.shape[0]), "k": K, "sequence_topk_ms": seq,
                   "read_once_ms": m.numel() * m.element_size() / rate * 1e3}
            if dtype == torch.float64:
                sub = m[row0:]
                l0 = kw.get("limit0", n) + row0 * kw.get("limit_step", 0)
                rec["topk_rows_f64_ms"] = timed(lambda: eng.topk_rows_f64(sub, l0, kw.get("limit_step", 0), K))
            out.append(rec)
            del m
    return out


def bench_detector(eng, frames=1063, batch=32, p=30, h=2500, rounds=5):
    """Milliseconds per `frames` frames through query_and_insert in batches of `batch`, with and without sequence=10,
    alternating; the median over `rounds` after one warm-up round of each."""
    g = torch.Generator(device=eng.device)
    g.manual_seed(2)
    ds = torch.sigmoid(4.0 * torch.randn((frames, p, h), generator=g, device=eng.device, dtype=torch.float64))
    score = eng.distinctive_score(ds, 0.5, 0.2)

    def one(sequence):
        det = dlc.SdavLoopClosureDetector(score, patches=p, width=h, k=K, exclusion=30, capacity=frames, sequence=sequence)
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for lo in range(0, frames, batch):
            det.query_and_insert(ds[lo:lo + batch])
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    ms = {None: [], 10: []}
    for r in range(rounds + 1):
        for sequence in (None, 10):
            t = one(sequence)
            if r:
                ms[sequence].append(t)
    return {"frames": frames, "batch": batch, "plain_ms": statistics.median(ms[None]), "sequence10_ms": statistics.median(ms[10]),
            "plain_all_ms": ms[None], "sequence10_all_ms": ms[10]}


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--json", help="also write the results to this file")
    ap.add_argument("--no-detector", action="store_true")
    ap.add_argument("--trace", action="store_true",
                    help="for a run under rocprofv3 --kernel-trace --stats: one call per shape and L, then the detector with "
                         "sequence=10 over 1063 frames twice; nothing is timed")
    args = ap.parse_args()
    eng = dlc.default_engine()
    if args.trace:
        global WARMUP, REPEATS
        WARMUP, REPEATS = 0, 1
        bench_shapes(eng, 1.0)
        ds = torch.sigmoid(4.0 * torch.randn((1063, 30, 2500), device=eng.device, dtype=torch.float64))
        for _ in range(2):
            det = dlc.SdavLoopClosureDetector(eng.distinctive_score(ds, 0.5, 0.2), k=K, exclusion=30, capacity=1063, sequence=10)
            for lo in range(0, 1063, 32):
                det.query_and_insert(ds[lo:lo + 32])
        torch.cuda.synchronize()
        return 0
    rate = copy_rate(eng)
    res = {"device": torch.cuda.get_device_name(eng.device), "copy_read_GBps": rate / 1e9, "shapes": bench_shapes(eng, rate)}
    if not args.no_detector:
        res["detector"] = bench_detector(eng)
    print("device copy: %.0f GB/s read (+ as much written)" % (rate / 1e9))
    for r in res["shapes"]:
        base = ("%.3f" % r["topk_rows_f64_ms"]) if "topk_rows_f64_ms" in r else "n/a"
        print("%-40s L=%-2d slopes=%d  sequence_topk %.3f ms   topk_rows_f64 %s ms   one read of the matrix %.3f ms"
              % (r["shape"], r["L"], r["slopes"], r["sequence_topk_ms"], base, r["read_once_ms"]))
    if "detector" in res:
        d = res["detector"]
        print("SdavLoopClosureDetector, %d frames in batches of %d: %.1f ms plain, %.1f ms with sequence=10 (%+.1f %%)"
              % (d["frames"], d["batch"], d["plain_ms"], d["sequence10_ms"], 100.0 * (d["sequence10_ms"] / d["plain_ms"] - 1.0)))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
