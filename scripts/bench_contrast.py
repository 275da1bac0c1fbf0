"""Timing of the local contrast normalisation of score rows (dlc_contrast_rows) beside a device-to-device copy that moves
the same bytes (GPU box only).  One JSON line per (shape, radius), all in one process: the time from device events,
median of 20 launches after 3 warm-ups, the call and the copy timed ALTERNATELY (call, copy, call, ...) so that a drift of
the clock falls on both.

The kernel reads every offered cell once (8 bytes; the halo of a slab comes from the caches) and writes it once (8
bytes): rows * n * 16 bytes when every cell is offered.  The copy beside it moves the same bytes -- an int64 [rows, n]
tensor copied into another, 8 bytes read and 8 written per cell -- so `ratio_to_copy` = 1 would be the memory floor.
There is no pass bar: the windows are summed per cell in fp64 (2 (2 R + 1) dependent additions, two divisions and a
square root per cell), so the call is bound by the fp64 pipe and not by HBM, the more the larger the radius.

  shapes   1063 x 1063 int64 (an all-vs-all matrix of the reference's data set), 32 x 4096 int64 with limit_step = 1 (a
           streamed batch: row r offers 4096 - 32 + r cells) and 256 x 100 000 fp64
  radius   5 (SeqSLAM's R_window = 10) and 32

    python scripts/bench_contrast.py [--quick]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import deeploopcloser_amd as dlc  # noqa: E402

SHAPES = [(1063, 1063, torch.int64, None, 0), (32, 4096, torch.int64, 4096 - 32, 1), (256, 100_000, torch.float64, None, 0)]
RADII = (5, 32)


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


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="fewer repetitions")
    args = ap.parse_args(argv)
    eng = dlc.default_engine()
    dev = eng.device
    g = torch.Generator(device=dev).manual_seed(0)
    reps = 5 if args.quick else 20
    for rows, n, dtype, limit0, step in SHAPES:
        if dtype == torch.int64:
            m = torch.randint(0, 4097, (rows, n), dtype=torch.int64, device=dev, generator=g)
        else:
            m = torch.randn((rows, n), dtype=torch.float64, device=dev, generator=g)
        out = torch.empty((rows, n), dtype=torch.float64, device=dev)
        src = torch.zeros((rows, n), dtype=torch.int64, device=dev)            # 8 bytes read + 8 written per cell
        dst = torch.empty_like(src)
        for radius in RADII:
            fns = {"contrast": lambda: eng.contrast_rows(m, radius, limit0=limit0, limit_step=step, out=out),
                   "copy": lambda: dst.copy_(src)}
            t = time_alternately_ms(fns, 3, reps)
            med, best = t["contrast"]
            print(json.dumps({"what": "contrast_rows", "rows": rows, "n": n, "dtype": str(dtype).replace("torch.", ""),
                              "limit0": limit0, "limit_step": step, "radius": radius, "launches": reps,
                              "ms_median": round(med, 4), "ms_best": round(best, 4), "copy_bytes_moved": rows * n * 16,
                              "copy_ms_median": round(t["copy"][0], 4), "ratio_to_copy": round(med / t["copy"][0], 2)}), flush=True)
        del m, out, src, dst
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
