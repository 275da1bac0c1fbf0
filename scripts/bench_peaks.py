"""Timing of the windowed peak top-k of score rows (dlc_peak_topk_rows) beside dlc_topk_rows_f64 on the same rows (GPU
box only).  One JSON line per case, all in one process: the time from device events, median of 20 calls after 3
warm-ups, the two calls timed ALTERNATELY (peaks, top-k, peaks, ...) so that a drift of the clock falls on both.

Both calls read every offered cell once -- rows * n * 8 bytes -- and write 16 bytes per slot; the peak selection adds
16 bytes per 256 columns written and read back k times (its chunk table) and a second launch.  At suppress = 0, k = 5
the two should be near parity; the one-workgroup-per-row yardstick reads its row k times, so it falls behind with k
and with n.  There is no pass bar.

  shapes    32 x 100 000 (a streamed batch against a large store) and 1063 x 1063 (an all-vs-all matrix of the
            reference's data set), fp64 and int64 (the yardstick then runs on the same values as fp64)
  cases     k = 5 with suppress 0, 5, 32; k = 128 with suppress 5
  detector  one streamed step of CnnVtlLoopClosureDetector(sequence=10), 32 frames against ~1100 key-frames, with and
            without suppress=5: host clock around a step that ends in a device synchronise, median of the steps

    python scripts/bench_peaks.py [--quick]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import deeploopcloser_amd as dlc  # noqa: E402

SHAPES = [(32, 100_000), (1063, 1063)]
CASES = [(5, 0), (5, 5), (5, 32), (128, 5)]                          # (k, suppress)


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


def detector_steps_ms(dev, suppress, steps, g):
    """Median wall-clock of a 32-frame step behind 1056 resident key-frames."""
    det = dlc.CnnVtlLoopClosureDetector(4096, k=5, exclusion=30, capacity=4096, sequence=10, suppress=suppress)
    frames = torch.randint(-128, 128, (1056 + 32 * steps, 4096), dtype=torch.int8, device=dev, generator=g)
    for lo in range(0, 1056, 32):                                    # (the first steps are the warm-up)
        det.query_and_insert(frames[lo:lo + 32])
    torch.cuda.synchronize()
    ms = []
    for lo in range(1056, frames.shape[0], 32):
        t0 = time.perf_counter()
        det.query_and_insert(frames[lo:lo + 32])
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return sorted(ms)[len(ms) // 2]


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="fewer repetitions")
    args = ap.parse_args(argv)
    eng = dlc.default_engine()
    dev = eng.device
    g = torch.Generator(device=dev).manual_seed(0)
    reps = 5 if args.quick else 20
    for rows, n in SHAPES:
        for dtype in (torch.float64, torch.int64):
            if dtype == torch.int64:
                m = torch.randint(0, 4097, (rows, n), dtype=torch.int64, device=dev, generator=g)
            else:
                m = torch.randn((rows, n), dtype=torch.float64, device=dev, generator=g)
            same = m.to(torch.float64)                               # the yardstick's rows: the same values as fp64
            for k, suppress in CASES:
                fns = {"peaks": lambda: eng.peak_topk_rows(m, k, suppress),
                       "topk": lambda: eng.topk_rows_f64(same, n, 0, k)}
                t = time_alternately_ms(fns, 3, reps)
                med, best = t["peaks"]
                print(json.dumps({"what": "peak_topk_rows", "rows": rows, "n": n, "dtype": str(dtype).replace("torch.", ""),
                                  "k": k, "suppress": suppress, "calls": reps, "ms_median": round(med, 4),
                                  "ms_best": round(best, 4), "bytes_read_once": rows * n * 8,
                                  "topk_rows_f64_ms_median": round(t["topk"][0], 4),
                                  "ratio_to_topk_rows_f64": round(med / t["topk"][0], 2)}), flush=True)
            del m, same
            torch.cuda.empty_cache()
    steps = 4 if args.quick else 16
    plain, apart = detector_steps_ms(dev, None, steps, g), detector_steps_ms(dev, 5, steps, g)
    print(json.dumps({"what": "CnnVtlLoopClosureDetector step", "frames": 32, "key_frames": 1056, "sequence": 10, "k": 5,
                      "steps": steps, "ms_median_plain": round(plain, 4), "ms_median_suppress_5": round(apart, 4)}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
