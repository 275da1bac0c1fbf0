"""Timing of the cosine score rows (dlc_cosine_score_rows) beside the calls they are measured against, and of the
streaming cosine detector with and without sequence=L (GPU box only).  One JSON line per shape, all in one process: the
time from device events, median of 20 after 3 warm-ups, the calls of a shape timed ALTERNATELY (rows, scores, top-k,
rows, ...) on the same operands so that a drift of the clock falls on all of them, and the floor the shape sets:

    fp64  one fp64 fma per product at the least: Q * N * D / 64 wave instructions at 4 cycles per instruction and SIMD
          over 256 CUs x 4 SIMDs x clock.  The conversions to fp64 come on top (two instructions per element, amortised
          by the register tile: at 4 x 4 pairs per wave they equal the fmas, so half the floor is this kernel's ceiling).

`frac_of_floor` = floor / measured time.  The clock is a parameter (--clock-ghz, default 2.4): the chip runs below it
under its power cap, so the real floor is higher than the one reported.

  1. "cosine_rows": the call (scores and keys) at D = 4096 bf16, Q in {1, 32, 256}, N in {1063, 100 000}, limits of a
     streamed batch (limit0 = N - Q, limit_step = 1); beside it dlc_cosine_scores (the fp32 MFMA block, which only
     chooses candidates) and dlc_cosine_topk_older at k = 20 (the fused path of sequence=None) on the same operands.
  2. "detector_step": one LoopClosureDetector.query_and_insert of 32 frames against 1063 resident key-frames,
     sequence=None (the fused top-k) and sequence=10 (key rows + sequence search), ALTERNATING, five rounds each of
     200 steps, host clock around a synchronised round (the store grows by 32 frames a step; the resident frames are
     stored without being searched: with sequence=10 the first steps' context rows hold no keys, which changes what is
     ranked and not what it costs).

    python scripts/bench_cosine_rows.py [--quick] [--clock-ghz 2.4]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import deeploopcloser_amd as dlc  # noqa: E402

D = 4096
K = 20


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
    ap.add_argument("--clock-ghz", type=float, default=2.4)
    ap.add_argument("--quick", action="store_true", help="fewer repetitions")
    args = ap.parse_args(argv)
    eng = dlc.default_engine()
    dev = eng.device
    g = torch.Generator(device=dev).manual_seed(0)
    reps = 5 if args.quick else 20
    simds = 256 * 4 * args.clock_ghz * 1e9
    for n in (1063, 100_000):
        db = eng.normalize(torch.randn((n, D), dtype=torch.float32, device=dev, generator=g), "bf16")
        for q in (1, 32, 256):
            qs = eng.normalize(torch.randn((q, D), dtype=torch.float32, device=dev, generator=g), "bf16")
            out_s = torch.empty((q, n), dtype=torch.float64, device=dev)
            out_k = torch.empty((q, n), dtype=torch.int64, device=dev)
            fns = {"rows": lambda: eng.cosine_score_rows(qs, db, limit0=n - q, limit_step=1, out=out_s, out_keys=out_k),
                   "scores": lambda: eng.cosine_scores(qs, db),
                   "topk": lambda: eng.match_topk(qs, db, K, older_than=n - q)}
            t = time_alternately_ms(fns, 3, reps)
            med, best = t["rows"]
            pairs = q * (n - q) + q * (q - 1) // 2                     # what the limits offer
            floor = pairs * D / 64 * 4 / simds * 1e3
            print(json.dumps({"what": "cosine_rows", "N": n, "D": D, "Q": q, "dtype": "bf16", "ms_median": round(med, 4),
                              "ms_best": round(best, 4), "scores_f32_ms_median": round(t["scores"][0], 4),
                              "topk_k": K, "topk_ms_median": round(t["topk"][0], 4),
                              "rows_over_scores": round(med / t["scores"][0], 2), "rows_over_topk": round(med / t["topk"][0], 2),
                              "floor_fp64_ms": round(floor, 4), "clock_ghz": args.clock_ghz,
                              "frac_of_floor": round(floor / med, 3)}), flush=True)
        del db
        torch.cuda.empty_cache()
    # the streaming detector: one batch appended and searched, against `resident` frames already stored
    b, steps, rounds, resident = 32, (40 if args.quick else 200), 5, 1063
    base = torch.randn((resident, D), dtype=torch.float32, device=dev, generator=g)
    batch = torch.randn((b, D), dtype=torch.float32, device=dev, generator=g)
    dets = {}
    for sequence in (None, 10):
        det = dlc.LoopClosureDetector(D, k=5, exclusion=30, capacity=resident + b * (steps * rounds + 8), sequence=sequence)
        det.db.append(base)                          # resident frames stored without being searched
        for _ in range(3):
            det.query_and_insert(batch)
        dets[sequence] = det
    host = {sequence: [] for sequence in dets}
    for _ in range(rounds):
        for sequence, det in dets.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                det.query_and_insert(batch)
            torch.cuda.synchronize()
            host[sequence].append((time.perf_counter() - t0) / steps * 1e3)
    for sequence, ms in host.items():
        med = sorted(ms)[len(ms) // 2]
        print(json.dumps({"what": "detector_step", "resident_at_start": resident, "batch": b, "k": 5, "D": D,
                          "sequence": sequence, "rounds": rounds, "steps_per_round": steps,
                          "ms_per_batch_host_median": round(med, 4), "ms_per_batch_host_rounds": [round(m, 4) for m in ms],
                          "frames_per_s": round(b / med * 1e3, 1)}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
