"""Timing of the rectangular cnn_vtl distance rows (dlc_cnnvtl_distance_rows) beside the calls it is measured against,
and of the streaming detector with and without sequence=L (GPU box only).  One JSON line per shape, all in one process:
the time from device events after a warm-up, the calls of a shape timed ALTERNATELY (rows, top-k, rows, top-k, ...) so
that a drift of the clock falls on both, and the floors the shape sets:

    HBM   N * D bytes of the database read once, plus Q * N * 8 bytes of rows written, at 8 TB/s (peak) and at
          6.0 TB/s (the measured sweep);
    VALU  3 * Q * N * ceil(D / 4) lane-instructions (an xor, a v_xad_u32 and a v_bcnt per word pair) over
          256 CUs x 4 SIMDs x 32 lanes x clock.

`frac_of_binding_floor` = max(HBM floor at 8 TB/s, VALU floor) / measured time.  The clock is a parameter (--clock-ghz,
default 2.4): the chip runs below it under its power cap, so the real floors are higher than the ones reported.

  1. "distance_rows": the call at D = 2243, Q in {1, 32, 256}, N in {1063, 100 000}; beside it dlc_cnnvtl_distance_topk
     (k = 20) on the same operands -- the same tile product with a filter and an insertion where this call has stores:
     `rows_over_topk` is the yardstick -- and, for N = 1063, the (N + Q)^2 dlc_cnnvtl_distance_matrix over [db; queries],
     the only way to those rows before this call.
  2. "detector_step": one CnnVtlLoopClosureDetector.query_and_insert of 32 frames against 1063 and 100 000 resident
     key-frames, sequence=None (the fused top-k) and sequence=10 (rows + sequence search), host clock around a
     synchronised run of 200 steps (the store grows by 32 frames a step; the resident frames are stored without being
     searched: with sequence=10 the first steps' context rows hold no distances, which changes what is ranked and not
     what it costs).

    python scripts/bench_distance_rows.py [--quick] [--clock-ghz 2.4]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import deeploopcloser_amd as dlc  # noqa: E402

D_REF = 2243                   # the reference's 192 x 240 frame width of the descriptor
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
    lanes = 256 * 4 * 32 * args.clock_ghz * 1e9
    for n in (1063, 100_000):
        db = torch.randint(-128, 128, (n, D_REF), dtype=torch.int8, device=dev, generator=g)
        db = eng._rows16(db, D_REF)                     # stored rows: 2256 bytes apart, as CnnVtlKeyframeDatabase keeps them
        for q in (1, 32, 256):
            qs = db[torch.randint(0, n, (q,), device=dev, generator=g)].clone()
            out = torch.empty((q, n), dtype=torch.int64, device=dev)
            fns = {"rows": lambda: eng.cnnvtl_distance_rows(qs, db, d=D_REF, out=out),
                   "topk": lambda: eng.cnnvtl_distance_topk(qs, db, K, d=D_REF)}
            if n == 1063:
                both = torch.cat([db, qs])
                square = torch.empty((n + q, n + q), dtype=torch.int64, device=dev)
                fns["matrix"] = lambda: eng.cnnvtl_distance_matrix(both, d=D_REF, out=square)
            t = time_alternately_ms(fns, 3, reps)
            med, best = t["rows"]
            nbytes = n * D_REF + q * n * 8
            hbm8, hbm6 = nbytes / 8e12 * 1e3, nbytes / 6e12 * 1e3
            valu = 3 * q * n * ((D_REF + 3) // 4) / lanes * 1e3
            floor = max(hbm8, valu)
            line = {"what": "distance_rows", "N": n, "D": D_REF, "Q": q, "ms_median": round(med, 4), "ms_best": round(best, 4),
                    "topk_k": K, "topk_ms_median": round(t["topk"][0], 4), "topk_ms_best": round(t["topk"][1], 4),
                    "rows_over_topk": round(med / t["topk"][0], 3)}
            if "matrix" in t:
                line.update({"matrix_rows": n + q, "matrix_ms_median": round(t["matrix"][0], 4),
                             "matrix_over_rows": round(t["matrix"][0] / med, 2)})
            line.update({"floor_hbm_8tbs_ms": round(hbm8, 4), "floor_hbm_6tbs_ms": round(hbm6, 4),
                         "floor_valu_ms": round(valu, 4), "clock_ghz": args.clock_ghz,
                         "bound": "valu" if valu > hbm8 else "hbm", "frac_of_binding_floor": round(floor / med, 3)})
            print(json.dumps(line), flush=True)
        del db
        torch.cuda.empty_cache()
    # the streaming detector: one batch appended and searched, against `resident` frames already stored
    b, steps = 32, (40 if args.quick else 200)               # (a few steps are a window of a millisecond: too short to time)
    for resident in (1063, 100_000):
        base = torch.randint(-128, 128, (resident, D_REF), dtype=torch.int8, device=dev, generator=g)
        batch = torch.randint(-128, 128, (b, D_REF), dtype=torch.int8, device=dev, generator=g)
        for sequence in (None, 10):
            det = dlc.CnnVtlLoopClosureDetector(D_REF, k=5, exclusion=30, capacity=resident + b * (steps + 8), sequence=sequence)
            det.db.append(base)                      # resident frames stored without being searched
            for _ in range(3):
                det.query_and_insert(batch)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                det.query_and_insert(batch)
            torch.cuda.synchronize()
            host = (time.perf_counter() - t0) / steps * 1e3
            print(json.dumps({"what": "detector_step", "resident": resident, "batch": b, "k": 5, "D": D_REF,
                              "sequence": sequence, "ms_per_batch_host": round(host, 4),
                              "frames_per_s": round(b / host * 1e3, 1)}), flush=True)
            del det
        del base
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
