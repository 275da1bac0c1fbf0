"""Timing of the fused cnn_vtl k-nearest search (dlc_cnnvtl_distance_topk) and of the streaming detector on top of it
(GPU box only).  One JSON line per shape: the kernel time from device events after a warm-up, and the two floors the
shape sets:

    HBM   N * D bytes of the database, once, at 8 TB/s (peak) and at 6.0 TB/s (the measured sweep);
    VALU  3 * Q * N * ceil(D / 4) lane-instructions (an xor, a v_xad_u32 and a v_bcnt per word pair) over
          256 CUs x 4 SIMDs x 32 lanes x clock.

`frac_of_binding_floor` = max(HBM floor at 8 TB/s, VALU floor) / measured time.  The clock is a parameter (--clock-ghz,
default 2.4): the chip runs below it under its power cap, so the real floors are higher than the ones reported.

    python scripts/bench_distance_topk.py [--quick] [--clock-ghz 2.4]
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


def time_ms(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    out = []
    for _ in range(reps):
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    out.sort()
    return out[len(out) // 2], out[0]


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
    for n in (1063, 100_000, 1_000_000):
        db = torch.randint(-128, 128, (n, D_REF), dtype=torch.int8, device=dev, generator=g)
        db = eng._rows16(db, D_REF)                     # stored rows: 2256 bytes apart, as CnnVtlKeyframeDatabase keeps them
        for q in (1, 32, 256):
            qs = db[torch.randint(0, n, (q,), device=dev, generator=g)].clone()
            med, best = time_ms(lambda: eng.cnnvtl_distance_topk(qs, db, K, d=D_REF), 3, reps)
            hbm8 = n * D_REF / 8e12 * 1e3
            hbm6 = n * D_REF / 6e12 * 1e3
            valu = 3 * q * n * ((D_REF + 3) // 4) / lanes * 1e3
            floor = max(hbm8, valu)
            print(json.dumps({"what": "distance_topk", "N": n, "D": D_REF, "Q": q, "k": K, "ms_median": round(med, 4),
                              "ms_best": round(best, 4), "floor_hbm_8tbs_ms": round(hbm8, 4),
                              "floor_hbm_6tbs_ms": round(hbm6, 4), "floor_valu_ms": round(valu, 4),
                              "clock_ghz": args.clock_ghz, "bound": "valu" if valu > hbm8 else "hbm",
                              "frac_of_binding_floor": round(floor / med, 3),
                              "frac_of_hbm_6tbs": round(hbm6 / med, 3)}), flush=True)
        del db
        torch.cuda.empty_cache()
    # the streaming detector: one batch appended and searched, against `resident` frames already stored
    for resident in (1063, 100_000):
        base = torch.randint(-128, 128, (resident, D_REF), dtype=torch.int8, device=dev, generator=g)
        for b in (16, 32):
            det = dlc.CnnVtlLoopClosureDetector(D_REF, k=5, exclusion=30, capacity=resident + 64 * (reps + 8))
            det.db.append(base)                      # resident frames stored without being searched
            batch = torch.randint(-128, 128, (b, D_REF), dtype=torch.int8, device=dev, generator=g)
            for _ in range(3):
                det.query_and_insert(batch)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                d, i = det.query_and_insert(batch)
            torch.cuda.synchronize()
            host = (time.perf_counter() - t0) / reps * 1e3
            print(json.dumps({"what": "detector_batch", "resident": resident, "batch": b, "k": 5, "D": D_REF,
                              "ms_per_batch_host": round(host, 4), "frames_per_s": round(b / host * 1e3, 1)}), flush=True)
        del base
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
