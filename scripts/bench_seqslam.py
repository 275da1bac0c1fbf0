"""Timing of SeqSLAM's front-end (dlc_seqslam_describe_u8, dlc_sad_u8_rows) at the reference's own size -- 1063 frames of
192 x 240, thumbnails of 32 x 64, so D = 2048 -- on tests/real_frames.tiled_u8_frames (GPU box only).  One JSON line per
measurement, all in one process: device events around every call after a warm-up, the calls of a group timed ALTERNATELY
so that a drift of the clock falls on all of them; median and best of `reps` rounds.

    "describe"   grey frames [1063, 192, 240] on the device -> descriptors; beside it the grey conversion, and the NumPy
                 oracle (tests/seqslam_oracle.py) on --oracle-frames frames, scaled to 1063.
                 floor_hbm: frames * (H * W + h * w) bytes at 8 TB/s.
    "sad_rows"   the full 1063 x 1063 matrix, a streamed batch of 32 against 1063 and -- random bytes, a size at which the
                 kernel and not its launch is timed -- the full --large x --large matrix; beside each, in the same rounds,
                 dlc_cnnvtl_distance_rows on int8 operands of the same Q, N, D -- the yardstick: the same tiles, the same
                 bytes, four VALU operations per word pair where this kernel has one (`sad_over_popcount`); and the NumPy
                 oracle of the SAD rows.
                 floor_valu: Q * N * D / 4 v_sad_u8 lane-operations over 256 CUs x 4 SIMDs x 32 lanes x clock;
                 floor_lds:  per tile (QT queries x DB db rows: the plan of distance_tile.h) and 64-byte step, 4 waves x
                             (QR + 4) ds_read_b128 x 4 LDS cycles plus (QT + DB) / 16 ds_write_b128 wave-instructions x 13
                             cycles, one LDS per CU;
                 floor_hbm:  (Q + N) * D bytes read, Q * N * 8 written, at 8 TB/s.
                 `frac_of_binding_floor` = the largest floor / the measured median.  The clock is a parameter
                 (--clock-ghz, default 2.4): under load the chip runs below it, so the real floors are higher.

    python scripts/bench_seqslam.py [--quick] [--clock-ghz 2.4] [--frames 1063]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import deeploopcloser_amd as dlc  # noqa: E402
import real_frames  # noqa: E402
import seqslam_oracle as sq  # noqa: E402

SIZE, PATCH, STRENGTH = (32, 64), 8, 32


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


def tile_plan(q):
    """(queries, db rows, queries per thread) of a tile: tk_plan of deeploopcloser_amd/csrc/distance_tile.h."""
    if q <= 4:
        return 1, 256, 1
    big, mid = -(-q // 64) * 64, -(-q // 16) * 16
    return (64, 64, 4) if big <= mid else (16, 256, 4)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--clock-ghz", type=float, default=2.4)
    ap.add_argument("--frames", type=int, default=1063)
    ap.add_argument("--oracle-frames", type=int, default=40, help="frames the NumPy oracle is timed on (scaled to --frames)")
    ap.add_argument("--large", type=int, default=8192, help="rows of the large random matrix (0: skip it)")
    ap.add_argument("--quick", action="store_true", help="fewer repetitions")
    args = ap.parse_args(argv)
    eng = dlc.default_engine()
    dev = eng.device
    n, reps = args.frames, (5 if args.quick else 30)
    clock = args.clock_ghz * 1e9
    frames = real_frames.tiled_u8_frames(dlc, n)
    rgb = torch.from_numpy(frames).to(dev)
    gray = eng.rgb_to_gray(rgb)
    hh, ww = gray.shape[1:]
    d = SIZE[0] * SIZE[1]
    desc = torch.empty((n, d), dtype=torch.uint8, device=dev)

    # ---- describe ---------------------------------------------------------------------------------------------------------
    t = time_alternately_ms({"describe": lambda: eng.seqslam_describe(gray, SIZE, PATCH, STRENGTH, out=desc),
                             "gray": lambda: eng.rgb_to_gray(rgb)}, 3, reps)
    m = min(n, args.oracle_frames)
    g_host = gray[:m].cpu().numpy()
    t0 = time.perf_counter()
    want = sq.describe(g_host, SIZE, PATCH, STRENGTH)
    oracle_ms = (time.perf_counter() - t0) * 1e3 * n / m
    assert np.array_equal(desc[:m].cpu().numpy(), want), "describe differs from the oracle"
    hbm = n * (hh * ww + d) / 8e12 * 1e3
    print(json.dumps({"what": "describe", "frames": n, "H": hh, "W": ww, "size": list(SIZE), "patch": PATCH,
                      "ms_median": round(t["describe"][0], 4), "ms_best": round(t["describe"][1], 4),
                      "rgb_to_gray_ms_median": round(t["gray"][0], 4), "numpy_oracle_ms_scaled": round(oracle_ms, 1),
                      "floor_hbm_8tbs_ms": round(hbm, 4), "frac_of_hbm_floor": round(hbm / t["describe"][0], 3)}), flush=True)

    # ---- SAD rows beside the popcount distance rows ---------------------------------------------------------------------------
    g = torch.Generator(device=dev).manual_seed(0)
    db8 = torch.randint(-128, 128, (n, d), dtype=torch.int8, device=dev, generator=g)
    host_desc = desc.cpu().numpy()
    lanes = 256 * 4 * 32 * clock
    for q, n in ((n, n), (32, n), (args.large, args.large)):
        if q == 0:
            continue
        if n != desc.shape[0]:                                 # the large case: random bytes
            desc = torch.randint(0, 256, (n, d), dtype=torch.uint8, device=dev, generator=g)
            db8 = torch.randint(-128, 128, (n, d), dtype=torch.int8, device=dev, generator=g)
            host_desc = desc.cpu().numpy()
        qs, qs8 = desc[n - q:], db8[n - q:]
        out = torch.empty((q, n), dtype=torch.int64, device=dev)
        out8 = torch.empty((q, n), dtype=torch.int64, device=dev)
        t = time_alternately_ms({"sad": lambda: eng.sad_rows(qs, desc, out=out),
                                 "popcount": lambda: eng.cnnvtl_distance_rows(qs8, db8, out=out8)}, 3, reps)
        mq = min(q, 32)
        t0 = time.perf_counter()
        want = sq.sad_rows(host_desc[n - mq:], host_desc)
        oracle_ms = (time.perf_counter() - t0) * 1e3 * q / mq
        assert np.array_equal(out[q - mq:].cpu().numpy(), want), "sad_rows differs from the oracle"
        med, best = t["sad"]
        valu = q * n * (d // 4) / lanes * 1e3
        hbm = ((q + n) * d + q * n * 8) / 8e12 * 1e3
        line = {"what": "sad_rows", "Q": q, "N": n, "D": d, "ms_median": round(med, 4), "ms_best": round(best, 4),
                "popcount_rows_ms_median": round(t["popcount"][0], 4), "popcount_rows_ms_best": round(t["popcount"][1], 4),
                "sad_over_popcount": round(med / t["popcount"][0], 3), "numpy_oracle_ms_scaled": round(oracle_ms, 1),
                "floor_valu_ms": round(valu, 4), "floor_hbm_8tbs_ms": round(hbm, 4), "clock_ghz": args.clock_ghz}
        floors = {"valu": valu, "hbm": hbm}
        qt, db_rows, qr = tile_plan(q)
        tiles, steps = -(-q // qt) * -(-n // db_rows), -(-d // 64)
        lds_cycles = tiles * steps * (4 * (qr + 4) * 4 + -(-(qt + db_rows) // 16) * 13)
        floors["lds"] = lds_cycles / min(tiles, 256) / clock * 1e3           # one LDS per CU, at most 256 CUs at work
        line.update({"tile": [qt, db_rows], "floor_lds_ms": round(floors["lds"], 4)})
        bound = max(floors, key=floors.get)
        line.update({"bound": bound, "frac_of_binding_floor": round(floors[bound] / med, 3)})
        print(json.dumps(line), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
