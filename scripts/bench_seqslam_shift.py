"""Timing of the lateral-shift tolerant SeqSLAM difference (dlc_sad_u8_shift_rows) at the reference's own descriptor --
thumbnails of 32 x 64, D = 2048 -- on random bytes (GPU box only).  One JSON line per case, all in one process: device
events around every call after a warm-up, the calls of a group timed ALTERNATELY so that a drift of the clock falls on all
of them; median and best of the rounds.

Cases: (Q, N) = (1063, 1063), (32, 1063) and (--large, --large), each for S in 1, 2, 4, 8.  Beside the fused call, in the
same rounds:
    "plain"     Engine.sad_rows without a shift: the same tiles, one sum per pair where the fused call has 2 S + 1;
    "composed"  what a user has without the fused call: for each of the 2 S + 1 shifts, cropped contiguous copies of both
                operands, Engine.sad_rows on them, the rescaling floor(v * w / (w - |s|)) and a running minimum with torch
                on the device -- 2 S + 1 round trips of the [Q, N] int64 matrix.
The fused values are asserted equal to the composed ones, and values and shifts to the NumPy oracle
(tests/seqslam_shift_oracle.py) on a few rows.
    per_shift_over_plain = ms / ((2 S + 1) * plain ms): 1 would be the plain kernel's rate on every shift;
    fused_over_composed  = ms / composed ms;
    floor_valu_ms        = (2 S + 1) * Q * N * D / 4 v_sad_u8 lane-operations over 256 CUs x 4 SIMDs x 32 lanes x clock (the
                           convention of scripts/bench_seqslam.py; --clock-ghz, default 2.4: under load the chip runs below it).

    python scripts/bench_seqslam_shift.py [--quick] [--clock-ghz 2.4] [--large 8192]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import deeploopcloser_amd as dlc  # noqa: E402
import seqslam_shift_oracle as ss  # noqa: E402

H, W = 32, 64


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


def composed(eng, qs, db, S):
    """The shifted values from the plain rows alone, on the device (the order of the shifts does not matter to a minimum)."""
    q3, d3 = qs.view(-1, H, W), db.view(-1, H, W)
    best = None
    for s in ss.shift_order(S):
        k = abs(s)
        qc = (q3[:, :, k:] if s < 0 else q3[:, :, :W - k]).reshape(q3.shape[0], -1)      # contiguous copies
        dc = (d3[:, :, :W - k] if s < 0 else d3[:, :, k:]).reshape(d3.shape[0], -1)
        v = eng.sad_rows(qc, dc)
        if k:
            v = torch.div(v.mul_(W), W - k, rounding_mode="floor")
        best = v if best is None else torch.minimum(best, v, out=best)
    return best


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--clock-ghz", type=float, default=2.4)
    ap.add_argument("--frames", type=int, default=1063)
    ap.add_argument("--large", type=int, default=8192, help="rows of the large random matrix (0: skip it)")
    ap.add_argument("--quick", action="store_true", help="fewer repetitions")
    args = ap.parse_args(argv)
    eng = dlc.default_engine()
    dev = eng.device
    d = H * W
    lanes = 256 * 4 * 32 * args.clock_ghz * 1e9
    g = torch.Generator(device=dev).manual_seed(0)
    for q, n in ((args.frames, args.frames), (32, args.frames), (args.large, args.large)):
        if q == 0:
            continue
        reps = 3 if args.quick else (5 if q * n > 1 << 24 else 20)
        db = torch.randint(0, 256, (n, d), dtype=torch.uint8, device=dev, generator=g)
        qs = db[n - q:]
        out = torch.empty((q, n), dtype=torch.int64, device=dev)
        sh = torch.empty((q, n), dtype=torch.int8, device=dev)
        plain = torch.empty((q, n), dtype=torch.int64, device=dev)
        rows, cols = min(q, 4), min(n, 2048)
        host_q, host_db = qs[:rows].cpu().numpy(), db[:cols].cpu().numpy()
        for S in (1, 2, 4, 8):
            kept = {}

            def run_composed():
                kept["v"] = composed(eng, qs, db, S)
            t = time_alternately_ms({"fused": lambda: eng.sad_rows(qs, db, out=out, shift=S, width=W, shift_out=sh),
                                     "plain": lambda: eng.sad_rows(qs, db, out=plain),
                                     "composed": run_composed}, 1, reps)
            assert torch.equal(out, kept["v"]), "the fused values differ from the composed ones"
            want_v, want_s = ss.shift_rows(host_q, host_db, H, W, S)
            assert np.array_equal(out[:rows, :cols].cpu().numpy(), want_v), "the fused values differ from the oracle"
            assert np.array_equal(sh[:rows, :cols].cpu().numpy(), want_s), "the fused shifts differ from the oracle"
            med, best = t["fused"]
            valu = (2 * S + 1) * q * n * (d // 4) / lanes * 1e3
            print(json.dumps({"what": "sad_shift_rows", "Q": q, "N": n, "D": d, "h": H, "w": W, "S": S,
                              "ms_median": round(med, 4), "ms_best": round(best, 4),
                              "plain_ms_median": round(t["plain"][0], 4), "composed_ms_median": round(t["composed"][0], 4),
                              "composed_ms_best": round(t["composed"][1], 4),
                              "per_shift_over_plain": round(med / ((2 * S + 1) * t["plain"][0]), 3),
                              "fused_over_composed": round(med / t["composed"][0], 3),
                              "floor_valu_ms": round(valu, 4), "frac_of_valu_floor": round(valu / med, 3),
                              "clock_ghz": args.clock_ghz, "rounds": reps}), flush=True)
            kept.clear()
    return 0


if __name__ == "__main__":
    sys.exit(main())
