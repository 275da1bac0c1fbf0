"""Timing of the binary place descriptor (dlc_ldb_describe_u8, dlc_hamming_rows) beside SeqSLAM's front-end (GPU box only).
One JSON line per measurement, all in one process: device events around every call after a warm-up, the calls of a group
timed ALTERNATELY so that a drift of the clock falls on all of them; median, best and worst of `reps` rounds.

    "describe"       grey frames [1063, 192, 240] (tests/real_frames.tiled_u8_frames) -> LDB codes at 48 x 48, levels
                     (2, 3, 4): 64 bytes a frame; beside it, in the same rounds, dlc_seqslam_describe_u8 on the same frames
                     (32 x 64, patch 8).  The first frames are checked against tests/ldb_oracle.py.
                     floor_hbm: frames * (H * W + row bytes) bytes at 8 TB/s.
    "hamming_rows"   D = 64 at 1063 x 1063 (the codes of the frames above, the Hamming matrix), a streamed batch of 32
                     against 1063, and on random bytes 8192 x 8192 and 32 x 1 000 000; beside each, in the same rounds,
                       sad_rows          dlc_sad_u8_rows on the same operands: the same tiles, loads and stores, one VALU
                                         operation per word pair where this kernel has two;
                       torch             the composition a user would write: xor, a 256-entry bit-count table gather, sum
                                         (in query chunks of at most 2^27 cells of the [Q, N, D] intermediate);
                       copy              out.copy_(other) of the int64 [Q, N] result: what writing that many bytes costs
                                         when nothing is computed (it reads as many) -- `store_over_copy` = copy / hamming.
                     floor_valu: Q * N * (D / 4) * 2 lane-operations over 256 CUs x 4 SIMDs x 32 lanes x clock (--clock-ghz,
                     default 2.4: under load the chip runs below it, so the real floor is higher);
                     floor_hbm:  (Q + N) * D bytes read, Q * N * 8 written, at 8 TB/s.
                     The last query rows are checked against tests/ldb_oracle.py.

    python scripts/bench_ldb.py [--quick] [--clock-ghz 2.4] [--frames 1063]
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
import ldb_oracle as lo  # noqa: E402
import real_frames  # noqa: E402

SIZE, LEVELS = (48, 48), (2, 3, 4)
SEQSLAM = ((32, 64), 8, 32)
CHUNK_CELLS = 1 << 27                                          # of the torch composition's [q, N, D] intermediate


def time_alternately_ms(fns, warmup, reps):
    """{name: (median, best, worst)} of the calls in fns, one of each per round: device events around every call."""
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
    return {name: (sorted(v)[len(v) // 2], min(v), max(v)) for name, v in out.items()}


def torch_hamming(q, db, table, out):
    """xor, table gather, sum -- in chunks of query rows that keep the intermediate at CHUNK_CELLS cells."""
    rows = max(1, CHUNK_CELLS // (db.shape[0] * db.shape[1]))
    for lo_ in range(0, q.shape[0], rows):
        x = q[lo_:lo_ + rows, None, :] ^ db[None, :, :]
        out[lo_:lo_ + rows] = table[x.long()].sum(dim=2)
    return out


def spread(name, t):
    return {name + "_ms_median": round(t[0], 4), name + "_ms_best": round(t[1], 4), name + "_ms_worst": round(t[2], 4)}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--clock-ghz", type=float, default=2.4)
    ap.add_argument("--frames", type=int, default=1063)
    ap.add_argument("--large", type=int, default=8192, help="rows of the large random matrix (0: skip it)")
    ap.add_argument("--long", type=int, default=1000000, help="key-frames of the long route, 32 queries against it (0: skip it)")
    ap.add_argument("--quick", action="store_true", help="fewer repetitions")
    args = ap.parse_args(argv)
    eng = dlc.default_engine()
    dev = eng.device
    n, reps = args.frames, (5 if args.quick else 30)
    clock = args.clock_ghz * 1e9
    gray = eng.rgb_to_gray(torch.from_numpy(real_frames.tiled_u8_frames(dlc, n)).to(dev))
    hh, ww = gray.shape[1:]
    d = eng.ldb_row_bytes(LEVELS)
    codes = torch.empty((n, d), dtype=torch.uint8, device=dev)
    thumbs = torch.empty((n, SEQSLAM[0][0] * SEQSLAM[0][1]), dtype=torch.uint8, device=dev)

    # ---- describe ---------------------------------------------------------------------------------------------------------
    t = time_alternately_ms({"ldb": lambda: eng.ldb_describe(gray, SIZE, LEVELS, out=codes),
                             "seqslam": lambda: eng.seqslam_describe(gray, *SEQSLAM, out=thumbs)}, 3, reps)
    m = min(n, 40)
    assert np.array_equal(codes[:m].cpu().numpy(), lo.describe(gray[:m].cpu().numpy(), SIZE, LEVELS)), "describe differs from the oracle"
    hbm = n * (hh * ww + d) / 8e12 * 1e3
    line = {"what": "describe", "frames": n, "H": hh, "W": ww, "size": list(SIZE), "levels": list(LEVELS), "row_bytes": d}
    line.update(spread("ldb", t["ldb"]))
    line.update(spread("seqslam", t["seqslam"]))
    line.update({"ldb_over_seqslam": round(t["ldb"][0] / t["seqslam"][0], 3), "floor_hbm_8tbs_ms": round(hbm, 4),
                 "frac_of_hbm_floor": round(hbm / t["ldb"][0], 3)})
    print(json.dumps(line), flush=True)

    # ---- Hamming rows beside the SAD rows, the torch composition and a copy of the result ---------------------------------
    g = torch.Generator(device=dev).manual_seed(0)
    table = torch.tensor([bin(v).count("1") for v in range(256)], dtype=torch.uint8, device=dev)
    lanes = 256 * 4 * 32 * clock
    for q, rows in ((n, n), (32, n), (args.large, args.large), (32, args.long)):
        if q == 0 or rows == 0:
            continue
        db = codes if rows == n else torch.randint(0, 256, (rows, d), dtype=torch.uint8, device=dev, generator=g)
        qs = db[rows - q:]
        out, out_sad, out_torch = (torch.empty((q, rows), dtype=torch.int64, device=dev) for _ in range(3))
        t = time_alternately_ms({"hamming": lambda: eng.hamming_rows(qs, db, out=out),
                                 "sad_rows": lambda: eng.sad_rows(qs, db, out=out_sad),
                                 "copy": lambda: out_sad.copy_(out)}, 3, reps)
        t.update(time_alternately_ms({"torch": lambda: torch_hamming(qs, db, table, out_torch)}, 1, 3 if q * rows > 1 << 22 else reps))
        assert torch.equal(out, out_torch), "hamming_rows differs from the torch composition"
        mq = min(q, 8)
        assert np.array_equal(out[q - mq:].cpu().numpy(), lo.hamming_rows(qs[q - mq:].cpu().numpy(), db.cpu().numpy())), \
            "hamming_rows differs from the oracle"
        med = t["hamming"][0]
        valu = q * rows * (d // 4) * 2 / lanes * 1e3
        hbm = ((q + rows) * d + q * rows * 8) / 8e12 * 1e3
        line = {"what": "hamming_rows", "Q": q, "N": rows, "D": d}
        for name in ("hamming", "sad_rows", "torch", "copy"):
            line.update(spread(name, t[name]))
        line.update({"hamming_over_sad": round(med / t["sad_rows"][0], 3), "hamming_over_torch": round(med / t["torch"][0], 4),
                     "store_bytes": q * rows * 8, "copy_gbs_written": round(q * rows * 8 / t["copy"][0] / 1e6, 1),
                     "store_over_copy": round(t["copy"][0] / med, 3), "lane_ops": q * rows * (d // 4) * 2,
                     "floor_valu_ms": round(valu, 4), "floor_hbm_8tbs_ms": round(hbm, 4), "clock_ghz": args.clock_ghz,
                     "bound": "valu" if valu > hbm else "hbm", "frac_of_binding_floor": round(max(valu, hbm) / med, 3)})
        print(json.dumps(line), flush=True)
        del out, out_sad, out_torch
    return 0


if __name__ == "__main__":
    sys.exit(main())
