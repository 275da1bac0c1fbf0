#!/usr/bin/env python3
"""Timing of place tracking (dlc_track_rows) on an MI355X: the per-row cost of its two plans -- RESIDENT, one workgroup
that keeps the state in LDS and runs every row in one launch, and ROWS, one launch per row -- on fp64 rows with steps
(0, 2), back-pointers written, at (1063 rows, n 1063), (256, 4096), (32, 4096) and the shapes around them, and ROWS alone at (64, 65536).  Beside
each, as context, the elastic sequence search (Engine.sequence_elastic_topk, L = 10, k = 5) over the same matrix.  The
plans and the search alternate call by call in one process, median of 20 calls each after 3 warm-ups, HIP events.  Then
the backtrace over the same rows.      usage: python scripts/bench_track.py [--json OUT]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import deeploopcloser_amd as dlc                                                          # noqa: E402

WARMUP, REPEATS = 3, 20
# rows, n, RESIDENT too.  (256, 2048), (256, 3072) and (256, 8192) bracket the n at which the two plans cross: AUTO's rule
CASES = [(1063, 1063, True), (256, 2048, True), (256, 3072, True), (256, 4096, True), (32, 4096, True), (1, 4096, True),
         (256, 8192, True), (64, 65536, False)]


def timed(fns):
    """Median milliseconds of each of fns, called in turn, each between two events on the current stream."""
    for _ in range(WARMUP):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(REPEATS):
        for fn, acc in zip(fns, ms):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            acc.append(a.elapsed_time(b))
    return [statistics.median(m) for m in ms]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    eng = dlc.default_engine()
    g = torch.Generator(device=eng.device)
    g.manual_seed(1)
    out = []
    for rows, n, resident in CASES:
        m = torch.randn((rows, n), generator=g, device=eng.device, dtype=torch.float64)
        back = torch.empty((rows, n), dtype=torch.int8, device=eng.device)

        V, head = eng.track_state(n, m.dtype)                     # (carried from call to call: the cost does not depend on it)

        def track(plan):
            return eng.track_rows(m, V, head, (0, 2), 4.0, 4.0, 2.0, plan=plan, back=back)

        fns = [lambda: track("rows")] + ([lambda: track("resident")] if resident else [])
        if rows >= 10:
            fns.append(lambda: eng.sequence_elastic_topk(m, 10, (0, 2), k=5))
        ms = timed(fns)
        place, gg, _, _, backU, _, _ = track("rows")
        trace = timed([lambda: eng.track_backtrace(back, backU, gg, place_last=place[-1:].clone())])[0]
        row = {"rows": rows, "n": n, "rows_plan_ms": ms[0], "rows_plan_us_per_row": 1e3 * ms[0] / rows,
               "resident_ms": ms[1] if resident else None, "resident_us_per_row": 1e3 * ms[1] / rows if resident else None,
               "elastic_L10_ms": ms[-1] if rows >= 10 else None, "backtrace_ms": trace}
        out.append(row)
        print(json.dumps(row), flush=True)
        del m, back
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
