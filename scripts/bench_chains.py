#!/usr/bin/env python3
"""Timing of the chains launch (dlc_sequence_elastic_chains / dlc_sequence_chains) on an MI355X against its yardstick, the
search whose candidates it serves, at a streamed batch's shape: 32 rows behind L - 1 context rows (row0 = L - 1, limit_step
1), n = 20 000 key-frames, k = 5.  The search alone and the search followed by the chains of its idx alternate call by call
in one process, median of 20 calls each after 3 warm-ups, HIP events; the chains launch on its own (over a fixed idx) is
timed the same way.

Shapes -- fp64 and int64 at L = 10 with steps (0, 2) and (0, 8), L = 64 with steps (0, 2) and (0, 8) (the 505-column
trapezoid, the 32 KB step table), and the lines (slope_offsets(L)) at L = 10 and 64.
usage: python scripts/bench_chains.py [--json OUT]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import deeploopcloser_amd as dlc                                                          # noqa: E402

WARMUP, REPEATS, K, BATCH, N = 3, 20, 5, 32, 20000


def timed(*fns):
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


def bench(eng):
    out = []
    g = torch.Generator(device=eng.device)
    g.manual_seed(1)
    for dtype in (torch.float64, torch.int64):
        for L, steps in ((10, (0, 2)), (10, (0, 8)), (64, (0, 2)), (64, (0, 8)), (10, None), (64, None)):
            r = BATCH + L - 1
            lower = dtype == torch.int64
            kw = dict(row0=L - 1, limit0=N - r - 30, limit_step=1, lower_is_better=lower)
            if dtype == torch.int64:
                m = torch.randint(0, 20000, (r, N), generator=g, device=eng.device, dtype=dtype)
            else:
                m = torch.randn((r, N), generator=g, device=eng.device, dtype=dtype)
            if steps is None:
                off = dlc.slope_offsets(L)
                search = lambda: eng.sequence_topk(m, L, off, k=K, **kw)
                chains = lambda idx: eng.sequence_chains(m, L, off, idx, **kw)
            else:
                search = lambda: eng.sequence_elastic_topk(m, L, steps, k=K, **kw)
                chains = lambda idx: eng.sequence_elastic_chains(m, L, steps, idx, **kw)
            idx = search()[1]
            assert bool((chains(idx)[0] >= 0).all())
            alone, both, launch = timed(search, lambda: chains(search()[1]), lambda: chains(idx))
            out.append({"dtype": str(dtype).split(".")[1], "rows": r, "row0": L - 1, "n": N, "L": L, "k": K,
                        "steps": None if steps is None else list(steps), "search_ms": alone, "search_and_chains_ms": both,
                        "chains_ms": launch, "chains_over_search": launch / alone})
            del m
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--json", help="also write the results to this file")
    args = ap.parse_args()
    eng = dlc.default_engine()
    res = {"device": torch.cuda.get_device_name(eng.device), "shapes": bench(eng)}
    for r in res["shapes"]:
        print("%-7s (32+L-1)x%d L=%-2d %-14s search %.3f ms   search + chains %.3f ms   chains alone %.3f ms   = %.2f of the search"
              % (r["dtype"], r["n"], r["L"], "lines" if r["steps"] is None else "steps=(%d, %d)" % tuple(r["steps"]), r["search_ms"],
                 r["search_and_chains_ms"], r["chains_ms"], r["chains_over_search"]))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
