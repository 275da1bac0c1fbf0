"""Timing of the ground-truth evaluation kernels (dlc_pr_cell_counts, dlc_positive_rank_rows) beside two yardsticks
measured in the same process (GPU box only).  One JSON line per case: the time from device events, median of the calls
after 3 warm-ups, the calls timed ALTERNATELY (counts, ranks, copy, torch, counts, ...) so that a drift of the clock falls
on all of them.

  cases       1063 x 1063 fp64 (an all-vs-all matrix of the reference's data set), 20 000 x 20 000 fp64 and int64 (the
              sequence benches' rows: 3.2 GB), T = 1000 thresholds, truth a band of 11 cells around the diagonal
  spread      normal scores (uniform integers for int64), the thresholds evenly over their range: the cells spread over
              the bins
  one_bin     the same matrix, every threshold above every score: all cells fall into one bin -- every lane of every wave
              adds to the same two LDS words, the case the in-wave combining is for
  copy        a device copy of the same rows * n * (element + 1) bytes (scores and mask): the one-pass floor, though a
              copy also writes what it reads
  torch       the same counts with torch: bucketize, then a bincount per class

There is no pass bar.    python scripts/bench_evaluate.py [--quick]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import deeploopcloser_amd as dlc  # noqa: E402
from bench_peaks import time_alternately_ms  # noqa: E402

CASES = [(1063, 1063, torch.float64), (20_000, 20_000, torch.float64), (20_000, 20_000, torch.int64)]
T, BAND = 1000, 5


def torch_counts(m, truth, table):
    """(pos, neg): the bin #{i : t_i <= x} of every cell, counted per class."""
    bins = torch.bucketize(m, table, right=True)
    return (torch.bincount(bins[truth], minlength=table.numel() + 1), torch.bincount(bins[~truth], minlength=table.numel() + 1))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="fewer repetitions, and not the 20 000 x 20 000 cases")
    args = ap.parse_args(argv)
    eng = dlc.default_engine()
    dev = eng.device
    g = torch.Generator(device=dev).manual_seed(0)
    for rows, n, dtype in CASES[:1] if args.quick else CASES:
        reps = 20 if rows * n < 1 << 24 else 7
        if dtype == torch.int64:
            m = torch.randint(0, 1 << 20, (rows, n), dtype=torch.int64, device=dev, generator=g)
            lo, hi = 0, 1 << 20
            spread = torch.arange(T, dtype=torch.int64, device=dev) * ((hi - lo) // T) + lo
            above = spread + (1 << 21)
        else:
            m = torch.randn((rows, n), dtype=torch.float64, device=dev, generator=g)
            spread = torch.linspace(-4.0, 4.0, T, dtype=torch.float64, device=dev)
            above = spread + 100.0
        r = torch.arange(rows, device=dev)
        truth = ((r[:, None] - torch.arange(n, device=dev)[None, :]).abs() <= BAND)
        mask = truth.to(torch.uint8)
        m2, mask2 = torch.empty_like(m), torch.empty_like(mask)
        element = m.element_size()
        for name, table in (("spread", spread), ("one_bin", above)):
            want = torch_counts(m, truth, table)
            got = eng.pr_cell_counts(m, mask, table)
            agrees = bool(torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]))
            fns = {"counts": lambda: eng.pr_cell_counts(m, mask, table),
                   "ranks": lambda: eng.positive_rank_rows(m, mask),
                   "copy": lambda: (m2.copy_(m), mask2.copy_(mask)),
                   "torch": lambda: torch_counts(m, truth, table)}
            t = time_alternately_ms(fns, 3, reps)
            nbytes = rows * n * (element + 1)
            print(json.dumps({"what": "evaluate", "rows": rows, "n": n, "dtype": str(dtype).replace("torch.", ""), "T": T,
                              "bins": name, "calls": reps, "agrees_with_torch": agrees, "bytes_read_once": nbytes,
                              "counts_ms_median": round(t["counts"][0], 4), "counts_ms_best": round(t["counts"][1], 4),
                              "counts_gb_per_s": round(nbytes / t["counts"][0] / 1e6, 1),
                              "ranks_ms_median": round(t["ranks"][0], 4), "ranks_ms_best": round(t["ranks"][1], 4),
                              "copy_ms_median": round(t["copy"][0], 4), "torch_ms_median": round(t["torch"][0], 4),
                              "counts_fraction_of_copy_rate": round(t["copy"][0] / t["counts"][0], 3),
                              "ranks_fraction_of_copy_rate": round(t["copy"][0] / t["ranks"][0], 3),
                              "torch_over_counts": round(t["torch"][0] / t["counts"][0], 2)}), flush=True)
        del m, m2, mask, mask2, truth
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
