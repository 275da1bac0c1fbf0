#!/usr/bin/env python3
"""DA training step (dlc_da_train_step) beside SDAV's on the same box: per-step wall time of DA steps at
(10, 30, 1681 -> 2500) and (10, 30, 2500 -> 2500), eager (train_step) and replayed (train_steps), SDAV layer-0 and
layer-1 replayed steps, all under latency_mode() as the fits run them; then SDA.fit_dataset's wall time on N synthetic
frames with the reference's network (five layers of 2500, batch 10, 100 epochs).  One JSON line per figure.

    python scripts/time_da_step.py [--steps 200] [--frames 1063] [--no-fit]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import deeploopcloser_amd as dlc                      # noqa: E402


def per_step_ms(run, steps, reps=5):
    """Median over `reps` runs of run(steps), in milliseconds per step (device-synchronised wall time)."""
    run(3)                                            # warm-up: captures, workspaces, kernel attributes
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        run(steps)
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3 / steps)
    return float(np.median(times))


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--frames", type=int, default=1063)
    ap.add_argument("--no-fit", action="store_true")
    a = ap.parse_args()
    eng = dlc.default_engine()
    rng = np.random.RandomState(0)
    x0 = torch.from_numpy(rng.uniform(0, 1, size=(10, 30, 1681))).to(eng.device)
    x1 = torch.from_numpy(rng.uniform(0, 1, size=(10, 30, 2500))).to(eng.device)
    out = lambda **kv: print(json.dumps(kv), flush=True)
    with eng.latency_mode():
        for k, x in ((1681, x0), (2500, x1)):
            da = dlc.DA([30, k], 2500, seed=1)
            da.corruption_masks()
            out(what="da_step_eager", shape=[10, 30, k, 2500],
                ms=per_step_ms(lambda n: [da.train_step(x) for _ in range(n)], a.steps))
            out(what="da_step_replayed", shape=[10, 30, k, 2500], ms=per_step_ms(lambda n: da.train_steps(x, n), a.steps))
        net = dlc.SDAV(seed=1)
        for layer in (0, 1):
            out(what="sdav_step_replayed", layer=layer, shape=[10, 30, 1681, 2500],
                ms=per_step_ms(lambda n: net.train_steps(layer, x0, n), a.steps))
    if not a.no_fit:
        frames = rng.uniform(0, 1, size=(a.frames, 30, 1681))
        sda = dlc.SDA([30, 1681], [2500] * 5, seed=1)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sda.fit_dataset(list(frames))
        torch.cuda.synchronize()
        steps = sum(l.global_step for l in sda.layers)
        out(what="sda_fit", frames=a.frames, steps=steps, s=time.perf_counter() - t0)


if __name__ == "__main__":
    main()
