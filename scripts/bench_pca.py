"""Timing of the PCA projection (dlc_pca_project) beside what a caller would write without it (GPU box only).  One
JSON line per (shape, basis dtype), all in one process: device events, median of 10 calls after 3 warm-ups, the plans and
the baselines timed ALTERNATELY so that a drift of the clock falls on all of them.

  shapes     D -> M = 40 000 -> 4096 (a 16-word VLAD row of the reference's SDAV), 75 000 -> 4096 (the concatenation) and
             4096 -> 256; rows 1, 32 and 1063; fp64 and fp32 basis; every plan the shape allows
  baselines  (fp64 basis; clocks, not checks: none of them has the defined sum order)
             gemm        the one-pass dlc_gemm_bias_act with the bias -mean . basis folded in, then the scale
             gemm_split  the same under engine.latency_mode() (split-K; rows <= 32), timed against AUTO in a round of its own
             matmul      torch.matmul in fp64 on (x - mean), then the scale
  floors     few rows: the basis bytes at 6.29 TB/s (the measured HBM copy rate); many rows: rows * D * M * 2 unfused fp64
             operations at half the 78.6 TFLOP/s the data sheet gives for fp64 fma.  `floor_ms` is the larger of the two.

After the timings, unless --skip-frames: one line `real_frames` -- the 20 real frames, each against its copy translated
4 px horizontally, default (untrained) SDAV weights: top-1 hits of the concatenation and of VLAD (16 words) through
KeyframeDatabase, as they are and behind Pca(16) fitted on the 20 key rows.

    python scripts/bench_pca.py [--quick] [--skip-frames]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import deeploopcloser_amd as dlc  # noqa: E402
from bench_vlad import time_alternately_ms  # noqa: E402

SHAPES = [(40000, 4096), (75000, 4096), (4096, 256)]
ROWS = (1, 32, 1063)
FP64_OPS_PER_S = 78.6e12 / 2
HBM_BYTES_PER_S = 6.29e12


def real_frames_line():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import real_frames
    from deeploopcloser_amd import pipeline
    frames = np.stack([dlc.read_ppm(p) for p in real_frames.frame_paths()])
    shift = 4
    moved = np.concatenate([np.repeat(frames[:, :, :1], shift, axis=2), frames[:, :, :-shift]], axis=2)
    net = dlc.SDAV()
    keys = pipeline.sdav_descriptors_from_frames(frames, net)
    queries = pipeline.sdav_descriptors_from_frames(np.ascontiguousarray(moved), net)
    vlad = dlc.Vlad(n_words=16, seed=0).fit(keys, iters=20)
    n = frames.shape[0]
    truth = torch.arange(n)

    def hits(d_rows, q_rows):
        db = dlc.KeyframeDatabase(d_rows.to(torch.float32))
        _, i = db.match_topk(db.prepare_queries(q_rows.to(torch.float32)), 1)
        return int((i[:, 0].cpu() == truth).sum())
    res = {}
    for name, d_rows, q_rows in (("concatenation", keys.view(n, -1), queries.view(n, -1)),
                                 ("vlad", vlad.transform_tensor(keys), vlad.transform_tensor(queries))):
        res[name] = hits(d_rows, q_rows)
        for whiten in (True, False):
            m = dlc.Pca(16, whiten=whiten).fit(d_rows)
            res["%s_pca16%s" % (name, "_whitened" if whiten else "")] = hits(m.transform_tensor(d_rows), m.transform_tensor(q_rows))
    return {"what": "real_frames", "queries": n, "shift_px": shift, "words": 16, "components": 16, "top1_hits": res}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="fewer repetitions")
    ap.add_argument("--skip-frames", action="store_true", help="timings only")
    args = ap.parse_args(argv)
    eng = dlc.default_engine()
    dev = eng.device
    g = torch.Generator(device=dev).manual_seed(0)
    reps = 4 if args.quick else 10
    print(json.dumps({"what": "device", "name": torch.cuda.get_device_name(dev),
                      "compute_units": torch.cuda.get_device_properties(dev).multi_processor_count}), flush=True)
    for d, m in SHAPES:
        b64 = torch.randn((d, m), dtype=torch.float64, device=dev, generator=g)
        mean = torch.rand(d, dtype=torch.float64, device=dev, generator=g)
        scale = torch.rand(m, dtype=torch.float64, device=dev, generator=g) + 0.5
        bias = -(mean @ b64)
        for basis in (b64, b64.float()):
            f64 = basis.dtype == torch.float64
            for rows in ROWS:
                x = torch.rand((rows, d), dtype=torch.float64, device=dev, generator=g)
                plans = ("one_pass", "split", "auto") if rows <= dlc._lib.DLC_PCA_SPLIT_MAX_ROWS else ("one_pass", "auto")
                fns = {p: (lambda p=p: eng.pca_project(x, basis, mean, scale, plan=p)) for p in plans}
                if f64:
                    fns["gemm"] = lambda: eng.gemm_bias_act(x, basis, bias=bias).mul_(scale)
                    fns["matmul"] = lambda: torch.matmul(x - mean, basis).mul_(scale)
                t = time_alternately_ms(fns, 3, reps)
                floor_ms = max(basis.numel() * basis.element_size() / HBM_BYTES_PER_S, rows * d * m * 2 / FP64_OPS_PER_S) * 1e3
                line = {"what": "pca_project", "rows": rows, "D": d, "M": m, "basis": "f64" if f64 else "f32", "calls": reps,
                        "auto_is": "split" if eng.lib.dlc_pca_project_workspace_bytes(rows, d, m, 0) else "one_pass",
                        "floor_ms": round(floor_ms, 4)}
                for name, (med, best) in t.items():
                    line[name + "_ms_median"], line[name + "_ms_best"] = round(med, 4), round(best, 4)
                line["floor_share_auto"] = round(floor_ms / t["auto"][0], 3)
                if f64:
                    line["gemm_over_auto"] = round(t["gemm"][0] / t["auto"][0], 2)
                    line["matmul_over_auto"] = round(t["matmul"][0] / t["auto"][0], 2)
                    if rows <= 32:
                        with eng.latency_mode():
                            t2 = time_alternately_ms({"auto": fns["auto"], "gemm_split": fns["gemm"]}, 3, reps)
                        line["gemm_split_ms_median"], line["auto_beside_it_ms_median"] = round(t2["gemm_split"][0], 4), round(t2["auto"][0], 4)
                        line["gemm_split_over_auto"] = round(t2["gemm_split"][0] / t2["auto"][0], 2)
                print(json.dumps(line), flush=True)
                del x
        del b64, basis
        torch.cuda.empty_cache()
    if not args.skip_frames:
        print(json.dumps(real_frames_line()), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
