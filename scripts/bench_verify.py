"""Timing of the geometric verification (dlc_verify_pairs) beside the same stage composed from torch ops on the device --
what a caller would write without it (GPU box only).  One JSON line per shape, all in one process: device events, median
of 10 calls after 3 warm-ups, the kernel and the torch composition timed ALTERNATELY so that a drift of the clock falls
on both.

  shapes   one streamed frame (1 x 5 pairs), a batch (32 x 5) and the re-ranking of a long list (256 x 20), all of 30
           patches x 2500 columns: the reference's SDAV.
  torch    torch.cdist in fp64 per pair + argmin both ways + the cross-check, then every two-match similarity hypothesis
           as one batched int64 tensor expression [pairs, 435, 30] and a max over the hypotheses.  Its distances are not
           DIST's serial chain and it keeps absent points: it is a clock, not a check.  `vs_torch` = torch's median over
           the kernel's (above 1: the kernel is faster).
  floors   the fp64 vector issue floor of the tables, pairs * P * P * H * 3 operations (a subtraction, a product, a sum,
           none fused) at half the 78.6 TFLOP/s the data sheet gives for fp64 fma; and the bytes of the pairs, 2 * P * H
           * 8 each, at the achievable device copy rate of 6.3 TB/s.  `*_share` = floor / median.

After the timings, unless --skip-experiments: two lines.
  planted_stream   40 places of 30 patches; then 40 ALIASED frames -- the identical patch set of a place, its key-points
           shuffled among the patches: another place that looks the same -- then 40 true revisits (descriptor noise, the
           key-points shifted and moved by up to 1 px).  Cosine LoopClosureDetector (k = 1) with and without the verifier
           in front of LoopClosureEvaluator: precision at full recall, average precision.
  real_frames      the 20 real frames against their copies translated 4 px horizontally, default (untrained) SDAV weights:
           the inlier counts of the 20 true pairs and of the 380 wrong pairs.

    python scripts/bench_verify.py [--quick] [--skip-experiments]
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

SHAPES = [("one streamed frame", 1, 5), ("a batch", 32, 5), ("re-ranking a long list", 256, 20)]
P, H, N = 30, 2500, 1063
FP64_OPS_PER_S = 78.6e12 / 2
COPY_BYTES_PER_S = 6.3e12
TORCH_CHUNK = 512                                          # pairs of the torch composition formed at once


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


def torch_verify(qd, qp, dd, dp, cand, tol=3, s16=32):
    """Inlier counts [Q, k] of the same stage in torch ops: similarity model, mutual matches."""
    q, k = cand.shape
    st, tt = torch.triu_indices(P, P, offset=1, device=qd.device)
    out = []
    flat_q = torch.arange(q, device=qd.device).repeat_interleave(k)
    flat_c = cand.reshape(-1)
    for lo in range(0, q * k, TORCH_CHUNK):
        rq, rc = flat_q[lo:lo + TORCH_CHUNK], flat_c[lo:lo + TORCH_CHUNK]
        d = torch.cdist(qd[rq], dd[rc])                                    # [pairs, P, P]
        m = d.argmin(dim=2)
        r = d.argmin(dim=1)
        kept = r.gather(1, m) == torch.arange(P, device=qd.device)[None]   # [pairs, P]
        a = qp[rq].to(torch.int64)
        b = dp[rc].to(torch.int64).gather(1, m[:, :, None].expand(-1, -1, 2))
        u, v = a[:, tt] - a[:, st], b[:, tt] - b[:, st]                    # [pairs, hyps, 2]
        uu, vv = (u * u).sum(-1), (v * v).sum(-1)
        valid = (uu > 0) & (vv > 0) & (256 * vv <= s16 * s16 * uu) & (256 * uu <= s16 * s16 * vv) & kept[:, st] & kept[:, tt]
        da, db = a[:, None, :, :] - a[:, st, None, :], b[:, None, :, :] - b[:, st, None, :]      # [pairs, hyps, P, 2]
        ux, uy, vx, vy = u[..., 0:1], u[..., 1:2], v[..., 0:1], v[..., 1:2]
        re = (db[..., 0] * ux - db[..., 1] * uy) - (vx * da[..., 0] - vy * da[..., 1])
        im = (db[..., 0] * uy + db[..., 1] * ux) - (vx * da[..., 1] + vy * da[..., 0])
        inl = ((re * re + im * im <= tol * tol * uu[..., None]) & kept[:, None, :]).sum(-1)
        out.append(torch.where(valid, inl, torch.zeros_like(inl)).max(dim=1).values)
    return torch.cat(out).view(q, k)


def planted_stream_line(eng):
    from deeploopcloser_amd.verification import keep_accepted
    rng = np.random.RandomState(0)
    places, dim = 40, 64
    desc = rng.standard_normal((places, P, dim))
    pts = np.stack([np.stack([f % 240, f // 240], 1) for f in (rng.choice(240 * 192, P, replace=False) for _ in range(places))])
    alias_pts = np.stack([pts[i][rng.permutation(P)] for i in range(places)])             # the same patches, elsewhere
    revisit = desc + 0.02 * rng.standard_normal(desc.shape)
    revisit_pts = np.clip(pts + rng.randint(-1, 2, size=pts.shape) + np.array([7, -3]), 0, 8191)
    all_desc = np.concatenate([desc, desc, revisit])
    all_pts = np.concatenate([pts, alias_pts, revisit_pts]).astype(np.int32)
    position = np.concatenate([np.arange(places), 1000 + np.arange(places), np.arange(places)]) * 10
    res = {}
    for verify in (False, True):
        det = dlc.LoopClosureDetector(P * dim, k=1, threshold=-1.0, exclusion=0, dtype="bf16", capacity=256)
        ver = dlc.GeometricVerifier(patches=P, width=dim, capacity=256, min_inliers=6)
        judge = dlc.LoopClosureEvaluator(position, 0, 0)
        for lo in range(0, all_desc.shape[0], 8):
            x = torch.from_numpy(all_desc[lo:lo + 8]).to(eng.device)
            s, i = det.query_and_insert(x.view(x.shape[0], -1).to(torch.float32))
            if verify:
                ver.append(x, all_pts[lo:lo + 8])
                inl, _ = ver.verify(lo, i)
                s, i = keep_accepted(inl >= ver.min_inliers, s, i, float("-inf"))
            judge.add(s, i, lo)
        curve, _ = judge.result()
        rows = curve.rows()
        full = [r for r in rows if r[4] == max(x[4] for x in rows)][0]
        res["verified" if verify else "appearance"] = {"precision_at_full_recall": round(full[3], 4), "recall": round(full[4], 4),
                                                        "ap": round(curve.average_precision, 4), "loops": curve.positives}
    return {"what": "planted_stream", "places": places, "aliased": places, "revisits": places, "min_inliers": 6, "tol": 3, **res}


def real_frames_line(eng):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import real_frames
    from deeploopcloser_amd import pipeline
    frames = np.stack([dlc.read_ppm(p) for p in real_frames.frame_paths()])                  # [20, 192, 240, 3] RGB
    shift = 4
    moved = np.concatenate([np.repeat(frames[:, :, :1], shift, axis=2), frames[:, :, :-shift]], axis=2)
    net = dlc.SDAV()
    keys, key_pts = pipeline.sdav_descriptors_from_frames(frames, net, return_key_points=True)
    queries, q_pts = pipeline.sdav_descriptors_from_frames(np.ascontiguousarray(moved), net, return_key_points=True)
    n = frames.shape[0]
    res = {}
    for model in ("similarity", "translation"):
        inl = []
        for lo in range(0, n, 5):                                                            # every query against every key-frame
            cand = torch.arange(n, device=eng.device)[None].expand(n, n)[:, lo:lo + 5].contiguous()
            inl.append(eng.verify_pairs(queries, q_pts, keys, key_pts, cand, model=model)[0])
        inl = torch.cat(inl, dim=1).cpu().numpy()
        true, wrong = np.diag(inl), inl[~np.eye(n, dtype=bool)]
        res[model] = {"true_min_median_max": [int(true.min()), float(np.median(true)), int(true.max())],
                      "wrong_min_median_max": [int(wrong.min()), float(np.median(wrong)), int(wrong.max())],
                      "true_pairs_above_every_wrong_pair_of_their_frame": int((np.diag(inl) > np.where(np.eye(n, dtype=bool), -1, inl).max(1)).sum())}
    return {"what": "real_frames", "queries": n, "shift_px": shift, "tol": 3, "max_scale": 2.0, **res}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--quick", action="store_true", help="fewer repetitions")
    ap.add_argument("--skip-experiments", action="store_true", help="timings only")
    args = ap.parse_args(argv)
    eng = dlc.default_engine()
    dev = eng.device
    g = torch.Generator(device=dev).manual_seed(0)
    reps = 4 if args.quick else 10
    print(json.dumps({"what": "device", "name": torch.cuda.get_device_name(dev),
                      "compute_units": torch.cuda.get_device_properties(dev).multi_processor_count}), flush=True)
    dd = torch.rand((N, P, H), dtype=torch.float64, device=dev, generator=g)                 # (sigmoid outputs lie in 0..1)
    dp = torch.randint(0, 240, (N, P, 2), dtype=torch.int32, device=dev, generator=g)
    for name, q, k in SHAPES:
        pairs = q * k
        cand = torch.randint(0, N, (q, k), dtype=torch.int64, device=dev, generator=g)
        # a query frame is its first candidate's patches, permuted and a little off: real matches, as a revisit has
        perm = torch.randperm(P, device=dev, generator=g)
        qd = dd[cand[:, 0]][:, perm] + 0.01 * torch.rand((q, P, H), dtype=torch.float64, device=dev, generator=g)
        qp = dp[cand[:, 0]][:, perm].contiguous()
        flops_ms = pairs * P * P * H * 3 / FP64_OPS_PER_S * 1e3
        bytes_ms = pairs * 2 * P * H * 8 / COPY_BYTES_PER_S * 1e3
        t = time_alternately_ms({"dlc": lambda: eng.verify_pairs(qd, qp, dd, dp, cand),
                                 "torch": lambda: torch_verify(qd, qp, dd, dp, cand)}, 3, reps)
        med, best = t["dlc"]
        agree = float((eng.verify_pairs(qd, qp, dd, dp, cand)[0] == torch_verify(qd, qp, dd, dp, cand)).float().mean())
        print(json.dumps({"what": "verify_pairs", "case": name, "pairs": pairs, "P": P, "H": H, "calls": reps,
                          "ms_median": round(med, 4), "ms_best": round(best, 4), "torch_ms_median": round(t["torch"][0], 4),
                          "vs_torch": round(t["torch"][0] / med, 2), "fp64_floor_ms": round(flops_ms, 4),
                          "fp64_floor_share": round(flops_ms / med, 3), "copy_floor_ms": round(bytes_ms, 5),
                          "copy_rate_share": round(bytes_ms / med, 4), "same_counts_as_torch": round(agree, 3)}), flush=True)
    del dd, dp
    torch.cuda.empty_cache()
    if not args.skip_experiments:
        print(json.dumps(planted_stream_line(eng)), flush=True)
        print(json.dumps(real_frames_line(eng)), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
