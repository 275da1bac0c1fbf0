"""Timing of the sign-random-projection hash (dlc_lsh_quantize_i8, dlc_lsh_hash_i8) beside the torch composition (GPU box
only).  One JSON line per measurement, all in one process: device events around every call after a warm-up, the calls of
a group timed ALTERNATELY so that a drift of the clock falls on all of them; median, best and worst of `reps` rounds.

    "hash"          bits = 1024, +-1 planes of lsh.lsh_planes, int8 rows, at rows x D of 1 x 4096, 32 x 4096, 1063 x 4096,
                    65 536 x 4096, 1 x 75 000 and 32 x 75 000: every plan that applies (one_pass, split up to 64 rows, auto); beside
                    them, in the same rounds,
                      quantize_hash   Engine.lsh_quantize from bf16 rows, then the hash (auto): two or three launches;
                      torch           the composition a user would write on the same operands: (q.float() @ planes.float().T
                                      > 0), then the bits packed by a weighted sum over groups of 8;
                      copy            planes copied to a buffer of their own size: what moving that many bytes costs.
                    frac_of_i8_mfma: rows * D * bits * 2 operations over 256 CUs x 4 SIMDs x 2048 a clock x clock
                    (--clock-ghz, default 2.4: under load the chip runs below it, so the real fraction is higher);
                    planes_rate_over_copy: the planes' bytes per second of the best plan over the copy's bytes read per
                    second -- the one-row case is bound by streaming the planes.
                    The last rows are checked against tests/lsh_oracle.py and the torch composition.
    "real_frames"   the 20 real frames of tests/golden, each against its copy shifted 4 px, UNTRAINED SDAV weights (the
                    protocol of docs/LAB.md 30 and 31): nearest neighbours right out of 20 by cosine (KeyframeDatabase)
                    and by Hamming at 256, 1024 and 4096 bits, centred on the key rows' mean and not.

    python scripts/bench_lsh.py [--quick] [--clock-ghz 2.4] [--no-real-frames]
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
import lsh_oracle as lo  # noqa: E402

BITS = 1024
SHAPES = ((1, 4096), (32, 4096), (1063, 4096), (65536, 4096), (1, 75000), (32, 75000))


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


def spread(name, t):
    return {name + "_ms_median": round(t[0], 4), name + "_ms_best": round(t[1], 4), name + "_ms_worst": round(t[2], 4)}


def torch_hash(q, planes_f, weights):
    on = (q.float() @ planes_f.t()) > 0
    return (on.view(on.shape[0], -1, 8).to(torch.uint8) * weights).sum(dim=2, dtype=torch.uint8)


def real_frames_line():
    import real_frames
    from deeploopcloser_amd import pipeline
    frames = np.stack([dlc.read_ppm(p) for p in real_frames.frame_paths()])
    shift = 4
    moved = np.concatenate([np.repeat(frames[:, :, :1], shift, axis=2), frames[:, :, :-shift]], axis=2)
    net = dlc.SDAV()
    n = frames.shape[0]
    keys = pipeline.sdav_descriptors_from_frames(frames, net).view(n, -1)
    queries = pipeline.sdav_descriptors_from_frames(np.ascontiguousarray(moved), net).view(n, -1)
    truth = torch.arange(n)
    db = dlc.KeyframeDatabase(keys.to(torch.float32))
    _, i = db.match_topk(db.prepare_queries(queries.to(torch.float32)), 1)
    res = {"cosine": int((i[:, 0].cpu() == truth).sum())}
    for bits in (256, 1024, 4096):
        for center in (True, False):
            h = dlc.Lsh(n_bits=bits, seed=0, center=center).fit(keys)
            dist = dlc.default_engine().hamming_rows(h.transform_tensor(queries), h.transform_tensor(keys)).cpu()
            best = dist.min(dim=1, keepdim=True).values
            first = (dist == best).to(torch.int8).argmax(dim=1)                    # the lowest key-frame among equals
            res["hamming_%d%s" % (bits, "_centred" if center else "")] = int((first == truth).sum())
    return {"what": "real_frames", "queries": n, "shift_px": shift, "width": int(keys.shape[1]), "top1_hits": res}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--clock-ghz", type=float, default=2.4)
    ap.add_argument("--quick", action="store_true", help="fewer repetitions")
    ap.add_argument("--no-real-frames", action="store_true")
    args = ap.parse_args(argv)
    eng = dlc.default_engine()
    dev = eng.device
    reps = 5 if args.quick else 20
    mfma = 256 * 4 * 2048 * args.clock_ghz * 1e9                                   # int8 operations a second
    g = torch.Generator(device=dev).manual_seed(0)
    weights = torch.tensor([1, 2, 4, 8, 16, 32, 64, 128], dtype=torch.uint8, device=dev)
    for rows, d in SHAPES:
        planes = torch.from_numpy(dlc.lsh_planes(BITS, d, 0)).to(dev)
        if d % 16:
            padded = torch.zeros((BITS, (d + 15) // 16 * 16), dtype=torch.int8, device=dev)
            padded[:, :d] = planes
            planes = padded[:, :d]
        planes_f, planes_copy = planes.float(), torch.empty((BITS, d), dtype=torch.int8, device=dev)
        x = torch.randn((rows, d), dtype=torch.float32, device=dev, generator=g).to(torch.bfloat16)
        q = eng.lsh_quantize(x)
        nb = eng.lsh_row_bytes(BITS)
        outs = {name: torch.empty((rows, nb), dtype=torch.uint8, device=dev) for name in ("one_pass", "split", "auto", "quantize_hash")}
        fns = {"one_pass": lambda: eng.lsh_hash(q, planes, out=outs["one_pass"], plan="one_pass")}
        if rows <= 64:
            fns["split"] = lambda: eng.lsh_hash(q, planes, out=outs["split"], plan="split")
        fns["auto"] = lambda: eng.lsh_hash(q, planes, out=outs["auto"], plan="auto")
        fns["quantize_hash"] = lambda: eng.lsh_hash(eng.lsh_quantize(x), planes, out=outs["quantize_hash"])
        fns["copy"] = lambda: planes_copy.copy_(planes)
        t = time_alternately_ms(fns, 3, reps)
        t.update(time_alternately_ms({"torch": lambda: torch_hash(q, planes_f, weights)}, 1, 3 if rows > 4096 else reps))
        want = torch_hash(q, planes_f, weights)                                    # (fp32 sums of +-1 products up to 127 * D: exact below 2^24)
        exact = 127 * d < 1 << 24
        for name in fns:
            if name != "copy":
                assert not exact or torch.equal(outs[name], want), "%s differs from the torch composition" % name
                assert torch.equal(outs[name], outs["one_pass"]), "%s differs from one_pass" % name
        m = min(rows, 4)
        assert np.array_equal(outs["one_pass"][rows - m:].cpu().numpy(), lo.hash_rows(q[rows - m:].cpu().numpy(), planes.cpu().numpy())), \
            "the hash differs from the oracle"
        best = min(t[name][0] for name in ("one_pass", "split", "auto") if name in t)
        ops = rows * d * BITS * 2
        line = {"what": "hash", "rows": rows, "D": d, "bits": BITS, "auto_is": "split" if lo.auto_plan(rows, d) == lo.SPLIT else "one_pass"}
        for name in ("one_pass", "split", "auto", "quantize_hash", "torch", "copy"):
            if name in t:
                line.update(spread(name, t[name]))
        line.update({"best_plan_over_torch": round(best / t["torch"][0], 4), "auto_over_torch": round(t["auto"][0] / t["torch"][0], 4),
                     "operations": ops, "clock_ghz": args.clock_ghz, "frac_of_i8_mfma": round(ops / mfma * 1e3 / best, 4),
                     "planes_bytes": BITS * d, "copy_gbs_read": round(BITS * d / t["copy"][0] / 1e6, 1),
                     "planes_gbs_best_plan": round(BITS * d / best / 1e6, 1), "planes_rate_over_copy": round(t["copy"][0] / best, 3)})
        print(json.dumps(line), flush=True)
        del outs, planes_f, planes_copy, x, q, want
    if not args.no_real_frames:
        print(json.dumps(real_frames_line()), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
