#!/usr/bin/env python3
"""Condense gpurun_out/prof_<tag>/ (scripts/collect_profiles.sh) into profiles/<tag>_*.{csv,json}."""
import collections, csv, glob, json, os, shutil, sys

tag = sys.argv[1] if len(sys.argv) > 1 else "r01"
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
src = os.path.join(root, "gpurun_out", "prof_" + tag)
dst = os.path.join(root, "profiles")
os.makedirs(dst, exist_ok=True)
OURS = ("score_gemm_kernel", "finish_topk_kernel", "merge_topk_kernel", "l2_normalize_kernel", "l2_normalize_regs_kernel",
        "gemm_dma_f64_kernel", "gemm_bias_act_kernel", "distance_matrix_kernel", "distinctive_score_kernel",
        "pair_score_kernel", "pair_score_tile_kernel", "transpose_f64_kernel", "splitk_groups_kernel", "splitk_dense_kernel", "maxpool_kernel", "row_minmax_kernel",
        "quant_gather_kernel", "row_stats_kernel", "gram_i8_kernel", "pair_score_amin_kernel", "gram_blocks_kernel", "sim_rows_kernel",
        "sim_range_kernel", "sim_pairwise_program_kernel", "exhaustive_topk_kernel", "score_gemv_kernel", "stream_argmin_kernel",
        "stream_score_kernel", "random_mask_kernel", "xent_grad_kernel", "hidden_grad_kernel", "sgd_kernel",
        "gemm_split_f16_kernel", "sp_split_rows_kernel", "sp_split_weights_kernel", "sim_colrange_kernel", "sim_sample_kernel",
        "sim_keys_init_kernel", "topk_rows_f64_kernel", "update_kernel", "max_row_norm_kernel", "tau_scale_kernel", "small_topk_kernel", "frame_norm_kernel", "colsum_kernel", "finish_topk_coop_kernel", "merge_topk_kernel", "keep_older_kernel")

newest = lambda pat: max(glob.glob(pat), key=os.path.getmtime)
stats = newest(os.path.join(src, "stats", "*", "*kernel_stats.csv"))
with open(stats) as f, open(os.path.join(dst, tag + "_bench_kernel_stats.csv"), "w") as g:
    for i, line in enumerate(f):
        if i == 0 or any(k in line for k in OURS):
            g.write(line)

import subprocess
try:
    commit = subprocess.check_output(["git", "-C", root, "rev-parse", "--short", "HEAD"], text=True).strip()
    dirty = bool(subprocess.check_output(["git", "-C", root, "status", "--porcelain", "--", "deeploopcloser_amd", "bench.py"], text=True).strip())
except Exception:
    commit, dirty = None, None
summary = {"tag": tag, "commit": commit, "tree_dirty_when_summarised": dirty, "command": "rocprofv3 --kernel-trace [--stats | --pmc ... (separate passes, --no-paths)] -- python3 bench.py --full --steps 40 --warmup 10 --no-cpu-baseline --no-power-probe --no-shard-emulation --no-configs",
           "kernels": {}}
HEADLINE = "score_gemm_kernel<dlc_bf16_tag, 0, false>"      # the 1 M-row launch of the timed loop (GROUPS epilogue, unmasked)
for row in csv.DictReader(open(stats)):
    if HEADLINE in row["Name"]:
        summary["kernels"]["score_gemm_kernel"] = {"calls": int(row["Calls"]), "total_ns": float(row["TotalDurationNs"]),
                                                    "avg_ns": float(row["AverageNs"]), "min_ns": float(row["MinNs"]),
                                                    "instantiation": HEADLINE}
        continue
    for k in OURS:
        if k == "score_gemm_kernel":
            continue
        if k + "<" in row["Name"] or k + "(" in row["Name"]:
            e = summary["kernels"].setdefault(k, {"calls": 0, "total_ns": 0.0})
            e["calls"] += int(row["Calls"])
            e["total_ns"] += float(row["TotalDurationNs"])
            e["avg_ns"] = e["total_ns"] / e["calls"]
# The headline launch alone, from the same pass's kernel TRACE: kernel_stats.csv aggregates by instantiation, and other rows
# of the bench (the 4096-wide SDAV row's batches against 31 890 patch descriptors, r06) launch the same instantiation on
# small grids.  The headline's launches are the ones with the largest grid (3907 tiles at 1 M rows).
trace = newest(os.path.join(src, "stats", "*", "*kernel_trace.csv"))
rows = [r for r in csv.DictReader(open(trace)) if HEADLINE in r["Kernel_Name"]]
if rows:
    gmax = max(int(r["Grid_Size_X"]) for r in rows)
    durs = [int(r["End_Timestamp"]) - int(r["Start_Timestamp"]) for r in rows if int(r["Grid_Size_X"]) == gmax]
    g = summary["kernels"].setdefault("score_gemm_kernel", {})
    g.update({"calls_all_grids": g.get("calls"), "avg_ns_all_grids": g.get("avg_ns"), "calls": len(durs),
              "avg_ns": sum(durs) / len(durs), "min_ns": min(durs), "max_ns": max(durs), "total_ns": float(sum(durs)),
              "grid_size_x": gmax, "source": "kernel trace of the --stats pass, launches of the largest grid only"})
    with open(os.path.join(dst, tag + "_bench_headline_launches.csv"), "w") as f:
        f.write("kernel,grid_size_x,launch,duration_ns\n")
        for i, d in enumerate(durs):
            f.write("%s,%d,%d,%d\n" % (HEADLINE.replace(",", ";"), gmax, i, d))
for sub in ("pmc_fetch", "pmc_write", "pmc_sq"):
    if not glob.glob(os.path.join(src, sub, "*", "*counter_collection.csv")):
        continue
    f = newest(os.path.join(src, sub, "*", "*counter_collection.csv"))
    agg = collections.defaultdict(list)
    for r in csv.DictReader(open(f)):
        if HEADLINE in r["Kernel_Name"]:
            agg[("score_gemm_kernel", r["Counter_Name"])].append(float(r["Counter_Value"]))
            continue
        for k in ("finish_topk_kernel", "l2_normalize_regs_kernel"):
            if k + "<" in r["Kernel_Name"] or k + "(" in r["Kernel_Name"]:
                agg[(k, r["Counter_Name"])].append(float(r["Counter_Value"]))
    for (k, c), v in agg.items():
        v = v[len(v) // 3:] or v                      # skip warm-up launches
        summary["kernels"].setdefault(k, {})[c] = sum(v) / len(v)
g = summary["kernels"].get("score_gemm_kernel", {})
if "FETCH_SIZE" in g:
    # MI355X_MICROARCH.md "HBM": FETCH_SIZE (KiB) reports 1/2 of a wide coalesced stream on gfx950 -> x2;
    # WRITE_SIZE (KiB) is exact for 16-B-per-lane stores (ours are 8-B float2 / 4-B: uncalibrated, small)
    g["hbm_read_bytes_per_launch_corrected"] = g["FETCH_SIZE"] * 1024 * 2
    g["hbm_write_bytes_per_launch"] = g.get("WRITE_SIZE", 0.0) * 1024
    g["hbm_traffic_bytes_per_launch"] = g["hbm_read_bytes_per_launch_corrected"] + g["hbm_write_bytes_per_launch"]
    g["workload"] = {"db_rows": 1000000, "dim": 4096, "queries": 256, "dtype": "bf16", "n_gpus": 1}
json.dump(summary, open(os.path.join(dst, tag + "_pmc_summary.json"), "w"), indent=1, sort_keys=True)
print(json.dumps(summary["kernels"].get("score_gemm_kernel", {}), indent=1))
