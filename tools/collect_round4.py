"""copies the summaries of `tools/measure_round4.sh` (gpurun_out/r04m, gpurun_out/r04*) into profiles/r04_* (tracked)"""
import csv, glob, json, os, re, shutil
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
o = os.path.join(R, "gpurun_out", "r04m")
P = os.path.join(R, "profiles")
head = open(os.path.join(o, "head.txt")).read().strip() if os.path.exists(os.path.join(o, "head.txt")) else "?"
shutil.copy(os.path.join(o, "bench.json"), os.path.join(P, "r04_bench.json"))
for f in glob.glob(os.path.join(o, "prof", "**", "*kernel_stats.csv"), recursive=True):
    shutil.copy(f, os.path.join(P, "r04_kernel_stats.csv"))
# per-launch durations of k_decode from the kernel trace
rows = []
for f in glob.glob(os.path.join(o, "prof", "**", "*kernel_trace.csv"), recursive=True):
    for r in csv.DictReader(open(f)):
        if "k_decode<" in r["Kernel_Name"]:
            rows.append((int(r["Start_Timestamp"]), (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6, r.get("Grid_Size_X", ""), r.get("VGPR_Count", ""), r.get("LDS_Block_Size", "")))
rows.sort()
with open(os.path.join(P, "r04_kernel_trace_k_decode.txt"), "w") as f:
    f.write(f"rocprofv3 --kernel-trace --stats -- python3 bench.py --steps 3 --warmup 1 --full --no-cpu-baseline   (tree {head})\n")
    f.write("k_decode launches in time order: duration ms, grid size, VGPRs, LDS bytes\n")
    for _, ms, g, v, l in rows:
        f.write(f"  {ms:9.3f}  grid {g}  vgpr {v}  lds {l}\n")
if os.path.exists(os.path.join(R, "gpurun_out", "r04_traffic.json")):
    shutil.copy(os.path.join(R, "gpurun_out", "r04_traffic.json"), os.path.join(P, "r04_traffic.json"))
for c in ("FETCH_SIZE", "WRITE_SIZE"):
    for f in glob.glob(os.path.join(R, "gpurun_out", "r04_traffic", c, "*counter_collection.csv")):
        keep = [l for i, l in enumerate(open(f)) if i == 0 or "k_decode" in l]
        open(os.path.join(P, f"r04_pmc_{c.lower()}.csv"), "w").writelines(keep)
shutil.copy(os.path.join(o, "pmc_decode.txt"), os.path.join(P, "r04_pmc_decode.txt"))
shutil.copy(os.path.join(o, "stamps.txt"), os.path.join(P, "r04_phase_stamps_and_voiced.txt"))
e = os.path.join(R, "gpurun_out", "r04", "enc_prof")
if os.path.exists(os.path.join(e, "summary.txt")):
    shutil.copy(os.path.join(e, "summary.txt"), os.path.join(P, "r04_encode_pmc_summary.txt"))
    shutil.copy(os.path.join(e, "timing.txt"), os.path.join(P, "r04_encode_timing.txt"))
    for f in glob.glob(os.path.join(e, "trace", "**", "*kernel_stats.csv"), recursive=True):
        shutil.copy(f, os.path.join(P, "r04_encode_kernel_stats.csv"))
txt = open(os.path.join(o, "ws_check.txt")).read() + "\n---- stage profile (-DFPC_WS_PROF -DFPC_WS_PROF_TAIL build, workgroup 5 of group 0; cycles per frame) ----\n" + \
    "\n".join(l for l in open(os.path.join(o, "ws_prof.txt")).read().splitlines() if "cycles/frame" in l or "frames" in l or "frame above" in l)
open(os.path.join(P, "r04_predictor_ws.txt"), "w").write(f"tree {head}; library: " + open(os.path.join(o, "build_info.txt")).read() + txt + "\n")
open(os.path.join(P, "r04_train_timing.txt"), "w").write(
    f"tree {head}; tools/time_train.py: the shipped step (forward on the weights-stationary kernel k_forward_ws<true>), then FPC_PRED_WS=0\n" +
    "".join(l for l in open(os.path.join(o, "train.txt")) if "amdgpu.ids" not in l))
if os.path.exists(os.path.join(o, "chunk.txt")):
    open(os.path.join(P, "r04_chunked_decode_rerun.txt"), "w").write(
        f"tree {head}; tools/chunk_bench.py 0 150 100 50 0 (the table of r04_chunked_decode.txt measured again in the round's last pass)\n" +
        "".join(l for l in open(os.path.join(o, "chunk.txt")) if "amdgpu.ids" not in l))
print("collected into profiles/r04_*")
