"""Summarise rocprofv3 --pmc passes (one counter_collection.csv per pass: FETCH_SIZE, WRITE_SIZE, SQ_*) into one JSON keyed by the
in-library profiler's kernel names (what bench.py's roofline/raster blocks look up).
HBM bytes per launch = 2 x FETCH_SIZE (gfx950 tallies 128-B requests of wide streams at 64 B, MI355X_MICROARCH.md section HBM) + WRITE_SIZE,
both reported by rocprofv3 in KB.
usage: pmc_summary.py OUT.json "source text" pass1.csv [pass2.csv ...]"""
import csv
import json
import re
import sys
from collections import defaultdict


def short_name(k: str) -> str:
    k = k.replace("void ", "").replace("mp::", "").replace("stem::", "")
    m = re.match(r"(\w+)(<(.*)>)?\(", k + "(")
    if not m:
        return k
    name, targs = m.group(1), (m.group(3) or "")
    args = [a.strip() for a in targs.split(",")] if targs else []
    if name == "conv_nhwc_f32_mfma" and len(args) >= 4:   # <BN, RAGGED, SPLITK, AHALF>
        s = f"{name}<128,{args[0]},64,{int(args[0]) // 2}>"
        if args[2] in ("true", "1"):
            s += "/splitk"
        return s
    if name == "conv3x3_wino_f32":
        return "conv3x3_wino_f32<64t,64c>"   # (the in-library profiler's row name of the Winograd kernel)
    if name == "conv3x3_wino_bf16x9":
        return "conv3x3_wino_bf16x9<64t,64c>"
    if name == "conv_stem_bf16x3" and len(args) >= 2:
        pool = len(args) >= 3 and args[2] in ("true", "1")
        return f"conv_stem_bf16x3{'+maxpool' if pool else ''}<{args[0]}x{args[0]},Q{args[1]}>"
    if name == "raster_tiles" and len(args) >= 2:
        return {"0": "raster_tiles", "1": "raster_tiles/f16", "2": "raster_tiles/xrec"}.get(args[1], name)
    return name


def main():
    out_path, source, files = sys.argv[1], sys.argv[2], sys.argv[3:]
    per = defaultdict(lambda: defaultdict(list))  # kernel -> counter -> per-dispatch values
    for f in files:
        with open(f, newline="") as fh:
            by_dispatch = defaultdict(float)
            meta = {}
            for row in csv.DictReader(fh):
                key = (row["Dispatch_Id"], row["Counter_Name"])
                by_dispatch[key] += float(row["Counter_Value"])  # one row per (dispatch, counter[, dimension])
                meta[row["Dispatch_Id"]] = row["Kernel_Name"]
            for (d, c), v in by_dispatch.items():
                if "mp::" in meta[d]:  # the engine's kernels only (torch fill/copy kernels of the harness are not ours)
                    per[short_name(meta[d])][c].append(v)
    kernels = {}
    for k, cs in per.items():
        e = {"launches": max(len(v) for v in cs.values())}
        for c, v in cs.items():
            if c in ("FETCH_SIZE", "WRITE_SIZE"):
                e[f"{c}_KB_per_launch"] = sum(v) / len(v)
            else:
                e[f"{c}_sum"] = sum(v)
        if "FETCH_SIZE_KB_per_launch" in e and "WRITE_SIZE_KB_per_launch" in e:
            e["hbm_bytes_per_launch_corrected"] = (2.0 * e["FETCH_SIZE_KB_per_launch"] + e["WRITE_SIZE_KB_per_launch"]) * 1024.0
        if "SQ_WAVE_CYCLES_sum" in e:
            for c in ("SQ_WAIT_ANY", "SQ_WAIT_INST_ANY", "SQ_ACTIVE_INST_ANY"):
                if f"{c}_sum" in e:
                    e[f"{c}_over_SQ_WAVE_CYCLES"] = e[f"{c}_sum"] / max(e["SQ_WAVE_CYCLES_sum"], 1.0)
        if "SQ_VALU_MFMA_BUSY_CYCLES_sum" in e and "SQ_BUSY_CU_CYCLES_sum" in e:
            e["mfma_busy_frac"] = e["SQ_VALU_MFMA_BUSY_CYCLES_sum"] / max(4.0 * e["SQ_BUSY_CU_CYCLES_sum"], 1.0)
        kernels[k] = e
    json.dump({"source": source, "note": "FETCH_SIZE / WRITE_SIZE in KB per launch (mean over the pass); hbm_bytes_per_launch_corrected = "
               "(2 x FETCH_SIZE + WRITE_SIZE) x 1024 bytes", "kernels": kernels}, open(out_path, "w"), indent=1)
    for k, e in sorted(kernels.items(), key=lambda kv: -kv[1].get("hbm_bytes_per_launch_corrected", 0) * kv[1]["launches"]):
        print(f"{k:50s} {e['launches']:5d} launches  {e.get('hbm_bytes_per_launch_corrected', 0) / 1e6:10.1f} MB/launch")


if __name__ == "__main__":
    main()
