#!/usr/bin/env python
"""Post-processes rocprofv3 PMC passes of `python bench.py` into profiles/pmc_traffic.json.

    rocprofv3 --pmc FETCH_SIZE --kernel-trace --output-format csv -d <out>/pmc_fetch -o p -- python bench.py --full ...
    rocprofv3 --pmc WRITE_SIZE --kernel-trace --output-format csv -d <out>/pmc_write -o p -- python bench.py --full ...
    python scripts/collect_pmc.py <out>/pmc_fetch <out>/pmc_write > profiles/pmc_traffic.json

Units / corrections (MI355X_MICROARCH.md §HBM): FETCH_SIZE and WRITE_SIZE are in KiB; on gfx950 FETCH_SIZE
counts 64 B per 128-B request for wide (16 B/lane) coalesced streams, so it is DOUBLED for the kernels whose
reads are such streams (the GEMM families and the row chain: 16-byte LDS-DMA / float4 operand loads).  WRITE_SIZE is
uncalibrated in the guide and is used AS REPORTED for every kernel (an upper bound for the GEMM store pattern: a launch
with a known byte count read 1.63x high in round 1).
"""
import collections
import csv
import glob
import json
import sys

FAMILY = [("gemm2_kernel<256, 128, 4, 2, 3, 2, true>", "gemm2_kernel<256,128,pool>"), ("gemm2_kernel<256, 128, 4, 2, 3, 2, false>", "gemm2_kernel<256,128>"),
          ("gemm2_kernel<128, 128, 2, 2, 3, 3, true>", "gemm2_kernel<128,128,pool>"), ("gemm2_kernel<128, 128, 2, 2, 3, 3, false>", "gemm2_kernel<128,128>"),
          ("gemm2_kernel<64, 128", "gemm2_kernel<64,128>"), ("mlp_gemm_kernel<3", "mlp_gemm_kernel<3>"), ("mlp_gemm_kernel<0", "mlp_gemm_kernel<0>"), ("mlp_gemm_kernel", "mlp_gemm_kernel"), ("sa3_premul_chain_kernel", "sa3_premul_chain_kernel"), ("sa_premul_chain_kernel", "sa_premul_chain_kernel"), ("fp_head_chain_kernel", "fp_head_chain_kernel"), ("sa_chain_kernel", "sa_chain_kernel"), ("fps_", "fps_kernel"), ("ball_query_kernel", "ball_query_kernel"),
          ("ball_query_grid_kernel", "ball_query_grid_kernel"), ("three_nn_kernel", "three_nn_kernel"),
          ("three_nn_grid_kernel", "three_nn_grid_kernel"), ("interp_concat_kernel", "interp_concat_kernel"),
          ("interp_affine_kernel", "interp_affine_kernel"), ("gather_max", "gather_max_kernel"),
          ("radius_group_kernel", "radius_group_kernel"), ("select_positive_kernel", "select_positive_kernel")]
WIDE_STREAM = {"gemm2_kernel<64,128>", "gemm2_kernel<256,128,pool>", "gemm2_kernel<256,128>", "gemm2_kernel<128,128,pool>", "gemm2_kernel<128,128>", "mlp_gemm_kernel", "mlp_gemm_kernel<3>", "mlp_gemm_kernel<0>", "fp_head_chain_kernel", "sa_premul_chain_kernel", "sa3_premul_chain_kernel", "interp_concat_kernel", "interp_affine_kernel"}
WRITE_CAL = {}   # WRITE_SIZE is used as reported (round 1 scaled the GEMM family by an empirical 0.612; dropped: the guide
                 # gives no calibration for writes, and the uncorrected totals are what DESIGN.md quotes)


def family(kernel_name):
    for pat, fam in FAMILY:
        if pat in kernel_name:
            return fam
    return None


NAMES = collections.defaultdict(set)   # family -> exact kernel names (rocprofv3's demangled spelling) the passes saw


def short_name(kernel_name):
    """'void fps_cluster_kernel<25, 8, false>(float const*, ...)' -> 'fps_cluster_kernel<25, 8, false>'."""
    name = kernel_name.strip()
    if name.startswith("void "):
        name = name[5:]
    depth = 0
    for i, ch in enumerate(name):
        depth += ch == "<"
        depth -= ch == ">"
        if ch == "(" and depth == 0:
            return name[:i]
    return name


def collect(directory, counter):
    tot, n = collections.Counter(), collections.Counter()
    for f in glob.glob(directory + "/**/*counter_collection.csv", recursive=True):
        for r in csv.DictReader(open(f)):
            fam = family(r["Kernel_Name"])
            if fam and r["Counter_Name"] == counter:
                tot[fam] += float(r["Counter_Value"])
                n[fam] += 1
                NAMES[fam].add(short_name(r["Kernel_Name"]))
    return tot, n


def main(fetch_dir, write_dir):
    ft, fn = collect(fetch_dir, "FETCH_SIZE")
    wt, wn = collect(write_dir, "WRITE_SIZE")
    out = {}
    for fam in sorted(set(ft) | set(wt)):
        fetch_kib = ft[fam] / max(fn[fam], 1)
        write_kib = wt[fam] / max(wn[fam], 1)
        corr = 2.0 if fam in WIDE_STREAM else 1.0
        wcal = WRITE_CAL.get(fam, 1.0)
        out[fam] = {"launches_profiled": int(max(fn[fam], wn[fam])),
                    "fetch_size_kib_per_launch_raw": round(fetch_kib, 1),
                    "fetch_correction": corr,
                    "write_size_kib_per_launch_raw": round(write_kib, 1),
                    "write_calibration": round(wcal, 4),
                    "hbm_bytes_per_launch": int((fetch_kib * corr + write_kib * wcal) * 1024),
                    # what bench.py holds against the library's kernel list (roofline.traffic_source.stale)
                    "kernel_names": sorted(NAMES[fam])}
    json.dump(out, sys.stdout, indent=1, sort_keys=True)
    print()


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
