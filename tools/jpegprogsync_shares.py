"""Kernel shares of a JpegFiles.run with scan_substreams from rocprofv3 kernel traces.

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/jpegprogsync_shares.py --run mix_B32
    python tools/jpegprogsync_shares.py --traces mix_B32=DIR1 1024x1024_B256=DIR2 [--bench profiles/jpegprogsync_bench.json]
                                        [--out profiles/jpegprogsync_kernel_shares.json]

--run decodes one case of tools/jpegprogsync_bench.py three times with the keyword on (the process to trace).  --traces reads
the kernel_trace.csv under each directory and writes, for the THIRD run of each process, every launch in order, the time of
the new kernel and of what is left of the entropy launches per level, and their shares of the run's kernel time.  The
three parts of the new kernel per scan kind (for an AC refinement: masks / skim / write) cannot come from a kernel trace:
they are copied from the tick stamps in --bench (scan_kinds[...].part_shares), when given."""
import argparse
import csv
import glob
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def run(case):
    import torch
    import jpegdec_bench as JB
    import jpegprog_bench as PB
    from attwarp_amd import jpeg
    B, sizes = JB.CASES[case]
    jf = jpeg.JpegFiles(PB.make_files("plain", JB.images(B, sizes), True), device="cuda:0", progressive=True, scan_substreams=True)
    for _ in range(3):
        jf.run()
    torch.cuda.synchronize()


def shares(case, d):
    rows = list(csv.DictReader(open(glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)[0])))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    ks = [(r["Kernel_Name"].split("(")[0].replace("attwarp::", ""), (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6)
          for r in rows if "attwarp::" in r["Kernel_Name"]]
    last = ks[-(len(ks) // 3):]
    total = sum(t for _, t in last)
    sub = [t for k, t in last if k == "jpegprog_substream_kernel"]
    ent = [t for k, t in last if k == "jpegprog_entropy_kernel"]
    return {"case": case, "launches": [k for k, _ in last], "kernel_ms_total": round(total, 3),
            "substream_ms_per_level": [round(t, 3) for t in sub], "entropy_ms_per_level": [round(t, 3) for t in ent],
            "other_ms": {k: round(t, 3) for k, t in last if not k.startswith("jpegprog_substream") and not k.startswith("jpegprog_entropy")},
            "substream_share_per_level": [round(t / total, 4) for t in sub], "entropy_share_per_level": [round(t / total, 4) for t in ent]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--run")
    ap.add_argument("--traces", nargs="*", default=[])
    ap.add_argument("--bench")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpegprogsync_kernel_shares.json"))
    args = ap.parse_args()
    if args.run:
        return run(args.run)
    out = {"source": "one rocprofv3 --kernel-trace run per case, the third JpegFiles.run of a process (scan_substreams='auto'); ms",
           "cases": [shares(*t.split("=", 1)) for t in args.traces]}
    if args.bench:
        bench = json.load(open(args.bench))
        out["parts_of_the_new_kernel_by_scan_kind"] = {
            c["case"]: {k: {"part_shares": v["part_shares"], "longest_scan_ms": v["longest_scan_ms"]} for k, v in c["scan_kinds"].items()}
            for c in bench["cases"]}
        out["parts"] = "first passes: rounds / sums and checks / write; refinements: counts and masks / skim / write; from the tick stamps in the per-scan records"
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
