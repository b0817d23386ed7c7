#!/usr/bin/env python
"""Per-kernel time split of a size-generic launch from a rocprofv3 kernel trace (--kernel-trace, csv): each dispatch is put in the
part of the pipeline it ran in by its place in the stream -- gen_embed_kernel .. gen_dwell_kernel frontend, then the encoder FFT
blocks up to gen_lenreg_kernel, then the decoder FFT blocks up to gen_emit_kernel -- so a kernel both stacks launch (the GEMM, the
LayerNorm, attention) is split into its encoder and decoder time.  Prints a markdown table.
    python tools/trace_split.py <..._kernel_trace.csv> [title] [chunks traced: adds ns per chunk]"""
import collections
import csv
import re
import sys


def split(path):
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    part, tot = "frontend / emit", collections.defaultdict(int)
    for r in rows:
        k = r["Kernel_Name"].split("(")[0].replace("void ", "")
        m = re.match(r"_Z\d+(\w+?)ILi(\d+)EE", k)              # a template instance the tracer left mangled
        if m:
            k = f"{m.group(1)}<{m.group(2)}>"
        if k.startswith("__amd"):
            continue
        if k.startswith(("gen_embed", "gen_lenreg", "gen_emit")):
            part = "frontend / emit"
        tot[(part, k)] += int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
        if k.startswith("gen_dwell"):
            part = "encoder"
        elif k.startswith("gen_lenreg"):
            part = "decoder"
    return tot


def main():
    tot = split(sys.argv[1])
    all_ = sum(tot.values())
    n = int(sys.argv[3]) if len(sys.argv) > 3 else 0
    per = f", {all_ / n:.0f} ns per chunk over {n} chunks" if n else ""
    print(f"### {sys.argv[2] if len(sys.argv) > 2 else sys.argv[1]}: {all_ / 1e6:.1f} ms of kernel time{per}\n")
    print("| part | kernel | ms | share |" + (" ns / chunk |\n|---|---|---:|---:|---:|" if n else "\n|---|---|---:|---:|"))
    for (p, k), v in sorted(tot.items(), key=lambda x: -x[1]):
        print(f"| {p} | `{k}` | {v / 1e6:.1f} | {100 * v / all_:.1f} % |" + (f" {v / n:.1f} |" if n else ""))
    by = collections.defaultdict(int)
    for (p, _), v in tot.items():
        by[p] += v
    print("\n" + ", ".join(f"{p} {100 * v / all_:.1f} %" for p, v in sorted(by.items(), key=lambda x: -x[1])))


if __name__ == "__main__":
    main()
