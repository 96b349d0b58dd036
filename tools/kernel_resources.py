#!/usr/bin/env python3
"""Tabulate hipcc's -Rpass-analysis=kernel-resource-usage remarks: one row per kernel.

  hipcc ... -Rpass-analysis=kernel-resource-usage -c pcv_cull.hip -o /dev/null 2> report.txt
  tools/kernel_resources.py report.txt [other_report.txt]     # with two reports: the rows that differ are marked

Runs without a GPU (the report comes from the compiler)."""
import re
import subprocess
import sys

FIELDS = ["VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "LDS Size [bytes/block]"]


def parse(path):
    rows, cur = {}, None
    for line in open(path, errors="replace"):
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            rows[cur] = {}
            continue
        m = re.search(r"remark:\s+(.+?): (\d+)(?:\s+\[-R.*\])?\s*$", line)
        if m and cur:
            rows[cur][m.group(1)] = int(m.group(2))
    return rows


def demangle(names):
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
        return dict(zip(names, (re.sub(r"\(.*", "", re.sub(r"^void ", "", o).replace("(anonymous namespace)::", "")) for o in out)))
    except Exception:
        return {n: n for n in names}


def main():
    a = parse(sys.argv[1])
    b = parse(sys.argv[2]) if len(sys.argv) > 2 else None
    names = demangle(sorted(set(a) | set(b or {})))
    print("| kernel | " + " | ".join(f.split(" [")[0] for f in FIELDS) + (" | vs first |" if b else " |"))
    print("|---|" + "---|" * (len(FIELDS) + (1 if b else 0)))
    for n in sorted(names, key=lambda k: names[k]):
        row = (b if b is not None else a).get(n)
        if row is None:
            print(f"| {names[n]} | " + " | ".join("-" for _ in FIELDS) + " | removed |")
            continue
        cells = " | ".join(str(row.get(f, "")) for f in FIELDS)
        if b is None:
            print(f"| {names[n]} | {cells} |")
        else:
            tag = "new" if n not in a else ("same" if all(a[n].get(f) == row.get(f) for f in FIELDS) else "CHANGED " + str([a[n].get(f) for f in FIELDS]))
            print(f"| {names[n]} | {cells} | {tag} |")


if __name__ == "__main__":
    main()
