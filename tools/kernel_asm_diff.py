#!/usr/bin/env python3
"""Per-kernel comparison of the device assembly of one translation unit before and after a change — or, when a source was
split or merged, of several (comma-separated files per side): which kernels are identical, differ, went or came.

  hipcc <CXXFLAGS of csrc/Makefile> [-DPCV_EXPERIMENTS] --offload-device-only -S pcv_sort.hip -o before/pcv_sort.s   (old tree)
  hipcc ... -o after/pcv_sort.s                                                                                        (new tree)
  tools/kernel_asm_diff.py before/pcv_sort.s after/pcv_sort.s
  tools/kernel_asm_diff.py before/pcv_query.s after/pcv_shapes.s,after/pcv_cull.s,after/pcv_query.s
  tools/kernel_asm_diff.py before/pcv_sort.s after/pcv_sort.s,after/pcv_sort_rec12.s

A kernel is its function body plus its .amdhsa_kernel descriptor. Assembler comments, .file / .loc / .ident lines and the
per-file function index inside local labels (.LBB<i>_<n>, .Lfunc_end<i>, .LJTI<i>_<n>) are dropped: they move when another
kernel of the file goes. Exit status 1 if a kernel differs or is new. Runs without a GPU."""
import re
import sys


def kernels(paths):
    out = {}
    for path in paths.split(","):
        one = kernels_of(path)
        dup = set(out) & set(one)
        if dup:
            sys.exit(f"{path}: kernels of another file of the same side: {sorted(dup)}")
        out.update(one)
    return out


def kernels_of(path):
    body, desc, cur, into = {}, {}, None, None
    for line in open(path, errors="replace"):
        line = line.rstrip("\n")
        if '"' not in line:
            line = re.sub(r"\s*;.*$", "", line)
        s = line.strip()
        if not s or re.match(r"\.(file|loc|ident)\b", s):
            continue
        m = re.match(r"^([A-Za-z_$][\w$.]*):", line)
        if m:
            cur, into = m.group(1), body
            body.setdefault(cur, [])
        m = re.match(r"\.amdhsa_kernel\s+(\S+)", s)
        if m:
            cur, into = m.group(1), desc
            desc.setdefault(cur, [])
        if cur is None:
            continue
        into[cur].append(re.sub(r"\.L(BB|JTI|func_begin|func_end)\d+", r".L\1", line))
        if s == ".end_amdhsa_kernel":
            cur = None
    return {k: "\n".join(body.get(k, []) + desc[k]) for k in desc}


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    bad = 0
    for k in sorted(set(a) | set(b)):
        tag = "removed" if k not in b else "NEW" if k not in a else "same" if a[k] == b[k] else "DIFFERS"
        bad += tag in ("NEW", "DIFFERS")
        if tag != "same":
            print(f"{tag:8s} {k}")
    print(f"{sum(1 for k in a if k in b and a[k] == b[k])} identical, {sum(1 for k in a if k not in b)} removed, {bad} differing or new")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
