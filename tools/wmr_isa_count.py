#!/usr/bin/env python3
"""Static count of the f64 operations of the web-mercator per-point chain: compiles tools/wmr_chain_probe.hip for gfx950 with the
library's flags (needs hipcc, no GPU), counts the v_*_f64 instructions of the one kernel by mnemonic and writes
profiles/wmr_isa_count.json. Static means every instruction once: the chain's branches (the NaN / infinity / subnormal guards,
the swap and quadrant fix-ups of atan2) are counted whether a lane takes them or not, and there is no loop in it.

usage: python tools/wmr_isa_count.py [--out FILE]"""
import argparse
import collections
import json
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wmr_isa_count.json"))
    args = ap.parse_args()
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as tmp:
        asm = os.path.join(tmp, "probe.s")
        subprocess.check_call([hipcc, "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "--offload-arch=gfx950",
                               "--cuda-device-only", "-S", os.path.join(ROOT, "tools", "wmr_chain_probe.hip"), "-o", asm])
        text = open(asm).read()
    body = text[text.index("wmr_chain_probe:"):text.index("s_endpgm")]
    ops = collections.Counter(m.group(1) for m in re.finditer(r"^\s+(v_\w+_f64(?:_e32|_e64)?)\b", body, re.M))
    ops = collections.Counter({re.sub(r"_e(32|64)$", "", k): 0 for k in ops}) + collections.Counter(
        {re.sub(r"_e(32|64)$", "", k): v for k, v in ops.items()})
    merged = collections.Counter()
    for k, v in ops.items():
        merged[k] += v
    total = sum(merged.values())
    valu = len(re.findall(r"^\s+v_\w+", body, re.M))
    # an fma counts two flops; v_div_scale / v_div_fmas / v_div_fixup / v_rcp / v_rsq / compares / conversions one operation each
    flops = total + merged.get("v_fma_f64", 0) + merged.get("v_fmac_f64", 0)
    out = {"tool": "tools/wmr_isa_count.py", "kernel": "wmr_chain_probe (one wmr::contains per thread)", "arch": "gfx950",
           "f64_instructions_per_point": total, "f64_flops_per_point_fma_as_two": flops, "valu_instructions_per_point": valu,
           "by_mnemonic": dict(sorted(merged.items(), key=lambda kv: -kv[1]))}
    print(json.dumps(out))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
