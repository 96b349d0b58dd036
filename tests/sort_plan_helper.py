"""The stand-alone plan driver (tests/sort_plan_driver.cpp + csrc/pcv_sort_plan.cpp, ASan + UBSan, no HIP, no library) for the
tests that pin plans on a machine without a GPU: tests/test_sort_plan_cpu.py and tests/test_sort_records_cpu.py."""
import json
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "point_cloud_viewer_amd", "csrc")
UPSWEEP, UPSWEEP_MAP, ROWS, ROWS_TRUE = range(4)  # PcvSortHist
KEYS, REC_UINT4, REC_UINT2, REC_PLANES, REC12_CHUNKS, REC12_PIECES = range(6)  # PcvSortDown
SANITIZE = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
            "-static-libasan", "-static-libubsan"]  # the runtimes inside the program: nothing to preload


def facts(n, begin, end, key_bytes=4, vec_in=0, vec_bytes=16, nwords=0, color_in=0, map=0, map_entries=0, rows=0, second=0,
          sort_rows2=1, sort_msd=0, bins=0):
    """One line of the driver's input file."""
    return (n, key_bytes, begin, end, vec_in, vec_bytes, nwords, color_in, map, map_entries, rows, second, sort_rows2, sort_msd, bins)


def build_driver(tmp):
    exe = tmp / "sort_plan_driver"
    subprocess.check_call(SANITIZE + [os.path.join(ROOT, "tests", "sort_plan_driver.cpp"), os.path.join(CSRC, "pcv_sort_plan.cpp"),
                                      "-o", str(exe)])
    return exe


def run_facts(exe, tmp, name, all_facts):
    """The driver over a file of facts -> (the finished process, its JSON lines: a plan and a scratch layout per sort)."""
    path = tmp / name
    path.write_text("".join(" ".join(str(int(v)) for v in f) + "\n" for f in all_facts))
    p = subprocess.run([str(exe), str(path)], capture_output=True, text=True)
    return p, [json.loads(line) for line in p.stdout.splitlines()]


def sanitizers_silent(p):
    assert p.returncode == 0, (p.stdout[-1000:] + p.stderr)[-3000:]
    assert "runtime error" not in p.stderr and "Sanitizer" not in p.stderr, p.stderr[-3000:]
