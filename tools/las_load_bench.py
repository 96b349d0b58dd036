#!/usr/bin/env python
"""LAS input, measured (GPU box; there is no CPU fallback). The cloud is bench.py's config-2 generator (--points Gaussian-cluster
points, seed 1) quantised to millimetres and written by the truth writer (tests/las_truth.py) onto tmpfs twice: as point data
record format 3 in LAS 1.2 (34 bytes per record) and as format 7 in LAS 1.4 (36 bytes), with 16-bit colours, a hashed
intensity, gps times, return numbers and classes of which class 2 is half. The same points also go out as a float-xyz + uchar-rgb
PLY (15 bytes per point), the file build_octree_from_file took before.

One process, a warm-up of every leg and then --runs rounds in which the legs alternate; medians and spreads:
  load_f3 / load_f7   Context.las_load with intensity and three extras (classification, return_number, gps_time): wall time,
                      and the record bytes of the file over it (the rate the link and pread sustain);
  load_f3_half        the same load of format 3 with classes=[2]: the filter keeps half;
  kernels_f3 / _f7    a load with per-launch profiling: the las_* kernels alone (ctx.kernel_stats);
  build_f3            Context.build_from_las of format 3 at 1 mm (load + octree build);
  build_ply           Context.build_from_ply of the PLY (the yardstick: upload + decode + the same build);
  host_f3             read_las, the one-pass host reader, same parameters as load_f3.
Prints one JSON line and writes it to --out.

usage: python tools/las_load_bench.py [--points N] [--runs R] [--tmp DIR] [--out FILE]"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import las_truth as T  # noqa: E402
import point_cloud_viewer_amd as pcv  # noqa: E402
from bench import make_cloud  # noqa: E402

LAS_KERNELS = ("las_tile_count_kernel", "las_tile_scan_kernel", "las_decode_kernel", "las_color_kernel")
EXTRAS = ["classification", "return_number", "gps_time"]
CHUNK = 1 << 23


def spread(values):
    v = np.asarray(values, dtype=np.float64)
    return dict(median=round(float(np.median(v)), 3), min=round(float(v.min()), 3), max=round(float(v.max()), 3), runs=[round(float(t), 3) for t in v])


def write_files(d, x, y, z, rgb):
    """The three files, chunk by chunk -> their paths."""
    n = len(x)
    paths = {3: os.path.join(d, "cloud_f3.las"), 7: os.path.join(d, "cloud_f7.las"), "ply": os.path.join(d, "cloud.ply")}
    handles = {}
    for fmt, minor in ((3, 2), (7, 4)):
        handles[fmt] = open(paths[fmt], "wb")
        handles[fmt].write(T.las_bytes(minor, fmt, b"", n, scale=(0.001,) * 3))
    handles["ply"] = open(paths["ply"], "wb")
    handles["ply"].write((f"ply\nformat binary_little_endian 1.0\nelement vertex {n}\nproperty float x\nproperty float y\nproperty float z\n"
                          "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n").encode())
    for s in range(0, n, CHUNK):
        e = min(n, s + CHUNK)
        i = np.arange(s, e, dtype=np.uint64)
        h = (i * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)
        f = dict(X=np.rint(x[s:e] * 1000.0).astype(np.int32), Y=np.rint(y[s:e] * 1000.0).astype(np.int32), Z=np.rint(z[s:e] * 1000.0).astype(np.int32),
                 intensity=(h >> np.uint64(9)).astype(np.uint16), return_number=(1 + (h >> np.uint64(3)) % np.uint64(3)).astype(np.uint8),
                 number_of_returns=np.full(e - s, 3, np.uint8), scan_direction=(h & np.uint64(1)).astype(np.uint8), edge=np.zeros(e - s, np.uint8),
                 classification=np.where(h & np.uint64(16), 2, 3 + (h >> np.uint64(5)) % np.uint64(4)).astype(np.uint8),
                 flags=np.zeros(e - s, np.uint8), channel=np.zeros(e - s, np.uint8), user_data=np.zeros(e - s, np.uint8),
                 scan_angle=((h >> np.uint64(11)) % np.uint64(60)).astype(np.int16), point_source_id=np.full(e - s, 7, np.uint16),
                 gps_bits=(3.0e8 + i.astype(np.float64) * 1e-5).view(np.uint64), r=rgb[s:e, 0].astype(np.uint16) * 257,
                 g=rgb[s:e, 1].astype(np.uint16) * 257, b=rgb[s:e, 2].astype(np.uint16) * 257, nir=np.zeros(e - s, np.uint16))
        for fmt in (3, 7):
            handles[fmt].write(T.pack_records(fmt, f))
        row = np.zeros(e - s, dtype=[("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("r", "u1"), ("g", "u1"), ("b", "u1")])
        row["x"], row["y"], row["z"] = f["X"] * 0.001, f["Y"] * 0.001, f["Z"] * 0.001
        row["r"], row["g"], row["b"] = rgb[s:e, 0], rgb[s:e, 1], rgb[s:e, 2]
        row.tofile(handles["ply"])
        print(f"written {e} of {n} points", file=sys.stderr, flush=True)
    for h in handles.values():
        h.close()
    return paths


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100_000_000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--tmp", default="/dev/shm" if os.path.isdir("/dev/shm") else None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "las_load_bench.json"))
    args = ap.parse_args()
    n = args.points
    x, y, z, rgb = (t.cpu().numpy() for t in make_cloud(torch, n, 1, "cuda:0"))
    torch.cuda.empty_cache()
    ctx = pcv.Context(0)
    with tempfile.TemporaryDirectory(dir=args.tmp) as d:
        t0 = time.perf_counter()
        paths = write_files(d, x, y, z, rgb)
        del x, y, z, rgb
        write_s = time.perf_counter() - t0
        record_bytes = {3: 34 * n, 7: 36 * n}
        kw = dict(extras=EXTRAS, keep_intensity=True)
        facts = {}

        def load(fmt, **more):
            t = time.perf_counter()
            c = ctx.las_load(paths[fmt], **kw, **more)
            ms = (time.perf_counter() - t) * 1e3
            facts[(fmt, tuple(sorted(more)))] = dict(kept=c.info["num_kept"], pieces=c.info["num_pieces"], color_rule=c.info["color_rule"])
            c.free()
            return ms

        def kernels(fmt):
            ctx.set_profiling(True)
            ctx.reset_kernel_stats()
            load(fmt)
            st = ctx.kernel_stats()
            ctx.set_profiling(False)
            return sum(st[k][1] for k in LAS_KERNELS if k in st)

        def build(what):
            t = time.perf_counter()
            tree = ctx.build_from_las(0.001, paths[3], keep_intensity=False) if what == "las" else ctx.build_from_ply(0.001, paths["ply"])
            ms = (time.perf_counter() - t) * 1e3
            facts["nodes_" + what] = tree.num_nodes
            tree.free()
            return ms

        def host():
            t = time.perf_counter()
            got = pcv.read_las(paths[3], **kw)
            ms = (time.perf_counter() - t) * 1e3
            facts["host_kept"] = got["info"]["num_kept"]
            return ms

        legs = {"load_f3": lambda: load(3), "load_f7": lambda: load(7), "load_f3_half": lambda: load(3, classes=[2]),
                "kernels_f3": lambda: kernels(3), "kernels_f7": lambda: kernels(7), "build_f3": lambda: build("las"),
                "build_ply": lambda: build("ply"), "host_f3": host}
        for k, leg in legs.items():  # warm-up: the pinned ring, the pool's blocks, the page cache
            print(f"warm-up {k}: {leg():.1f} ms", file=sys.stderr, flush=True)
        times = {k: [] for k in legs}
        for r in range(args.runs):
            for k, leg in legs.items():
                times[k].append(leg())
            print(f"round {r + 1} of {args.runs} done", file=sys.stderr, flush=True)
    ms = {k: spread(v) for k, v in times.items()}
    out = {"tool": "tools/las_load_bench.py", "points": n, "runs": args.runs, "files_on": args.tmp or tempfile.gettempdir(),
           "write_files_s": round(write_s, 1), "record_bytes": {"f3": record_bytes[3], "f7": record_bytes[7], "ply": 15 * n},
           "extras": EXTRAS, "ms": ms,
           "load_GB_per_s": {"f3": round(record_bytes[3] / ms["load_f3"]["median"] / 1e6, 2), "f7": round(record_bytes[7] / ms["load_f7"]["median"] / 1e6, 2)},
           "kernels_GB_per_s_of_records": {"f3": round(record_bytes[3] / ms["kernels_f3"]["median"] / 1e6, 1),
                                           "f7": round(record_bytes[7] / ms["kernels_f7"]["median"] / 1e6, 1)},
           "half_mask_kept": facts[(3, ("classes",))]["kept"], "pieces": facts[(3, ())]["pieces"], "color_rule": facts[(3, ())]["color_rule"],
           "nodes": {"las": facts["nodes_las"], "ply": facts["nodes_ply"]},
           "host_reader_over_load": round(ms["host_f3"]["median"] / ms["load_f3"]["median"], 1),
           "build_las_over_build_ply": round(ms["build_f3"]["median"] / ms["build_ply"]["median"], 2)}
    line = json.dumps(out)
    print(line)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
