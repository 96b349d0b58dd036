#!/usr/bin/env python
"""Stored against deflate PNG tiles measured (GPU box): the config-2 cloud (100 M Gaussian-cluster points, bench.py's
generator and seed) built once, its xray quadtree (tile_size_px = 256, pixel_size_m = 0.1, strategy xray, parents built),
then XrayTiles.write into a temporary directory per mode and step: directory bytes, median wall ms of write, the summed
kernel ms of the three xray_png_* kernels, and the bytes copied to the host (stored: every node image; deflate: the
compacted streams and their offsets).

Comparators: the stored write of the parent commit (profiles/r09_xray_pyramid_bench.json, 115 ms for 1 585 files), and for
size zlib.compress(level=1) over the same filtered scanlines (Sub on row 0, Up after it), computed here on the CPU.
Every deflate file of a sample is read back with Python's zlib and must give the stored file's pixels.
Prints one JSON line and writes it to --out.

usage: python tools/xray_png_bench.py [--points N] [--steps K] [--out FILE]"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import point_cloud_viewer_amd as pcv  # noqa: E402
import xray_png_oracle as PO  # noqa: E402
from bench import build_hash, make_cloud  # noqa: E402

TILE, PIXEL = 256, 0.1
KERNELS = ("xray_png_band_kernel", "xray_png_layout_kernel", "xray_png_gather_kernel")


def directory_bytes(d):
    return sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100_000_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "xray_png_bench.json"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    ctx = pcv.Context(0)
    x, y, z, rgb = make_cloud(torch, args.points, seed=1, device=dev)
    tree = ctx.build(0.001, None, x, y, z, rgb)
    del x, y, z, rgb
    torch.cuda.empty_cache()
    xt = tree.xray_quadtree(TILE, PIXEL, "xray")
    nodes = len(xt.node_ids)
    tmp = tempfile.mkdtemp(prefix="xray_png_bench_")
    rec = {}
    try:
        for mode in ("stored", "deflate"):
            d = os.path.join(tmp, mode)
            walls, kms = [], []
            for step in range(args.steps + 1):  # the first is a warm-up
                ctx.set_profiling(False)
                ctx.synchronize()
                t0 = time.perf_counter()
                xt.write(d, png=mode)
                wall = (time.perf_counter() - t0) * 1e3
                if step:
                    walls.append(wall)
            ctx.set_profiling(True)  # kernel times in a run of their own: the event pairs are not in the wall times
            ctx.reset_kernel_stats()
            xt.write(d, png=mode)
            st = ctx.kernel_stats()
            ctx.set_profiling(False)
            kms = {k: round(st[k][1], 4) for k in KERNELS}
            launches = {k: int(st[k][0]) for k in KERNELS}
            files = [f for f in os.listdir(d) if f.endswith(".png")]
            idat = sum(os.path.getsize(os.path.join(d, f)) - 57 for f in files)
            rec[mode] = {"directory_bytes": directory_bytes(d), "files": len(files) + 1,
                         "write_wall_ms": round(float(np.median(walls)), 1), "write_wall_ms_all": [round(w, 1) for w in walls],
                         "png_kernel_ms": kms, "png_kernel_launches": launches,
                         "bytes_copied_to_host": nodes * TILE * TILE * 4 if mode == "stored" else idat + 8 * (nodes + launches[KERNELS[0]])}
        # size comparator and the read-back, on the CPU
        z1 = raw = 0
        ok = True
        names = sorted(f for f in os.listdir(os.path.join(tmp, "stored")) if f.endswith(".png"))
        for k, f in enumerate(names):
            img = PO.decode(open(os.path.join(tmp, "stored", f), "rb").read())
            filt = PO.filtered(img).tobytes()
            raw += len(filt)
            z1 += len(zlib.compress(filt, 1))
            if k % 16 == 0:
                ok &= bool(np.array_equal(PO.decode(open(os.path.join(tmp, "deflate", f), "rb").read()), img))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    parent = None
    try:
        parent = json.load(open(os.path.join(ROOT, "profiles", "r09_xray_pyramid_bench.json")))["write_wall_ms"]
    except (OSError, KeyError, ValueError):
        pass
    out = {"tool": "tools/xray_png_bench.py", "build_hash": build_hash(), "device": torch.cuda.get_device_name(0),
           "cloud": f"config 2: {args.points} Gaussian-cluster points (bench.make_cloud, seed 1), resolution 0.001",
           "tile_size_px": TILE, "pixel_size_m": PIXEL, "strategy": "xray", "nodes": nodes, "stored": rec["stored"], "deflate": rec["deflate"],
           "filtered_scanline_bytes": raw, "zlib_level1_idat_bytes": z1,
           "deflate_idat_bytes": rec["deflate"]["directory_bytes"] - 57 * nodes,
           "parent_commit_stored_write_wall_ms": parent, "sample_reads_back_equal": ok,
           "note": "write wall times are medians of --steps runs after a warm-up, into a temporary directory (page cache, no fsync)"}
    xt.free()
    tree.free()
    print(json.dumps(out))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    ctx.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
