#!/usr/bin/env python
"""xray inpainting measured (GPU box): the config-2 cloud (100 M Gaussian-cluster points, bench.py's generator and seed)
built once, its xray leaf level with the transparent background (tile_size_px = 256, pixel_size_m = 0.1, strategy xray),
then XrayTiles.inpaint for inpaint_distance_px in {2, 8, 32}: median wall ms of the call (it ends in a stream
synchronise and includes the parent levels), the kernel ms of each inpaint kernel and of the parent kernel
(pcv_ctx_kernel_stats), the target, filled and blended pixel counts, and next to them the wall ms of the leaf build of the
same run as yardstick. Nothing is compared against the reference: its fill is texture synthesis.
Prints one JSON line and writes it to --out.

usage: python tools/xray_inpaint_bench.py [--points N] [--steps K] [--distances 2,8,32] [--out FILE]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import point_cloud_viewer_amd as pcv  # noqa: E402
from bench import build_hash, make_cloud  # noqa: E402

TILE, PIXEL = 256, 0.1
KERNELS = ("xray_inpaint_stitch_kernel", "xray_inpaint_row_kernel", "xray_inpaint_col_kernel", "xray_inpaint_list_kernel",
           "xray_inpaint_fill_kernel", "xray_inpaint_blend_kernel", "xray_parent_kernel")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100_000_000)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--distances", default="2,8,32")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "xray_inpaint_bench.json"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    ctx = pcv.Context(0)
    x, y, z, rgb = make_cloud(torch, args.points, seed=1, device=dev)
    tree = ctx.build(0.001, None, x, y, z, rgb)
    del x, y, z, rgb
    torch.cuda.empty_cache()
    leaf_ms = []
    for step in range(args.steps + 1):  # the first is a warm-up
        ctx.synchronize()
        t0 = time.perf_counter()
        xt = tree.xray_tiles(TILE, PIXEL, "xray", background="transparent")
        if step:
            leaf_ms.append((time.perf_counter() - t0) * 1e3)
        if step < args.steps:
            xt.free()
    ctx.set_profiling(True)
    runs = []
    for d in (int(v) for v in args.distances.split(",")):
        walls, kms, info = [], [], None
        for step in range(args.steps + 1):
            ctx.synchronize()
            ctx.reset_kernel_stats()
            t0 = time.perf_counter()
            out = xt.inpaint(d)
            wall = (time.perf_counter() - t0) * 1e3
            st = ctx.kernel_stats()
            if step:
                walls.append(wall)
                kms.append({k: st[k][1] for k in KERNELS})
                launches = {k: int(st[k][0]) for k in KERNELS}
            info = {k: int(v.sum()) for k, v in out.inpaint_info().items()}
            out.free()
        runs.append({"inpaint_distance_px": d, "inpaint_wall_ms": round(float(np.median(walls)), 3),
                     "inpaint_wall_ms_all": [round(w, 3) for w in walls],
                     "kernel_ms": {k: round(float(np.median([m[k] for m in kms])), 4) for k in KERNELS}, "kernel_launches": launches,
                     **info})
    ctx.set_profiling(False)
    res = {"tool": "tools/xray_inpaint_bench.py", "build_hash": build_hash(), "device": torch.cuda.get_device_name(0),
           "cloud": f"config 2: {args.points} Gaussian-cluster points (bench.make_cloud, seed 1), resolution 0.001",
           "tile_size_px": TILE, "pixel_size_m": PIXEL, "strategy": "xray", "background": "transparent",
           "deepest_level": xt.deepest_level, "leaf_tiles_created": xt.num_created,
           "leaf_build_wall_ms": round(float(np.median(leaf_ms)), 3), "leaf_build_wall_ms_all": [round(w, 3) for w in leaf_ms],
           "work_bytes_per_enlarged_tile": 44 * TILE * TILE, "runs": runs}
    xt.free()
    tree.free()
    print(json.dumps(res))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
