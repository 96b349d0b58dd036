#!/usr/bin/env python
"""colored_with_intensity and binning measured (GPU box): the config-2 cloud (bench.make_cloud, seed 1) with the f32
intensity plane of bench.py's intensity leg (uniform in [0, 4096), seed 99), built once. The xray leaves at
tile_size_px = 256 and pixel_size_m = 0.1 for colored, colored_with_intensity (min 0, max 4096), and both with
binning=("intensity", 256), in the same process. Reports median wall ms of the leaves, kernel ms and launch counts per
kernel (pcv_ctx_kernel_stats), created tiles and kept points. Prints one JSON line and writes it to --out.

usage: python tools/xray_intensity_bench.py [--points N] [--steps S] [--out FILE]"""
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
CASES = {"colored": dict(strategy="colored"),
         "colored_with_intensity": dict(strategy="colored_with_intensity", min_intensity=0.0, max_intensity=4096.0),
         "colored_binned": dict(strategy="colored", binning=("intensity", 256.0)),
         "colored_with_intensity_binned": dict(strategy="colored_with_intensity", min_intensity=0.0, max_intensity=4096.0,
                                               binning=("intensity", 256.0))}


def measure(ctx, tree, kw, steps):
    wall, st = [], None
    for step in range(steps + 1):  # the first is a warm-up
        ctx.reset_kernel_stats()
        t0 = time.perf_counter()
        xt = tree.xray_tiles(TILE, PIXEL, **kw)
        t1 = time.perf_counter()
        if step:
            wall.append((t1 - t0) * 1e3)
            st = ctx.kernel_stats()
        info = dict(created_tiles=xt.num_created, points_kept=int(xt.kept.sum()), points_drawn=int(xt.drawn.sum()))
        xt.free()
    kernels = {k.replace("_kernel", ""): dict(launches=int(v[0]), ms=round(v[1], 3)) for k, v in st.items() if v[0]}
    return dict(leaves_wall_ms=round(float(np.median(wall)), 2), wall_ms_all=[round(w, 2) for w in wall],
                kernel_ms_total=round(sum(v[1] for v in st.values()), 3), kernels=kernels, **info)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100_000_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "xray_intensity_bench.json"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    ctx = pcv.Context(0)
    x, y, z, rgb = make_cloud(torch, args.points, seed=1, device=dev)
    g = torch.Generator(device=dev)
    g.manual_seed(99)
    inten = torch.rand(args.points, generator=g, device=dev, dtype=torch.float32) * 4096.0
    tree = ctx.build(0.001, None, x, y, z, rgb, inten)
    del x, y, z, rgb, inten
    torch.cuda.empty_cache()
    ctx.set_profiling(True)
    res = {name: measure(ctx, tree, kw, args.steps) for name, kw in CASES.items()}
    ctx.set_profiling(False)
    out = {"tool": "tools/xray_intensity_bench.py", "build_hash": build_hash(), "device": torch.cuda.get_device_name(0),
           "cloud": f"config 2: {args.points} Gaussian-cluster points (bench.make_cloud, seed 1) + f32 intensity U[0, 4096) "
                    "(seed 99), resolution 0.001", "tile_size_px": TILE, "pixel_size_m": PIXEL, "steps": args.steps, **res}
    tree.free()
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
