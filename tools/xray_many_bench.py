#!/usr/bin/env python
"""xray over several octrees measured (GPU box): the config-2 cloud (100 M Gaussian-cluster points, bench.py's generator
and seed) built once as one octree and once as K = 4 octrees of 25 M points, split by point index so that their boxes
nearly coincide. For each, the whole xray quadtree at tile_size_px = 256 and pixel_size_m = 0.1 (xray strategy) as
build_xray_quadtree with one or with four point_cloud_locations: K = 1 through OctreeResult.xray_tiles (pcv_xray_run),
K = 4 through Context.xray_tiles (pcv_xray_run_many). Reports median wall ms of the leaves and of the parents, kernel ms
and launch counts per kernel (pcv_ctx_kernel_stats), created tiles, kept points, and the octrees' nodes and mean encoded
bytes per position. Prints one JSON line and writes it to --out.

usage: python tools/xray_many_bench.py [--points N] [--trees K] [--steps S] [--out FILE]"""
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
RASTER = ("xray_bin_kernel", "xray_scatter_kernel", "xray_accum_kernel")


def measure(ctx, run, steps):
    """median wall ms of the leaves (run()) and of the parents (build_parents), and the last step's kernel stats of each"""
    leaves, parents, st_leaves, st_parents = [], [], None, None
    for step in range(steps + 1):  # the first is a warm-up
        ctx.reset_kernel_stats()
        t0 = time.perf_counter()
        xt = run()
        t1 = time.perf_counter()
        s_l = ctx.kernel_stats()
        ctx.reset_kernel_stats()
        t2 = time.perf_counter()
        xt.build_parents()
        t3 = time.perf_counter()
        s_p = ctx.kernel_stats()
        if step:
            leaves.append((t1 - t0) * 1e3)
            parents.append((t3 - t2) * 1e3)
            st_leaves, st_parents = s_l, s_p
        info = dict(created_tiles=xt.num_created, points_kept=int(xt.kept.sum()), points_drawn=int(xt.drawn.sum()),
                    deepest_level=xt.deepest_level, nodes=len(xt.node_ids))
        xt.free()

    def table(st):
        return {k.replace("_kernel", ""): dict(launches=int(v[0]), ms=round(v[1], 3)) for k, v in st.items() if v[0]}
    return dict(leaves_wall_ms=round(float(np.median(leaves)), 2), parents_wall_ms=round(float(np.median(parents)), 2),
                leaves_kernel_ms_total=round(sum(v[1] for v in st_leaves.values()), 3),
                raster_ms=round(sum(st_leaves[k][1] for k in RASTER if k in st_leaves), 3),
                raster_launches={k.replace("_kernel", ""): int(st_leaves[k][0]) for k in RASTER if k in st_leaves},
                leaves_kernels=table(st_leaves), parents_kernels=table(st_parents), **info)


def position_bytes(trees):
    """(nodes, mean bytes of an encoded position per point) over the octrees: what xray_bin and xray_scatter decode"""
    bpc = {1: 1, 2: 2, 3: 4, 4: 8}
    nodes = pts = nbytes = 0
    for t in trees:
        for i in range(t.num_nodes):
            nd = t.node(i)
            nodes += 1
            pts += nd.num_points
            nbytes += nd.num_points * 3 * bpc[nd.encoding]
    return nodes, round(nbytes / max(pts, 1), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100_000_000)
    ap.add_argument("--trees", type=int, default=4)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "xray_many_bench.json"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    ctx = pcv.Context(0)
    x, y, z, rgb = make_cloud(torch, args.points, seed=1, device=dev)
    one = ctx.build(0.001, None, x, y, z, rgb)
    cut = [args.points * k // args.trees for k in range(args.trees + 1)]
    parts = [ctx.build(0.001, None, x[cut[k]:cut[k + 1]], y[cut[k]:cut[k + 1]], z[cut[k]:cut[k + 1]], rgb[cut[k]:cut[k + 1]])
             for k in range(args.trees)]
    del x, y, z, rgb
    torch.cuda.empty_cache()
    ctx.set_profiling(True)
    single = measure(ctx, lambda: one.xray_tiles(TILE, PIXEL, "xray"), args.steps)
    many = measure(ctx, lambda: ctx.xray_tiles(parts, TILE, PIXEL, "xray"), args.steps)
    ctx.set_profiling(False)
    boxes = [t.meta() for t in [one] + parts]
    single["octree_nodes"], single["position_bytes_per_point"] = position_bytes([one])
    many["octree_nodes"], many["position_bytes_per_point"] = position_bytes(parts)
    out = {"tool": "tools/xray_many_bench.py", "build_hash": build_hash(), "device": torch.cuda.get_device_name(0),
           "cloud": f"config 2: {args.points} Gaussian-cluster points (bench.make_cloud, seed 1), resolution 0.001",
           "tile_size_px": TILE, "pixel_size_m": PIXEL, "strategy": "xray",
           "k1": dict(octrees=1, **single),
           f"k{args.trees}": dict(octrees=args.trees, split="by point index, equal parts", **many),
           "bbox": {"k1": [list(boxes[0]["bbox_min"]), list(boxes[0]["bbox_max"])],
                    "parts": [[list(b["bbox_min"]), list(b["bbox_max"])] for b in boxes[1:]]}}
    for t in [one] + parts:
        t.free()
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
