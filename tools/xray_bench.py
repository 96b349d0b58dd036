#!/usr/bin/env python
"""xray leaf tiles measured (GPU box): the config-2 cloud (100 M Gaussian-cluster points, bench.py's generator and seed) built
once, then the whole leaf level of build_xray_quadtree with tile_size_px = 256 and pixel_size_m = 0.1 (deepest level 6, the
4 096 tiles of query_batch_bench.py's case (c)) for each strategy: median wall ms of OctreeResult.xray_tiles (query batch +
raster, images left on the device), kernel ms per kernel, created tiles, drawn points, points/s, and the raster passes' bytes
per kept point against the 8 TB/s HBM peak.

Comparator: the per-tile loop (query_points of one tile + the numpy rasteriser of tests/xray_oracle.py) on a sample of tiles,
extrapolated to the leaf level and labelled as such. Parity: on a 10 M-point cloud of the same generator, a digest of every
tile's bytes against the numpy oracle (xray strategy, exact). Prints one JSON line and writes it to --out.

usage: python tools/xray_bench.py [--points N] [--parity-points N] [--steps K] [--loop-tiles T] [--out FILE]"""
import argparse
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import oracle_lib as O  # noqa: E402
import point_cloud_viewer_amd as pcv  # noqa: E402
import xray_oracle as X  # noqa: E402
from bench import build_hash, make_cloud  # noqa: E402

HBM_PEAK = 8.0e12
TILE, PIXEL = 256, 0.1
RASTER = ("xray_bin_kernel", "xray_scatter_kernel", "xray_accum_kernel")
STRATEGIES = {"xray": "xray", "colored": "colored", "height_stddev_jet": ("height_stddev", 0.5, "jet")}


def build(ctx, n, dev):
    x, y, z, rgb = make_cloud(torch, n, seed=1, device=dev)
    tree = ctx.build(0.001, None, x, y, z, rgb)
    del x, y, z, rgb
    torch.cuda.empty_cache()
    return tree


def raster_bytes(tree, xt, strategy):
    """Bytes the three raster passes move: per kept point the node bytes and flag twice (bin, scatter), colour once
    (scatter, colored), the record written and read (8 B; 16 B with z); the images written once."""
    bpc = {1: 1, 2: 2, 3: 4, 4: 8}
    kept = int(xt.kept.sum())
    m = tree.num_nodes
    npts = sum(tree.node(i).num_points for i in range(m))
    mean_pos = sum(tree.node(i).num_points * 3 * bpc[tree.node(i).encoding] for i in range(m)) / max(npts, 1)
    rec = 16 if strategy != "xray" and strategy != "colored" else 8
    per_point = 2 * (mean_pos + 1) + (3 if strategy == "colored" else 0) + 2 * rec
    return per_point, per_point * kept + 4 * TILE * TILE * xt.num_created


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100_000_000)
    ap.add_argument("--parity-points", type=int, default=10_000_000)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--loop-tiles", type=int, default=32)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08_xray_bench.json"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    ctx = pcv.Context(0)
    tree = build(ctx, args.points, dev)
    ctx.set_profiling(True)
    recs = {}
    for label, strat in STRATEGIES.items():
        walls, st = [], None
        for step in range(args.steps + 1):  # the first is a warm-up
            ctx.reset_kernel_stats()
            t0 = time.perf_counter()
            xt = tree.xray_tiles(TILE, PIXEL, strat)
            wall = (time.perf_counter() - t0) * 1e3
            if step:
                walls.append(wall)
                st = ctx.kernel_stats()
            if step < args.steps:
                xt.free()
        kms = {k.replace("_kernel", ""): round(v[1], 3) for k, v in st.items() if v[0]}
        raster_ms = sum(st[k][1] for k in RASTER)
        per_point, total = raster_bytes(tree, xt, strat)
        drawn = int(xt.drawn.sum())
        wall = float(np.median(walls))
        recs[label] = dict(wall_ms=round(wall, 2), kernel_ms=kms, kernel_ms_total=round(sum(v[1] for v in st.values()), 3),
                           raster_ms=round(raster_ms, 3), leaf_tiles=len(xt.leaf_ids), deepest_level=xt.deepest_level,
                           created_tiles=xt.num_created, points_kept=int(xt.kept.sum()), points_drawn=drawn,
                           points_per_s_wall=round(drawn / (wall * 1e-3), 1),
                           raster_bytes_per_kept_point=round(per_point, 2),
                           raster_share_of_hbm_peak=round(total / (raster_ms * 1e-3) / HBM_PEAK, 3))
        if label == "xray":
            xray_tiles = xt
        else:
            xt.free()
    # comparator: the per-tile loop on a sample of tiles, extrapolated
    meta = tree.meta()
    geo = pcv.xray_leaf_tiles(TILE, PIXEL, meta["bbox_min"], meta["bbox_max"])
    sample = np.linspace(0, len(geo["leaf_ids"]) - 1, args.loop_tiles).astype(int)
    shapes = ctx.shapes([("aabb", b[:3], b[3:]) for b in geo["tile_bbox"][sample]])
    ctx.set_profiling(False)
    t0 = time.perf_counter()
    for k in range(len(sample)):
        q = tree.query_points(shapes, k)
        if q["count"]:
            b = geo["tile_bbox"][sample[k]]
            X.tile_image(q["x"], q["y"], q["z"], q["rgb"].reshape(-1, 3), b[:3], b[3:], TILE, "xray")
    loop_ms = (time.perf_counter() - t0) * 1e3 * len(geo["leaf_ids"]) / len(sample)
    xray_tiles.free()
    tree.free()
    torch.cuda.empty_cache()
    # parity on a smaller cloud of the same generator: the numpy oracle over the octree's own node bytes
    small = build(ctx, args.parity_points, dev)
    xt = small.xray_tiles(TILE, PIXEL, "xray")
    got = hashlib.sha256()
    imgs = xt.images()
    for i, n in enumerate(xt.created_ids):
        got.update(n.encode() + imgs[i].tobytes())
    nodes = small.to_dict()
    meta = small.meta()
    tp = X.TreePoints(nodes, lambda name: (nodes[name]["cube_min"], nodes[name]["cube_edge"]), meta["bbox_min"], meta["bbox_max"])
    want, _ = X.xray_tiles(tp, TILE, PIXEL, "xray")
    ref = hashlib.sha256()
    for n in (n for n in xt.leaf_ids if n in want):
        ref.update(n.encode() + want[n][0].tobytes())
    parity = got.hexdigest() == ref.hexdigest() and list(want) != [] and set(want) == set(xt.created_ids)
    out = {"tool": "tools/xray_bench.py", "build_hash": build_hash(), "device": torch.cuda.get_device_name(0),
           "cloud": f"config 2: {args.points} Gaussian-cluster points (bench.make_cloud, seed 1), resolution 0.001",
           "tile_size_px": TILE, "pixel_size_m": PIXEL, "strategies": recs,
           "per_tile_loop": {"label": f"EXTRAPOLATED from {len(sample)} tiles: query_points + numpy raster per tile",
                             "wall_ms_extrapolated": round(loop_ms, 1)},
           "xray_vs_loop_wall": round(loop_ms / recs["xray"]["wall_ms"], 1),
           "parity": {"points": args.parity_points, "created_tiles": xt.num_created, "digest": got.hexdigest(),
                      "oracle_digest": ref.hexdigest(), "match": bool(parity)}}
    xt.free()
    small.free()
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    ctx.close()
    return 0 if parity else 1


if __name__ == "__main__":
    sys.exit(main())
