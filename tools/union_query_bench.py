#!/usr/bin/env python
"""Cell-union point queries over an octree measured (GPU box): the 100 M-point ECEF tree of tools/wmr_query_bench.py (Gaussian
clusters, bench.py's generator and seed, in a 1 000 m cube 1.5 km above 37.4 N 122.1 W), built once, then, alternating in one
process, `--pairs` times each, one pcv_query_batch_run over
  (u) the level-20 S2 cells under the cloud, one union per cell (PCV_SHAPE_S2_CELL_UNION),
  (p) the same cells as [c, c.next()] pairs (the reference's get_cell_union_query),
  (a) the same number of AABB tiles over the same octree and (w) the zoom-20 map tiles under it, as yardsticks.
Per leg: wall time of the run, kernel time per stage from ctx.kernel_stats() (node lists, flags), candidate points and flag time
per candidate point. The rect table of the tree (union_node_rects_kernel) is built by the first union query: its time is read
off that run. Kept counts of --check unions are compared with pcv_s2_union_contains on the points query_points returns.

usage: python tools/union_query_bench.py [--points N] [--level L] [--pairs P] [--check C] [--out FILE]"""
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
from point_cloud_viewer_amd import synthetic  # noqa: E402

STAGES = ("batch_nodes_kernel", "batch_chunks_kernel", "batch_flags_kernel", "batch_scan_kernel", "union_node_rects_kernel")


def run(ctx, tree, shapes):
    ctx.reset_kernel_stats()
    t0 = time.perf_counter()
    b = tree.query_batch(shapes)
    wall = (time.perf_counter() - t0) * 1e3
    st = ctx.kernel_stats()
    return wall, {k.replace("_kernel", ""): st[k][1] for k in STAGES if k in st and st[k][0]}, b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100_000_000)
    ap.add_argument("--resolution", type=float, default=0.001)
    ap.add_argument("--level", type=int, default=20)
    ap.add_argument("--zoom", type=int, default=20)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--check", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "union_query_bench.json"))
    args = ap.parse_args()

    dev = torch.device("cuda", 0)
    rot, ground = synthetic.ecef_from_local(37.407204, -122.147604)
    origin = ground + 1500.0 * rot[:, 2] - 500.0
    x, y, z, rgb = make_cloud(torch, args.points, seed=1, device=dev, offset=tuple(float(c) for c in origin))
    ctx = pcv.Context(0)
    # the level-20 cells under the cloud: those of every 97th point
    ids = ctx.s2_cell_ids(x[::97].contiguous(), y[::97].contiguous(), z[::97].contiguous(), level=args.level)
    cells = np.unique(ids.cpu().numpy().view(np.uint64))
    tree = ctx.build(args.resolution, None, x, y, z, rgb)
    del x, y, z, rgb, ids
    torch.cuda.empty_cache()
    meta = tree.meta()
    bmin, bmax = np.asarray(meta["bbox_min"]), np.asarray(meta["bbox_max"])
    m = tree.num_nodes
    npts = np.array([tree.node(i).num_points for i in range(m)], dtype=np.int64)
    T = int(cells.size)
    nxt = cells + ((cells & (~cells + np.uint64(1))) << np.uint64(1))  # CellID::next: id + 2 * lsb (wraps past the last face)
    singles = [("s2_cells", [int(c)]) for c in cells]
    pairs = [("s2_cells", sorted([int(c), int(n)])) for c, n in zip(cells, nxt) if int(n) != 0]
    side = max(1, int(round(T ** 0.5)))
    tiles = []
    for k in range(T):
        i, j, rows = k % side, k // side, -(-T // side)
        lo = [bmin[0] + (bmax[0] - bmin[0]) * i / side, bmin[1] + (bmax[1] - bmin[1]) * j / rows, bmin[2]]
        hi = [bmin[0] + (bmax[0] - bmin[0]) * (i + 1) / side, bmin[1] + (bmax[1] - bmin[1]) * (j + 1) / rows, bmax[2]]
        tiles.append(("aabb", lo, hi))
    cs = np.array([[(bmax if (c >> k) & 1 else bmin)[k] for k in range(3)] for c in range(8)])
    u, v = pcv.wmr_project(cs[:, 0], cs[:, 1], cs[:, 2])
    n = float(1 << args.zoom)
    rects = []
    for ty in range(int(v.min() * n), int(v.max() * n) + 1):
        for tx in range(int(u.min() * n), int(u.max() * n) + 1):
            rects.append(pcv.web_mercator_rect_from_zoomed((256.0 * tx, 256.0 * ty), (256.0 * (tx + 1), 256.0 * (ty + 1)), args.zoom))
    legs = {"union_single": ctx.shapes(singles), "union_pair": ctx.shapes(pairs), "aabb": ctx.shapes(tiles), "wmr": ctx.shapes(rects)}
    ctx.set_profiling(True)
    rect_table_ms = None
    for name, s in legs.items():  # warm-up; the first union run builds the tree's rect table
        _, split, b = run(ctx, tree, s)
        if rect_table_ms is None and "union_node_rects" in split:
            rect_table_ms = split["union_node_rects"]
        b.free()
    samples = {k: [] for k in legs}
    info = {}
    ok = True
    for _ in range(args.pairs):
        for name, s in legs.items():  # alternating
            wall, split, b = run(ctx, tree, s)
            samples[name].append(dict(split, wall=wall))
            if name not in info:
                first, nodes, off = b.segments()
                info[name] = dict(shapes=s.count, segments=b.num_segments, kept_points=b.num_points, candidate_points=int(npts[nodes].sum()))
                if name == "union_single":
                    for t in list(range(0, T, max(1, T // max(1, args.check))))[:args.check]:
                        got = tree.query_points(s, t, capacity=1 << 23)
                        ok = ok and got["count"] == int(off[first[t + 1]] - off[first[t]])
                        if got["count"] <= (1 << 23):
                            ok = ok and int(pcv.s2_union_contains(singles[t][1], got["x"], got["y"], got["z"]).sum()) == got["count"]
            b.free()
    rec = {}
    for name, rows in samples.items():
        med = {k: round(float(np.median([r[k] for r in rows])), 4) for k in rows[0]}
        rec[name] = dict(info[name], median_ms=med,
                         flags_ns_per_candidate_point=round(med["batch_flags"] * 1e6 / max(1, info[name]["candidate_points"]), 5))
    out = {"tool": "tools/union_query_bench.py", "build_hash": build_hash(), "device": torch.cuda.get_device_name(0),
           "cloud": f"{args.points} Gaussian-cluster points (bench.make_cloud, seed 1) in a 1 000 m cube 1.5 km above 37.4 N 122.1 W, "
                    f"ECEF, resolution {args.resolution}", "nodes": m, "level": args.level, "cells": T, "pairs": args.pairs,
           "rect_table_build_ms": rect_table_ms, "checked_against_host_chain": bool(ok), "legs": rec}
    print(json.dumps(out))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    tree.free()
    ctx.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
