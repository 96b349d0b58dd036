#!/usr/bin/env python
"""Polygon point queries measured (GPU box). Two clouds, one after the other in one process, each built once:

  xy frame   the config-2 cloud (100 M Gaussian-cluster points, bench.py's generator and seed) and the 64 x 64 grid of
             tools/query_batch_bench.py: per tile (a) an octagon inscribed in the tile (8 edges) and (b) a 256-edge outline of the
             same radius, against (y) the tiles' bounding Aabbs, the yardstick, over the same tree in the same process;
  web-mercator  the 100 M-point ECEF tree of tools/wmr_query_bench.py and 1 000 web-mercator octagons under it, against their
             bounding web_mercator_rect batch.

Per leg, medians of `--rounds` alternating rounds after a warm-up: wall time of pcv_query_batch_run, the walk's time (node
lists), the flags' time, candidates per kept point, and the flag pass's f64 operations — 6 per candidate and edge: a subtraction,
a product, a sum and three comparisons — over its time, against the f64 issue roof (CUs x clock x 64 lanes). No time is promised.

usage: python tools/polygon_query_bench.py [--points N] [--tiles T] [--rounds R] [--octagons K] [--out FILE]"""
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

STAGES = ("batch_nodes_kernel", "batch_chunks_kernel", "batch_flags_kernel", "batch_scan_kernel")
OPS_PER_EDGE = 6


def run(ctx, tree, shapes):
    ctx.reset_kernel_stats()
    t0 = time.perf_counter()
    b = tree.query_batch(shapes)
    wall = (time.perf_counter() - t0) * 1e3
    st = ctx.kernel_stats()
    return wall, {k.replace("_kernel", ""): st[k][1] for k in STAGES if k in st and st[k][0]}, b


def gon(n, cx, cy, rx, ry):
    a = 2.0 * np.pi * (np.arange(n) + 0.5) / n
    return np.stack([cx + rx * np.cos(a), cy + ry * np.sin(a)], axis=1)


def measure(ctx, tree, legs, edges, rounds, roof):
    npts = np.array([tree.node(i).num_points for i in range(tree.num_nodes)], dtype=np.int64)
    for s in legs.values():  # warm-up
        run(ctx, tree, s)[2].free()
    samples, info = {k: [] for k in legs}, {}
    for _ in range(rounds):
        for name, s in legs.items():  # alternating
            wall, split, b = run(ctx, tree, s)
            samples[name].append(dict(split, wall=wall))
            if name not in info:
                _, nodes, _ = b.segments()
                info[name] = dict(shapes=s.count, segments=b.num_segments, kept_points=b.num_points, candidate_points=int(npts[nodes].sum()))
            b.free()
    rec = {}
    for name, rows in samples.items():
        med = {k: round(float(np.median([r[k] for r in rows])), 4) for k in rows[0]}
        cand = info[name]["candidate_points"]
        rec[name] = dict(info[name], median_ms=med, walk_ms=med.get("batch_nodes"), flags_ms=med.get("batch_flags"),
                         candidates_per_kept_point=round(cand / max(1, info[name]["kept_points"]), 3))
        if edges.get(name):
            ops = OPS_PER_EDGE * edges[name] * cand
            rate = ops / (med["batch_flags"] * 1e-3)
            rec[name].update(edges=edges[name], flag_f64_ops=ops, flag_f64_ops_per_s=round(rate, 1), share_of_f64_issue_roof=round(rate / roof, 4))
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100_000_000)
    ap.add_argument("--resolution", type=float, default=0.001)
    ap.add_argument("--tiles", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--octagons", type=int, default=1000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "polygon_query_bench.json"))
    args = ap.parse_args()

    dev = torch.device("cuda", 0)
    prop = torch.cuda.get_device_properties(0)
    clock_hz = float(getattr(prop, "clock_rate", 2_400_000)) * 1e3
    roof = prop.multi_processor_count * clock_hz * 64.0
    ctx = pcv.Context(0)
    ctx.set_profiling(True)

    # ---- xy frame ----
    x, y, z, rgb = make_cloud(torch, args.points, seed=1, device=dev)
    tree = ctx.build(args.resolution, None, x, y, z, rgb)
    del x, y, z, rgb
    torch.cuda.empty_cache()
    meta = tree.meta()
    bmin, bmax = np.asarray(meta["bbox_min"]), np.asarray(meta["bbox_max"])
    T = args.tiles
    w, h = (bmax[0] - bmin[0]) / T, (bmax[1] - bmin[1]) / T
    boxes, octagons, outlines = [], [], []
    for j in range(T):
        for i in range(T):
            lo = [bmin[0] + w * i, bmin[1] + h * j, bmin[2]]
            hi = [bmin[0] + w * (i + 1), bmin[1] + h * (j + 1), bmax[2]]
            boxes.append(("aabb", lo, hi))
            cx, cy = lo[0] + w / 2, lo[1] + h / 2
            octagons.append(("polygon", [gon(8, cx, cy, w / 2, h / 2)]))
            outlines.append(("polygon", [gon(256, cx, cy, w / 2, h / 2)]))
    legs = {"aabb_tiles": ctx.shapes(boxes), "octagons_8": ctx.shapes(octagons), "outlines_256": ctx.shapes(outlines)}
    xy = measure(ctx, tree, legs, {"octagons_8": 8, "outlines_256": 256}, args.rounds, roof)
    xy_nodes = tree.num_nodes
    for s in legs.values():
        s.free()
    tree.free()
    torch.cuda.empty_cache()

    # ---- web-mercator frame ----
    rot, ground = synthetic.ecef_from_local(37.407204, -122.147604)
    origin = ground + 1500.0 * rot[:, 2] - 500.0
    x, y, z, rgb = make_cloud(torch, args.points, seed=1, device=dev, offset=tuple(float(c) for c in origin))
    tree = ctx.build(args.resolution, None, x, y, z, rgb)
    del x, y, z, rgb
    torch.cuda.empty_cache()
    meta = tree.meta()
    bmin, bmax = np.asarray(meta["bbox_min"]), np.asarray(meta["bbox_max"])
    cs = np.array([[(bmax if (c >> k) & 1 else bmin)[k] for k in range(3)] for c in range(8)])
    u, v = pcv.wmr_project(cs[:, 0], cs[:, 1], cs[:, 2])
    side = max(1, int(round(args.octagons ** 0.5)))
    du, dv = (u.max() - u.min()) / side, (v.max() - v.min()) / side
    wm, rects = [], []
    for k in range(args.octagons):
        i, j = k % side, k // side
        ring = gon(8, u.min() + du * (i + 0.5), v.min() + dv * (j + 0.5), du / 2, dv / 2)
        wm.append(("polygon_web_mercator", [ring]))
        rects.append(("web_mercator_rect", ring.min(axis=0), ring.max(axis=0)))
    legs = {"web_mercator_rects": ctx.shapes(rects), "web_mercator_octagons_8": ctx.shapes(wm)}
    web = measure(ctx, tree, legs, {"web_mercator_octagons_8": 8}, args.rounds, roof)
    web_nodes = tree.num_nodes

    out = {"tool": "tools/polygon_query_bench.py", "build_hash": build_hash(), "device": torch.cuda.get_device_name(0),
           "rounds": args.rounds, "f64_issue_roof_ops_per_s": roof, "f64_ops_per_candidate_and_edge": OPS_PER_EDGE,
           "xy": {"cloud": f"config 2: {args.points} Gaussian-cluster points (bench.make_cloud, seed 1), resolution {args.resolution}",
                  "nodes": xy_nodes, "grid": f"{T} x {T}", "legs": xy},
           "web_mercator": {"cloud": f"{args.points} Gaussian-cluster points in a 1 000 m cube 1.5 km above 37.4 N 122.1 W, ECEF",
                            "nodes": web_nodes, "polygons": args.octagons, "legs": web}}
    print(json.dumps(out))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    for s in legs.values():
        s.free()
    tree.free()
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
