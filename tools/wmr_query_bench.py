#!/usr/bin/env python
"""Map-tile point queries measured (GPU box): Gaussian clusters (bench.py's generator and seed) moved to an ECEF origin — the
cube's centre 1.5 km above the ground at 37.4 N 122.1 W, so every point lies inside the rectangles' polyhedra —, built once, then,
alternating in one process, `--pairs` times each:
  (w) one pcv_query_batch_run over the slippy-map tiles of zoom level --zoom under the cloud (PCV_SHAPE_WEB_MERCATOR_RECT),
  (a) the same number of AABB tiles over the same octree (x and y of the box split evenly, z whole),
  (r) 1 000 of the map tiles alone, for the cost of their node lists (the rectangles' lists come from the one-lane-per-shape flat
      kernel, not from the wave-per-shape walk: DESIGN §4).
Per leg: wall time of the run (ends in a stream synchronise), kernel time per stage from ctx.kernel_stats(), candidate points,
the flags pass's bytes (encoded positions of every (shape, node) pair + one flag byte per candidate) and TB/s. Medians over the
pairs. The static f64 operation count of the chain comes from profiles/wmr_isa_count.json (tools/wmr_isa_count.py) when present.
Every kept count of the map tiles is checked against pcv_wmr_contains on the host for --check tiles.

usage: python tools/wmr_query_bench.py [--points N] [--zoom Z] [--pairs P] [--check C] [--out FILE]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import point_cloud_viewer_amd as pcv  # noqa: E402
from bench import build_hash, make_cloud  # noqa: E402
from point_cloud_viewer_amd import synthetic  # noqa: E402

STAGES = ("batch_nodes_kernel", "batch_chunks_kernel", "batch_flags_kernel", "batch_scan_kernel")


def run(ctx, tree, shapes):
    ctx.reset_kernel_stats()
    t0 = time.perf_counter()
    b = tree.query_batch(shapes)
    wall = (time.perf_counter() - t0) * 1e3
    st = ctx.kernel_stats()
    return wall, {k.replace("_kernel", ""): st[k][1] for k in STAGES if st[k][0]}, b


def candidates(npts, stride, batch):
    _, nodes, _ = batch.segments()
    cand = int(npts[nodes].sum())
    return cand, int((npts[nodes] * stride[nodes]).sum()) + cand


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100_000_000)
    ap.add_argument("--resolution", type=float, default=0.001)
    ap.add_argument("--zoom", type=int, default=20)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--check", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wmr_query_bench.json"))
    args = ap.parse_args()

    dev = torch.device("cuda", 0)
    rot, ground = synthetic.ecef_from_local(37.407204, -122.147604)
    origin = ground + 1500.0 * rot[:, 2] - 500.0  # make_cloud's centres fill a 1 000 m cube from its offset
    x, y, z, rgb = make_cloud(torch, args.points, seed=1, device=dev, offset=tuple(float(c) for c in origin))
    ctx = pcv.Context(0)
    tree = ctx.build(args.resolution, None, x, y, z, rgb)
    del x, y, z, rgb
    torch.cuda.empty_cache()
    meta = tree.meta()
    bmin, bmax = np.asarray(meta["bbox_min"]), np.asarray(meta["bbox_max"])
    m = tree.num_nodes
    npts = np.array([tree.node(i).num_points for i in range(m)], dtype=np.int64)
    stride = np.array([3 * {1: 1, 2: 2, 3: 4, 4: 8}[tree.node(i).encoding] for i in range(m)], dtype=np.int64)

    # the map tiles under the projection of the box's corners
    cs = np.array([[(bmax if (c >> k) & 1 else bmin)[k] for k in range(3)] for c in range(8)])
    u, v = pcv.wmr_project(cs[:, 0], cs[:, 1], cs[:, 2])
    n = float(1 << args.zoom)
    tx0, tx1, ty0, ty1 = int(u.min() * n), int(u.max() * n), int(v.min() * n), int(v.max() * n)
    rects = []
    for ty in range(ty0, ty1 + 1):
        for tx in range(tx0, tx1 + 1):
            r = pcv.web_mercator_rect_from_zoomed((256.0 * tx, 256.0 * ty), (256.0 * (tx + 1), 256.0 * (ty + 1)), args.zoom)
            assert r is not None
            rects.append(r)
    T = len(rects)
    side = max(1, int(round(T ** 0.5)))
    tiles = []
    for k in range(T):  # the same number of AABB tiles: a side x ceil(T / side) grid, cut off at T
        i, j, rows = k % side, k // side, -(-T // side)
        lo = [bmin[0] + (bmax[0] - bmin[0]) * i / side, bmin[1] + (bmax[1] - bmin[1]) * j / rows, bmin[2]]
        hi = [bmin[0] + (bmax[0] - bmin[0]) * (i + 1) / side, bmin[1] + (bmax[1] - bmin[1]) * (j + 1) / rows, bmax[2]]
        tiles.append(("aabb", lo, hi))
    legs = {"wmr": ctx.shapes(rects), "aabb": ctx.shapes(tiles),
            "wmr_1000_node_lists": ctx.shapes([rects[k % T] for k in range(1000)])}
    ctx.set_profiling(True)
    for s in legs.values():  # warm-up
        run(ctx, tree, s)[2].free()
    samples = {k: [] for k in legs}
    info = {}
    for _ in range(args.pairs):
        for name, s in legs.items():  # alternating
            wall, split, b = run(ctx, tree, s)
            samples[name].append(dict(split, wall=wall))
            if name not in info:
                cand, nbytes = candidates(npts, stride, b)
                info[name] = dict(shapes=s.count, segments=b.num_segments, kept_points=b.num_points, candidate_points=cand,
                                  flags_pass_bytes=nbytes)
                if name == "wmr":  # kept counts against the host chain
                    first, nodes, off = b.segments()
                    ok = True
                    for t in range(0, T, max(1, T // max(1, args.check)))[:args.check]:
                        got = tree.query_points(legs["wmr"], t, capacity=1 << 23)
                        ok = ok and got["count"] == int(off[first[t + 1]] - off[first[t]])
                        if got["count"] <= (1 << 23):  # every returned point is inside on the host too
                            ok = ok and int(pcv.wmr_contains(rects[t], got["x"], got["y"], got["z"]).sum()) == got["count"]
                    info[name]["checked_against_host_chain"] = bool(ok)
            b.free()
    rec = {}
    for name, rows in samples.items():
        med = {k: round(float(np.median([r[k] for r in rows])), 4) for k in rows[0]}
        lo_hi = {k: [round(min(r[k] for r in rows), 4), round(max(r[k] for r in rows), 4)] for k in ("wall", "batch_nodes", "batch_flags")}
        rec[name] = dict(info[name], median_ms=med, min_max_ms=lo_hi,
                         flags_pass_tb_s=round(info[name]["flags_pass_bytes"] / (med["batch_flags"] * 1e-3) / 1e12, 4),
                         flags_ns_per_candidate_point=round(med["batch_flags"] * 1e6 / max(1, info[name]["candidate_points"]), 5))
    isa = None
    isa_path = os.path.join(ROOT, "profiles", "wmr_isa_count.json")
    if os.path.exists(isa_path):
        isa = json.load(open(isa_path))
        pts_per_s = rec["wmr"]["candidate_points"] / (rec["wmr"]["median_ms"]["batch_flags"] * 1e-3)
        rec["wmr"]["f64_instructions_per_candidate_point_static"] = isa["f64_instructions_per_point"]
        rec["wmr"]["f64_instructions_per_second"] = round(pts_per_s * isa["f64_instructions_per_point"], 0)
    out = {"tool": "tools/wmr_query_bench.py", "build_hash": build_hash(), "device": torch.cuda.get_device_name(0),
           "cloud": f"{args.points} Gaussian-cluster points (bench.make_cloud, seed 1) in a 1 000 m cube 1.5 km above 37.4 N 122.1 W, "
                    f"ECEF, resolution {args.resolution}", "nodes": m, "zoom": args.zoom, "map_tiles": T, "pairs": args.pairs,
           "legs": rec,
           "wmr_vs_aabb": {"flags_ms": round(rec["wmr"]["median_ms"]["batch_flags"] / rec["aabb"]["median_ms"]["batch_flags"], 2),
                           "flags_ns_per_candidate": round(rec["wmr"]["flags_ns_per_candidate_point"] /
                                                           rec["aabb"]["flags_ns_per_candidate_point"], 2),
                           "nodes_ms": round(rec["wmr"]["median_ms"]["batch_nodes"] / rec["aabb"]["median_ms"]["batch_nodes"], 2)},
           "fast_path": "none: every candidate point takes the full chain (share 1.0)",
           "node_lists_ms_per_1000_rectangles": rec["wmr_1000_node_lists"]["median_ms"]["batch_nodes"]}
    print(json.dumps(out))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    tree.free()
    ctx.close()
    return 0 if rec["wmr"].get("checked_against_host_chain", False) else 1


if __name__ == "__main__":
    sys.exit(main())
