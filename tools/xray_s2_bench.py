#!/usr/bin/env python
"""xray leaf tiles over an S2 cell cloud measured against the same points as an octree (GPU box; there is no CPU fallback).

The cloud: 100 M Gaussian-cluster points (bench.make_cloud, seed 1, the 1000 m cube centred on the local origin) placed in
ECEF with synthetic.ecef_from_local(37.407204, -122.147604). It is split into S2 cells at level 20 (Context.s2_split) and
built as an octree (resolution 1 mm). With query_from_global into the local frame, 256 px tiles and tools/xray_bench.py's
pixel size (0.1 m), `xray` and `colored` are timed over the S2 cloud (pcv_xray_run_s2) and over the octree (pcv_xray_run):
one process, a warm-up of both, then the two alternating, `--steps` repeats each, a wall clock around calls that end in a
synchronise. Per leg: the wall times and their spread, the kernel_stats split of one profiled run, the candidates per kept
point, and the bytes the flags pass and the two bin passes read, computed from counts, with their bytes/s.

--octree-only times the octree leg alone: it runs on a library without pcv_xray_run_s2 too, which gives the octree leg's
baseline at the commit before the S2 path. --baseline FILE merges such a record into this run's JSON (both octree figures,
their spreads, and whether they are apart by more than those).

--attr is a leg of its own (no octree is built): the same cloud with an f32 intensity, an I64 `timestamp` extra (seven 30 s
slices and a jitter below the bin) and a U8 `ring` extra, `colored` four ways from one process, alternating: unbinned, binned
on intensity, binned on timestamp=30000000000 (pcv_xray_run_s2_ex: the scatter pass reads the column), and that with the filter
ring in [64, 191]. The record goes to profiles/xray_s2_attr_bench.json.

usage: python tools/xray_s2_bench.py [--points N] [--steps K] [--octree-only] [--attr] [--baseline FILE] [--out FILE]"""
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

TILE, PIXEL, LEVEL = 256, 0.1, 20
LAT, LNG = 37.407204, -122.147604
S2_KERNELS = ("s2_pair_kernel", "s2_flags_kernel", "batch_scan_kernel", "xray_bin_kernel", "xray_scatter_kernel", "xray_accum_kernel")
STRATEGIES = ("xray", "colored")


def quat_of(m):
    """Unit quaternion (i, j, k, w) of a rotation matrix with a positive trace or not (Shepperd's choice of the pivot)."""
    d = [m[0, 0], m[1, 1], m[2, 2]]
    t = d[0] + d[1] + d[2]
    if t > 0.0:
        s = 2.0 * np.sqrt(t + 1.0)
        q = [(m[2, 1] - m[1, 2]) / s, (m[0, 2] - m[2, 0]) / s, (m[1, 0] - m[0, 1]) / s, 0.25 * s]
    else:
        i = int(np.argmax(d))
        j, k = (i + 1) % 3, (i + 2) % 3
        s = 2.0 * np.sqrt(1.0 + d[i] - d[j] - d[k])
        q = [0.0, 0.0, 0.0, (m[k, j] - m[j, k]) / s]
        q[i], q[j], q[k] = 0.25 * s, (m[j, i] + m[i, j]) / s, (m[k, i] + m[i, k]) / s
    q = np.asarray(q, dtype=np.float64)
    return [float(v) for v in q / np.linalg.norm(q)]


def ecef_cloud(n, dev):
    """(x, y, z, rgb) device tensors in ECEF and query_from_global back into the local frame"""
    x, y, z, rgb = make_cloud(torch, n, seed=1, device=dev, offset=(-500.0, -500.0, -500.0))
    rot, centre = synthetic.ecef_from_local(LAT, LNG)
    r = torch.tensor(rot, dtype=torch.float64, device=dev)
    local = torch.stack([x, y, z])
    del x, y, z
    p = r @ local + torch.tensor(centre, dtype=torch.float64, device=dev)[:, None]
    del local
    iso = [float(v) for v in -(rot.T @ centre)] + quat_of(rot.T)
    return p[0].contiguous(), p[1].contiguous(), p[2].contiguous(), rgb, iso


def candidates_of(ctx, cloud, bbox_min, bbox_max, iso):
    """candidate points of the leaf tiles' S2 queries: the sizes of the cells each tile's shape lists (counts call, then the
    lists at the longest one's length)"""
    geo = pcv.xray_leaf_tiles(TILE, PIXEL, bbox_min, bbox_max, iso)
    obb = geo["query_obb"]
    shapes = ctx.shapes([("obb", o[0:3], o[3:7], o[7:10]) for o in obb])
    counts = np.zeros(shapes.count, dtype=np.uint32)
    ctx._check(ctx.lib.pcv_s2_cells_in_location(cloud.handle, shapes.handle, 0, None, None, 0, counts.ctypes.data, None))
    cap = int(counts.max())
    lists = np.zeros((shapes.count, max(cap, 1)), dtype=np.uint32)
    ctx._check(ctx.lib.pcv_s2_cells_in_location(cloud.handle, shapes.handle, 0, None, None, cap, counts.ctypes.data, lists.ctypes.data))
    sizes = cloud.cells[1].astype(np.int64)
    listed = np.arange(lists.shape[1])[None, :] < counts[:, None]
    shapes.free()
    return int(sizes[lists[listed]].sum()), int(counts.sum()), cap


def timed(ctx, run):
    t0 = time.perf_counter()
    xt = run()
    ctx.synchronize()
    return xt, (time.perf_counter() - t0) * 1e3


def stats(walls):
    w = np.asarray(walls)
    return dict(wall_ms=[round(float(v), 2) for v in w], wall_ms_median=round(float(np.median(w)), 2),
                wall_ms_spread=round(float(w.max() - w.min()), 2))


def s2_bytes(strategy, candidates, kept, drawn, ms):
    """bytes read, from counts: the flags pass reads 24 B of position per candidate; each bin pass reads 4 B of flag per
    candidate and 24 B of position per kept point, the scatter 3 B of colour per drawn point with `colored`"""
    flags = 24 * candidates
    count = 4 * candidates + 24 * kept
    scatter = count + (3 * drawn if strategy == "colored" else 0)
    rate = lambda b, k: round(b / (ms[k] * 1e-3), 1) if ms.get(k) else None  # noqa: E731
    return dict(flags_pass_bytes_read=flags, bin_pass_bytes_read=count, scatter_pass_bytes_read=scatter,
                flags_and_offsets_bytes_per_candidate=12,
                flags_pass_bytes_per_s=rate(flags, "s2_flags_kernel"), bin_pass_bytes_per_s=rate(count, "xray_bin_kernel"),
                scatter_pass_bytes_per_s=rate(scatter, "xray_scatter_kernel"))


ATTR_KERNELS = ("s2_flags_kernel", "s2_attr_filter_kernel", "batch_scan_kernel", "xray_bin_kernel", "xray_scatter_kernel", "xray_accum_kernel",
                "xray_sorted_kernel")


def attr_leg(args, ctx, dev):
    """`colored` over the S2 cloud: today's two forms against binning on an I64 extra, without and with a U8 filter"""
    x, y, z, rgb, iso = ecef_cloud(args.points, dev)
    i = torch.arange(args.points, dtype=torch.int64, device=dev)
    h = (i * 2654435761) % 1000003
    timestamp = ((h % 7) - 3) * 30000000000 + (i % 1000) * 1000000
    ring = (h % 256).to(torch.uint8)
    intensity = (h % 1009).to(torch.float32) * 0.25
    del i, h
    cloud = ctx.s2_split(dict(x=x, y=y, z=z, color=rgb, intensity=intensity, attributes={"timestamp": timestamp, "ring": ring}), LEVEL)
    del x, y, z, rgb, intensity, timestamp, ring
    torch.cuda.empty_cache()
    legs = {"colored": {}, "colored_binned_intensity": dict(binning=("intensity", 16.0)),
            "colored_binned_timestamp": dict(binning=("timestamp", 30000000000.0)),
            "colored_binned_timestamp_filter_ring": dict(binning=("timestamp", 30000000000.0), filter_intervals={"ring": (64, 191)})}
    run = lambda kw: cloud.xray_tiles(TILE, PIXEL, "colored", query_from_global=iso, **kw)  # noqa: E731
    out = {"tool": "tools/xray_s2_bench.py --attr", "build_hash": build_hash(), "device": torch.cuda.get_device_name(0),
           "cloud": f"{args.points} Gaussian-cluster points (bench.make_cloud, seed 1) placed with synthetic.ecef_from_local({LAT}, {LNG}); "
                    "f32 intensity, I64 timestamp, U8 ring",
           "tile_size_px": TILE, "pixel_size_m": PIXEL, "split_level": LEVEL, "steps": args.steps, "s2_cells": cloud.num_cells, "legs": {}}
    for kw in legs.values():  # the warm-up of all four
        run(kw).free()
    ctx.synchronize()
    walls = {name: [] for name in legs}
    for _ in range(args.steps):  # alternating
        for name, kw in legs.items():
            xt, ms = timed(ctx, lambda: run(kw))
            walls[name].append(ms)
            xt.free()
    for name, kw in legs.items():  # one profiled run per leg for the kernel split and the counts
        ctx.set_profiling(True)
        ctx.reset_kernel_stats()
        xt = run(kw)
        st = ctx.kernel_stats()
        ctx.set_profiling(False)
        kms = {k: round(v[1], 3) for k, v in st.items() if v[0]}
        out["legs"][name] = dict(stats(walls[name]), kernel_ms_split={k: kms.get(k) for k in ATTR_KERNELS}, kernel_ms=kms,
                                 kernel_launches={k: v[0] for k, v in st.items() if v[0]}, leaf_tiles=len(xt.leaf_ids),
                                 created_tiles=xt.num_created, points_kept=int(xt.kept.sum()), points_drawn=int(xt.drawn.sum()))
        xt.free()
    print(json.dumps(out))
    path = args.out if args.out != DEFAULT_OUT else os.path.join(ROOT, "profiles", "xray_s2_attr_bench.json")
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    ctx.close()
    return 0


DEFAULT_OUT = os.path.join(ROOT, "profiles", "xray_s2_bench.json")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100_000_000)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--octree-only", action="store_true")
    ap.add_argument("--baseline", default=None)
    ap.add_argument("--attr", action="store_true")
    ap.add_argument("--out", default=DEFAULT_OUT)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/xray_s2_bench.py needs a device: there is no CPU fallback")
    dev = torch.device("cuda", 0)
    ctx = pcv.Context(0)
    if args.attr:
        return attr_leg(args, ctx, dev)
    x, y, z, rgb, iso = ecef_cloud(args.points, dev)
    tree = ctx.build(0.001, None, x, y, z, rgb)
    cloud = None if args.octree_only else ctx.s2_split(dict(x=x, y=y, z=z, color=rgb), LEVEL)
    del x, y, z, rgb
    torch.cuda.empty_cache()
    legs = {"octree": lambda s: tree.xray_tiles(TILE, PIXEL, s, query_from_global=iso)}
    if cloud is not None:
        legs["s2"] = lambda s: cloud.xray_tiles(TILE, PIXEL, s, query_from_global=iso)
    out = {"tool": "tools/xray_s2_bench.py", "build_hash": build_hash(), "device": torch.cuda.get_device_name(0),
           "cloud": f"{args.points} Gaussian-cluster points (bench.make_cloud, seed 1) placed with synthetic.ecef_from_local({LAT}, {LNG})",
           "tile_size_px": TILE, "pixel_size_m": PIXEL, "split_level": LEVEL, "steps": args.steps, "octree_nodes": tree.num_nodes,
           "s2_cells": cloud.num_cells if cloud is not None else None, "legs": {}}
    for strategy in STRATEGIES:
        for name, run in legs.items():  # the warm-up of both
            run(strategy).free()
        ctx.synchronize()
        walls = {name: [] for name in legs}
        for _ in range(args.steps):  # alternating
            for name, run in legs.items():
                xt, ms = timed(ctx, lambda: run(strategy))
                walls[name].append(ms)
                xt.free()
        for name, run in legs.items():  # one profiled run per leg for the kernel split and the counts
            ctx.set_profiling(True)
            ctx.reset_kernel_stats()
            xt = run(strategy)
            st = ctx.kernel_stats()
            ctx.set_profiling(False)
            kms = {k: round(v[1], 3) for k, v in st.items() if v[0]}
            kept, drawn = int(xt.kept.sum()), int(xt.drawn.sum())
            rec = dict(stats(walls[name]), kernel_ms=kms, kernel_launches={k: v[0] for k, v in st.items() if v[0]},
                       leaf_tiles=len(xt.leaf_ids), created_tiles=xt.num_created, points_kept=kept, points_drawn=drawn)
            if name == "s2":
                candidates, listed, longest = candidates_of(ctx, cloud, cloud.bbox_min, cloud.bbox_max, iso)
                rec.update(kernel_ms_split={k: kms.get(k) for k in S2_KERNELS}, candidates=candidates, listed_cells=listed,
                           longest_cell_list=longest, candidates_per_kept_point=round(candidates / max(kept, 1), 3),
                           **s2_bytes(strategy, candidates, kept, drawn, kms))
            out["legs"][f"{name}_{strategy}"] = rec
            xt.free()
    if args.baseline:
        base = json.load(open(args.baseline))
        cmp = {}
        for strategy in STRATEGIES:
            a, b = out["legs"][f"octree_{strategy}"], base["legs"][f"octree_{strategy}"]
            apart = abs(a["wall_ms_median"] - b["wall_ms_median"])
            cmp[strategy] = dict(this_ms=a["wall_ms_median"], this_spread_ms=a["wall_ms_spread"], parent_ms=b["wall_ms_median"],
                                 parent_spread_ms=b["wall_ms_spread"], apart_ms=round(apart, 2),
                                 apart_by_more_than_spread=bool(apart > max(a["wall_ms_spread"], b["wall_ms_spread"])))
        out["octree_leg_vs_parent"] = dict(parent_build_hash=base.get("build_hash"), **cmp)
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
