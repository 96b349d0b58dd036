#!/usr/bin/env python
"""The batched point query measured (GPU box): the config-2 cloud (100 M Gaussian-cluster points, bench.py's generator and seed)
built once, then
  (a) one pcv_query_batch_run over the 10 000 config-4 frusta (bench.py's query leg: eyes uniform in the box, seed 3), every
      segment copied to device buffers;
  (b) the single-location loop, pcv_query_points per frustum, over the first 1 000 of those frusta — extrapolated to 10 000;
  (c) a 64 x 64 grid of AABB tiles over the box (x and y split, z whole), as xray's tile generation issues them.
Wall time is taken around work that ends in a stream synchronise; kernel time from ctx.kernel_stats(). The flags pass's bytes
are the encoded positions of every (shape, node) pair it decodes plus one flag byte per candidate point, over its kernel time,
against the 8 TB/s HBM peak. Per-shape counts of the batch are checked against the loop for every frustum both ran, and for
the first 256 tiles. Prints one JSON line and writes it to --out.

usage: python tools/query_batch_bench.py [--points N] [--frusta F] [--loop-frusta L] [--tiles T] [--steps K] [--out FILE]"""
import argparse
import json
import math
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
from bench import build_hash, make_cloud  # noqa: E402

HBM_PEAK = 8.0e12
BATCH_KERNELS = ("batch_nodes_kernel", "batch_chunks_kernel", "batch_flags_kernel", "batch_scan_kernel", "batch_compact_kernel")


def kernel_ms(ctx, names):
    st = ctx.kernel_stats()
    return {k.replace("_kernel", ""): round(st[k][1], 3) for k in names if st[k][0]}


def run_batch(ctx, tree, shapes, steps):
    """(median wall ms, kernel ms split, batch of the last step, flags-pass bytes) of run + copy of every segment to the device."""
    walls, split = [], None
    for step in range(steps + 1):  # the first is a warm-up
        ctx.reset_kernel_stats()
        t0 = time.perf_counter()
        b = tree.query_batch(shapes)
        n = b.num_points
        out = dict(x=torch.empty(n, dtype=torch.float64, device="cuda"), y=torch.empty(n, dtype=torch.float64, device="cuda"),
                   z=torch.empty(n, dtype=torch.float64, device="cuda"), rgb=torch.empty((n, 3), dtype=torch.uint8, device="cuda"))
        b.points(out=out)
        wall = (time.perf_counter() - t0) * 1e3
        if step:
            walls.append(wall)
            split = kernel_ms(ctx, BATCH_KERNELS)
        if step < steps:
            b.free()
        del out
    return float(np.median(walls)), split, b


def flags_bytes(tree, batch):
    m = tree.num_nodes
    npts = np.array([tree.node(i).num_points for i in range(m)], dtype=np.int64)
    bpc = np.array([{1: 1, 2: 2, 3: 4, 4: 8}[tree.node(i).encoding] for i in range(m)], dtype=np.int64)
    _, nodes, _ = batch.segments()
    cand = int(npts[nodes].sum())
    return cand, int((npts[nodes] * 3 * bpc[nodes]).sum()) + cand


def shape_counts(batch):
    first, _, off = batch.segments()
    return (off[first[1:]] - off[first[:-1]]).astype(np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100_000_000)
    ap.add_argument("--resolution", type=float, default=0.001)
    ap.add_argument("--frusta", type=int, default=10_000)
    ap.add_argument("--loop-frusta", type=int, default=1_000)
    ap.add_argument("--tiles", type=int, default=64)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07_query_batch_bench.json"))
    args = ap.parse_args()

    dev = torch.device("cuda", 0)
    x, y, z, rgb = make_cloud(torch, args.points, seed=1, device=dev)
    ctx = pcv.Context(0)
    tree = ctx.build(args.resolution, None, x, y, z, rgb)
    del x, y, z, rgb
    torch.cuda.empty_cache()
    meta = tree.meta()
    bmin, bmax = meta["bbox_min"], meta["bbox_max"]
    # config-4 frusta exactly as bench.py's query leg draws them
    rng = np.random.default_rng(3)
    persp = O.perspective3_new(1.0, 1.2, 0.1, 100.0)
    mats = []
    for _ in range(args.frusta):
        eye = rng.uniform(bmin, bmax)
        q = rng.normal(size=4)
        q = q / math.sqrt(float(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]))
        c, _ = O.frustum_new(eye, q, persp)
        mats.append(c)
    shapes = ctx.shapes([("frustum", m) for m in mats])
    ctx.set_profiling(True)

    # (a) one batch over every frustum
    wall_a, split_a, batch = run_batch(ctx, tree, shapes, args.steps)
    counts_a = shape_counts(batch)
    cand, fbytes = flags_bytes(tree, batch)
    rec_a = dict(frusta=args.frusta, wall_ms=round(wall_a, 3), kernel_ms=split_a, kernel_ms_total=round(sum(split_a.values()), 3),
                 segments=batch.num_segments, points=batch.num_points, candidate_points=cand, flags_pass_bytes=fbytes,
                 flags_pass_tb_s=round(fbytes / (split_a["batch_flags"] * 1e-3) / 1e12, 3),
                 flags_pass_kernel_share_of_hbm_peak=round(fbytes / (split_a["batch_flags"] * 1e-3) / HBM_PEAK, 3))
    batch.free()

    # (b) the single-location loop over the first L frusta, extrapolated
    L = min(args.loop_frusta, args.frusta)
    tree.query_points(shapes, 0, capacity=1 << 22)  # warm-up
    ctx.reset_kernel_stats()
    t0 = time.perf_counter()
    counts_b = np.array([tree.query_points(shapes, f, capacity=1 << 22)["count"] for f in range(L)], dtype=np.int64)
    wall_b = (time.perf_counter() - t0) * 1e3
    st = ctx.kernel_stats()
    k_b = sum(st[k][1] for k in ("cull_nodes_kernel", "cull_points_kernel", "query_compact_kernel"))
    scale = args.frusta / L
    rec_b = dict(frusta_run=L, wall_ms_run=round(wall_b, 3), kernel_ms_run=round(k_b, 3),
                 wall_ms_extrapolated=round(wall_b * scale, 3), kernel_ms_extrapolated=round(k_b * scale, 3),
                 note=f"EXTRAPOLATED linearly from {L} to {args.frusta} frusta (per-frustum cost is independent of the others); "
                      "outputs to host buffers of 2^22 points, as bench.py's query leg")
    counts_match_loop = bool(np.array_equal(counts_a[:L], counts_b))

    # (c) xray-style tiles
    T = args.tiles
    tiles = []
    for i in range(T):
        for j in range(T):
            lo = [bmin[0] + (bmax[0] - bmin[0]) * i / T, bmin[1] + (bmax[1] - bmin[1]) * j / T, bmin[2]]
            hi = [bmin[0] + (bmax[0] - bmin[0]) * (i + 1) / T, bmin[1] + (bmax[1] - bmin[1]) * (j + 1) / T, bmax[2]]
            tiles.append(("aabb", lo, hi))
    tshapes = ctx.shapes(tiles)
    wall_c, split_c, tb = run_batch(ctx, tree, tshapes, args.steps)
    counts_c = shape_counts(tb)
    tcand, tbytes = flags_bytes(tree, tb)
    rec_c = dict(tiles=T * T, wall_ms=round(wall_c, 3), kernel_ms=split_c, kernel_ms_total=round(sum(split_c.values()), 3),
                 segments=tb.num_segments, points=tb.num_points, candidate_points=tcand, flags_pass_bytes=tbytes,
                 flags_pass_kernel_share_of_hbm_peak=round(tbytes / (split_c["batch_flags"] * 1e-3) / HBM_PEAK, 3))
    tb.free()
    K = min(256, T * T)
    tile_counts = np.array([tree.query_points(tshapes, t, capacity=1)["count"] for t in range(K)], dtype=np.int64)
    tiles_match_loop = bool(np.array_equal(counts_c[:K], tile_counts))

    ratio_wall = rec_b["wall_ms_extrapolated"] / rec_a["wall_ms"]
    out = {"tool": "tools/query_batch_bench.py", "build_hash": build_hash(), "device": torch.cuda.get_device_name(0),
           "cloud": f"config 2: {args.points} Gaussian-cluster points (bench.make_cloud, seed 1), resolution {args.resolution}",
           "nodes": tree.num_nodes, "a_batch": rec_a, "b_loop": rec_b, "c_tiles": rec_c,
           "batch_vs_loop_wall": round(ratio_wall, 2),
           "batch_vs_loop_kernel": round(rec_b["kernel_ms_extrapolated"] / rec_a["kernel_ms_total"], 2),
           "counts_match_loop": counts_match_loop, "tile_counts_match_loop": tiles_match_loop,
           "verdicts": {"batch_wins_by_10x_wall": ratio_wall > 10.0,
                        "flags_pass_at_least_0.50_of_hbm_peak": rec_a["flags_pass_kernel_share_of_hbm_peak"] >= 0.50}}
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    tree.free()
    ctx.close()
    return 0 if counts_match_loop and tiles_match_loop else 1


if __name__ == "__main__":
    sys.exit(main())
