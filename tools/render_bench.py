#!/usr/bin/env python
"""The frame renderer measured (GPU box): the config-2 cloud (100 M Gaussian-cluster points, bench.py's generator and seed)
built once, then the first 100 config-4 frusta (bench.py's query leg: eyes uniform in the box, seed 3) rendered at
1920 x 1080 in one pcv_render_views call, with point_size 1 and 3. Per point size: median wall time of --steps calls (after a
warm-up), the per-kernel times of ctx.kernel_stats() for the last call, points submitted and drawn per second
of splat-kernel time, and two bounds for the splat kernel next to its time: the node bytes it reads per submitted point over
the 8 TB/s HBM peak, and 8 atomic bytes per covered (point, pixel) pair — which the tool cannot count exactly, so the floor
of one pair per drawn point is used — over the chip-wide rate of no-return global atomics measured for gfx950 (about
1.3 TB/s of operand bytes when a wave's 64 operands are contiguous; a splat's operands are scattered, so this bound is loose).
View 0 is checked against the numpy oracle (tests/render_oracle.py) run over the node bytes the library holds for the nodes
of the oracle's own visible list: the SHA-256 of both images is recorded, and whether they are equal.
Prints one JSON line and writes it to --out.

usage: python tools/render_bench.py [--points N] [--views V] [--size WxH] [--steps K] [--out FILE]"""
import argparse
import hashlib
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
import render_oracle as R  # noqa: E402
from bench import build_hash, make_cloud  # noqa: E402

HBM_PEAK = 8.0e12
ATOMIC_PEAK_BYTES = 1.3e12  # chip-wide no-return global atomics, operand bytes per second
KERNELS = ("visible_nodes_kernel", "render_chunks_kernel", "render_splat_kernel", "render_resolve_kernel")


def oracle_view(tree, matrix, W, H, point_size, gamma):
    """View `matrix` by the numpy oracle over the library's node bytes (the tree's own bytes are checked by the suite)."""
    m = tree.num_nodes
    infos = [tree.node(i) for i in range(m)]
    names = [pcv.node_name(nd.id_high, nd.id_low) for nd in infos]
    meta = tree.meta()
    nodes = {n: dict(id=(nd.id_high, nd.id_low), num_points=nd.num_points) for n, nd in zip(names, infos)}
    index = {n: i for i, n in enumerate(names)}
    visible = O.get_visible_nodes(meta["bbox_min"], meta["bbox_max"], nodes, matrix)
    drawn = [dict(encoding=infos[index[n]].encoding, xyz=tree.node_data(index[n], 0), rgb=tree.node_data(index[n], 1),
                  cube_min=np.array(infos[index[n]].cube_min[:]), cube_edge=infos[index[n]].cube_edge) for n in (visible or [])]
    return R.draw_nodes(drawn, matrix, W, H, point_size, R.gamma_lut(gamma))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100_000_000)
    ap.add_argument("--resolution", type=float, default=0.001)
    ap.add_argument("--views", type=int, default=100)
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "render_bench.json"))
    args = ap.parse_args()
    W, H = (int(v) for v in args.size.split("x"))

    dev = torch.device("cuda", 0)
    x, y, z, rgb = make_cloud(torch, args.points, seed=1, device=dev)
    ctx = pcv.Context(0)
    tree = ctx.build(args.resolution, None, x, y, z, rgb)
    del x, y, z, rgb
    torch.cuda.empty_cache()
    meta = tree.meta()
    bmin, bmax = meta["bbox_min"], meta["bbox_max"]
    rng = np.random.default_rng(3)  # config-4 frusta exactly as bench.py's query leg draws them
    persp = O.perspective3_new(1.0, 1.2, 0.1, 100.0)
    mats = []
    for _ in range(args.views):
        eye = rng.uniform(bmin, bmax)
        q = rng.normal(size=4)
        q = q / math.sqrt(float(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]))
        mats.append(O.frustum_new(eye, q, persp)[0])
    shapes = ctx.shapes([("frustum", m) for m in mats])
    stride = {1: 3, 2: 6, 3: 12, 4: 24}
    node_stride = np.array([stride[tree.node(i).encoding] for i in range(tree.num_nodes)], dtype=np.int64)
    node_points = np.array([tree.node(i).num_points for i in range(tree.num_nodes)], dtype=np.int64)
    lists, _ = tree.visible_nodes(shapes)
    node_bytes = int(sum(int((node_stride[l] * node_points[l]).sum()) for l in lists))
    ctx.set_profiling(True)

    runs, ok = [], True
    for point_size in (1.0, 3.0):
        walls, split, infos, digest = [], None, None, None
        for step in range(args.steps + 1):  # the first is a warm-up
            ctx.reset_kernel_stats()
            t0 = time.perf_counter()
            rv = tree.render(shapes, W, H, point_size=point_size)
            wall = (time.perf_counter() - t0) * 1e3
            if step:
                walls.append(wall)
            if step == args.steps:
                st = ctx.kernel_stats()
                split = {k.replace("_kernel", ""): round(st[k][1], 3) for k in KERNELS if st[k][0]}
                infos = [rv.info(v) for v in range(args.views)]
                img0 = rv.images(0, 1)[0].cpu().numpy()
                digest = hashlib.sha256(img0.tobytes()).hexdigest()
            rv.close()
        want = oracle_view(tree, mats[0], W, H, point_size, 1.0)
        want_digest = hashlib.sha256(want["image"].tobytes()).hexdigest()
        ok = ok and digest == want_digest
        submitted = sum(i["points_submitted"] for i in infos)
        drawn = sum(i["points_drawn"] for i in infos)
        splat_s = split.get("render_splat", 0.0) * 1e-3
        rec = dict(point_size=point_size, wall_ms_median=round(float(np.median(walls)), 3), wall_ms=[round(w, 3) for w in walls],
                   kernel_ms=split, nodes_drawn=sum(i["nodes_drawn"] for i in infos), points_submitted=submitted, points_drawn=drawn,
                   pixels_covered=sum(i["pixels_covered"] for i in infos), node_bytes_read=node_bytes,
                   view0_digest=digest, view0_oracle_digest=want_digest, view0_equals_oracle=digest == want_digest)
        if splat_s > 0:
            rec.update(points_submitted_per_s=round(submitted / splat_s), points_drawn_per_s=round(drawn / splat_s),
                       splat_bound_hbm_ms=round(node_bytes / HBM_PEAK * 1e3, 4),
                       splat_bound_atomics_ms_floor=round(8 * drawn / ATOMIC_PEAK_BYTES * 1e3, 4))
        runs.append(rec)
    out = {"tool": "tools/render_bench.py", "build_hash": build_hash(), "device": torch.cuda.get_device_name(0),
           "cloud": f"config 2: {args.points} Gaussian-cluster points (bench.make_cloud, seed 1), resolution {args.resolution}",
           "nodes": tree.num_nodes, "views": args.views, "size": [W, H], "steps": args.steps, "runs": runs}
    print(json.dumps(out))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    tree.free()
    ctx.close()
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
