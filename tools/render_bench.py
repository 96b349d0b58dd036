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

--outlines: the same case with show_octree_nodes off and on in one process (profiles/render_outline_bench.json): per point
size and setting the wall time, the per-kernel times (render_outline_kernel among them), outline_pixels and the segments, and
view 0 against tests/render_outline_oracle.py. With --parent-library (a libpcv_hip.so built from the parent commit) the
outlines-off wall time is also measured next to the parent's: fresh processes, one library each, alternating --ab-reps
times (the way tools/ab_libs.sh alternates variants), each building the cloud itself. The off path launches the instances
the parent launches, so a difference beyond the spread of those runs is a finding, recorded with the figures.

--terrain: the same case without and with one terrain layer built from the same tree (resolution_m 0.1, tile size 256; the
viewer's window of 1024 vertices around each eye), alternating in one process (profiles/render_terrain_bench.json): per
point size and setting the wall time, the per-kernel times (render_terrain_gather_kernel and render_terrain_edges_kernel
among them), the edges and the pixels the layer won, and view 0 against tests/render_terrain_oracle.py when the layer has
at most 256 tiles (the oracle holds them on the host).

usage: python tools/render_bench.py [--points N] [--views V] [--size WxH] [--steps K] [--out FILE]
       python tools/render_bench.py --outlines [--parent-library FILE] [--ab-reps R] [...]
       python tools/render_bench.py --terrain [--terrain-resolution R] [--terrain-window N] [...]"""
import argparse
import hashlib
import json
import math
import os
import subprocess
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
import render_outline_oracle as RO  # noqa: E402
import render_terrain_oracle as RT  # noqa: E402
from bench import build_hash, make_cloud  # noqa: E402

HBM_PEAK = 8.0e12
ATOMIC_PEAK_BYTES = 1.3e12  # chip-wide no-return global atomics, operand bytes per second
KERNELS = ("visible_nodes_kernel", "render_chunks_kernel", "render_splat_kernel", "render_outline_kernel", "render_terrain_gather_kernel",
           "render_terrain_edges_kernel", "render_resolve_kernel")


def oracle_view(tree, matrix, W, H, point_size, gamma, outlines=False):
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
    return (RO if outlines else R).draw_nodes(drawn, matrix, W, H, point_size, R.gamma_lut(gamma))


def setup(args):
    """The config-2 tree and the config-4 frusta of the case: (ctx, tree, mats, shapes); the eyes are left in args.eyes."""
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
    mats, args.eyes = [], []
    for _ in range(args.views):
        eye = rng.uniform(bmin, bmax)
        args.eyes.append(eye)
        q = rng.normal(size=4)
        q = q / math.sqrt(float(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]))
        mats.append(O.frustum_new(eye, q, persp)[0])
    return ctx, tree, mats, ctx.shapes([("frustum", m) for m in mats])


def measure(ctx, tree, shapes, W, H, steps, point_size, **render_kw):
    """steps calls after a warm-up: (wall times in ms, kernel split of the last call, its infos, its outline infos, view 0)."""
    walls, split, infos, oinfos, img0 = [], None, None, None, None
    for step in range(steps + 1):
        ctx.reset_kernel_stats()
        t0 = time.perf_counter()
        rv = tree.render(shapes, W, H, point_size=point_size, **render_kw)
        wall = (time.perf_counter() - t0) * 1e3
        if step:
            walls.append(wall)
        if step == steps:
            st = ctx.kernel_stats()
            split = {k.replace("_kernel", ""): round(st[k][1], 3) for k in KERNELS if k in st and st[k][0]}
            infos = [rv.info(v) for v in range(shapes.count)]
            oinfos = [rv.outline_info(v) for v in range(shapes.count)] if hasattr(rv, "outline_info") and render_kw else None
            img0 = rv.images(0, 1)[0].cpu().numpy()
        rv.close()
    return walls, split, infos, oinfos, img0


def wall_only(args, W, H):
    """One process of the parent comparison: outlines off, wall times only, through the library PCV_HIP_LIBRARY names."""
    if os.environ.get("PCV_HIP_LIBRARY"):  # a library of an earlier commit lacks the entry points added since: they leave
        import ctypes                      # this process's binding table, which otherwise refuses such a library
        from point_cloud_viewer_amd import _lib
        older = ctypes.CDLL(_lib.LIB_PATH)
        for name in [n for n in _lib._SIGNATURES if not hasattr(older, n)]:
            del _lib._SIGNATURES[name]
    ctx, tree, _, shapes = setup(args)
    out = {"library": os.environ.get("PCV_HIP_LIBRARY") or "this tree's", "build_hash": build_hash(), "runs": []}
    for point_size in (1.0, 3.0):
        walls = measure(ctx, tree, shapes, W, H, args.steps, point_size)[0]
        out["runs"].append(dict(point_size=point_size, wall_ms_median=round(float(np.median(walls)), 3), wall_ms=[round(w, 3) for w in walls]))
    print(json.dumps(out))
    tree.free()
    ctx.close()
    return 0


def against_parent(args):
    """Outlines off, this tree's library and the parent's alternating in fresh processes; the figures and their spread."""
    base = [sys.executable, os.path.abspath(__file__), "--wall-only", "--points", str(args.points), "--resolution", str(args.resolution),
            "--views", str(args.views), "--size", args.size, "--steps", str(args.steps)]
    runs = {"parent": [], "this": []}
    for _ in range(args.ab_reps):
        for name in ("parent", "this"):
            env = dict(os.environ)
            env.pop("PCV_HIP_LIBRARY", None)
            if name == "parent":
                env["PCV_HIP_LIBRARY"] = os.path.abspath(args.parent_library)
            p = subprocess.run(base, env=env, capture_output=True, text=True, timeout=600)
            if p.returncode != 0:
                raise SystemExit(f"render_bench: the {name} run failed ({p.returncode}): {p.stderr[-2000:]}")
            runs[name].append(json.loads(p.stdout.strip().splitlines()[-1])["runs"])
    out = []
    for k, point_size in enumerate((1.0, 3.0)):
        med = {name: [r[k]["wall_ms_median"] for r in runs[name]] for name in runs}
        spread = max(max(v) - min(v) for v in med.values())
        diff = float(np.median(med["this"]) - np.median(med["parent"]))
        out.append(dict(point_size=point_size, parent_wall_ms_medians=med["parent"], this_wall_ms_medians=med["this"],
                        run_to_run_spread_ms=round(spread, 3), this_minus_parent_ms=round(diff, 3),
                        finding=("within the run-to-run spread of this job" if abs(diff) <= spread else
                                 "beyond the run-to-run spread of this job: the off path launches the parent's instances, so the "
                                 "difference is not explained by the kernels; see the per-run figures")))
    return out


def outlines(args, W, H):
    """--outlines: show_octree_nodes off and on in one process."""
    versus = against_parent(args) if args.parent_library else None  # before this process opens the device
    ctx, tree, mats, shapes = setup(args)
    ctx.set_profiling(True)
    runs, ok = [], True
    for point_size in (1.0, 3.0):
        for on in (False, True):
            kw = dict(show_octree_nodes=True) if on else {}
            walls, split, infos, oinfos, img0 = measure(ctx, tree, shapes, W, H, args.steps, point_size, **kw)
            want = oracle_view(tree, mats[0], W, H, point_size, 1.0, outlines=on)
            digest, want_digest = hashlib.sha256(img0.tobytes()).hexdigest(), hashlib.sha256(want["image"].tobytes()).hexdigest()
            ok = ok and digest == want_digest
            rec = dict(point_size=point_size, outlines=on, wall_ms_median=round(float(np.median(walls)), 3), wall_ms=[round(w, 3) for w in walls],
                       kernel_ms=split, nodes_drawn=sum(i["nodes_drawn"] for i in infos), points_submitted=sum(i["points_submitted"] for i in infos),
                       points_drawn=sum(i["points_drawn"] for i in infos), pixels_covered=sum(i["pixels_covered"] for i in infos),
                       view0_digest=digest, view0_oracle_digest=want_digest, view0_equals_oracle=digest == want_digest)
            if on:
                rec.update(segments_submitted=sum(i["segments_submitted"] for i in oinfos), segments_drawn=sum(i["segments_drawn"] for i in oinfos),
                           outline_pixels=sum(i["outline_pixels"] for i in oinfos), view0_outline_pixels=want["outline_pixels"])
            runs.append(rec)
    out = {"tool": "tools/render_bench.py --outlines", "build_hash": build_hash(), "device": torch.cuda.get_device_name(0),
           "cloud": f"config 2: {args.points} Gaussian-cluster points (bench.make_cloud, seed 1), resolution {args.resolution}",
           "nodes": tree.num_nodes, "views": args.views, "size": [W, H], "steps": args.steps, "runs": runs}
    if versus is not None:
        out["outlines_off_vs_parent"] = dict(method=f"fresh processes alternating parent / this, {args.ab_reps} of each, median of {args.steps} calls per run",
                                            runs=versus)
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    tree.free()
    ctx.close()
    return 0 if ok else 1


def terrain(args, W, H):
    """--terrain: no layer and one layer of the same tree, alternating in one process."""
    ctx, tree, mats, shapes = setup(args)
    eyes = np.array(args.eyes)
    t0 = time.perf_counter()
    layer = tree.terrain(resolution_m=args.terrain_resolution, tile_size=256)
    build_ms = (time.perf_counter() - t0) * 1e3
    info = layer.info()
    small = info["tiles"] <= 256
    layer_dict = None
    if small:
        layer_dict = dict(tile_size=256, resolution_m=args.terrain_resolution, origin=np.zeros(3), world_from_terrain=np.array([0.0, 0, 0, 0, 0, 0, 1]),
                          tiles=layer.tiles(), heights=layer.heights(), colors=layer.colors())
    ctx.set_profiling(True)
    runs, ok = [], True
    for point_size in (1.0, 3.0):
        for on in (False, True, False, True):
            kw = dict(terrain=[layer], camera_positions=eyes, terrain_window=args.terrain_window) if on else {}
            walls, split, infos, _, img0 = measure(ctx, tree, shapes, W, H, args.steps, point_size, **kw)
            rec = dict(point_size=point_size, terrain=on, wall_ms_median=round(float(np.median(walls)), 3), wall_ms=[round(w, 3) for w in walls],
                       kernel_ms=split, points_submitted=sum(i["points_submitted"] for i in infos), pixels_covered=sum(i["pixels_covered"] for i in infos))
            if on:
                rv = tree.render(shapes, W, H, point_size=point_size, **kw)
                tinfo = [rv.terrain_info(v, 0) for v in range(shapes.count)]
                rv.close()
                rec.update(edges_submitted=sum(t["edges_submitted"] for t in tinfo), edges_drawn=sum(t["edges_drawn"] for t in tinfo),
                           pixels_won=sum(t["pixels_won"] for t in tinfo))
            if small or not on:
                want = oracle_view(tree, mats[0], W, H, point_size, 1.0)
                if on:
                    want.update(status=0)
                    RT.add_layers(want, want["points_submitted"], [layer_dict], eyes[0], mats[0], W, H, args.terrain_window)
                digest, want_digest = hashlib.sha256(img0.tobytes()).hexdigest(), hashlib.sha256(want["image"].tobytes()).hexdigest()
                ok = ok and digest == want_digest
                rec.update(view0_digest=digest, view0_oracle_digest=want_digest, view0_equals_oracle=digest == want_digest)
            runs.append(rec)
    out = {"tool": "tools/render_bench.py --terrain", "build_hash": build_hash(), "device": torch.cuda.get_device_name(0),
           "cloud": f"config 2: {args.points} Gaussian-cluster points (bench.make_cloud, seed 1), resolution {args.resolution}",
           "nodes": tree.num_nodes, "views": args.views, "size": [W, H], "steps": args.steps,
           "terrain": dict(resolution_m=args.terrain_resolution, tile_size=256, window=args.terrain_window, tiles=info["tiles"],
                           set_vertices=info["set_vertices"], rendered_quads=info["rendered_quads"], build_ms=round(build_ms, 1)), "runs": runs}
    print(json.dumps(out))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    layer.free()
    tree.free()
    ctx.close()
    return 0 if ok else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100_000_000)
    ap.add_argument("--resolution", type=float, default=0.001)
    ap.add_argument("--views", type=int, default=100)
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--outlines", action="store_true")
    ap.add_argument("--terrain", action="store_true")
    ap.add_argument("--terrain-resolution", type=float, default=0.1)
    ap.add_argument("--terrain-window", type=int, default=1024)
    ap.add_argument("--parent-library", default=None)
    ap.add_argument("--ab-reps", type=int, default=2)
    ap.add_argument("--wall-only", action="store_true", help="one process of the parent comparison (used by --outlines)")
    args = ap.parse_args()
    W, H = (int(v) for v in args.size.split("x"))
    if args.out is None:
        args.out = os.path.join(ROOT, "profiles", "render_outline_bench.json" if args.outlines else
                                "render_terrain_bench.json" if args.terrain else "render_bench.json")
    if args.wall_only:
        return wall_only(args, W, H)
    if args.outlines:
        return outlines(args, W, H)
    if args.terrain:
        return terrain(args, W, H)

    ctx, tree, mats, shapes = setup(args)
    stride = {1: 3, 2: 6, 3: 12, 4: 24}
    node_stride = np.array([stride[tree.node(i).encoding] for i in range(tree.num_nodes)], dtype=np.int64)
    node_points = np.array([tree.node(i).num_points for i in range(tree.num_nodes)], dtype=np.int64)
    lists, _ = tree.visible_nodes(shapes)
    node_bytes = int(sum(int((node_stride[l] * node_points[l]).sum()) for l in lists))
    ctx.set_profiling(True)

    runs, ok = [], True
    for point_size in (1.0, 3.0):
        walls, split, infos, _, img0 = measure(ctx, tree, shapes, W, H, args.steps, point_size)
        digest = hashlib.sha256(img0.tobytes()).hexdigest()
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
