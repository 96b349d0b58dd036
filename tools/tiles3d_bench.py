#!/usr/bin/env python
"""The 3D Tiles export, measured (GPU box; there is no CPU fallback). The tree is the config-2 octree: --points (100 M)
Gaussian-cluster points (bench.py's generator, seed 1, colour), resolution 0.001. One process, a warm-up round and then --runs
rounds in which the legs alternate; medians and spreads:
  tile_files   every .pnts file into device memory, position mode auto, quantized and float: wall, and tiles3d_pack_kernel alone
               (ctx.kernel_stats). Bytes read (the nodes' .xyz and .rgb bytes) and written (the files) are computed here from
               the node table, and their sum over the kernel's time is set against the 8 TB/s HBM peak.
  write        Tiles3D.write onto tmpfs (mode auto): wall, pieces = launches of the kernel
Yardsticks in the same process and rounds, for the README and no pass criterion: ply_rows of AllPoints over the same tree into
device memory (ply_rows_kernel alone; 27-byte rows, its bytes counted the same way) and pcv_octree_write_dir of the tree onto the
same tmpfs.
Prints one JSON line and writes it to --out.

usage: python tools/tiles3d_bench.py [--points N] [--runs R] [--tmp DIR] [--out FILE]"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import point_cloud_viewer_amd as pcv  # noqa: E402
from bench import HBM_PEAK_GBS, build_hash, make_cloud  # noqa: E402

PACK, ROWS = "tiles3d_pack_kernel", "ply_rows_kernel"
SRC_BYTES = {1: 3, 2: 6, 3: 12, 4: 24}  # a point of a node's .xyz by PCV_ENC_*


def spread(values):
    v = np.asarray(values, dtype=np.float64)
    return dict(median=round(float(np.median(v)), 3), min=round(float(v.min()), 3), max=round(float(v.max()), 3), runs=[round(float(t), 3) for t in v])


def timed(ctx, fn):
    ctx.reset_kernel_stats()
    t0 = time.perf_counter()
    fn()
    ctx.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100_000_000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--tmp", default="/dev/shm" if os.path.isdir("/dev/shm") else tempfile.gettempdir())
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tiles3d_bench.json"))
    args = ap.parse_args()
    n = args.points
    dev = torch.device("cuda", 0)
    ctx = pcv.Context(0)
    x, y, z, rgb = make_cloud(torch, n, seed=1, device=dev)
    tree = ctx.build(0.001, None, x, y, z, rgb)
    del x, y, z, rgb
    torch.cuda.empty_cache()
    nodes = [tree.node(i) for i in range(tree.num_nodes)]
    enc_points = {e: int(sum(nd.num_points for nd in nodes if nd.encoding == e)) for e in SRC_BYTES}
    read_bytes = int(sum(nd.num_points * (SRC_BYTES[nd.encoding] + 3) for nd in nodes))
    shapes = ctx.shapes([("all",)])
    batch = tree.query_batch(shapes)
    st = os.statvfs(args.tmp)
    if st.f_bavail * st.f_frsize < (16 << 30):  # a small tmpfs: the system's temporary directory instead
        args.tmp = tempfile.gettempdir()
    tmp = tempfile.mkdtemp(prefix="tiles3d_bench_", dir=args.tmp)
    plans = {mode: tree.tiles3d(position_mode=mode) for mode in ("auto", "quantized", "float")}
    infos = {mode: t.info for mode, t in plans.items()}
    ctx.set_profiling(True)
    ms, pieces, rows_bytes, dir_bytes = {}, 0, 0, {}
    for rnd in range(args.runs + 1):  # round 0 warms every leg up
        rec = {}
        for mode, t in plans.items():
            rec[f"tile_files_{mode}_wall"] = timed(ctx, lambda: t.tile_files(device=True))
            rec[f"tile_files_{mode}_kernel"] = ctx.kernel_stats()[PACK][1]
            torch.cuda.empty_cache()
        out_dir = os.path.join(tmp, "tiles")
        rec["write_wall"] = timed(ctx, lambda: plans["auto"].write(out_dir))
        rec["write_kernel"], pieces = ctx.kernel_stats()[PACK][1], ctx.kernel_stats()[PACK][0]
        dir_bytes["tiles3d"] = sum(os.path.getsize(os.path.join(out_dir, f)) for f in os.listdir(out_dir))
        shutil.rmtree(out_dir)

        def rows():
            out, _ = batch.ply_rows(device=True)[:2]
            return out
        ctx.reset_kernel_stats()
        t0 = time.perf_counter()
        r = rows()
        ctx.synchronize()
        rec["ply_rows_wall"] = (time.perf_counter() - t0) * 1e3
        rec["ply_rows_kernel"] = ctx.kernel_stats()[ROWS][1]
        rows_bytes = int(r.numel() * r.element_size())
        del r
        torch.cuda.empty_cache()
        oct_dir = os.path.join(tmp, "octree")
        rec["octree_write_dir_wall"] = timed(ctx, lambda: tree.write_dir(oct_dir))
        dir_bytes["octree"] = sum(os.path.getsize(os.path.join(oct_dir, f)) for f in os.listdir(oct_dir))
        shutil.rmtree(oct_dir)
        if rnd:
            for leg, v in rec.items():
                ms.setdefault(leg, []).append(v)
    os.rmdir(tmp)
    med = lambda leg: float(np.median(ms[leg]))
    out = {"tool": "tools/tiles3d_bench.py", "build_hash": build_hash(), "device": torch.cuda.get_device_name(0),
           "tree": f"config-2 distribution: {n} Gaussian-cluster points (bench.make_cloud, seed 1), octree resolution 0.001, {len(nodes)} nodes",
           "points_by_encoding": {"uint8": enc_points[1], "uint16": enc_points[2], "float32": enc_points[3], "float64": enc_points[4]},
           "runs": args.runs, "tmp": args.tmp, "info": infos, "write_pieces": pieces, "directory_bytes": dir_bytes,
           "legs_ms": {leg: spread(v) for leg, v in ms.items()}}
    derived = {}
    for mode in plans:
        moved = read_bytes + infos[mode]["total_file_bytes"]
        gbs = moved / (med(f"tile_files_{mode}_kernel") * 1e-3) / 1e9
        derived[mode] = dict(bytes_read=read_bytes, bytes_written=infos[mode]["total_file_bytes"], kernel_gb_per_s=round(gbs, 1),
                             share_of_hbm_peak=round(gbs / HBM_PEAK_GBS, 4),
                             points_per_s=round(infos[mode]["points"] / (med(f"tile_files_{mode}_kernel") * 1e-3), 1))
    out["derived"] = derived
    rows_read = read_bytes + batch.num_points  # the node bytes and one keep flag per point
    gbs = (rows_read + rows_bytes) / (med("ply_rows_kernel") * 1e-3) / 1e9
    out["ply_rows_yardstick"] = dict(rows=batch.num_points, bytes_read=int(rows_read), bytes_written=rows_bytes, kernel_gb_per_s=round(gbs, 1),
                                     share_of_hbm_peak=round(gbs / HBM_PEAK_GBS, 4),
                                     points_per_s=round(batch.num_points / (med("ply_rows_kernel") * 1e-3), 1))
    for t in plans.values():
        t.free()
    batch.free()
    shapes.free()
    tree.free()
    print(json.dumps(out))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
