#!/usr/bin/env python
"""LAS output, measured (GPU box; there is no CPU fallback). Two sources of --points (100 M) points each: the config-2 octree
(bench.py's Gaussian clusters, seed 1, colour, resolution 0.001) with AllPoints in formats 2 and 7, and the same distribution as
an ECEF S2 cloud with the extras classification, return_number and gps_time (format AUTO = 3). One process, a warm-up round and
then --runs rounds in which the legs alternate; medians and spreads:
  las_records   the records into device memory with a given offset: wall, and las_records_kernel alone (ctx.kernel_stats). Bytes
                read (positions, colour, flags, offsets, extras) and written (the records) are computed here, and their sum
                over the kernel's time is set against the 8 TB/s HBM peak.
  min_pass      las_min_kernel alone, from a las_records call with the offset left to the library
  write_las     the file onto tmpfs (auto offset): wall
Yardsticks in the same process and rounds, for the README and no pass criterion: ply_rows_kernel and write_ply of the same result,
points() into device buffers (octree), and Context.las_load of the file just written.
Prints one JSON line and writes it to --out.

usage: python tools/las_write_bench.py [--points N] [--runs R] [--tmp DIR] [--out FILE]"""
import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import point_cloud_viewer_amd as pcv  # noqa: E402
from bench import HBM_PEAK_GBS, build_hash, make_cloud  # noqa: E402
from point_cloud_viewer_amd import synthetic  # noqa: E402

RECORDS, MIN, ROWS = "las_records_kernel", "las_min_kernel", "ply_rows_kernel"
SRC_BYTES = {1: 3, 2: 6, 3: 12, 4: 24}  # a point of a node's .xyz by PCV_ENC_*


def spread(values):
    v = np.asarray(values, dtype=np.float64)
    return dict(median=round(float(np.median(v)), 3), min=round(float(v.min()), 3), max=round(float(v.max()), 3), runs=[round(float(t), 3) for t in v])


def timed(ctx, fn):
    ctx.reset_kernel_stats()
    t0 = time.perf_counter()
    r = fn()
    ctx.synchronize()
    return (time.perf_counter() - t0) * 1e3, r


def measure(ctx, batch, formats, offset, read_bytes, rows_read, tmp, runs, with_points):
    n = batch.num_points
    ms, sizes = {}, {}
    dev = f"cuda:{ctx.device}"
    for rnd in range(runs + 1):  # round 0 warms every leg up
        rec = {}
        for fmt in formats:
            wall, (r, info) = timed(ctx, lambda: batch.las_records(device=True, point_format=fmt, offset=offset))
            rec[f"las_records_f{fmt}_wall"], rec[f"las_records_f{fmt}_kernel"] = wall, ctx.kernel_stats()[RECORDS][1]
            sizes[f"f{fmt}"] = int(r.numel())
            assert info["out_of_range"] == 0
            del r
            torch.cuda.empty_cache()
            _, (r, info) = timed(ctx, lambda: batch.las_records(device=True, point_format=fmt))
            rec[f"min_pass_f{fmt}_kernel"] = ctx.kernel_stats()[MIN][1]
            del r
            torch.cuda.empty_cache()
            path = os.path.join(tmp, f"out_f{fmt}.las")
            rec[f"write_las_f{fmt}_wall"], _ = timed(ctx, lambda: batch.write_las(path, point_format=fmt))
            sizes[f"file_f{fmt}"] = os.path.getsize(path)
            wall, cloud = timed(ctx, lambda: ctx.las_load(path))
            rec[f"las_load_f{fmt}_wall"] = wall
            cloud.free()
            os.unlink(path)
        wall, (r, _) = timed(ctx, lambda: batch.ply_rows(device=True))
        rec["ply_rows_wall"], rec["ply_rows_kernel"] = wall, ctx.kernel_stats()[ROWS][1]
        sizes["ply_rows"] = int(r.numel())
        del r
        torch.cuda.empty_cache()
        path = os.path.join(tmp, "out.ply")
        rec["write_ply_wall"], _ = timed(ctx, lambda: batch.write_ply(path))
        sizes["file_ply"] = os.path.getsize(path)
        os.unlink(path)
        if with_points:
            out = dict(x=torch.empty(n, dtype=torch.float64, device=dev), y=torch.empty(n, dtype=torch.float64, device=dev),
                       z=torch.empty(n, dtype=torch.float64, device=dev), rgb=torch.empty(3 * n, dtype=torch.uint8, device=dev))
            rec["points_to_device_wall"], _ = timed(ctx, lambda: batch.points(out=out))
            del out
            torch.cuda.empty_cache()
        if rnd:
            for leg, v in rec.items():
                ms.setdefault(leg, []).append(v)
    med = lambda leg: float(np.median(ms[leg]))
    derived = {}
    for fmt in formats:
        moved = read_bytes[fmt] + sizes[f"f{fmt}"]
        gbs = moved / (med(f"las_records_f{fmt}_kernel") * 1e-3) / 1e9
        derived[f"f{fmt}"] = dict(bytes_read=int(read_bytes[fmt]), bytes_written=sizes[f"f{fmt}"], kernel_tb_per_s=round(gbs / 1e3, 3),
                                  share_of_hbm_peak=round(gbs / HBM_PEAK_GBS, 4),
                                  points_per_s=round(n / (med(f"las_records_f{fmt}_kernel") * 1e-3), 1))
    gbs = (rows_read + sizes["ply_rows"]) / (med("ply_rows_kernel") * 1e-3) / 1e9
    derived["ply_rows"] = dict(bytes_read=int(rows_read), bytes_written=sizes["ply_rows"], kernel_tb_per_s=round(gbs / 1e3, 3),
                               share_of_hbm_peak=round(gbs / HBM_PEAK_GBS, 4))
    return dict(points=n, sizes=sizes, legs_ms={leg: spread(v) for leg, v in ms.items()}, derived=derived)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100_000_000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--level", type=int, default=20)
    ap.add_argument("--tmp", default="/dev/shm" if os.path.isdir("/dev/shm") else tempfile.gettempdir())
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "las_write_bench.json"))
    args = ap.parse_args()
    n = args.points
    dev = torch.device("cuda", 0)
    ctx = pcv.Context(0)
    ctx.set_profiling(True)
    st = os.statvfs(args.tmp)
    if st.f_bavail * st.f_frsize < 3 * (n * 40 + 4096):  # a small tmpfs: the system's temporary directory instead
        args.tmp = tempfile.gettempdir()
    tmp = tempfile.mkdtemp(prefix="las_write_bench_", dir=args.tmp)
    out = {"tool": "tools/las_write_bench.py", "build_hash": build_hash(), "device": torch.cuda.get_device_name(0), "points": n, "runs": args.runs,
           "tmp": args.tmp, "hbm_peak_gb_per_s": HBM_PEAK_GBS}

    # ---- the octree ----
    x, y, z, rgb = make_cloud(torch, n, seed=1, device=dev)
    tree = ctx.build(0.001, None, x, y, z, rgb)
    del x, y, z, rgb
    torch.cuda.empty_cache()
    nodes = [tree.node(i) for i in range(tree.num_nodes)]
    node_bytes = int(sum(nd.num_points * (SRC_BYTES[nd.encoding] + 3) for nd in nodes)) + n  # .xyz, .rgb and one keep flag a point
    bmin = tree.meta()["bbox_min"]
    batch = tree.query_batch(ctx.shapes([("all",)]))
    out["octree_all"] = measure(ctx, batch, (2, 7), tuple(float(np.floor(v)) for v in bmin), {2: node_bytes, 7: node_bytes}, node_bytes, tmp,
                                args.runs, True)
    batch.free()
    tree.free()
    ctx.trim()

    # ---- the S2 cloud ----
    rot, ground = synthetic.ecef_from_local(37.407204, -122.147604)
    origin = ground + 1500.0 * rot[:, 2] - 500.0
    x, y, z, rgb = make_cloud(torch, n, seed=1, device=dev, offset=tuple(float(c) for c in origin))
    gen = torch.Generator(device=dev).manual_seed(7)
    cls = torch.randint(0, 32, (n,), dtype=torch.uint8, device=dev, generator=gen)
    ret = torch.randint(1, 6, (n,), dtype=torch.uint8, device=dev, generator=gen)
    gps = torch.rand((n,), dtype=torch.float64, device=dev, generator=gen) * 4e8
    lo = tuple(float(torch.floor(v.min())) for v in (x, y, z))
    torch.cuda.synchronize()
    cloud = ctx.s2_split(dict(x=x, y=y, z=z, color=rgb, attributes=dict(classification=cls, return_number=ret, gps_time=gps)), args.level)
    del x, y, z, rgb, cls, ret, gps
    torch.cuda.empty_cache()
    batch = cloud.query_batch(ctx.shapes([("all",)]))
    base = n * (24 + 3 + 4 + 8)  # position, colour, flag, scanned offset
    out["s2_all"] = measure(ctx, batch, (3,), lo, {3: base + n * 10}, base + n * 10, tmp, args.runs, False)
    batch.free()
    cloud.free()
    os.rmdir(tmp)
    print(json.dumps(out))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    ctx.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
