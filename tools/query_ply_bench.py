#!/usr/bin/env python
"""Query results as PLY files, measured (GPU box; there is no CPU fallback). Three results:
  octree_all    AllPoints over the config-2 tree (100 M Gaussian-cluster points, bench.py's generator and seed 1, colour);
  octree_tiles  a 64 x 64 grid of AABB tiles over the same tree (x and y split, z whole), as xray's tile generation issues them;
  s2_all        AllPoints over the same points placed in ECEF (tools/s2_attr_bench.py's cloud) and split into S2 cells at
                level 20, with one U8 and one I64 extra: rows of 24 + 3 + 1 + 8 = 36 bytes.
Four legs per result, one process, a warm-up of all four and then --runs rounds in which they alternate; medians and spreads:
  (a) rows      ply_rows into a device buffer: wall time, and ply_rows_kernel alone (ctx.kernel_stats) over the bytes it reads
                and writes, computed from counts, against the 8 TB/s HBM peak;
      compact   pcv_query_batch_points / pcv_s2_query_points (+ pcv_s2_query_attribute per extra) of the same range into device
                buffers: the compaction moves the same payload into planes; packer kernel time / compaction kernel time is the
                ratio the README quotes;
  (b) file      write_ply onto tmpfs (the pipeline: pack, copy, pwrite in pieces);
  (c) by_hand   what a user did before write_ply existed: points() (+ attribute()) to host arrays, a packed numpy structured
                array filled from them, the header and tofile — to the same tmpfs. Its file is compared with (b)'s, byte for byte.
Prints one JSON line and writes it to --out.

usage: python tools/query_ply_bench.py [--points N] [--tiles T] [--runs R] [--chunk-points C] [--tmp DIR] [--out FILE]"""
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
from bench import build_hash, make_cloud  # noqa: E402
from point_cloud_viewer_amd import synthetic  # noqa: E402

HBM_PEAK = 8.0e12
PACK = "ply_rows_kernel"
COMPACT = {"octree": ("batch_compact_kernel",), "s2": ("s2_gather_points_kernel", "s2_attr_gather_points_kernel")}


def kernel_ms(ctx, names):
    st = ctx.kernel_stats()
    return sum(st[k][1] for k in names if k in st)


def spread(values):
    v = np.asarray(values, dtype=np.float64)
    return dict(median=round(float(np.median(v)), 3), min=round(float(v.min()), 3), max=round(float(v.max()), 3), runs=[round(float(t), 3) for t in v])


def packer_bytes(kind, batch, tree_or_cloud, stride):
    """(read, written) by the packer, from counts: the flags of every candidate, the source bytes of every kept point, the rows."""
    _, owner, off = batch.segments()
    kept = np.diff(off.astype(np.int64))
    if kind == "octree":
        m = tree_or_cloud.num_nodes
        npts = np.array([tree_or_cloud.node(i).num_points for i in range(m)], dtype=np.int64)
        bpc = np.array([{1: 1, 2: 2, 3: 4, 4: 8}[tree_or_cloud.node(i).encoding] for i in range(m)], dtype=np.int64)
        read = int(npts[owner].sum()) + int((kept * 3 * bpc[owner]).sum()) + int(kept.sum()) * (stride - 24)
    else:
        sizes = tree_or_cloud.cells[1].astype(np.int64)
        read = int(sizes[owner].sum()) * 12 + int(kept.sum()) * stride  # a u32 flag and a u64 offset per candidate
    return read, int(kept.sum()) * stride


def by_hand(batch, extras, layout, path):
    """points() / attribute() to the host, a packed structured array, the header, tofile."""
    pts = batch.points()
    rows = np.empty(pts["count"], dtype=layout["dtype"])
    rows["x"], rows["y"], rows["z"] = pts["x"], pts["y"], pts["z"]
    rgb = pts["rgb"].reshape(-1, 3)
    rows["red"], rows["green"], rows["blue"] = rgb[:, 0], rgb[:, 1], rgb[:, 2]
    for name in extras:
        rows[name] = batch.attribute(name)
    with open(path, "wb") as f:
        f.write(pcv.ply_header(layout["types"], len(rows)))
        rows.tofile(f)
        f.write(b"\n")
    return len(rows)


def measure(ctx, kind, label, batch, owner, extras, args, tmp):
    layout = batch.ply_layout()
    stride, n = layout["stride"], batch.num_points
    read, written = packer_bytes(kind, batch, owner, stride)
    dev = f"cuda:{ctx.device}"
    planes = dict(x=torch.empty(n, dtype=torch.float64, device=dev), y=torch.empty(n, dtype=torch.float64, device=dev),
                  z=torch.empty(n, dtype=torch.float64, device=dev), rgb=torch.empty((n, 3), dtype=torch.uint8, device=dev))
    columns = {name: torch.empty(n, dtype={"u8": torch.uint8, "i64": torch.int64}[owner.attributes[name]], device=dev) for name in extras}
    rows_dev = torch.empty((n, stride), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    fn_rows = batch._fn("ply_rows")
    f_file, f_hand = os.path.join(tmp, f"{label}_file.ply"), os.path.join(tmp, f"{label}_hand.ply")

    def leg_rows():
        s, r = pcv._lib.C.c_uint32(), pcv._lib.C.c_uint64()
        ctx._check(fn_rows(batch.handle, 0, batch.num_segments, None, 0, n * stride, pcv._lib.MEM_DEVICE, rows_dev.data_ptr(), pcv._lib.C.byref(s), pcv._lib.C.byref(r)))
        return PACK

    def leg_compact():
        batch.points(out=planes)
        for name, col in columns.items():
            ctx._check(ctx.lib.pcv_s2_query_attribute(batch.handle, name.encode(), 0, batch.num_segments, n, pcv._lib.MEM_DEVICE, col.data_ptr()))
        return COMPACT[kind]

    def leg_file():
        assert batch.write_ply(f_file, chunk_points=args.chunk_points) == n
        return None

    def leg_hand():
        assert by_hand(batch, extras, layout, f_hand) == n
        return None

    legs = dict(rows=leg_rows, compact=leg_compact, file=leg_file, by_hand=leg_hand)
    wall = {k: [] for k in legs}
    kern = {k: [] for k in ("rows", "compact")}
    for rnd in range(args.runs + 1):  # round 0 warms every leg up
        for name, leg in legs.items():
            ctx.reset_kernel_stats()
            t0 = time.perf_counter()
            kernels = leg()
            ctx.synchronize()
            ms = (time.perf_counter() - t0) * 1e3
            if rnd:
                wall[name].append(ms)
                if kernels:
                    kern[name].append(kernel_ms(ctx, (kernels,) if isinstance(kernels, str) else kernels))
    same = open(f_file, "rb").read() == open(f_hand, "rb").read() if n * stride < (8 << 30) else None
    os.unlink(f_file), os.unlink(f_hand)
    pack_ms, compact_ms = float(np.median(kern["rows"])), float(np.median(kern["compact"]))
    rec = dict(points=n, segments=batch.num_segments, stride=stride, columns=layout["names"], packer_bytes_read=read, packer_bytes_written=written,
               rows_wall_ms=spread(wall["rows"]), rows_kernel_ms=spread(kern["rows"]),
               rows_kernel_bytes_per_s=round((read + written) / (pack_ms * 1e-3), 1), rows_kernel_share_of_hbm_peak=round((read + written) / (pack_ms * 1e-3) / HBM_PEAK, 4),
               compact_wall_ms=spread(wall["compact"]), compact_kernel_ms=spread(kern["compact"]),
               packer_over_compaction_kernel_time=round(pack_ms / compact_ms, 3),
               packer_slower_beyond_spread=bool(min(kern["rows"]) > max(kern["compact"])),
               file_wall_ms=spread(wall["file"]), file_bytes_per_s=round((written + 1) / (float(np.median(wall["file"])) * 1e-3), 1),
               by_hand_wall_ms=spread(wall["by_hand"]), by_hand_over_file=round(float(np.median(wall["by_hand"])) / float(np.median(wall["file"])), 2),
               files_identical=same)
    del planes, columns, rows_dev
    torch.cuda.empty_cache()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100_000_000)
    ap.add_argument("--tiles", type=int, default=64)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--level", type=int, default=20)
    ap.add_argument("--chunk-points", type=int, default=0)
    ap.add_argument("--tmp", default="/dev/shm" if os.path.isdir("/dev/shm") else tempfile.gettempdir())
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "query_ply_bench.json"))
    args = ap.parse_args()
    n = args.points
    dev = torch.device("cuda", 0)
    ctx = pcv.Context(0)
    ctx.set_profiling(True)
    need = 2 * (n * 36 + 4096)  # the two files of the widest result stand side by side
    st = os.statvfs(args.tmp)
    if st.f_bavail * st.f_frsize < 2 * need:  # a small tmpfs (a container's 64 MiB /dev/shm): the system's temporary directory instead
        args.tmp = tempfile.gettempdir()
    tmp = tempfile.mkdtemp(prefix="query_ply_bench_", dir=args.tmp)
    out = {"tool": "tools/query_ply_bench.py", "build_hash": build_hash(), "device": torch.cuda.get_device_name(0), "points": n, "runs": args.runs,
           "tmp": args.tmp, "chunk_points": args.chunk_points or "default (2^20)", "hbm_peak_bytes_per_s": HBM_PEAK}

    # ---- the octree ----
    x, y, z, rgb = make_cloud(torch, n, seed=1, device=dev)
    tree = ctx.build(0.001, None, x, y, z, rgb)
    del x, y, z, rgb
    torch.cuda.empty_cache()
    meta = tree.meta()
    bmin, bmax = meta["bbox_min"], meta["bbox_max"]
    batch = tree.query_batch(ctx.shapes([("all",)]))
    out["octree_all"] = measure(ctx, "octree", "octree_all", batch, tree, [], args, tmp)
    batch.free()
    T = args.tiles
    tiles = [("aabb", [bmin[0] + (bmax[0] - bmin[0]) * i / T, bmin[1] + (bmax[1] - bmin[1]) * j / T, bmin[2]],
              [bmin[0] + (bmax[0] - bmin[0]) * (i + 1) / T, bmin[1] + (bmax[1] - bmin[1]) * (j + 1) / T, bmax[2]]) for i in range(T) for j in range(T)]
    batch = tree.query_batch(ctx.shapes(tiles))
    out["octree_tiles"] = measure(ctx, "octree", "octree_tiles", batch, tree, [], args, tmp)
    batch.free()
    tree.free()
    ctx.trim()

    # ---- the S2 cloud ----
    rot, ground = synthetic.ecef_from_local(37.407204, -122.147604)
    origin = ground + 1500.0 * rot[:, 2] - 500.0
    x, y, z, rgb = make_cloud(torch, n, seed=1, device=dev, offset=tuple(float(c) for c in origin))
    gen = torch.Generator(device=dev).manual_seed(7)
    ring = torch.randint(0, 256, (n,), dtype=torch.uint8, device=dev, generator=gen)
    stamp = torch.randint(0, 1 << 62, (n,), dtype=torch.int64, device=dev, generator=gen)
    torch.cuda.synchronize()
    cloud = ctx.s2_split(dict(x=x, y=y, z=z, color=rgb, attributes=dict(ring=ring, timestamp=stamp)), args.level)
    del x, y, z, rgb, ring, stamp
    torch.cuda.empty_cache()
    batch = cloud.query_batch(ctx.shapes([("all",)]))
    out["s2_all"] = measure(ctx, "s2", "s2_all", batch, cloud, ["ring", "timestamp"], args, tmp)
    batch.free()
    cloud.free()
    os.rmdir(tmp)
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    ctx.close()
    ok = all(out[k]["files_identical"] is not False for k in ("octree_all", "octree_tiles", "s2_all"))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
