#!/usr/bin/env python
"""xray parent levels measured (GPU box): the config-2 cloud (100 M Gaussian-cluster points, bench.py's generator and
seed) built once, its xray leaf level (tile_size_px = 256, pixel_size_m = 0.1, strategy xray), then
XrayTiles.build_parents on a fresh leaf level per step: median wall ms of build_parents, the summed kernel ms of
xray_parent_kernel (one launch per level; the profiler sums a call's launches, so per level the mean is given next to
each level's parent count), the parent count, bytes moved against the 8 TB/s HBM peak, and the median wall ms of
XrayTiles.write into a temporary directory.

Comparator: the numpy restatement (tests/xray_pyramid_oracle.py: build_parent + the 2:1 Lanczos3 resize) on a sample of
parents, extrapolated to all parents and labelled as such; the sampled parents must equal the device's bytes.
Prints one JSON line and writes it to --out.

usage: python tools/xray_pyramid_bench.py [--points N] [--steps K] [--sample-parents P] [--out FILE]"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import point_cloud_viewer_amd as pcv  # noqa: E402
import xray_pyramid_oracle as P  # noqa: E402
from bench import build_hash, make_cloud  # noqa: E402

HBM_PEAK = 8.0e12
TILE, PIXEL = 256, 0.1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=100_000_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--sample-parents", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09_xray_pyramid_bench.json"))
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    ctx = pcv.Context(0)
    x, y, z, rgb = make_cloud(torch, args.points, seed=1, device=dev)
    tree = ctx.build(0.001, None, x, y, z, rgb)
    del x, y, z, rgb
    torch.cuda.empty_cache()
    ctx.set_profiling(True)
    walls, kms, write_ms = [], [], []
    tmp = tempfile.mkdtemp(prefix="xray_pyramid_bench_")
    try:
        for step in range(args.steps + 1):  # the first is a warm-up
            xt = tree.xray_tiles(TILE, PIXEL, "xray")
            ctx.synchronize()
            ctx.reset_kernel_stats()
            t0 = time.perf_counter()
            xt.build_parents()
            wall = (time.perf_counter() - t0) * 1e3
            st = ctx.kernel_stats()["xray_parent_kernel"]
            t0 = time.perf_counter()
            xt.write(os.path.join(tmp, "q"))
            wms = (time.perf_counter() - t0) * 1e3
            if step:
                walls.append(wall)
                kms.append(st[1])
                write_ms.append(wms)
                launches = st[0]
            if step < args.steps:
                xt.free()
        files = len(os.listdir(os.path.join(tmp, "q")))
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    ctx.set_profiling(False)
    level, index = xt.nodes()
    nc = xt.num_created
    parents = int(level.size - nc)
    per_level = {int(l): int((level[nc:] == l).sum()) for l in sorted(set(level[nc:].tolist()), reverse=True)}
    kernel_ms = float(np.median(kms))
    # HBM bytes: each parent reads its four children's pixels (16 B per output pixel, missing children read nothing) and
    # writes its own (4 B per pixel); LDS reuse means each input pixel is fetched once per output block (+ block halos)
    bytes_moved = parents * TILE * TILE * 4 * (4 + 1)
    # comparator: the restatement on a sample of parents, extrapolated
    sample = np.linspace(nc, level.size - 1, min(args.sample_parents, parents)).astype(int) if parents else np.zeros(0, int)
    pos = {(int(l), int(i)): k for k, (l, i) in enumerate(zip(level.tolist(), index.tolist()))}
    bg = P.background("white")
    tp = P.taps(TILE)
    t_np, match = 0.0, True
    for k in sample:
        lv, ix = int(level[k]), int(index[k])
        ch = []
        for c in range(4):
            j = pos.get((lv + 1, (ix << 2) + c))
            ch.append(xt.node_images(j, 1)[0] if j is not None else None)
        t0 = time.perf_counter()
        want = P.resize_half(P.build_parent(ch, TILE, bg), tp)
        t_np += time.perf_counter() - t0
        match &= bool(np.array_equal(want, xt.node_images(int(k), 1)[0]))
    np_ms = t_np * 1e3 / max(len(sample), 1) * parents
    out = {"tool": "tools/xray_pyramid_bench.py", "build_hash": build_hash(), "device": torch.cuda.get_device_name(0),
           "cloud": f"config 2: {args.points} Gaussian-cluster points (bench.make_cloud, seed 1), resolution 0.001",
           "tile_size_px": TILE, "pixel_size_m": PIXEL, "strategy": "xray", "deepest_level": xt.deepest_level,
           "leaf_tiles_created": nc, "parents": parents, "parents_per_level": per_level,
           "build_parents_wall_ms": round(float(np.median(walls)), 3), "build_parents_wall_ms_all": [round(w, 3) for w in walls],
           "parent_kernel_ms": round(kernel_ms, 4), "parent_kernel_launches": int(launches),
           "parent_kernel_ms_mean_per_level": round(kernel_ms / max(int(launches), 1), 4),
           "parent_hbm_bytes": bytes_moved, "parent_share_of_hbm_peak": round(bytes_moved / (kernel_ms * 1e-3) / HBM_PEAK, 3) if kernel_ms else None,
           "write_wall_ms": round(float(np.median(write_ms)), 1), "files_written": files,
           "numpy_restatement": {"label": f"EXTRAPOLATED from {len(sample)} parents: build_parent + resize_half in numpy per parent",
                                 "wall_ms_extrapolated": round(np_ms, 1), "sample_equal_to_device": match},
           "restatement_vs_device_wall": round(np_ms / float(np.median(walls)), 1) if walls else None}
    xt.free()
    tree.free()
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(out, indent=1) + "\n")
    ctx.close()
    return 0 if match else 1


if __name__ == "__main__":
    sys.exit(main())
