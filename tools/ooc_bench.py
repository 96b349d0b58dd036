#!/usr/bin/env python
"""The out-of-core build measured (GPU box): the config-3 cloud (64 Gaussian clusters, 1 B points by default) generated in
500 000-point batches from the seed — never whole on the host — through pcv_ooc_* to a directory, timed from the first append to
meta.pb; then the same batches through the in-core ingest, and the two directories compared by one digest over (node name, kind,
bytes), meta.pb included. Prints one JSON line.

usage: python tools/ooc_bench.py [--points N] [--pass-points M] [--resolution R] [--seed S] [--dir D] [--no-parity]"""
import argparse
import hashlib
import json
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import point_cloud_viewer_amd as pcv  # noqa: E402
from bench import CLOUD_BLOCK, build_hash, make_cloud_slice  # noqa: E402

BATCH = 500_000


def dir_digest(path):
    """blake2b-128 over (node name, kind, bytes) of every file of an octree directory, meta.pb included, in name order."""
    h = hashlib.blake2b(digest_size=16)
    for name in sorted(os.listdir(path)):
        stem, _, kind = name.rpartition(".")
        h.update(f"{stem}\0{kind}\0".encode())
        with open(os.path.join(path, name), "rb") as f:
            while True:
                b = f.read(1 << 24)
                if not b:
                    break
                h.update(b)
    return h.hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1_000_000_000)
    ap.add_argument("--pass-points", type=int, default=0, help="max_points_per_pass (default: points / 8, >= 8 passes)")
    ap.add_argument("--resolution", type=float, default=0.001)
    ap.add_argument("--seed", type=int, default=2, help="seed of the config-3 cloud")
    ap.add_argument("--dir", default=None, help="where the directories are written (default: the temp dir)")
    ap.add_argument("--no-parity", action="store_true", help="skip the in-core build and the digest comparison")
    args = ap.parse_args()
    total = args.points
    per_pass = args.pass_points or -(-total // 8)
    dev = torch.device("cuda", 0)

    def batches():  # device-generated blocks of the one cloud, handed to the host as PointsBatches
        for b0 in range(0, total, CLOUD_BLOCK):
            x, y, z, rgb = make_cloud_slice(torch, total, b0, min(CLOUD_BLOCK, total - b0), seed=args.seed, device=dev)
            pos, col = torch.stack([x, y, z], dim=1).cpu().numpy(), rgb.cpu().numpy()
            for at in range(0, pos.shape[0], BATCH):
                yield pos[at:at + BATCH], col[at:at + BATCH]

    lo = torch.full((3,), float("inf"), dtype=torch.float64, device=dev)
    hi = -lo
    for b0 in range(0, total, CLOUD_BLOCK):  # the bounding box up front: the out-of-core stream is read once
        x, y, z, _ = make_cloud_slice(torch, total, b0, min(CLOUD_BLOCK, total - b0), seed=args.seed, device=dev)
        p = torch.stack([x, y, z], dim=1)
        lo, hi = torch.minimum(lo, p.min(dim=0).values), torch.maximum(hi, p.max(dim=0).values)
    bbox = pcv.Aabb(lo.cpu().numpy(), hi.cpu().numpy())
    ctx = pcv.Context(0)
    work = tempfile.mkdtemp(prefix="pcv_ooc_bench_", dir=args.dir)
    out = {"mode": "out_of_core", "points": total, "max_points_per_pass": per_pass, "batch": BATCH, "resolution": args.resolution,
           "build_hash": build_hash()}
    try:
        gen_s = 0.0
        ooc = ctx.out_of_core(args.resolution, bbox, False, per_pass)
        t0 = time.perf_counter()
        it = batches()
        while True:
            g0 = time.perf_counter()
            nxt = next(it, None)
            gen_s += time.perf_counter() - g0
            if nxt is None:
                break
            ooc.append(nxt[0], nxt[1])
        st = ooc.finish(os.path.join(work, "ooc"))
        wall = time.perf_counter() - t0
        out["e2e_s"] = round(wall, 3)
        out["generate_s"] = round(gen_s, 3)
        out["points_per_s"] = round(total / wall, 1)
        out["points_per_s_without_generation"] = round(total / max(wall - gen_s, 1e-9), 1)
        out["stats"] = {k: (round(v, 3) if isinstance(v, float) else v) for k, v in st.items()}

        def gbs(nbytes, ms):
            return round(nbytes / (ms * 1e6), 2) if ms > 0 else None

        out["link"] = {"h2d_GBps": gbs(st["h2d_bytes"], st["h2d_ms"]), "d2h_GBps": gbs(st["d2h_bytes"], st["d2h_ms"]),
                       "model": "per point (Float32 level 1): 27 B of input + 2 x 16 B of partition uploads H2D, 16 B (+1 B of "
                                "octant digits) of spill D2H, at the 46-52 GB/s large DMAs reach (DESIGN.md section 6)",
                       "model_h2d_bytes": total * (27 + 32), "model_d2h_bytes": total * 17}
        out["ooc_digest"] = dir_digest(os.path.join(work, "ooc"))
        shutil.rmtree(os.path.join(work, "ooc"))
        if not args.no_parity:
            ing = ctx.ingest(total, False)
            for pos, col in batches():
                ing.append(pos, col)
            tree = ing.finish(args.resolution, bbox)
            tree.write_dir(os.path.join(work, "in"))
            out["in_core_nodes"] = int(tree.num_nodes)
            tree.free()
            out["in_core_digest"] = dir_digest(os.path.join(work, "in"))
            out["digest_equal"] = out["in_core_digest"] == out["ooc_digest"]
    finally:
        shutil.rmtree(work, ignore_errors=True)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
