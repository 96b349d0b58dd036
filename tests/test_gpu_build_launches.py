"""The launch sequence of the octree build, pinned: which kernels a build launches and how often, and what
build_info() reports, for the four paths through the build's host code — the single-chain build without and with the
depth-binned pass, the exact pipeline, and a build that computes its own bounding box (K1 runs inside the build).
tests/golden/build_launches.json was recorded on an MI355X at the commit named inside it, before the build's host code
was split into files; it is a record of that commit and is not regenerated from later code. (Recording: run this file
with PCV_RECORD_BUILD_LAUNCHES=<commit hash> at that commit.)"""
import json
import os

import numpy as np
import pytest

import point_cloud_viewer_amd as pcv
from point_cloud_viewer_amd import synthetic

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "build_launches.json")
RECORD = os.environ.get("PCV_RECORD_BUILD_LAUNCHES", "")

SMALL = dict(n=200_000, cap=300, clusters=4, extent=40.0, sigma=(0.005, 1.0), seed=5, with_int=False)  # < 2^20: no depth grid
LARGE = dict(n=1_300_000, cap=30_000, clusters=7, extent=220.0, sigma=(0.1, 7.0), seed=7, with_int=True)  # depth-binned pass
BUILDS = {  # name: (cloud, bounding box given, keyword arguments of Context.build)
    "single_chain": (SMALL, True, dict(single_chain=True, check_resolve=True)),
    "exact": (SMALL, True, dict(single_chain=False)),
    "device_bbox": (SMALL, False, dict(single_chain=True, check_resolve=True)),
    "depth_binned_intensity": (LARGE, True, dict(single_chain=True)),
}


@pytest.fixture(scope="module")
def ctx():
    c = pcv.Context(0)
    c.set_profiling(1)
    yield c
    c.close()


@pytest.fixture(scope="module")
def golden():
    if RECORD:
        return {"commit": RECORD, "builds": {}}
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize("name", list(BUILDS))
def test_build_launches_the_recorded_kernels(ctx, golden, name):
    cloud, with_box, kwargs = BUILDS[name]
    n = cloud["n"]
    x, y, z, rgb, bmin, bmax = synthetic.gaussian_clusters(n, seed=cloud["seed"], num_clusters=cloud["clusters"],
                                                           extent=cloud["extent"], sigma_range=cloud["sigma"])
    inten = (np.arange(n) % 509).astype(np.float32) * 0.5 if cloud["with_int"] else None
    ctx.reset_kernel_stats()
    t = ctx.build(0.001, pcv.Aabb(bmin, bmax) if with_box else None, x, y, z, rgb, inten, max_points_per_node=cloud["cap"], **kwargs)
    ctx.synchronize()
    launches = {k: int(v[0]) for k, v in sorted(ctx.kernel_stats().items()) if v[0] > 0}
    info = {k: (bool(v) if isinstance(v, bool) else int(v)) for k, v in t.build_info().items() if not k.endswith("_ms")}
    t.free()
    print(name, "launches:", launches)
    print(name, "build_info:", info)
    if RECORD:
        golden["builds"][name] = {"launches": launches, "build_info": info}
        if len(golden["builds"]) == len(BUILDS):
            with open(GOLDEN, "w") as f:
                json.dump(golden, f, indent=1, sort_keys=True)
                f.write("\n")
        return
    want = golden["builds"][name]
    assert launches == want["launches"]
    assert info == want["build_info"]
