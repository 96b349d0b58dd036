"""colored_with_intensity and binning on the device (pcv_xray_run_ex, OctreeResult / Context .xray_tiles with
min_intensity / max_intensity / binning) against tests/xray_intensity_oracle.py: the created set, drawn and negative counts,
and every byte of every tile (the oracle takes the device's documented order: f32 sums in ascending (pixel, bin, value
bits) order, exact integer colour sums); binned colored; bytes independent of scheduling, tile grouping, the LDS limit of the
sorted accumulation and octree order; an edge cloud of negative, NaN and infinite intensities; two octrees; the quadtree
and its PNG files."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as O
import point_cloud_viewer_amd as pcv
import xray_intensity_oracle as I
import xray_pyramid_oracle as P
from point_cloud_viewer_amd import synthetic
from test_gpu_query import ctx, scene  # noqa: F401  (module fixtures)
from test_gpu_query_batch import scene_of
from test_gpu_xray import tree_points

pytestmark = pytest.mark.gpu
W, PX = 64, 0.25
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def tp(scene):  # noqa: F811
    return tree_points(scene)


def run(tree, strategy, **kw):
    xt = tree.xray_tiles(kw.pop("tile_size_px", W), kw.pop("pixel_size_m", PX), strategy, **kw)
    imgs = xt.images() if xt.num_created else np.zeros((0, W, W, 4), np.uint8)
    got = {n: (imgs[i], int(xt.drawn[i]), int(xt.negative[i])) for i, n in enumerate(xt.created_ids)}
    xt.free()
    return got


def check(got, want):
    """byte for byte: the sorted strategies reduce in key order, which the oracle restates"""
    assert set(got) == set(want)
    total = 0
    for name, (img, drawn, neg) in want.items():
        g = got[name][0]
        assert got[name][1] == drawn and got[name][2] == neg, name
        d = np.abs(g.astype(int) - img.astype(int))
        assert d.max() == 0, (name, int((d > 0).any(-1).sum()), int(d.max()))
        total += int((img[..., 3] == 255).sum())
    assert total > 0
    print(f"sorted: {len(want)} tiles, {total} drawn pixels, all equal")


def digest(got):
    return hashlib.sha256(b"".join(n.encode() + got[n][0].tobytes() for n in sorted(got))).hexdigest()


@pytest.mark.parametrize("lo,hi", [(0.0, 250.0), (10.0, 200.0), (100.0, 100.5), (0.0, 1.0)])
@pytest.mark.parametrize("bin_size", [None, 16.0])
def test_colored_with_intensity_matches_oracle(scene, tp, lo, hi, bin_size):  # noqa: F811
    binning = ("intensity", bin_size) if bin_size is not None else None
    got = run(scene["tree"], "colored_with_intensity", min_intensity=lo, max_intensity=hi, binning=binning)
    want, _ = I.xray_tiles([tp], W, PX, "colored_with_intensity", lo, hi, bin_size)
    assert 8 < len(want) < 64 and all(v[2] == 0 for v in want.values())
    check(got, want)


@pytest.mark.parametrize("bin_size", [16.0, 1e-3])
def test_binned_colored_matches_oracle(scene, tp, bin_size):  # noqa: F811
    got = run(scene["tree"], "colored", binning=("intensity", bin_size))
    want, _ = I.xray_tiles([tp], W, PX, "colored", bin_size=bin_size)
    check(got, want)
    # one bin (every i % 251 / 1e30 truncates to 0) through xray_sorted equals unbinned colored through xray_accum byte for
    # byte: the same exact channel sums, rounded once
    plain = run(scene["tree"], "colored")
    assert digest(run(scene["tree"], "colored", binning=("intensity", 1e30))) == digest(plain)
    # binning ignored where the strategy never reads it
    for strategy in ("xray", ("height_stddev", 1.5, "jet")):
        a, b = run(scene["tree"], strategy), run(scene["tree"], strategy, binning=("intensity", bin_size))
        assert set(a) == set(b) and all(np.array_equal(a[n][0], b[n][0]) for n in a)


def dense_scene(ctx):  # noqa: F811
    """the scene's distribution plus 60 000 points in a 1 m square: buckets far above the LDS limit"""
    x, y, z, rgb, bmin, bmax = synthetic.gaussian_clusters(200_000, seed=4, num_clusters=5, extent=100.0, sigma_range=(0.5, 6.0))
    rng = np.random.default_rng(7)
    c = np.array([x[0], y[0], z[0]])
    n = 60_000
    x = np.concatenate([x, c[0] + rng.uniform(0, 1.0, n)])
    y = np.concatenate([y, c[1] + rng.uniform(0, 1.0, n)])
    z = np.concatenate([z, c[2] + rng.uniform(0, 1.0, n)])
    rgb = np.concatenate([rgb, rng.integers(0, 256, (n, 3)).astype(np.uint8)])
    inten = (np.arange(x.size) % 251).astype(np.float32)
    bmin, bmax = np.minimum(bmin, [x.min(), y.min(), z.min()]), np.maximum(bmax, [x.max(), y.max(), z.max()])
    return dict(scene_of(ctx, x, y, z, rgb, inten, bmin, bmax, 2000), x=x, y=y, z=z, rgb=rgb, inten=inten)


CHILD = ("import sys, json, hashlib; sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + '/tests')\n"
         "import numpy as np, point_cloud_viewer_amd as pcv\n"
         "x, y, z, rgb, inten, lo, hi = (np.load(sys.argv[2])[k] for k in ('x', 'y', 'z', 'rgb', 'inten', 'lo', 'hi'))\n"
         "t = pcv.Context(0).build(0.001, pcv.Aabb(lo, hi), x, y, z, rgb, inten, max_points_per_node=2000)\n"
         "out = {}\n"
         "for key, kw in json.loads(sys.argv[3]).items():\n"
         "    xt = t.xray_tiles(%d, %r, kw.pop('strategy'), binning=tuple(kw.pop('binning')) if kw.get('binning') else None, **kw)\n"
         "    im = xt.images()\n"
         "    out[key] = hashlib.sha256(b''.join(n.encode() + im[i].tobytes() for i, n in sorted(enumerate(xt.created_ids), key=lambda e: e[1]))).hexdigest()\n"
         "print('DIGESTS', json.dumps(out))\n") % (W, PX)


def test_determinism_grouping_and_global_path(ctx, tmp_path):  # noqa: F811
    s = dense_scene(ctx)
    tpp = tree_points(s)
    tree = s["tree"]
    cases = {"cwi": dict(strategy="colored_with_intensity", min_intensity=0.0, max_intensity=250.0),
             "cwi_bin": dict(strategy="colored_with_intensity", min_intensity=0.0, max_intensity=250.0, binning=["intensity", 1e-3]),
             "col_bin": dict(strategy="colored", binning=["intensity", 1e-3])}
    ref = {}
    for key, kw in cases.items():
        kw = dict(kw)
        strategy, binning = kw.pop("strategy"), kw.pop("binning", None)
        binning = tuple(binning) if binning else None
        a = run(tree, strategy, binning=binning, **kw)
        b = run(tree, strategy, binning=binning, **kw)
        c = run(tree, strategy, binning=binning, max_workspace_bytes=1_000_000, **kw)
        assert digest(a) == digest(b) == digest(c), key
        ref[key] = digest(a)
        want, _ = I.xray_tiles([tpp], W, PX, strategy, kw.get("min_intensity", 0.0), kw.get("max_intensity", 1.0),
                               binning[1] if binning else None)
        check(a, want)
        # the 60 000 points of the 1 m square fall into at most 4 buckets of 8 m, so one holds more than 8 192 records,
        # the LDS limit: the global path ran
        assert sum(v[1] for v in want.values()) > 60_000 and max(v[1] for v in want.values()) > 15_000
    # the experiment build with the LDS limit forced down to 64 records: nearly every bucket takes the global path
    np.savez(tmp_path / "cloud.npz", x=s["x"], y=s["y"], z=s["z"], rgb=s["rgb"], inten=s["inten"], lo=s["bmin"], hi=s["bmax"])
    import json
    env = dict(os.environ, PCV_HIP_LIBRARY="exp", PCV_XRAY_SORT_LDS_RECORDS="64")
    out = subprocess.run([sys.executable, "-c", CHILD, ROOT, str(tmp_path / "cloud.npz"), json.dumps(cases)], env=env,
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    line = [ln for ln in out.stdout.splitlines() if ln.startswith("DIGESTS ")][0]
    assert json.loads(line[len("DIGESTS "):]) == ref
    tree.free()


def test_edge_intensities(ctx):  # noqa: F811
    """one point per pixel on a grid over 2 x 2 tiles, intensities from a list of special values; tile r0 holds negatives"""
    edge = W * PX
    gx, gy = np.meshgrid(np.arange(0.0, 2 * edge, PX) + PX / 2, np.arange(0.0, 2 * edge, PX) + PX / 2)
    x, y = gx.ravel(), gy.ravel()
    z = np.full(x.size, 4.0)
    special = np.array([0.0, -0.0, 1.0, 5.0, 5.5, 6.0, 100.0, 250.0, np.nan, np.inf, 3e38, 1e-40, 7.25, 0.5], np.float32)
    inten = special[np.arange(x.size) % special.size]
    # negatives (and -inf) only in the tile at min x, min y (r0: y < edge, x < edge)
    lowtile = (x < edge) & (y < edge)
    neg_vals = np.array([-1.0, -np.inf, -1e-30], np.float32)
    idx = np.flatnonzero(lowtile)[::5]
    inten[idx] = neg_vals[np.arange(idx.size) % 3]
    p = np.concatenate([np.stack([x, y, z], 1), [[0.0, 0.0, 0.0], [2 * edge - 1e-9, 2 * edge - 1e-9, 8.0]]])
    inten = np.concatenate([inten, [2.0, 2.0]]).astype(np.float32)
    rgb = np.random.default_rng(3).integers(0, 256, (p.shape[0], 3)).astype(np.uint8)
    s = scene_of(ctx, *(np.ascontiguousarray(p[:, a]) for a in range(3)), rgb, inten, p.min(0), p.max(0), 20_000)
    tpp = tree_points(s)
    for lo, hi in ((0.0, 250.0), (5.0, 6.0), (5.0, 5.5), (10.0, 3.0), (np.nan, 100.0), (0.0, np.nan), (0.0, 1.0)):
        for bin_size in (None, 0.0, np.nan, 2.0):
            binning = ("intensity", bin_size) if bin_size is not None else None
            got = run(s["tree"], "colored_with_intensity", min_intensity=lo, max_intensity=hi, binning=binning)
            want, _ = I.xray_tiles([tpp], W, PX, "colored_with_intensity", lo, hi, bin_size)
            assert sum(v[2] for v in want.values()) == idx.size
            # one point per pixel: every mean is exact, so every pixel is, in tiles with and without negatives
            check(got, want)
            neg_tiles = {n for n, v in want.items() if v[2]}
            assert neg_tiles == {"r0"}
        got = run(s["tree"], "colored", binning=("intensity", 0.0))
        want, _ = I.xray_tiles([tpp], W, PX, "colored", bin_size=0.0)
        check(got, want)
        assert all(v[2] == 0 for v in got.values())
    s["tree"].free()


def test_two_octrees_and_order(ctx, scene, tp):  # noqa: F811
    s = scene
    n = s["x"].size
    inten = (np.arange(n) % 251).astype(np.float32)
    cut = n // 3
    # the same cloud split by point index into two octrees, through scene_of (which keeps the oracle's points)
    rgb = np.random.default_rng(2).integers(0, 256, (n, 3)).astype(np.uint8)
    sa = scene_of(ctx, s["x"][:cut], s["y"][:cut], s["z"][:cut], rgb[:cut], inten[:cut], s["bmin"], s["bmax"], 2000)
    sb = scene_of(ctx, s["x"][cut:], s["y"][cut:], s["z"][cut:], rgb[cut:], inten[cut:], s["bmin"], s["bmax"], 2000)
    parts = [sa["tree"], sb["tree"]]
    kw = dict(min_intensity=10.0, max_intensity=240.0, binning=("intensity", 32.0))
    xt = ctx.xray_tiles(parts, W, PX, "colored_with_intensity", **kw)
    im = xt.images()
    got = {n: (im[i], int(xt.drawn[i]), int(xt.negative[i])) for i, n in enumerate(xt.created_ids)}
    xt.free()
    want, _ = I.xray_tiles([tree_points(sa), tree_points(sb)], W, PX, "colored_with_intensity", 10.0, 240.0, 32.0)
    check(got, want)
    xt = ctx.xray_tiles(parts[::-1], W, PX, "colored_with_intensity", **kw)
    im = xt.images()
    rev = {n: (im[i], 0, 0) for i, n in enumerate(xt.created_ids)}
    xt.free()
    assert digest(rev) == digest(got)
    for t in parts:
        t.free()


def test_sorted_kernel_in_the_stats(ctx, scene):  # noqa: F811
    """one xray_sorted launch per tile group, under its own name; the other strategies keep xray_accum"""
    ctx.set_profiling(True)
    try:
        for kw, sorted_launches in ((dict(strategy="colored_with_intensity", max_intensity=250.0), 1),
                                    (dict(strategy="colored", binning=("intensity", 8.0)), 1), (dict(strategy="colored"), 0)):
            ctx.reset_kernel_stats()
            run(scene["tree"], **kw)
            st = ctx.kernel_stats()
            assert st["xray_sorted_kernel"][0] == sorted_launches and st["xray_accum_kernel"][0] == 1 - sorted_launches, kw
    finally:
        ctx.set_profiling(False)


def test_quadtree_and_png(scene, tmp_path):  # noqa: F811
    xt = scene["tree"].xray_quadtree(W, PX, "colored_with_intensity", min_intensity=0.0, max_intensity=250.0,
                                     binning=("intensity", 8.0), background="transparent")
    leaves = xt.node_images(0, xt.num_created)
    idx = [int(xt.leaf_index[int(c)]) for c in xt.created]
    want, _ = P.pyramid(dict(zip(idx, leaves)), xt.deepest_level, 0, W, "transparent")
    level, index = xt.nodes()
    nodes = list(zip(level.tolist(), index.tolist()))
    got = xt.node_images()
    assert len(nodes) > xt.num_created
    for k, nd in enumerate(nodes):
        assert np.array_equal(got[k], want[nd]), nd
    xt.write(tmp_path / "q")
    for k, (lv, ix) in enumerate(nodes):
        name = "r" + "".join(str((ix >> (2 * l)) & 3) for l in range(lv - 1, -1, -1))
        assert np.array_equal(P.read_png((tmp_path / "q" / f"{name}.png").read_bytes()), got[k]), name
    xt.free()
