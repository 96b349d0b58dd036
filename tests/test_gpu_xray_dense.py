"""`colored` where a pixel holds more than 2^24 points: alpha is a sum of n ones in f32, which stops at 2^24, over
`n as f32` — 240 for the 2^24 + 2^20 points of the column here — while the channel sums stay exact integers. Byte for
byte against xray_truth's exact-integer oracle. The arrival-order oracle walks a pixel point by point and is not run here.

The oracle takes the points as they were given to the builder, not as the octree decodes them: every point sits at least
a tenth of a pixel (25 mm) inside its pixel and the octree's resolution is 1 mm, so no point can change pixel."""
import time

import numpy as np
import pytest

import point_cloud_viewer_amd as pcv
import xray_oracle as X
import xray_truth as T
from test_gpu_query import ctx  # noqa: F401  (module fixture)

pytestmark = pytest.mark.gpu
W, PX = 64, 0.25
SLAB = 1 << 20
SLABS = 17  # 17 x 2^20 = 2^24 + 2^20 points in one pixel column, a constant colour per z slab
COLUMN = (5.1, 7.1)


def slab_color(k):
    return 15 * k, 255 - 15 * k, (37 * k) % 256


@pytest.fixture(scope="module")
def dense(ctx):  # noqa: F811
    t0 = time.time()
    n = SLABS * SLAB
    rng = np.random.default_rng(17)
    m = 2000  # ordinary pixels beside the column, each point within 0.3 pixels of its pixel's centre
    ox = (rng.integers(32, 60, m) + 0.5 + rng.uniform(-0.3, 0.3, m)) * PX
    oy = (rng.integers(4, 60, m) + 0.5 + rng.uniform(-0.3, 0.3, m)) * PX
    x = np.concatenate([np.full(n, COLUMN[0]), ox, [0.0, 15.9]])
    y = np.concatenate([np.full(n, COLUMN[1]), oy, [0.0, 0.0]])  # the two box pins lie on y == 0: image row H, never drawn
    z = np.concatenate([(np.arange(n) + 0.5) * (64.0 / n), rng.uniform(0.0, 64.0, m), [0.0, 64.0]])  # spread in z: a shallow octree
    rgb = np.empty((n + m + 2, 3), np.uint8)
    rgb[:n] = np.array([slab_color(k) for k in range(SLABS)], np.uint8)[np.arange(n) >> 20]
    rgb[n:] = rng.integers(0, 256, (m + 2, 3))
    bmin, bmax = np.array([0.0, 0.0, 0.0]), np.array([15.9, 15.0, 64.0])
    tree = ctx.build(0.001, pcv.Aabb(bmin, bmax), x, y, z, rgb, max_points_per_node=100_000)
    yield dict(tree=tree, x=x, y=y, z=z, rgb=rgb, bmin=bmin, bmax=bmax, n=n, t0=t0)
    tree.free()


def test_colored_beyond_2_pow_24_points_in_a_pixel(dense):
    d = dense
    g = X.leaf_geometry(W, PX, d["bmin"], d["bmax"])
    assert g["leaf_ids"] == ["r"]
    mn, mx = g["tile_bbox"][0]
    want, drawn = T.colored_image(d["x"], d["y"], d["z"], d["rgb"], mn, mx, W)
    xt = d["tree"].xray_tiles(W, PX, "colored")
    assert xt.created_ids == ["r"] and int(xt.drawn[0]) == drawn == d["x"].size - 2 <= int(xt.kept[0])
    got = xt.images()[0]
    xt.free()
    # the column's pixel by hand: mean red 15 * (0 + .. + 16) / 17 = 120, green 255 - 120, alpha 2^24 / (17 x 2^20) * 255 = 240
    row, col = W - 1 - int(COLUMN[1] / PX), int(COLUMN[0] / PX)
    sums = [SLAB * sum(slab_color(k)[c] for k in range(SLABS)) for c in range(3)]
    by_hand = T.colored_rgba([sums[0]], [sums[1]], [sums[2]], [d["n"]])[0]
    assert by_hand.tolist()[:2] == [120, 135] and by_hand[3] == 240
    assert got[row, col].tolist() == want[row, col].tolist() == by_hand.tolist()
    assert np.array_equal(got, want), int((got != want).any(-1).sum())
    assert int((want[..., :3] != 255).any(-1).sum()) > 500  # the ordinary pixels beside it
    print(f"colored beyond 2^24: {W * W} pixels compared, all equal; {time.time() - d['t0']:.1f} s with the build")
