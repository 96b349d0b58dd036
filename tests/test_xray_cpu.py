"""pcv_xray_leaf_tiles and pcv_xray_finalize (host code, no GPU) against xray_oracle's restatement of xray/src/generation.rs,
quadtree/src/lib.rs and colormap.rs; quadtree's own unit tests as known answers; parameter validation."""
import math

import numpy as np
import pytest

import point_cloud_viewer_amd as pcv
import xray_oracle as X
from point_cloud_viewer_amd import _lib as L

ISO = [4_000_123.25, -1_200_456.5, 4_700_789.75] + list(np.array([0.1, -0.2, 0.3, 0.9]) / math.sqrt(0.01 + 0.04 + 0.09 + 0.81))


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("case", [
    # (tile px, pixel m, bmin, bmax, iso, root)
    (256, 0.1, (0.0, 0.0, 0.0), (102.4, 51.2, 7.0), None, "r"),           # diag.x lands exactly on 4 tiles
    (256, 0.1, (-3.0, 1.0, -2.0), (20.0, 99.9, 5.0), None, "r"),          # diag.x < diag.y
    (64, 0.25, (0.3, -7.7, 1.0), (130.0, 110.0, 9.0), None, "r21"),       # a non-trivial root node
    (64, 0.25, (0.3, -7.7, 1.0), (130.0, 110.0, 9.0), None, "r3"),
    (100, 0.37, (10.0, 20.0, -5.0), (80.0, 60.0, 5.0), ISO, "r"),         # with an isometry (ECEF-sized translation)
    (32, 1.0, (0.0, 0.0, 0.0), (32.0, 32.0, 1.0), None, "r"),             # one tile: deepest level 0
])
def test_leaf_geometry_matches_restatement(case):
    W, px, bmin, bmax, iso, root = case
    got = pcv.xray_leaf_tiles(W, px, bmin, bmax, iso, root)
    want = X.leaf_geometry(W, px, bmin, bmax, iso, root)
    assert got["deepest_level"] == want["deepest_level"]
    assert same_bytes(got["rect"], want["rect"])
    assert got["leaf_ids"] == want["leaf_ids"]
    assert [int(i) for i in got["leaf_index"]] == want["leaf_index"]
    assert same_bytes(got["tile_bbox"], [list(a) + list(b) for a, b in want["tile_bbox"]])
    if iso is not None:
        assert same_bytes(got["query_obb"], [X.tile_obb(iso, a, b) for a, b in want["tile_bbox"]])
    # tiles tile the root node's rect: every leaf edge equals the rect edge / 2^(depth)
    depth = want["deepest_level"] - X.node_id(root)[0]
    assert len(got["leaf_ids"]) == 4 ** depth


def test_leaf_order_is_get_nodes_at_level_pop_order():
    got = pcv.xray_leaf_tiles(256, 0.1, (0, 0, 0), (50.0, 50.0, 1.0), None, "r")
    assert got["deepest_level"] == 1
    assert got["leaf_ids"] == ["r3", "r2", "r1", "r0"]
    boxes = got["tile_bbox"]
    assert boxes[0][0] == 25.6 and boxes[0][1] == 25.6 and boxes[3][0] == 0.0  # r3 = +x +y, r0 = the min corner


def test_quadtree_known_answers():
    # quadtree/src/lib.rs:363-398
    assert X.parent_id(*pcv.quadtree_node_id("r123210")) == pcv.quadtree_node_id("r12321")
    assert X.child_index(*pcv.quadtree_node_id("r123321")) == 1
    assert X.child_index(*pcv.quadtree_node_id("r123323")) == 3
    assert X.child_index(*pcv.quadtree_node_id("r")) is None
    for s in ("r", "r0", "r123323"):
        assert pcv.quadtree_node_name(*pcv.quadtree_node_id(s)) == s
    with pytest.raises(ValueError):
        pcv.quadtree_node_id("r4")


def test_xray_value_table():
    n = np.arange(1, 1026, dtype=np.float64)
    got = pcv.xray_finalize("xray", n)
    want = np.array([X.xray_value(int(k)) for k in n], dtype=np.uint8)
    assert np.array_equal(got[:, 0], want) and np.array_equal(got[:, 1], want) and np.array_equal(got[:, 2], want)
    assert np.all(got[:, 3] == 255)
    assert got[0, 0] == 255 and got[1023, 0] == 0 and got[1024, 0] == 0  # n = 1024: ln/ln = 1; n = 1025 saturates to 0
    assert tuple(pcv.xray_finalize("xray", [0.0])[0]) == (255, 255, 255, 0)  # no point: TRANSPARENT


def test_colormaps_at_breakpoints():
    vals = np.array([0.0, 1.0, 0.125, 0.25, 0.375, 0.5, 0.625, 0.75, 0.875, 1 / 3, 0.9999], dtype=np.float32)
    for fn, ref in (("jet", X.jet), ("purplish", X.purplish)):
        got = pcv.xray_finalize(fn, vals.astype(np.float64))
        assert np.array_equal(got, ref(vals)), fn
    # by hand: jet(0) = (base(-0.5), base(0), base(0.5)) = (0.5, 1, 0.5); jet(1) = (base(0.5), base(1), base(1.5)) = (0.5, 0, 0)
    assert tuple(pcv.xray_finalize("jet", [0.0])[0]) == (127, 255, 127, 255)
    assert tuple(pcv.xray_finalize("jet", [1.0])[0]) == (127, 0, 0, 255)
    assert tuple(pcv.xray_finalize("purplish", [0.0])[0]) == (204, 204, 255, 255)
    assert tuple(pcv.xray_finalize("purplish", [1.0])[0]) == (0, 0, 0, 255)


def test_to_u8_truncates_and_saturates():
    c = np.array([[0.5, 1.0, 0.999, 0.0], [-0.1, 2.0, np.nan, 0.502]], dtype=np.float64)
    got = pcv.xray_finalize("to_u8", c)
    assert tuple(got[0]) == (127, 255, 254, 0)
    assert tuple(got[1]) == (0, 255, 0, 128)
    assert np.array_equal(got, X.to_u8(*c.astype(np.float32).T))


def test_colored_mean_and_alpha():
    # alpha: a sum of n ones in f32 stops at 2^24; divided by `n as f32`
    for n in (1, 7, 1 << 24, (1 << 24) + 1, (1 << 24) + 3, 1 << 25):
        got = pcv.xray_finalize("colored", [[0.0, 0.0, 0.0, float(n)]])[0]
        want = X.sat_u8(np.float32(min(n, 1 << 24)) / np.float32(n) * np.float32(255))
        assert got[3] == want, n
    assert pcv.xray_finalize("colored", [[0.0, 0.0, 0.0, float(1 << 25)]])[0][3] == 127
    # exact sums: the mean of 3 points (10, 20, 30) on red is 20 -> 20 / 255 * 255 -> 19 or 20 as f32 rounds
    got = pcv.xray_finalize("colored", [[60.0, 3 * 255.0, 0.0, 3.0]])[0]
    assert got[1] == 255 and got[2] == 0 and got[0] in (19, 20)


def test_parameter_validation():
    with pytest.raises(pcv.PcvError, match="2\\^24"):  # 13 levels below the root: 4^13 leaves
        pcv.xray_leaf_tiles(1, 1.0, (0, 0, 0), (8192.0, 8192.0, 1.0))
    assert len(pcv.xray_leaf_tiles(1, 1.0, (0, 0, 0), (8192.0, 8192.0, 1.0), root_node_id="r000000")["leaf_ids"]) == 4 ** 7
    with pytest.raises(pcv.PcvError):
        pcv.xray_leaf_tiles(0, 1.0, (0, 0, 0), (1.0, 1.0, 1.0))
    with pytest.raises(pcv.PcvError):
        pcv.xray_leaf_tiles(64, 0.0, (0, 0, 0), (1.0, 1.0, 1.0))
    with pytest.raises(pcv.PcvError, match="outside"):
        pcv.xray_leaf_tiles(64, 1.0, (0, 0, 0), (100.0, 100.0, 1.0), root_node_id="r000")
    lib = L.load_library()
    assert lib.pcv_xray_finalize(99, 0, None, None) == L.PCV_E_INVALID
    assert lib.pcv_xray_run(None, None, None, None) == L.PCV_E_INVALID


def test_run_parameter_checks():
    """pcv_xray_check_params: what pcv_xray_run refuses before any device work."""
    ok = pcv.xray_params(256, 0.1, ("height_stddev", 0.5, "purplish"), intensity_interval=(0.0, 1.0), background="transparent")
    pcv.xray_check_params(ok, tree_has_intensity=True)
    pcv.xray_check_params(pcv.xray_params(256, 0.1, "colored"), tree_has_intensity=False)
    bad = [("unknown strategy", dict(strategy=7)), ("max_stddev", dict(strategy=L.XRAY_HEIGHT_STDDEV, max_stddev=0.0)),
           ("max_stddev", dict(strategy=L.XRAY_HEIGHT_STDDEV, max_stddev=-1.0)),
           ("max_stddev", dict(strategy=L.XRAY_HEIGHT_STDDEV, max_stddev=float("inf"))),
           ("max_stddev", dict(strategy=L.XRAY_HEIGHT_STDDEV, max_stddev=float("nan"))),
           ("colormap", dict(strategy=L.XRAY_HEIGHT_STDDEV, max_stddev=1.0, colormap=2)),
           ("background", dict(background=2)), ("only intensity", dict(interval_attribute=b"color"))]
    for msg, kw in bad:
        p = L.XrayParams(tile_size_px=256, pixel_size_m=0.1, **kw)
        with pytest.raises(pcv.PcvError, match=msg) as e:
            pcv.xray_check_params(p)
        assert e.value.code == L.PCV_E_INVALID
    with pytest.raises(pcv.PcvError, match="no intensity"):
        pcv.xray_check_params(ok, tree_has_intensity=False)
    for strategy in ("binned", ("height_stddev", 1.0, "viridis"), ("colored_with_intensity", 0.0, 1.0)):
        with pytest.raises(ValueError):
            pcv.xray_params(256, 0.1, strategy)
