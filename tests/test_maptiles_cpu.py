"""Map tiles, the part that needs no device (csrc/pcv_maptiles_dev.h and the host entries of csrc/pcv_maptiles.hip; DESIGN
§9i): the pixel rule against tests/maptiles_truth.py and against an independent long-double / mpmath truth, the slippy <->
quadtree index mapping, tiles.json and the parameter rules."""
import json
import math

import numpy as np
import pytest

import point_cloud_viewer_amd as pcv
from point_cloud_viewer_amd import _lib as L
from point_cloud_viewer_amd import synthetic

import maptiles_truth as MT
import wmr_oracle as W

DELTA = 1e-10  # normalised map units, the value test_wmr_cpu.py uses: the band around a pixel boundary left to either side
MAX_AMBIGUOUS = 0.01


@pytest.mark.parametrize("zoom", [0, 1, 19, 23])
def test_pixels_host_equals_the_truth_on_the_edge_set(zoom):
    x, y, z = MT.edge_points(19)
    gx, gy, ok = pcv.map_tile_pixels(zoom, x, y, z)
    wx, wy, wok = MT.pixels(zoom, x, y, z)
    assert np.array_equal(ok, wok) and np.array_equal(gx, wx) and np.array_equal(gy, wy)
    assert ok.any() and (~ok).any() and gx.max() < (256 << zoom) and gy.max() < (256 << zoom)


def test_the_edge_set_holds_what_it_says():
    x, y, z = MT.edge_points(19)
    gx, gy, ok = pcv.map_tile_pixels(19, x, y, z)
    assert not ok[~(np.isfinite(x) & np.isfinite(y) & np.isfinite(z))].any()
    axis = (x < -1e6) & (y == 0) & np.isfinite(z)  # the points near the centre of the Earth have no latitude to speak of
    plus, minus = axis & ~np.signbit(y), axis & np.signbit(y)
    assert plus.sum() >= 9 and minus.sum() >= 9
    assert not ok[plus].any()                                # lng = pi: u = 1
    assert ok[minus].all() and (gx[minus] == 0).all()        # lng = -pi: u = 0
    u, v = pcv.wmr_project(x, y, z)
    # a clamped latitude: the chain's v is -7.8e-16 in the north and 1 + 8.9e-16 in the south, both outside
    clamped = np.isfinite(u) & ((v < 0.0) | (v >= 1.0))
    assert (clamped & (v < 0.0)).sum() >= 30 and (clamped & (v >= 1.0)).sum() >= 30 and not ok[clamped].any()
    assert np.abs(v[clamped] - np.round(v[clamped])).max() < 1e-15
    # the seams: 3 x 3 tiles, and pixels on both sides of every seam
    seam = np.arange(len(x)) >= len(x) - 16 * 2 * 27
    tiles = {(int(a) >> 8, int(b) >> 8) for a, b in zip(gx[seam & ok], gy[seam & ok])}
    assert len(tiles) >= 16 and {int(a) & 255 for a in gx[seam & ok]} == {0, 255} == {int(b) & 255 for b in gy[seam & ok]}


def test_pixels_host_refuses_zoom_24():
    with pytest.raises(pcv.PcvError, match="0 ..= 23") as e:
        pcv.map_tile_pixels(24, [1.0], [2.0], [3.0])
    assert e.value.code == L.PCV_E_INVALID


def test_quad_index_is_a_bijection_that_commutes_with_the_parent():
    for zoom in range(0, 5):
        seen = set()
        for x in range(1 << zoom):
            for y in range(1 << zoom):
                i = pcv.map_tile_quad_index(zoom, x, y)
                assert i == MT.quad_index(zoom, x, y) and i < 4 ** zoom
                assert pcv.map_tile_from_quad_index(zoom, i) == (x, y)
                seen.add(i)
                if zoom:
                    assert i >> 2 == pcv.map_tile_quad_index(zoom - 1, x >> 1, y >> 1)
                    assert (i & 3) == 2 * (x & 1) + (1 - (y & 1))  # 1 top-left, 0 bottom-left, 3 top-right, 2 bottom-right
        assert seen == set(range(4 ** zoom))
    rng = np.random.default_rng(3)
    for x, y in rng.integers(0, 1 << 23, (2000, 2)):
        i = pcv.map_tile_quad_index(23, int(x), int(y))
        assert i == MT.quad_index(23, int(x), int(y)) and pcv.map_tile_from_quad_index(23, i) == (int(x), int(y))
        assert i >> 2 == pcv.map_tile_quad_index(22, int(x) >> 1, int(y) >> 1)
    for bad in ((3, 8, 0), (3, 0, 8), (24, 0, 0)):
        with pytest.raises(pcv.PcvError):
            pcv.map_tile_quad_index(*bad)
    with pytest.raises(pcv.PcvError):
        pcv.map_tile_from_quad_index(2, 16)


@pytest.mark.parametrize("zoom", [14, 16])
def test_the_chain_gives_the_high_precision_pixel(zoom):
    """Independent of pcv_wmr_project: (u, v) in long double, through mpmath for the points within DELTA + 1e-13 of their
    nearest pixel boundary. Every point farther than DELTA from a pixel boundary must land in the truth's pixel."""
    n = 20_000
    x, y, z = synthetic.uniform_ecef(n)[:3]
    S = np.longdouble(256 << zoom)
    u0, v0 = W.truth_uv_ld(x, y, z)
    ub = sorted({float(b) for b in np.rint(u0 * S) / S})
    vb = sorted({float(b) for b in np.rint(v0 * S) / S})
    assert len(ub) < 200 and len(vb) < 200
    u, v, redone = W.truth_uv(x, y, z, ub, vb, DELTA)
    us, vs = u * S, v * S
    far = (np.abs(us - np.rint(us)) > DELTA * S) & (np.abs(vs - np.rint(vs)) > DELTA * S)
    gx, gy, ok = pcv.map_tile_pixels(zoom, x, y, z)
    assert ok.all()
    bad = far & ((gx.astype(np.int64) != np.floor(us).astype(np.int64)) | (gy.astype(np.int64) != np.floor(vs).astype(np.int64)))
    left_out = 1.0 - float(far.mean())
    print(f"zoom {zoom}: {100 * left_out:.3f} % of the points within {DELTA:g} of a pixel boundary, {redone} through mpmath")
    assert not bad.any(), (int(bad.sum()), float(us[bad][0]), float(vs[bad][0]))
    assert left_out <= MAX_AMBIGUOUS


def test_json_round_trips_and_its_bounds_are_pythons(tmp_path):
    tiles = {17: [[20957, 50784]], 18: [[41914, 101568], [41915, 101569]], 19: [[83828, 203137], [83828, 203138], [83831, 203139]]}
    text = pcv.map_tiles_json(tiles)
    meta = json.loads(text)
    assert meta["scheme"] == "xyz" and meta["format"] == "png" and meta["tile_size"] == 256 and (meta["minzoom"], meta["maxzoom"]) == (17, 19)
    assert {int(k): v for k, v in meta["tiles"].items()} == tiles and list(meta["tiles"]) == ["17", "18", "19"]
    want = MT.bounds(19, tiles[19])
    assert all(abs(a - b) <= 1e-9 for a, b in zip(meta["bounds"], want)), (meta["bounds"], want)
    west, south, east, north = meta["bounds"]
    assert -123.0 < west < east < -122.0 and 37.0 < south < north < 38.0
    assert text == MT.json_text(tiles, meta["bounds"])  # the layout, and doubles in their shortest round-trip form
    # through a directory: read_map_tiles gives the lists back (no tile files are needed for empty lists)
    empty = pcv.map_tiles_json({3: [], 4: []})
    assert json.loads(empty)["bounds"] == [0.0, 0.0, 0.0, 0.0] and empty == MT.json_text({3: [], 4: []})
    (tmp_path / "tiles.json").write_text(empty)
    back = pcv.read_map_tiles(tmp_path)
    assert (back["minzoom"], back["maxzoom"], back["tile_size"]) == (3, 4, 256) and all(len(back["tiles"][z]) == 0 for z in (3, 4))
    with pytest.raises(ValueError):
        pcv.map_tiles_json({3: [], 5: []})


def test_the_whole_map_at_zoom_0_has_the_web_mercator_bounds():
    b = json.loads(pcv.map_tiles_json({0: [[0, 0]]}))["bounds"]
    lat = math.degrees(math.atan(math.sinh(math.pi)))
    assert abs(b[0] + 180.0) <= 1e-9 and abs(b[2] - 180.0) <= 1e-9 and abs(b[3] - lat) <= 1e-9 and abs(b[1] + lat) <= 1e-9


def test_check_params():
    pcv.map_tiles_check_params(23, min_zoom=0)
    pcv.map_tiles_check_params(0)
    for kw, what in ((dict(zoom=24), "0 ..= 23"), (dict(zoom=19, max_tiles=0), "max_tiles"), (dict(zoom=19, max_tiles=(1 << 22) + 1), "max_tiles"),
                     (dict(zoom=12, min_zoom=13), "min_zoom")):
        with pytest.raises(pcv.PcvError, match=what) as e:
            pcv.map_tiles_check_params(**kw)
        assert e.value.code == L.PCV_E_INVALID
    assert pcv.map_tiles_params(19, background=(1, 2, 3, 4)).background == 0x04030201 and pcv.map_tiles_params(19).max_tiles == 1 << 20
