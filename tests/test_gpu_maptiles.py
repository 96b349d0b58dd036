"""Map tiles on the device (csrc/pcv_maptiles.hip) against tests/maptiles_truth.py, byte for byte: tile lists,
images, counts, counters, parents, PNG files and the directory. The main cloud is 2 000 sites in the config-1 box with ten
points each: at zoom 19 it covers 4 x 4 tiles with about ten points in most drawn pixels."""
import json
import os

import numpy as np
import pytest

import point_cloud_viewer_amd as pcv
from point_cloud_viewer_amd import _lib as L

import maptiles_truth as MT

pytestmark = pytest.mark.gpu
ZOOM = 19


@pytest.fixture(scope="module")
def ctx():
    c = pcv.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def cloud():
    return MT.main_cloud()


@pytest.fixture(scope="module")
def want(cloud):
    return MT.reduce(ZOOM, *cloud)


def results(m):
    return dict(tiles=m.tiles(), images=m.images(), counts=m.counts(), info=m.info())


def run(ctx, zoom, x, y, z, rgb, calls=1, device=False, cuts=None, **params):
    m = ctx.map_tiles_begin(zoom, **params)
    try:
        cuts = np.linspace(0, len(x), calls + 1).astype(int) if cuts is None else cuts
        for a, b in zip(cuts[:-1], cuts[1:]):
            part = [np.ascontiguousarray(v[a:b]) for v in (x, y, z, rgb)]
            if device:
                import torch
                part = [torch.from_numpy(v).to(f"cuda:{ctx.device}") for v in part]
            m.add_points(*part)
        m.finish()
        return results(m)
    finally:
        m.free()


def assert_same(got, want, n=None):
    assert np.array_equal(got["tiles"], want["tiles"]), (got["tiles"], want["tiles"])
    assert np.array_equal(got["counts"], want["counts"])
    assert np.array_equal(got["images"], want["images"])
    if "info" in got and "dropped" in want:
        inf = got["info"]
        assert (inf["dropped"], inf["drawn"]) == (want["dropped"], want["drawn"]), (inf, want["dropped"], want["drawn"])
        assert inf["tiles"][inf["zoom"]] == len(want["tiles"]) and inf["finished"] and inf["pool_bytes"] == 0
        if n is not None:
            assert inf["points_added"] == n


@pytest.fixture(scope="module")
def got(ctx, cloud):
    return run(ctx, ZOOM, *cloud, device=True)


# ---- 1, 2: the main cloud ---------------------------------------------------------------------------------------------------
def test_device_planes_equal_the_truth(cloud, want, got):
    assert len(want["tiles"]) == 16 and len(set(want["tiles"][:, 0])) == 4 and want["dropped"] == 0
    per = want["counts"][want["counts"] > 0]
    assert 8 <= np.median(per) <= 12 and (want["images"][..., 3] == 255).sum() == per.size
    assert_same(got, want, len(cloud[0]))


@pytest.mark.parametrize("how", ["one call", "seven uneven calls", "host memory", "two halves on disjoint tiles"])
def test_pieces_order_and_source_do_not_reach_the_bytes(ctx, cloud, want, got, how):
    x, y, z, rgb = cloud
    n = len(x)
    if how == "one call":
        res = run(ctx, ZOOM, x, y, z, rgb, device=True, staging_points=n)
    elif how == "seven uneven calls":
        res = run(ctx, ZOOM, x, y, z, rgb, device=True, cuts=np.array([0, 1, 64, 65, 321, 7000, 7001, n]), staging_points=1000)
    elif how == "host memory":
        order = np.random.default_rng(1).permutation(n)
        res = run(ctx, ZOOM, x[order], y[order], z[order], rgb[order], staging_points=777)
    else:
        gx, _, _ = MT.pixels(ZOOM, x, y, z)
        west = (gx >> 8) < np.sort(np.unique(gx >> 8))[2]
        order = np.concatenate([np.flatnonzero(~west), np.flatnonzero(west)])  # the eastern tiles come first
        res = run(ctx, ZOOM, x[order], y[order], z[order], rgb[order], cuts=np.array([0, int((~west).sum()), n]))
    assert_same(res, want, n)
    assert np.array_equal(res["images"], got["images"]) and np.array_equal(res["tiles"], got["tiles"])


# ---- 3: edges ---------------------------------------------------------------------------------------------------------------
def test_the_edge_set_in_one_add(ctx):
    x, y, z = MT.edge_points(ZOOM)
    rgb = np.random.default_rng(4).integers(0, 256, (len(x), 3), dtype=np.uint8)
    gx, gy, ok = pcv.map_tile_pixels(ZOOM, x, y, z)
    w = MT.reduce(ZOOM, x, y, z, rgb)
    assert w["dropped"] == int((~ok).sum()) > 20 and w["drawn"] > 500 and len(w["tiles"]) > 20
    res = run(ctx, ZOOM, x, y, z, rgb, device=True)
    assert_same(res, w, len(x))
    # every point's flag and pixel, through the count planes: the host entry's pixels, counted
    slot = {(int(a), int(b)): k for k, (a, b) in enumerate(res["tiles"])}
    counts = np.zeros_like(res["counts"])
    for a, b in zip(gx[ok].astype(np.int64), gy[ok].astype(np.int64)):
        counts[slot[(a >> 8, b >> 8)], b & 255, a & 255] += 1
    assert np.array_equal(counts, res["counts"])
    assert (res["tiles"][:, 0] == 0).any()  # y = -0.0 on the -x axis: u = 0


# ---- 4, 5: one pixel ----------------------------------------------------------------------------------------------------------
def test_one_pixel_whose_sums_pass_2_16_and_2_24(ctx, cloud):
    n = 70_000
    x, y, z = (np.full(n, v[0]) for v in cloud[:3])
    rng = np.random.default_rng(5)
    rgb = np.stack([rng.integers(240, 256, n), rng.integers(0, 256, n), rng.integers(0, 3, n)], axis=1).astype(np.uint8)
    sums = rgb.astype(np.int64).sum(axis=0)
    assert sums[0] > 1 << 24 and 1 << 16 < sums[2] < 1 << 24 and sums[1] > 1 << 16
    w = MT.reduce(ZOOM, x, y, z, rgb)
    assert len(w["tiles"]) == 1 and w["counts"].max() == n and (w["counts"] > 0).sum() == 1
    assert_same(run(ctx, ZOOM, x, y, z, rgb, device=True, staging_points=9000), w, n)


def test_more_than_2_24_points_in_a_pixel_fail_finish(ctx, cloud):
    import torch
    n = (1 << 24) + 1
    dev = f"cuda:{ctx.device}"
    before = ctx.pool_stats()[0]
    m = ctx.map_tiles_begin(ZOOM)
    try:
        x, y, z = (torch.full((n,), float(v[0]), dtype=torch.float64, device=dev) for v in cloud[:3])
        m.add_points(x, y, z, torch.full((n, 3), 200, dtype=torch.uint8, device=dev))
        assert m.info()["tiles"] == {ZOOM: 1} and m.info()["points_added"] == n
        with pytest.raises(pcv.PcvError, match="choose a larger zoom") as e:
            m.finish()
        assert e.value.code == L.PCV_E_INVALID
        with pytest.raises(pcv.PcvError, match="only be freed"):
            m.tiles()
    finally:
        m.free()
    assert ctx.pool_stats()[0] == before


# ---- 6, 7, 8: query sources ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tree(ctx, cloud):
    x, y, z, rgb = cloud
    inten = (np.arange(len(x)) % 100).astype(np.float32)
    t = ctx.build(0.001, None, x, y, z, rgb, inten, max_points_per_node=3000)
    yield t
    t.free()


def test_an_octree_through_the_query_adder(ctx, tree):
    shapes = ctx.shapes([("all",)])
    batch = tree.query_batch(shapes)
    try:
        pts = batch.points()
        sizes = np.diff(batch.segments()[2].astype(np.int64))
        assert pts["count"] == 20_000 and batch.num_segments > 4 and sizes.max() > 1000  # pieces of 1 000 cut inside chunks
        w = MT.reduce(ZOOM, pts["x"], pts["y"], pts["z"], pts["rgb"])
        assert len(w["tiles"]) == 16
        m = batch.map_tiles(ZOOM, staging_points=1000)
        assert_same(results(m), w, pts["count"])
        m.free()
        assert_same(run(ctx, ZOOM, pts["x"], pts["y"], pts["z"], pts["rgb"].reshape(-1, 3)), w, pts["count"])
        m = tree.map_tiles(ZOOM)  # the cloud's own method, the default piece
        assert_same(results(m), w, pts["count"])
        m.free()
    finally:
        batch.free()
    some = tree.query_batch(shapes, intervals=[(10.0, 29.0)])
    try:
        pts = some.points()
        assert 3000 < pts["count"] < 5000
        m = some.map_tiles(ZOOM, staging_points=1000)
        assert_same(results(m), MT.reduce(ZOOM, pts["x"], pts["y"], pts["z"], pts["rgb"]), pts["count"])
        m.free()
    finally:
        some.free()
        shapes.free()


def test_an_s2_cloud_gives_the_bytes_of_the_points_themselves(ctx, cloud, want, got):
    x, y, z, rgb = cloud
    s2 = ctx.s2_split(dict(x=x, y=y, z=z, color=rgb), 19)
    try:
        assert s2.num_cells > 4
        m = s2.map_tiles(ZOOM, staging_points=1000)  # the positions are the stored f64
        res = results(m)
        m.free()
        assert_same(res, want, len(x))
        assert np.array_equal(res["images"], got["images"])
    finally:
        s2.free()


def test_tile_counts_equal_the_web_mercator_rect_queries(ctx, tree):
    m = tree.map_tiles(ZOOM)
    tiles, counts = m.tiles(), m.counts()
    m.free()
    rects = [pcv.web_mercator_rect_from_zoomed((256.0 * a, 256.0 * b), (256.0 * (a + 1), 256.0 * (b + 1)), ZOOM) for a, b in tiles.tolist()]
    shapes = ctx.shapes(rects)
    batch = tree.query_batch(shapes)
    try:
        first, _, off = batch.segments()
        kept = [int(off[int(first[s + 1])] - off[int(first[s])]) for s in range(len(rects))]
    finally:
        batch.free()
        shapes.free()
    assert kept == counts.reshape(len(tiles), -1).sum(axis=1).tolist() and sum(kept) == 20_000


# ---- 9: parents ---------------------------------------------------------------------------------------------------------------
def test_parents_down_to_zoom_15(ctx, cloud, want):
    m = ctx.map_tiles_begin(ZOOM).add_points(*cloud).finish().build_parents(15)
    try:
        truth = MT.parents(ZOOM, 15, want["tiles"], want["images"])
        info = m.info()
        assert info["min_zoom"] == 15 and info["tiles"] == {z: len(truth[z][0]) for z in range(15, ZOOM + 1)}
        for zoom in range(15, ZOOM + 1):
            tiles, images = truth[zoom]
            assert np.array_equal(m.tiles(zoom), tiles) and tiles.tolist() == sorted(tiles.tolist())
            assert np.array_equal(m.images(zoom), images), zoom
            if len(tiles) > 1:
                assert np.array_equal(m.images(zoom, 1, 1)[0], images[1])
        assert len(truth[18][0]) >= 4 and 1 <= len(truth[15][0]) <= 4
        m.build_parents(15)  # again: nothing to do
        with pytest.raises(pcv.PcvError, match="already"):
            m.build_parents(14)
        with pytest.raises(pcv.PcvError, match="not built"):
            m.tiles(14)
    finally:
        m.free()


def test_a_parent_shows_each_child_in_its_quadrant(ctx, cloud):
    """Four sibling tiles filled pixel by pixel, each in one colour: north-west, south-west, north-east, south-east."""
    gx0, gy0, _ = pcv.map_tile_pixels(ZOOM, *(v[:1] for v in cloud[:3]))
    px, py = (int(gx0[0]) >> 9) << 1, (int(gy0[0]) >> 9) << 1  # the even tile of a parent
    colours = {(0, 0): (250, 10, 20), (0, 1): (30, 240, 50), (1, 0): (60, 70, 230), (1, 1): (200, 190, 40)}
    S = float(256 << ZOOM)
    us, vs, cs = [], [], []
    for (dx, dy), c in colours.items():
        col, row = np.meshgrid(np.arange(256), np.arange(256))
        us.append(((px + dx) * 256 + col.ravel() + 0.5) / S)
        vs.append(((py + dy) * 256 + row.ravel() + 0.5) / S)
        cs.append(np.tile(np.array(c, dtype=np.uint8), (256 * 256, 1)))
    lat, lng = pcv.wmr_to_lat_lng(np.concatenate(us), np.concatenate(vs))
    x, y, z = (np.ascontiguousarray(a) for a in MT.ecef_from_lat_lng(lat, lng, 12.0))
    rgb = np.concatenate(cs)
    w = MT.reduce(ZOOM, x, y, z, rgb)
    assert len(w["tiles"]) == 4 and (w["counts"] == 1).all()
    m = ctx.map_tiles_begin(ZOOM, background=(9, 8, 7, 0)).add_points(x, y, z, rgb).finish().build_parents(ZOOM - 1)
    try:
        assert_same(results(m), w)
        assert m.tiles(ZOOM - 1).tolist() == [[px >> 1, py >> 1]]
        img = m.images(ZOOM - 1)[0]
        assert np.array_equal(img, MT.parents(ZOOM, ZOOM - 1, w["tiles"], w["images"], background=(9, 8, 7, 0))[ZOOM - 1][1][0])
        for (dx, dy), c in colours.items():
            quadrant = img[128 * dy + 16:128 * dy + 112, 128 * dx + 16:128 * dx + 112]  # row 0 is north
            assert (quadrant == np.array(c + (255,), dtype=np.uint8)).all(), (dx, dy)
    finally:
        m.free()


# ---- 10: files ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("png", ["stored", "deflate"])
def test_the_directory(ctx, cloud, tmp_path, png):
    m = ctx.map_tiles_begin(ZOOM).add_points(*cloud).finish().build_parents(17)
    try:
        out = tmp_path / png
        m.write(out, png=png)
        tiles = {z: m.tiles(z) for z in (17, 18, 19)}
        want_files = {"tiles.json"} | {f"{z}/{a}/{b}.png" for z, t in tiles.items() for a, b in t.tolist()}
        have = {os.path.relpath(os.path.join(d, f), out) for d, _, fs in os.walk(out) for f in fs}
        assert have == want_files
        text = open(out / "tiles.json").read()
        assert text == pcv.map_tiles_json({z: t.tolist() for z, t in tiles.items()})
        meta = json.loads(text)
        assert all(abs(a - b) <= 1e-9 for a, b in zip(meta["bounds"], MT.bounds(ZOOM, tiles[ZOOM]))) and meta["minzoom"] == 17
        assert text == MT.json_text({z: t.tolist() for z, t in tiles.items()}, meta["bounds"])
        for z, t in tiles.items():
            images, files = m.images(z), m.tile_pngs(z, png=png)
            assert len(files) == len(t)
            for k, (a, b) in enumerate(t.tolist()):
                data = open(out / str(z) / str(a) / f"{b}.png", "rb").read()
                assert data == files[k]
                assert np.array_equal(pcv.png_decode(data), images[k])
            if len(t) >= 3:
                assert m.tile_pngs(z, 1, 2, png=png) == files[1:3]
        back = pcv.read_map_tiles(out)
        assert (back["minzoom"], back["maxzoom"], back["scheme"], back["format"]) == (17, 19, "xyz", "png")
        for z, t in tiles.items():
            assert np.array_equal(back["tiles"][z], t) and np.array_equal(back["images"][z], m.images(z))
        if png == "deflate":
            stored = sum(len(f) for f in m.tile_pngs(ZOOM))
            assert sum(len(f) for f in m.tile_pngs(ZOOM, png="deflate")) < stored // 4
    finally:
        m.free()


def test_build_map_tiles_from_a_directory(ctx, tree, tmp_path):
    tree.write_dir(str(tmp_path / "octree"))
    m = pcv.build_map_tiles(tmp_path / "octree", tmp_path / "tiles", ZOOM, 16, png="deflate", ctx=ctx)
    try:
        direct = tree.map_tiles(ZOOM, min_zoom=16)
        back = pcv.read_map_tiles(tmp_path / "tiles")
        for z in range(16, ZOOM + 1):
            assert np.array_equal(back["tiles"][z], direct.tiles(z)) and np.array_equal(back["images"][z], direct.images(z))
        direct.free()
    finally:
        m.free()


# ---- 11: failures -----------------------------------------------------------------------------------------------------------------
def test_failures(ctx, cloud, tree):
    x, y, z, rgb = cloud
    before = ctx.pool_stats()[0]
    m = ctx.map_tiles_begin(ZOOM, max_tiles=4)
    with pytest.raises(pcv.PcvError, match="max_tiles = 4") as e:
        m.add_points(x, y, z, rgb)
    assert e.value.code == L.PCV_E_OOM and m.info()["pool_bytes"] == 0
    for call in (m.finish, m.tiles, lambda: m.add_points(x, y, z, rgb)):
        with pytest.raises(pcv.PcvError, match="only be freed"):
            call()
    m.free()
    assert ctx.pool_stats()[0] == before
    # exactly as many tiles as allowed: no failure
    assert len(run(ctx, ZOOM, x, y, z, rgb, max_tiles=16)["tiles"]) == 16
    # a pool cap below the touched tiles
    m = ctx.map_tiles_begin(ZOOM, max_pool_bytes=3 << 20)
    with pytest.raises(pcv.PcvError, match="max_pool_bytes") as e:
        m.add_points(x, y, z, rgb)
    assert e.value.code == L.PCV_E_OOM
    m.free()
    assert ctx.pool_stats()[0] == before
    # finished layers take no points; unfinished ones give no tiles
    m = ctx.map_tiles_begin(ZOOM)
    with pytest.raises(pcv.PcvError, match="not finished"):
        m.tiles()
    m.add_points(x[:10], y[:10], z[:10], rgb[:10]).finish()
    with pytest.raises(pcv.PcvError, match="no more points") as e:
        m.add_points(x[:10], y[:10], z[:10], rgb[:10])
    assert e.value.code == L.PCV_E_INVALID
    shapes = ctx.shapes([("all",)])
    batch = tree.query_batch(shapes)
    with pytest.raises(pcv.PcvError, match="no more points"):
        m.add_query_batch(batch)
    m.free()
    # a batch of another context
    other = pcv.Context(0)
    try:
        m = other.map_tiles_begin(ZOOM)
        with pytest.raises(pcv.PcvError, match="another context") as e:
            m.add_query_batch(batch)
        assert e.value.code == L.PCV_E_INVALID
        m.free()
    finally:
        other.close()
        batch.free()
        shapes.free()
    # an empty layer: no tiles, a directory with tiles.json only
    m = ctx.map_tiles_begin(3).finish().build_parents(1)
    assert m.tiles().shape == (0, 2) and m.images(2).shape == (0, 256, 256, 4) and m.info()["tiles"] == {1: 0, 2: 0, 3: 0}
    m.free()
    with pytest.raises(pcv.PcvError, match="0 ..= 23"):
        ctx.map_tiles_begin(24)
