"""Terrain layers in the viewer's frame, the parts that need no device: the window's host twin against
tests/render_terrain_oracle.py, the refusals of pcv_render_check_terrain_host, the reader of meta.json, and self-checks of the
oracle on cases small enough to work out by hand."""
import json

import numpy as np
import pytest

import point_cloud_viewer_amd as pcv
import render_terrain_oracle as RT

Q90 = [0.0, 0.0, np.sqrt(0.5), np.sqrt(0.5)]  # a quarter turn about z


def grid(**kw):
    base = dict(tile_size=8, resolution_m=0.5, origin=(0.0, 0.0, 0.0), world_from_terrain=[0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0])
    base.update(kw)
    return base


FRAMES = [grid(),
          grid(origin=(1.25, -7.5, 3.0), resolution_m=0.1),
          grid(world_from_terrain=[10.0, -20.0, 5.0] + Q90),
          grid(world_from_terrain=[-3.5, 2.25, 1.0, 0.0, 0.0, float(np.sin(0.15)), float(np.cos(0.15))], origin=(-4.0, 9.0, 0.0), resolution_m=0.3),
          grid(world_from_terrain=[0.5, 0.5, 0.5, float(np.sin(0.4)), 0.0, 0.0, float(np.cos(0.4))], resolution_m=2.0)]


@pytest.mark.parametrize("params", FRAMES)
@pytest.mark.parametrize("window", [2, 16, 64, 1024])
def test_window_equals_the_oracle(params, window):
    rng = np.random.default_rng(window)
    cams = np.concatenate([rng.uniform(-500.0, 500.0, (40, 3)), -rng.uniform(0.0, 1e9, (10, 3)), [[0.0, 0.0, 0.0]]])
    seen_negative = False
    for c in cams:
        want = RT.window_pos(params, c, window)
        assert pcv.render_terrain_window(params, c, window) == want, (c, want)
        seen_negative |= want[0] + window // 2 < 0 and want[1] + window // 2 < 0
    assert seen_negative


def test_window_of_a_camera_on_a_grid_line():
    """floor(u), not the accumulate chain's floor(u + 0.5): on the line the camera belongs to the cell that starts there; half
    a cell further the vertex rule would already round up, the window does not."""
    p = grid()
    for x, gx in [(1.5, 3), (-1.5, -3), (0.0, 0), (1.75, 3), (-1.75, -4), (1.4999999999999998, 2)]:
        assert pcv.render_terrain_window(p, (x, 0.0, 0.0), 16) == (gx - 8, -8) == RT.window_pos(p, (x, 0.0, 0.0), 16)
    i, _, _, _ = pcv.terrain_vertex(p, [1.75], [0.0], [0.0])
    assert int(i[0]) == 4  # the vertex rule differs from the window rule
    # under the quarter turn the terrain's x is the world's y
    r = grid(world_from_terrain=[0.0, 0.0, 0.0] + Q90)
    assert pcv.render_terrain_window(r, (100.0, 1.5, 0.0), 2)[0] == 3 - 1


def test_unrepresentable_window_is_refused():
    p = grid(resolution_m=1.0)
    assert pcv.render_terrain_window(p, (2.0 ** 53 - 1.0, -(2.0 ** 53 - 1.0), 0.0), 1024) == (2 ** 53 - 1 - 512, -(2 ** 53 - 1) - 512)
    for cam in [(2.0 ** 53, 0.0, 0.0), (0.0, -(2.0 ** 53), 0.0), (1e300, 0.0, 0.0), (np.inf, 0.0, 0.0), (0.0, np.nan, 0.0)]:
        with pytest.raises(pcv.PcvError) as e:
            pcv.render_terrain_window(p, cam, 16)
        assert e.value.code == pcv.PCV_E_INVALID and "Terrain location not representable." in str(e.value)
        with pytest.raises(RT.NotRepresentable):
            RT.window_pos(p, cam, 16)
    for window in (0, 15, 1026):
        with pytest.raises(pcv.PcvError):
            pcv.render_terrain_window(p, (0.0, 0.0, 0.0), window)


def test_check_terrain():
    pcv.render_check_terrain(0, 15)  # no layers: nothing else is read
    pcv.render_check_terrain(0, 0, layers=None, camera_positions=None)
    for window in (2, 16, 1024):
        pcv.render_check_terrain(3, window)
    for window in (0, 1, 15, 1023, 1026, 4096):
        with pytest.raises(pcv.PcvError) as e:
            pcv.render_check_terrain(1, window)
        assert e.value.code == pcv.PCV_E_INVALID and "window" in str(e.value) and "1024" in str(e.value)
    for kw, word in [(dict(layers=None), "null terrain layer array"), (dict(layers=[1, None, 1]), "a terrain layer is null"),
                     (dict(camera_positions=None), "camera positions")]:
        with pytest.raises(pcv.PcvError) as e:
            pcv.render_check_terrain(3, 16, **kw)
        assert e.value.code == pcv.PCV_E_INVALID and word in str(e.value)
    lib = pcv.load_library()
    assert lib.pcv_render_check_terrain_host(None, None, 0) == pcv.PCV_OK  # a null struct: nothing is drawn


def test_meta_reader():
    p = grid(tile_size=32, origin=(1.5, -2.0, 1e-3), resolution_m=0.05, world_from_terrain=[1e6 + 0.125, -3.0, 7.0] + Q90)
    tiles = [[-3, 5], [0, 0], [2, -1]]
    text = pcv.terrain_meta_json(p, tiles)
    got = pcv.terrain_meta_read(text)
    assert got["tile_size"] == 32 and got["resolution_m"] == 0.05 and got["tiles"].tolist() == tiles
    assert np.array_equal(got["origin"], np.array(p["origin"])) and np.array_equal(got["world_from_terrain"], np.array(p["world_from_terrain"]))
    assert pcv.terrain_meta_read(pcv.terrain_meta_json(p, []))["tiles"].shape == (0, 2)
    # the keys in any order, at both levels, with white space and a key serde would skip
    d = json.loads(text)
    shuffled = {"tile_positions": d["tile_positions"], "extra": {"nested": [1, {"deep": None}, "x]"], "flag": True},
                "resolution_m": d["resolution_m"], "origin": d["origin"], "tile_size": d["tile_size"],
                "world_from_terrain": {"translation": d["world_from_terrain"]["translation"], "note": "kept",
                                       "rotation": d["world_from_terrain"]["rotation"]}}
    again = pcv.terrain_meta_read(json.dumps(shuffled, indent=2))
    assert again["tiles"].tolist() == tiles and np.array_equal(again["world_from_terrain"], got["world_from_terrain"]) and again["tile_size"] == 32
    # a file cut off in the middle: the key whose value was being read is named
    for key in ("tile_size", "world_from_terrain", "origin", "resolution_m", "tile_positions"):
        cut = text[:text.index('"' + key + '"') + len(key) + 5]
        with pytest.raises(pcv.PcvError) as e:
            pcv.terrain_meta_read(cut)
        assert e.value.code == pcv.PCV_E_INVALID and '"' + key + '"' in str(e.value), (key, str(e.value))
    with pytest.raises(pcv.PcvError) as e:
        pcv.terrain_meta_read(text[:-1])  # only the closing brace is missing
    assert e.value.code == pcv.PCV_E_INVALID
    # a missing key, and values the parameter check refuses
    for key in d:
        with pytest.raises(pcv.PcvError) as e:
            pcv.terrain_meta_read(json.dumps({k: v for k, v in d.items() if k != key}))
        assert e.value.code == pcv.PCV_E_INVALID and '"' + key + '"' in str(e.value)
    for bad in [dict(d, tile_size=0), dict(d, tile_size=4097), dict(d, resolution_m=0.0), dict(d, tile_positions=[[1, 2, 3]]),
                dict(d, tile_positions=[[1.5, 2]]), dict(d, origin=[1.0, 2.0])]:
        with pytest.raises(pcv.PcvError) as e:
            pcv.terrain_meta_read(json.dumps(bad))
        assert e.value.code == pcv.PCV_E_INVALID


# ---- self-checks of the oracle ------------------------------------------------------------------------------------------------

def masks(is_set, i0=0, j0=0):
    return pcv.terrain_quad_masks(np.asarray(is_set, np.uint8), i0, j0)


@pytest.mark.parametrize("i0,j0", [(0, 0), (-7, 11), (2, -4)])
def test_a_shared_edge_is_emitted_once(i0, j0):
    edges = RT.drawn_edges(masks(np.ones((2, 3)), i0, j0))  # two rendered quads side by side
    assert len(edges) == len(set(edges)) == 9  # 4 H, 3 V, 2 D: the V edge between the quads once
    assert edges.count((1, 0, RT.V_EDGE)) == 1
    assert sorted(e for e in edges if e[2] == RT.D_EDGE) == [(0, 0, RT.D_EDGE), (1, 0, RT.D_EDGE)]
    full = RT.drawn_edges(masks(np.ones((5, 6)), i0, j0))
    assert len(full) == len(set(full)) == 5 * 5 + 6 * 4 + 5 * 4  # H: 5 per row, V: 4 per column, D: one per quad


@pytest.mark.parametrize("i0,j0", [(0, 0), (-7, 11)])
def test_a_quad_with_an_unset_corner_keeps_only_the_shared_edge(i0, j0):
    is_set = np.ones((2, 3), np.uint8)
    is_set[1, 2] = 0  # quad (1, 0) loses a corner, quad (0, 0) is whole
    edges = RT.drawn_edges(masks(is_set, i0, j0))
    assert sorted(edges) == sorted([(0, 0, RT.H_EDGE), (0, 0, RT.V_EDGE), (0, 0, RT.D_EDGE), (0, 1, RT.H_EDGE), (1, 0, RT.V_EDGE)])
    # its three remaining corners are set and still none of its own edges is drawn
    for own in [(1, 0, RT.H_EDGE), (1, 0, RT.D_EDGE), (2, 0, RT.V_EDGE), (1, 1, RT.H_EDGE)]:
        assert own not in edges
    assert RT.drawn_edges(masks(np.array([[1, 1], [1, 0]]), i0, j0)) == []  # three corners of a lone quad: neither triangle


def test_mask_conversion():
    m = np.array([0.0, 1.0, 511.0, 511.9, -1.0, -0.0, np.nan, np.inf, -np.inf, 4294967296.0, 4294967040.0], np.float32)
    assert RT.mask_u32(m).tolist() == [0, 1, 511, 511, 0, 0, 0, 0, 0, 0, 4294967040]


def tiny_layer():
    """One tile of 2 x 2 set vertices at 4 m spacing: one quad, five edges; red runs 0 -> 200 along x, green 10 -> 250 along y."""
    heights = np.zeros((1, 2, 2, 2), np.float32)
    heights[0, :, :, 1] = masks(np.ones((2, 2))).astype(np.float32)
    colors = np.zeros((1, 2, 2, 4), np.uint8)
    colors[0, 0, 0], colors[0, 0, 1], colors[0, 1, 0], colors[0, 1, 1] = [0, 10, 7, 255], [200, 10, 7, 255], [0, 250, 7, 255], [200, 250, 7, 255]
    return dict(tile_size=2, resolution_m=4.0, origin=np.zeros(3), world_from_terrain=np.array([0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0]),
                tiles=np.array([[0, 0]], np.int32), heights=heights, colors=colors)


def test_a_single_quad_worked_out_by_hand():
    """x, y of [0, 8] onto an 8 x 8 image, w = 1, flat depth: vertex (i, j) sits on window point (4 i, 4 j)."""
    m = np.zeros((4, 4))
    m[0, 0] = m[1, 1] = 0.25
    m[0, 3] = m[1, 3] = -1.0
    m[3, 3] = 1.0
    matrix = m.ravel(order="F")
    layer, W, H, wn = tiny_layer(), 8, 8, 4
    f = RT.layer_fragments(layer, (0.0, 0.0, 0.0), matrix, W, H, wn)
    assert f["pos"] == (-2, -2) and f["edges_submitted"] == 5 and f["edges_drawn"] == 5
    base = 3 * (2 * wn + 2)  # the quad's lower corner is window vertex (2, 2)
    assert sorted(set(f["edge"].tolist())) == [base, base + 1, base + 2, 3 * (2 * wn + 3) + 1, 3 * (3 * wn + 2)]
    out = dict(image=np.zeros((H, W, 4), np.uint8), depth=np.ones((H, W), np.float32), winner=np.full((H, W), -1, np.int64))
    out["image"][..., 3] = 255
    RT.add_layers(out, 0, [layer], (0.0, 0.0, 0.0), matrix, W, H, wn)
    img = out["image"][::-1]  # row 0 at the bottom, as gy counts
    # H edge (0, 0) -> (4, 0): pixel centres 0.5 .. 3.5 of row 0, t = (i + 0.5) / 4, red 200 t
    assert img[0, :4, 0].tolist() == [25, 75, 125, 175] and img[0, :4, 1].tolist() == [10, 10, 10, 10] and (img[0, :4, 3] == 255).all()
    assert out["winner"][::-1][0, :4].tolist() == [base] * 4  # at equal depth the H edge beats V (pixel 0) and D (pixel 3)
    # V edge (0, 0) -> (0, 4): column 0, green 10 + 240 t; its pixel (0, 0) went to the H edge
    assert img[1:4, 0, 1].tolist() == [100, 160, 220] and out["winner"][::-1][1:4, 0].tolist() == [base + 1] * 3
    # the far H and V edges lie on pixel centres 4.0: [min, max) covers 0.5 .. 3.5 of row / column 4
    assert img[4, :4, 0].tolist() == [25, 75, 125, 175] and img[4, :4, 1].tolist() == [250] * 4
    assert img[:4, 4, 1].tolist() == [40, 100, 160, 220] and img[:4, 4, 0].tolist() == [200] * 4
    # D edge (4, 0) -> (0, 4), x-major on the tie: pixel i has t = (4 - (i + 0.5)) / 4 and y = 4 t, so row floor(3.5 - i); at
    # equal depth its ends lose to the V edge (pixel 0 of row 3) and to the H edge (pixel 3 of row 0)
    assert [int(out["winner"][::-1][3 - i, i]) for i in range(4)] == [base + 1, base + 2, base + 2, base]
    assert img[2, 1].tolist() == [75, 160, 7, 255]  # s = t = 0.625 from (200, 10) to (0, 250)
    assert out["terrain"] == [dict(pos=(-2, -2), edges_submitted=5, edges_drawn=5, pixels_won=int((out["winner"] >= 0).sum()))]
    assert out["pixels_covered"] == 4 + 3 + 4 + 4 + 2 and (out["depth"][out["winner"] >= 0] == 0.5).all()
    # the same layer again: every fragment ties with the first layer's and loses on the rank
    twice = dict(image=np.zeros((H, W, 4), np.uint8), depth=np.ones((H, W), np.float32), winner=np.full((H, W), -1, np.int64))
    twice["image"][..., 3] = 255
    RT.add_layers(twice, 0, [layer, layer], (0.0, 0.0, 0.0), matrix, W, H, wn)
    assert np.array_equal(twice["image"], out["image"]) and twice["terrain"][1]["pixels_won"] == 0
