"""The host side of the terrain layer (csrc/pcv_terrain_dev.h, pcv_terrain_files.cpp) against tests/terrain_truth.py: the
chain bit for bit, the frame, the quad masks and the shader's requirement, tile names, meta.json, parameter errors. No device."""
import ctypes as C
import json

import numpy as np
import pytest

import point_cloud_viewer_amd as pcv
from point_cloud_viewer_amd import _lib as L

import terrain_truth as TT

R = float(np.sqrt(0.5))
EXACT = {  # quaternions ijkw whose matrices have entries in {0, +-1}
    "identity": [0, 0, 0, 1],
    "z +90": [0, 0, R, R], "z -90": [0, 0, -R, R], "x +90": [R, 0, 0, R], "y -90": [0, -R, 0, R],
    "x 180": [1, 0, 0, 0], "y 180": [0, 1, 0, 0], "z 180": [0, 0, 1, 0],
    "halves": [0.5, 0.5, 0.5, 0.5], "halves, one negative": [0.5, -0.5, 0.5, 0.5],
}
GENERAL = [0.18257418583505536, 0.3651483716701107, 0.5477225575051661, 0.7302967433402214]  # (1, 2, 3, 4) / sqrt(30)


def lib_params(p, **more):
    return pcv.terrain_params(tile_size=p["tile_size"], resolution_m=p["resolution_m"], origin=p["origin"],
                              world_from_terrain=p["world_from_terrain"], statistic=p["statistic"], min_points=p["min_points"], **more)


def cloud(seed, n, scale=100.0, centre=(0.0, 0.0, 0.0)):
    rng = np.random.default_rng(seed)
    return tuple(rng.normal(c, scale, n) for c in centre)


@pytest.mark.parametrize("name", sorted(EXACT))
def test_exact_frames_and_the_chain_bit_for_bit(name):
    iso = [12.5, -7.25, 3.0] + EXACT[name]
    p = TT.params(tile_size=16, resolution_m=0.3, origin=(1.5, -2.0, 0.25), world_from_terrain=iso)
    m, t = pcv.terrain_frame(lib_params(p))
    tm, tt = TT.frame(iso)
    assert np.array_equal(m, tm) and np.array_equal(t, tt)
    assert set(np.unique(np.abs(m))) <= {0.0, 1.0} and np.array_equal(np.abs(m).sum(axis=0), [1, 1, 1])
    x, y, z = cloud(5, 20_000)
    x[:6] = [np.nan, np.inf, 1e300, 0.0, 0.0, 12.5]
    z[3:5] = [1e39, -1e39]  # heights that overflow f32
    i, j, h, ok = pcv.terrain_vertex(lib_params(p), x, y, z)
    c = TT.chain(p, x, y, z)
    assert np.array_equal(ok, c["ok"]) and not ok[:5].any() and ok[5:].all()
    assert np.array_equal(i, c["i"]) and np.array_equal(j, c["j"]) and np.array_equal(h.view(np.uint32), c["h"].view(np.uint32))


def test_heights_round_the_edge_of_f32():
    """Up to the midpoint 2^128 - 2^103 above FLT_MAX a height rounds to FLT_MAX and stays; from the midpoint on it has no
    finite f32 and the point is dropped. The host twin decides this without casting out of f32's range."""
    fmax, mid = float(np.finfo(np.float32).max), 2.0 ** 128 - 2.0 ** 103
    z = np.array([fmax, np.nextafter(fmax, np.inf), np.nextafter(mid, 0.0), mid, np.nextafter(mid, np.inf), 1e39, np.inf])
    z = np.concatenate([z, -z])
    p = TT.params(tile_size=4, resolution_m=1.0)
    i, j, h, ok = pcv.terrain_vertex(lib_params(p), np.zeros(z.size), np.zeros(z.size), z)
    c = TT.chain(p, np.zeros(z.size), np.zeros(z.size), z)
    assert ok.tolist() == [True, True, True, False, False, False, False] * 2 and np.array_equal(ok, c["ok"])
    assert np.array_equal(h.view(np.uint32), c["h"].view(np.uint32)) and h[:3].tolist() == [fmax] * 3 and h[7:10].tolist() == [-fmax] * 3


def test_a_general_quaternion_agrees_away_from_the_cell_borders():
    """The frame of a general quaternion is rounded, not exact: the host's matrix and the truth's are the same formula, and
    the indices are required to agree on every point whose u + 0.5 and v + 0.5 lie further than 1e-9 from an integer; at
    most 0.1 % of the points may be left out, by the truth alone."""
    iso = [6_378_137.0 * 0.6, -6_378_137.0 * 0.5, 6_378_137.0 * 0.62] + GENERAL
    p = TT.params(tile_size=64, resolution_m=0.05, origin=(0.0, 0.0, 0.0), world_from_terrain=iso)
    x, y, z = cloud(11, 100_003, scale=40.0, centre=iso[:3])
    c = TT.chain(p, x, y, z)
    near = lambda a: np.abs((a + 0.5) - np.rint(a + 0.5)) <= 1e-9
    judged = c["ok"] & ~near(c["u"]) & ~near(c["v"])
    assert (~judged).sum() <= x.size // 1000
    i, j, h, ok = pcv.terrain_vertex(lib_params(p), x, y, z)
    assert ok[judged].all() and np.array_equal(i[judged], c["i"][judged]) and np.array_equal(j[judged], c["j"][judged])
    m, _ = pcv.terrain_frame(lib_params(p))
    assert np.allclose(m @ m.T, np.eye(3), atol=1e-15) and np.array_equal(m, TT.frame(iso)[0])


SHADER_EXAMPLE = np.array([[1, 1, 1], [0, 0, 1], [0, 1, 1]], dtype=bool)  # terrain.gs's picture, bottom row first


def counter_example():
    """Section 1's: quads (x - 1, y - 1), (x + 1, y - 1), (x - 1, y + 1) rendered round the unrendered quad (x, y); x = y = 2."""
    s = np.zeros((6, 6), dtype=bool)
    for qx, qy in ((1, 1), (3, 1), (1, 3)):
        s[qy:qy + 2, qx:qx + 2] = True
    assert not s[3, 3]
    return s


def parity_masks(is_set, i0=0, j0=0):
    """Two residues per axis: the id coding the issue rules out."""
    s = np.asarray(is_set, dtype=bool)
    out = np.zeros(s.shape, dtype=np.uint32)
    for r in range(s.shape[0] - 1):
        for c in range(s.shape[1] - 1):
            if s[r:r + 2, c:c + 2].all():
                out[r:r + 2, c:c + 2] |= np.uint32(1 << (((c + i0) % 2) + 2 * ((r + j0) % 2)))
    return out


@pytest.mark.parametrize("i0,j0", [(0, 0), (-7, 5), (-1, -1), (2 ** 40 + 1, -2 ** 40 - 2)])
def test_quad_masks_equal_the_truth_and_meet_the_shaders_requirement(i0, j0):
    rng = np.random.default_rng(3)
    windows = [SHADER_EXAMPLE, counter_example(), np.ones((5, 7), bool), np.zeros((4, 4), bool), np.ones((1, 9), bool), np.ones((6, 1), bool)]
    windows += [rng.random((h, w)) < fill for h, w, fill in ((17, 23, 0.5), (31, 19, 0.8), (40, 40, 0.93), (9, 64, 0.97))]
    for s in windows:
        got = pcv.terrain_quad_masks(s, i0, j0)
        assert np.array_equal(got, TT.quad_masks(s, i0, j0)) and got.max(initial=0) <= 511
        assert TT.check_property(got, s) == []
        assert not got[~s].any()
    assert not pcv.terrain_quad_masks(SHADER_EXAMPLE).any()  # no quad of the picture has four corners


def test_the_checker_refuses_parity_ids():
    s = counter_example()
    bad = TT.check_property(parity_masks(s), s)
    assert any((c, r) == (2, 2) and not rendered for c, r, _, _, rendered in bad), bad
    assert TT.check_property(TT.quad_masks(s), s) == [] and TT.check_property(pcv.terrain_quad_masks(s), s) == []


def test_tile_names():
    assert pcv.terrain_tile_name(-3, 12) == "x-0000003_y00000012"
    assert pcv.terrain_tile_name(0, 0) == "x00000000_y00000000"
    assert pcv.terrain_tile_name(12345678, -1) == "x12345678_y-0000001"
    assert pcv.terrain_tile_name(2 ** 31 - 1, -2 ** 31) == "x2147483647_y-2147483648"  # wider than the field, as {:08} leaves it
    assert pcv.terrain_tile_name(123456789, -12345678) == "x123456789_y-12345678"


def test_meta_json_round_trips_every_double():
    r3 = 1.0 / 3.0
    quat = [2.0 / 3.0, -r3, 2.0 * r3, 0.0]
    iso = [6378137.0 * 0.123456789, -6.4e6 + 0.001, 6_356_752.314245179] + quat
    origin = [0.1, 1e-7, -0.0]
    p = TT.params(tile_size=256, resolution_m=1e22, origin=origin, world_from_terrain=iso, statistic="mean", min_points=2)
    tiles = [[-3, 12], [0, 0], [5, -1]]
    text = pcv.terrain_meta_json(lib_params(p), tiles)
    meta = json.loads(text)
    assert list(meta) == ["tile_size", "world_from_terrain", "origin", "resolution_m", "tile_positions"]
    assert list(meta["world_from_terrain"]) == ["rotation", "translation"]
    same = lambda a, b: np.array_equal(np.array(a, dtype=np.float64).view(np.uint64), np.array(b, dtype=np.float64).view(np.uint64))
    assert meta["tile_size"] == 256 and meta["tile_positions"] == tiles
    assert same(meta["world_from_terrain"]["rotation"], quat) and same(meta["world_from_terrain"]["translation"], iso[:3])
    assert same(meta["origin"], origin) and same([meta["resolution_m"]], [1e22])
    assert '"origin":[0.1,1e-07,-0.0]' in text and " " not in text and "\n" not in text
    for v in meta["world_from_terrain"]["rotation"] + meta["origin"]:
        assert isinstance(v, float)  # integral values carry ".0": json gives floats, not ints
    assert '"rotation":[0.0,0.0,0.0,1.0]' in pcv.terrain_meta_json(lib_params(TT.params()), [])
    assert pcv.terrain_meta_json(lib_params(TT.params()), []).endswith('"tile_positions":[]}')


@pytest.mark.parametrize("change,word", [
    (dict(tile_size=0), "tile_size"), (dict(tile_size=4097), "tile_size"), (dict(resolution_m=0.0), "resolution_m"),
    (dict(resolution_m=-1.0), "resolution_m"), (dict(resolution_m=float("nan")), "resolution_m"),
    (dict(world_from_terrain=[0, 0, 0, 0, 0, 0.6, 0.9]), "unit length"), (dict(world_from_terrain=[0, 0, 0, 0, 0, 0, 0]), "unit length"),
    (dict(min_points=0), "min_points"), (dict(statistic=3), "statistic"), (dict(origin=(0.0, float("inf"), 0.0)), "origin"),
])
def test_parameter_errors_carry_a_code_and_a_message(change, word):
    args = dict(tile_size=4, resolution_m=1.0)
    args.update(change)
    pr = pcv.terrain_params(**args)
    lib = pcv.load_library()
    assert lib.pcv_terrain_check_params_host(C.byref(pr)) == L.PCV_E_INVALID and word in lib.pcv_host_last_error().decode()
    with pytest.raises(pcv.PcvError, match=word) as e:
        pcv.terrain_check_params(pr)
    assert e.value.code == L.PCV_E_INVALID
    with pytest.raises(pcv.PcvError, match=word):  # the other host entry points refuse the same way
        pcv.terrain_vertex(pr, [0.0], [0.0], [0.0])
    pcv.terrain_check_params(pcv.terrain_params(tile_size=4096, resolution_m=1e-3, min_points=1, statistic="mean"))


def test_params_struct_layout():
    assert C.sizeof(L.TerrainParams) == 120 and L.TerrainParams.resolution_m.offset == 8 and L.TerrainParams.origin.offset == 16
    assert L.TerrainParams.world_from_terrain.offset == 40 and L.TerrainParams.min_points.offset == 96
    assert L.TerrainParams.max_pool_bytes.offset == 104 and L.TerrainParams.staging_points.offset == 112
    assert C.sizeof(L.TerrainInfo) == 72 and L.TerrainInfo.vertex_min.offset == 48 and L.TerrainInfo.finished.offset == 64
