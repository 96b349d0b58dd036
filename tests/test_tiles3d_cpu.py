"""The 3D Tiles export without a device (csrc/pcv_tiles3d_files.cpp, csrc/pcv_tiles3d_dev.h) against
tests/tiles3d_truth.py, byte for byte: pcv_tiles3d_tile_host over every encoding, mode and small size, pcv_tiles3d_tileset_json_host
over the oracle's trees of scenes A, E and K and over hand-made node tables, the parameter rules, and the same cases through a
stand-alone sanitizer build of the host code."""
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import point_cloud_viewer_amd as pcv
from point_cloud_viewer_amd import _lib as L

import oracle_lib as O
import tiles3d_truth as TT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "point_cloud_viewer_amd", "csrc")
SIZES = [1, 2, 3, 5, 9, 10, 64, 65, 99, 100, 2049]
MODES = ["auto", "quantized", "float"]
# (cube_min, cube_edge): the unit cube, and Earth-fixed cubes whose centres are no float32 values
CUBES = {"unit": ((0.0, 0.0, 0.0), 1.0), "ecef": ((4_000_123.4567, 500_000.0 + 1.0 / 3.0, -4_930_777.125), 1000.0 / 64.0)}


def make_node(enc, cube, n, seed):
    rng = np.random.default_rng(seed)
    if enc == TT.U8:
        xyz = rng.integers(0, 256, (n, 3), dtype=np.uint8)
        xyz.flat[0] = 255
    elif enc == TT.U16:
        xyz = rng.integers(0, 65536, (n, 3)).astype("<u2")
        xyz.flat[0] = 65535
    else:
        xyz = rng.random((n, 3)).astype("<f4" if enc == TT.F32 else "<f8")
        xyz.flat[0] = 1.0  # the cube's far face: trunc(65535 * 1.0) is the largest code
        if n > 1:
            xyz.flat[3], xyz.flat[4] = 0.0, np.nextafter(xyz.dtype.type(1.0), xyz.dtype.type(0.0))
    mn, edge = CUBES[cube]
    return dict(id=(0, 0), level=0, num_points=n, encoding=enc, cube_min=mn, cube_edge=edge, xyz=xyz.tobytes(),
                rgb=rng.integers(0, 256, (n, 3), dtype=np.uint8).tobytes(), intensity=(rng.random(n) * 100 - 50).astype("<f4").tobytes())


def all_cases():
    for enc in (TT.U8, TT.U16, TT.F32, TT.F64):
        for cube in CUBES:
            for n in SIZES:
                yield enc, cube, n, make_node(enc, cube, n, 1000 * enc + n)


@pytest.mark.parametrize("cube", list(CUBES))
@pytest.mark.parametrize("enc", [TT.U8, TT.U16, TT.F32, TT.F64])
def test_tile_host_equals_the_truth(enc, cube):
    for n in SIZES:
        node = make_node(enc, cube, n, 1000 * enc + n)
        for mode in MODES:
            for inten in (False, True):
                want, plan = TT.tile_file(node, mode, inten)
                got, got_plan = pcv.tiles3d_tile_host(node, node["xyz"], node["rgb"], node["intensity"] if inten else None, with_plan=True,
                                                      position_mode=mode)
                assert got == want, (enc, cube, n, mode, inten)
                for key in ("file_bytes", "feature_json_offset", "feature_binary_offset", "batch_json_offset", "batch_binary_offset"):
                    assert got_plan[key] == plan[key], key
                assert got_plan["mode"] == plan["mode"]
                # every section length and offset is a multiple of 8 (the feature JSON begins after the 28-byte header)
                magic, version, total, fj, fb, bj, bb = struct.unpack_from("<4sIIIIII", got, 0)
                assert (magic, version, total) == (b"pnts", 1, len(got)) and 28 + fj + fb + bj + bb == total
                assert (28 + fj) % 8 == 0 and fb % 8 == 0 and bj % 8 == 0 and bb % 8 == 0 and total % 8 == 0
                assert all(got_plan[k] % 8 == 0 for k in ("feature_binary_offset", "batch_json_offset", "batch_binary_offset", "file_bytes"))
                assert (bj == 0 and bb == 0) if not inten else (bj > 0 and bb == (4 * n + 7) // 8 * 8)
                ft = json.loads(got[28:28 + fj])
                assert ft["POINTS_LENGTH"] == n and ft["RGB"]["byteOffset"] == n * (6 if plan["mode"] == "quantized" else 12)


def test_the_cases_hit_every_residue_of_the_feature_json_length():
    res = set()
    for enc, cube, n, node in all_cases():
        for mode in ("quantized", "float"):
            res.add(len(TT.feature_json(node, mode)) % 8)
    assert res == set(range(8)), res


def test_rtc_is_a_float32_value_and_the_offset_is_exact():
    for cube, (mn, edge) in CUBES.items():
        node = dict(id=(0, 0), level=0, num_points=1, encoding=TT.U16, cube_min=mn, cube_edge=edge)
        rc = pcv.tiles3d_rtc(node)
        assert np.array_equal(rc, TT.rtc(node)) and np.array_equal(rc, rc.astype(np.float32).astype(np.float64))
        centre = np.array(mn) + edge / 2
        # a float32 has 24 bits: at 6.4e6 its spacing is 0.5, so the centre moves by at most 0.25
        assert np.all(np.abs(rc - centre) <= np.maximum(np.abs(centre), 1e-30) * 2.0 ** -24)
    assert np.any(pcv.tiles3d_rtc(dict(id=(0, 0), level=0, num_points=1, cube_min=CUBES["ecef"][0], cube_edge=CUBES["ecef"][1])) !=
                  np.array(CUBES["ecef"][0]) + CUBES["ecef"][1] / 2)


# ---- tileset.json -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scenes():
    O.build_oracle()
    return {name: TT.oracle_nodes(make(), O) for name, make in TT.SCENES.items()}


def test_scene_a_has_the_stated_shape(scenes):
    nodes = scenes["A"]
    enc = [n["encoding"] for n in nodes if n["num_points"] > 0]  # the encodings of the 163 nodes that become files
    by_name = {n["name"]: n for n in nodes}
    assert len(nodes) == 164 and max(n["level"] for n in nodes) == 21 and sum(n["num_points"] > 0 for n in nodes) == 163
    assert (enc.count(TT.F64), enc.count(TT.F32), enc.count(TT.U16), enc.count(TT.U8)) == (1, 58, 64, 40)
    assert by_name["r7"]["num_points"] == 0 and by_name["r4"]["num_points"] == 1 and max(n["num_points"] for n in nodes) == 2292
    k = scenes["K"]
    assert [(n["name"], n["num_points"] > 0) for n in k] == [("r", True), ("r0", False), ("r4", True)]
    e = scenes["E"]
    assert {n["encoding"] for n in e} == {TT.U8, TT.U16, TT.F32, TT.F64}
    assert any(np.any(TT.rtc(n) != np.array(n["cube_min"]) + n["cube_edge"] / 2) for n in e)


@pytest.mark.parametrize("scene", ["A", "E", "K"])
def test_tileset_of_the_oracles_trees(scenes, scene):
    nodes = scenes[scene]
    for kw in (dict(), dict(error_factor=0.25, transform=np.arange(1.0, 17.0))):
        want, names = TT.tileset(nodes, **{"error_factor": TT.DEFAULT_ERROR_FACTOR, **kw})
        got = pcv.tiles3d_tileset_json(nodes, **kw)
        assert got == want
        tiles, content = TT.check_structure(got)
        assert content == len(names) == sum(n["num_points"] > 0 for n in nodes) and tiles >= content
    assert " " not in got and "\n" not in got
    if scene == "A":
        assert '"r7.pnts"' not in got and '"r4.pnts"' in got and tiles == 163
    if scene == "K":
        assert tiles == 2 and '"r0.pnts"' not in got


def child_cube(mn, edge, c):
    h = edge / 2.0
    return (mn[0] + h * ((c >> 2) & 1), mn[1] + h * ((c >> 1) & 1), mn[2] + h * (c & 1)), h


def hand_table(paths, root_min=(10.0, -20.0, 30.5), root_edge=64.0):
    """A node table from {octal path: num_points}: every path's ancestors must be keys too."""
    nodes = []
    for path, count in paths.items():
        mn, edge, idx = root_min, root_edge, 0
        for ch in path:
            mn, edge = child_cube(mn, edge, int(ch))
            idx = idx * 8 + int(ch)
        level = len(path)
        nodes.append(dict(id=(level << 56 | idx >> 64, idx & (2 ** 64 - 1)), level=level, num_points=count, encoding=TT.U8, cube_min=mn, cube_edge=edge))
    return sorted(nodes, key=lambda n: (n["level"], TT.node_index(n)))


DEEP = "7123456701234567012345670123456701234565"  # 40 levels: the index needs 120 bits
HAND = {
    "inner node without points": {"": 5, "3": 0, "30": 2, "37": 1, "5": 4},
    "pruned subtree": {"": 5, "2": 0, "20": 0, "21": 0, "210": 0, "6": 1},
    "root without points": {"": 0, "1": 3, "4": 0},
    "level 40": dict({DEEP[:k]: 0 for k in range(40)}, **{DEEP: 5, "": 1}),
}


@pytest.mark.parametrize("name", list(HAND))
def test_tileset_of_hand_made_tables(name):
    nodes = hand_table(HAND[name])
    transform = [1.0, 0.0, 0.0, 0.0, 0.0, 0.5, 0.0, 0.0, 0.0, 0.0, 2.0, 0.0, 4e6, -1.5, 1.0 / 3.0, 1.0] if name != "pruned subtree" else None
    want, names = TT.tileset(nodes, error_factor=0.125, transform=transform)
    got = pcv.tiles3d_tileset_json(nodes, error_factor=0.125, transform=transform)
    assert got == want
    tiles, content = TT.check_structure(got)
    doc = json.loads(got)
    assert ("transform" in doc["root"]) == (transform is not None)
    if name == "inner node without points":
        mid = doc["root"]["children"][0]
        assert "content" not in mid and [c["content"]["uri"] for c in mid["children"]] == ["r30.pnts", "r37.pnts"] and (tiles, content) == (5, 4)
        assert mid["geometricError"] == 32.0 * 0.125 and mid["children"][0]["geometricError"] == 0.0
    if name == "pruned subtree":
        assert (tiles, content) == (2, 2) and [c["content"]["uri"] for c in doc["root"]["children"]] == ["r6.pnts"]
    if name == "root without points":
        assert "content" not in doc["root"] and (tiles, content) == (2, 1)
    if name == "level 40":
        assert (tiles, content) == (41, 2) and ('"r%s.pnts"' % DEEP) in got


def test_tileset_refusals():
    nodes = hand_table(HAND["inner node without points"])
    for bad, word in ((nodes[:-2] + [nodes[-1], nodes[-2]], "ascending"), ([nodes[0]] + nodes[2:], "parent"), ([], "empty"), (nodes[1:], "root"),
                      (hand_table({"": 0, "1": 0}), "no point")):
        with pytest.raises(pcv.PcvError) as e:
            pcv.tiles3d_tileset_json(bad)
        assert e.value.code == L.PCV_E_INVALID and word in str(e.value), (word, str(e.value))


def test_check_params_refusals():
    pcv.tiles3d_check_params()
    pcv.tiles3d_check_params(error_factor=0.0, chunk_bytes=4 << 20, position_mode="float", intensity=True, transform=np.eye(4))
    bad_t = np.eye(4)
    bad_t[2, 3] = np.inf
    for kw, word in ((dict(error_factor=-1e-9), "error_factor"), (dict(error_factor=np.nan), "error_factor"), (dict(error_factor=np.inf), "error_factor"),
                     (dict(transform=bad_t), "transform"), (dict(position_mode=3), "position_mode"), (dict(chunk_bytes=(4 << 20) - 1), "chunk_bytes"),
                     (dict(chunk_bytes=1), "chunk_bytes")):
        with pytest.raises(pcv.PcvError) as e:
            pcv.tiles3d_check_params(**kw)
        assert e.value.code == L.PCV_E_INVALID and word in str(e.value), (kw, str(e.value))
    pr = pcv.tiles3d_params()
    pr.flags = 6
    with pytest.raises(pcv.PcvError, match="flags"):
        pcv.tiles3d_check_params(params=pr)
    node = make_node(TT.U8, "unit", 3, 1)
    with pytest.raises(pcv.PcvError, match="no point"):
        pcv.tiles3d_tile_host(dict(node, num_points=0), b"", b"")
    assert pcv.tiles3d_params().error_factor == 0.0625 and pcv.tiles3d_params().chunk_bytes == 0


# ---- the host code under the sanitizers ---------------------------------------------------------------------------------------------
def test_sanitizer_build_of_the_host_code_runs_clean(tmp_path, scenes):
    """pcv_tiles3d_files.cpp and tests/tiles3d_host_driver.cpp as one stand-alone program with ASan and UBSan: the file cases of
    this module and the node tables, each also at truncated and oversized capacities; the results equal the truth."""
    blob, want = [], []
    for enc, cube, n, node in all_cases():
        for mode in range(3):
            for flags in (0, 1):
                mn, edge = CUBES[cube]
                blob.append(struct.pack("<5I4d", 1, enc, mode, flags, n, *mn, edge) + node["xyz"] + node["rgb"] + node["intensity"])
                want.append((0, TT.tile_file(node, MODES[mode], bool(flags))[0]))
    tables = [(scenes["K"], 0.0625, None), (scenes["A"], 0.5, list(np.arange(16.0)))]
    tables += [(hand_table(t), 0.125, None) for t in HAND.values()]
    tables += [(hand_table(HAND["pruned subtree"])[::-1], 0.125, None), (hand_table({"": 0, "1": 0}), 0.125, None)]
    for nodes, ef, tr in tables:
        b = struct.pack("<2Id16d", 2, len(nodes), ef, *(tr or [0.0] * 16))
        for n in nodes:
            b += struct.pack("<2QqII4d", n["id"][0], n["id"][1], n["num_points"], n["level"], n["encoding"], *n["cube_min"], n["cube_edge"])
        blob.append(b)
        try:
            want.append((0, TT.tileset(nodes, ef, tr)[0].encode()))
            if nodes != sorted(nodes, key=lambda n: (n["level"], TT.node_index(n))) or sum(n["num_points"] for n in nodes) == 0:
                want[-1] = (L.PCV_E_INVALID, b"")
        except Exception:
            want.append((L.PCV_E_INVALID, b""))
    (tmp_path / "cases.bin").write_bytes(struct.pack("<I", len(blob)) + b"".join(blob))
    exe = tmp_path / "tiles3d_host_driver"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan",  # the runtimes inside the program: nothing to preload
                           "-I", CSRC, os.path.join(ROOT, "tests", "tiles3d_host_driver.cpp"), os.path.join(CSRC, "pcv_tiles3d_files.cpp"),
                           os.path.join(CSRC, "pcv_terrain_files.cpp"), "-o", str(exe)])
    p = subprocess.run([str(exe), str(tmp_path / "cases.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    out, at = (tmp_path / "out.bin").read_bytes(), 0
    for k, (rc, data) in enumerate(want):
        got_rc, ln = struct.unpack_from("<iQ", out, at)
        at += 12
        assert got_rc == rc and out[at:at + ln] == data, k
        at += ln
    assert at == len(out) and len(want) == 4 * 2 * len(SIZES) * 6 + len(tables)
