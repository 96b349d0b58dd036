"""xray over S2 cell clouds, the parts that need no device: the oracle of the device tests (xray_s2_oracle.S2Points) against
the brute-force filter of all points under the truth's own precondition, pcv_cloud_kind on written metas, the example's
usage, and the new declarations against the ctypes prototypes."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import meta_proto
import point_cloud_viewer_amd as pcv
import s2_region_truth as R
import xray_s2_oracle as S
from point_cloud_viewer_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (tile px, pixel size m, with the transform, split level, box) -> (leaves, created tiles), worked out with the truth
# modules. box "points": the exact min / max of the points, which is what S2Splitter's meta and pcv_s2_split carry and what
# the device tests run; box "scene": s2_region_truth.scene()'s loose box (the transformed local box), a slightly larger
# quadtree rect over the same points.
SETUPS = [((64, 0.5, True, 20, "points"), (256, 64)), ((64, 0.5, True, 16, "points"), (256, 64)),
          ((32, 0.25, True, 20, "points"), (4096, 675)), ((64, 0.5, False, 20, "points"), (64, 39)),
          ((64, 0.5, True, 20, "scene"), (256, 56)), ((32, 0.25, True, 20, "scene"), (4096, 672)),
          ((64, 0.5, False, 20, "scene"), (64, 39))]


@pytest.mark.parametrize("setup,want", SETUPS)
def test_oracle_equals_brute_force_and_the_precondition_holds(setup, want):
    W, px, transform, level, box = setup
    x, y, z, rgb, bmin, bmax = R.scene()[:6]
    sp = S.S2Points(x, y, z, rgb, None, level)
    assert sp.cell_ids.size == (675 if level == 20 else 5)
    assert np.array_equal(sp.bmin, [x.min(), y.min(), z.min()]) and np.array_equal(sp.bmax, [x.max(), y.max(), z.max()])
    if box == "scene":
        sp.bmin, sp.bmax = bmin, bmax
    iso = S.local_from_ecef() if transform else None
    g = S.geometry([sp], W, px, iso)
    bounds = R.cell_bounds(sp.cell_ids)
    created = 0
    for name, (kind, params) in zip(g["leaf_ids"], S.tile_shapes(g, iso)):
        brute, bad = S.brute_force(sp, kind, params, bounds=bounds)
        listed = sp.query_indices(kind, params)  # CPU corners: s2_region_truth.spec_corners
        assert np.array_equal(np.sort(listed), brute), name
        if brute.size:
            created += 1
            assert not bad, (name, bad)  # the cap on tiles left out of the brute-force comparison is zero
    assert (len(g["leaf_ids"]), created) == want


def test_query_order_is_cells_ascending_then_file_order():
    x, y, z, rgb = R.scene()[:4]
    sp = S.S2Points(x, y, z, rgb, None, 20)
    idx = sp.query_indices(0, None, corners=np.zeros((8, 3)))  # AllPoints: every cell
    assert idx.size == x.size and np.array_equal(np.sort(idx), np.arange(x.size))
    cells = sp.point_cell[idx]
    assert (np.diff(cells.astype(np.int64) >> 1) >= 0).all()
    same = cells[1:] == cells[:-1]
    assert (np.diff(idx)[same] > 0).all()


def _write_meta(directory, version, arm):
    m = meta_proto.classes()["Meta"]()
    m.version = version
    m.bounding_box.min.x, m.bounding_box.max.x = -1.0, 1.0
    if arm == "s2":
        c = m.s2.cells.add()
        c.id, c.num_points = 0x89c2590000000000, 3
    elif arm == "octree":
        m.octree.resolution = 0.001
    os.makedirs(directory, exist_ok=True)
    with open(os.path.join(directory, "meta.pb"), "wb") as f:
        f.write(m.SerializeToString())


def test_cloud_kind(tmp_path):
    for name, version, arm, want in (("s2", 13, "s2", "s2"), ("octree", 13, "octree", "octree"), ("old", 9, None, "octree"),
                                     ("bare", 13, None, "s2"), ("old_s2", 11, "s2", "octree")):
        _write_meta(str(tmp_path / name), version, arm)
        assert pcv.cloud_kind(tmp_path / name) == want, name
    with pytest.raises(pcv.PcvError) as e:
        pcv.cloud_kind(tmp_path / "missing")
    assert e.value.code == pcv.PCV_E_IO and "meta.pb" in str(e.value) and "missing" in str(e.value)
    kind = C.c_int(7)
    assert pcv.load_library().pcv_cloud_kind(None, C.byref(kind)) == pcv.PCV_E_INVALID


def test_example_compiles_and_names_s2_directories():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "examples")])
    p = subprocess.run([os.path.join(ROOT, "examples", "bin", "build_xray_quadtree")], capture_output=True, text=True)
    assert p.returncode == 2 and "usage" in p.stderr and "S2" in p.stderr
    p = subprocess.run([os.path.join(ROOT, "examples", "bin", "build_xray_quadtree"), "--resolution"], capture_output=True, text=True)
    assert p.returncode == 2 and "S2 cell cloud dir" in p.stderr


def test_new_declarations_agree_with_the_prototypes():
    header = open(os.path.join(ROOT, "include", "pcv_hip.h")).read()
    lib = pcv.load_library()
    ctype_of = {"pcv_ctx*": C.c_void_p, "pcv_s2_cloud* const*": C.c_void_p, "uint32_t": C.c_uint32,
                "const pcv_xray_params*": C.POINTER(_lib.XrayParams), "const pcv_xray_coloring*": C.POINTER(_lib.XrayColoring),
                "pcv_xray**": C.POINTER(C.c_void_p), "const char*": C.c_char_p, "int*": C.POINTER(C.c_int)}
    for name in ("pcv_xray_run_s2", "pcv_cloud_kind"):
        m = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert m, name
        args = [re.sub(r"/\*.*?\*/", "", a).strip() for a in " ".join(m.group(1).split()).split(",")]
        types = [re.sub(r"\s*\w+$", "", a) for a in args]  # drop the parameter name
        res, want = _lib._SIGNATURES[name]
        assert res is C.c_int and [ctype_of[t] for t in types] == want, (name, types)
        assert hasattr(lib, name)
    assert re.search(r"#define PCV_CLOUD_OCTREE 0\b", header) and re.search(r"#define PCV_CLOUD_S2 1\b", header)
    assert (_lib.CLOUD_OCTREE, _lib.CLOUD_S2) == (0, 1)
    assert lib.pcv_abi_version() == 2
