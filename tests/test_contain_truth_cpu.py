"""The truths of contain_truth.py against the CPU oracle, and what its planted inputs are worth.

Oriented boxes and frusta have the longest f64 chains of the query path (quat_rotate, m4_transform_point, the three-product
corner sums of the SAT); random points and random shapes never come within an ulp of a face, so comparing them with the oracle
decides nothing about the last bit. Here: the oracle equals the exact rule on the exact scenes (no exceptions) and on bulk
points outside the chain's forward error bound; every planted face gets both flags, every planted family leaves its target on
both sides; and a build of the oracle's own sources with `-ffp-contract=fast -mfma` — the change a kernel edit or a dropped
build flag makes on the device — is caught by the planted inputs and by nothing random.

Measured (x86-64 with FMA, g++ -O2):

    fused build != oracle, planted points:     4 677 of 22 800 (oriented boxes), 2 548 of 22 800 (frusta)
    fused build != oracle, planted relations:  116 (oriented boxes), 42 (frusta), of 312 shapes x 612 cubes each;
                                               the touching cube's Relation changes within 23 of the 48 families
    fused build != oracle, random points:      0 of 1 000 000
    bulk points inside the error bound (left out): 0 of 600 000
"""
import ctypes as C
import subprocess

import numpy as np
import pytest

import contain_truth as T
import oracle_lib as O

KIND = {"obb": O.SHAPE_OBB, "frustum": O.SHAPE_FRUSTUM, "frustum2": O.SHAPE_FRUSTUM2}


class MakeFrustum:
    """The reference's Perspective3 + Frustum::new as the oracle restates them: matrices only."""
    perspective = staticmethod(O.perspective3_new)
    from_perspective = staticmethod(O.frustum_new)

    def __call__(self, eye, quat, persp):
        return O.frustum_new(eye, quat, O.perspective3_new(*persp))


MAKE_FRUSTUM = MakeFrustum()


def params_of(shape):
    return np.concatenate([np.asarray(p, dtype=np.float64).ravel() for p in shape[1:]])


def node_cubes(target=None, extent=64.0, levels=4):
    """Every cube of levels 0..levels-1 of [0, extent]^3 (min xyz, edge), and the target cube (min xyz, edge) with its 26 neighbours."""
    cubes = []
    for level in range(levels):
        e = extent / 2 ** level
        g = np.arange(2 ** level) * e
        gx, gy, gz = (v.ravel() for v in np.meshgrid(g, g, g, indexing="ij"))
        cubes.append(np.stack([gx, gy, gz, np.full(gx.size, e)], axis=1))
    if target is not None:
        m, e = target
        cubes.append(np.array([[m[0] + dx * e, m[1] + dy * e, m[2] + dz * e, e] for dx in (0, -1, 1) for dy in (0, -1, 1) for dz in (0, -1, 1)]))
    return np.concatenate(cubes)


@pytest.fixture(scope="module")
def planted():
    return {scale: T.planted_points_scene(scale, MAKE_FRUSTUM) for scale in T.SCALES}


@pytest.fixture(scope="module")
def node_shapes():
    cubes = [(m, e) for _, m, e in T.node_cube_targets(24)]
    return cubes, T.planted_node_shapes(MAKE_FRUSTUM, cubes)


def test_exact_scenes_equal_the_exact_rule():
    s = T.obb_exact_scene()
    assert len(s["shapes"]) == 23 and s["finite"] == 17 ** 3
    for sh, want in zip(s["shapes"], s["want"]):
        got = O.cull_points(O.SHAPE_OBB, params_of(("obb", *sh)), s["x"], s["y"], s["z"]).astype(bool)
        assert np.array_equal(got, want), sh
    assert sum(s["on_face"][:20]) == 6120 and min(s["on_face"][:20]) > 100  # kept points ON a face: a scene that lost its ties fails
    assert s["on_face"][20] > 0 and not s["want"][21].any() and not s["want"][22].any()  # flat: its own plane; negative, NaN: nothing
    assert not any(w[s["finite"]:].any() for w in s["want"])  # NaN / inf coordinates are in no box
    f = T.frustum_exact_scene()
    assert f["finite"] == 33 * 17 * 21
    for m, want in zip(f["shapes"], f["want"]):
        got = O.cull_points(O.SHAPE_FRUSTUM, m, f["x"], f["y"], f["z"]).astype(bool)
        assert np.array_equal(got, want)
    assert f["kept"][0] == 851 and f["on_plane"][0] == 578 and min(f["on_plane"]) >= 45 and sum(f["on_plane"]) > 3000
    assert f["kept"][-1] > 0  # the zero bottom row: no division, still a slab of kept points
    # the scalar rules (Fractions, the formulas as the reference writes them) agree with the array rules
    rng = np.random.default_rng(2)
    for k in rng.integers(0, s["finite"], 60):
        p = (s["x"][k], s["y"][k], s["z"][k])
        assert all(T.obb_contains_exact(*sh, p) == bool(w[k]) for sh, w in zip(s["shapes"][::5], s["want"][::5]))
    for k in rng.integers(0, f["finite"], 60):
        p = (f["x"][k], f["y"][k], f["z"][k])
        assert all(T.frustum_contains_exact(m, p) == bool(w[k]) for m, w in zip(f["shapes"], f["want"]))


def test_python_chains_are_the_oracle(planted):
    """obb_contains_f64 / frustum_contains_f64 (what the planted shapes are walked with) flag for flag on planted points."""
    for scale, sc in planted.items():
        pick = np.arange(0, sc["x"].size, 37)
        for i, sh in enumerate(sc["shapes"][::3]):
            want = O.cull_points(KIND[sh[0]], params_of(sh), sc["x"][pick], sc["y"][pick], sc["z"][pick]).astype(bool)
            if sh[0] == "obb":
                got = [T.obb_contains_f64(*sh[1:], (sc["x"][k], sc["y"][k], sc["z"][k])) for k in pick]
            else:
                got = [T.frustum_contains_f64(sh[1], (sc["x"][k], sc["y"][k], sc["z"][k])) for k in pick]
            assert np.array_equal(np.array(got), want), (scale, i)


@pytest.mark.parametrize("scale", list(T.SCALES))
def test_bulk_points_equal_the_exact_rule_outside_the_error_bound(planted, scale):
    rng = np.random.default_rng(11 if scale == "local" else 12)
    shapes = planted[scale]["shapes"]
    left_out = total = 0
    for sh in shapes[:3] + shapes[10:13]:
        x, y, z = (T.SCALES[scale][a] + rng.uniform(0.0, 64.0, 50_000) for a in range(3))
        got = O.cull_points(KIND[sh[0]], params_of(sh), x, y, z).astype(bool)
        if sh[0] == "obb":
            want, _, margin = T.obb_exact(*sh[1:], x, y, z)
            decided = margin > T.obb_error_bound(sh[1], x, y, z)
        else:
            want, _, gap, w = T.frustum_exact(sh[1], x, y, z)
            decided = T.frustum_decided(sh[1], x, y, z, gap, w)
        assert np.array_equal(got[decided], want[decided]), sh[0]
        assert want.any() and not want.all()
        left_out += int((~decided).sum())
        total += x.size
    print(f"bulk points left out at {scale}: {left_out} of {total}")
    assert left_out * 10_000 <= total  # the cap; measured 0


def test_every_planted_face_gets_both_flags(planted):
    for scale, sc in planted.items():
        assert len(sc["shapes"]) == 20
        for i, sh in enumerate(sc["shapes"]):
            keep = O.cull_points(KIND[sh[0]], params_of(sh), sc["x"], sc["y"], sc["z"]).astype(bool)
            mine = sc["owner"] == i
            for face in range(6):
                k = keep[mine & (sc["face"] == face)]
                assert k.size == 190 and k.any() and not k.all(), (scale, i, sh[0], face)


def _both_sides(shapes, first, count, target):
    flags = {int(O.cull_points(KIND[shapes[first + j][0]], params_of(shapes[first + j]), [target[0]], [target[1]], [target[2]])[0]) for j in range(count)}
    return flags == {0, 1}


def test_every_planted_family_leaves_its_target_on_both_sides(node_shapes):
    _, (families, shapes) = node_shapes
    assert len(shapes) == 624
    for kind, corner, first in families:
        assert _both_sides(shapes, first, 13, corner), (kind, corner)
    # stored points: decoded positions of an oracle-built ECEF octree, every encoding it has
    rng = np.random.default_rng(4)
    x, y, z = (T.SCALES["ecef"][a] + np.concatenate([rng.uniform(0.0, 30000.0, 20_000), 15000.0 + rng.normal(0.0, 0.03, 10_000)]) for a in range(3))
    bmin, bmax = np.array([x.min(), y.min(), z.min()]), np.array([x.max(), y.max(), z.max()])
    with O.max_points_per_node(400):
        tree = O.build_closed(0.001, bmin, bmax, x, y, z, np.zeros((x.size, 3), np.uint8), threads=4)
    targets, encodings = [], set()
    for name, nd in tree.nodes.items():
        if nd["num_points"] and nd["encoding"] not in encodings:
            encodings.add(nd["encoding"])
            cmin, edge = O.find_bounding_cube(*nd["id"], *_root_cube(bmin, bmax))
            px, py, pz = O.decode_positions(nd["encoding"], cmin, edge, nd["xyz"])
            targets.append(np.array([px[0], py[0], pz[0]]))
    assert encodings == {1, 2, 3, 4}, encodings  # UInt8, UInt16, Float32, Float64
    families, shapes = T.planted_stored_shapes(MAKE_FRUSTUM, targets)
    for fam in families:
        p = targets[fam["target"]]
        assert _both_sides(shapes, fam["first"], fam["count"], p), fam
        if fam["kind"] == "pair":  # kept at the closed face, dropped one step inside it: the chain, and the exact rule too
            closed, lower = shapes[fam["first"]], shapes[fam["first"] + 1]
            assert fam["exact"] and T.obb_contains_exact(*closed[1:], p) and not T.obb_contains_exact(*lower[1:], p)
            assert O.cull_points(O.SHAPE_OBB, params_of(closed), [p[0]], [p[1]], [p[2]])[0] == 1


def _root_cube(bmin, bmax):
    out, edge = np.zeros(3), C.c_double()
    O.lib().pcvo_cube_bounding(bmin.ctypes.data_as(O._dp), bmax.ctypes.data_as(O._dp), out.ctypes.data_as(O._dp), C.byref(edge))
    return out, edge.value


def _fused_oracle(tmp_path):
    """The oracle's two sources with contraction allowed and FMA available, every other flag as oracle/Makefile has it."""
    so = tmp_path / "libpcv_oracle_fused.so"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-fopenmp", "-fno-fast-math", "-ffp-contract=fast", "-mfma", "-shared",
                           "-Wl,-Bsymbolic", "-o", str(so), f"{O.ORACLE_DIR}/pcv_oracle_build.cpp", f"{O.ORACLE_DIR}/pcv_oracle_query.cpp", "-lm"])
    lib = C.CDLL(str(so))
    lib.pcvo_cull_points.argtypes = O.lib().pcvo_cull_points.argtypes
    lib.pcvo_cull_cubes.argtypes, lib.pcvo_cull_cubes.restype = O.lib().pcvo_cull_cubes.argtypes, C.c_int
    return lib


def _cull_points(lib, shape, x, y, z):
    x, y, z, p = (np.ascontiguousarray(v, dtype=np.float64) for v in (x, y, z, params_of(shape)))
    keep = np.zeros(x.size, dtype=np.uint8)
    lib.pcvo_cull_points(KIND[shape[0]], O._d(p), x.size, O._d(x), O._d(y), O._d(z), None, None, keep.ctypes.data_as(O._u8p))
    return keep


def _cull_cubes(lib, shape, cubes):
    cubes, p = np.ascontiguousarray(cubes, dtype=np.float64).ravel(), np.ascontiguousarray(params_of(shape))
    rel = np.zeros(cubes.size // 4, dtype=np.uint8)
    assert lib.pcvo_cull_cubes(KIND[shape[0]], O._d(p), rel.size, O._d(cubes), rel.ctypes.data_as(O._u8p), None) == 0
    return rel


def _has_fma():
    try:
        with open("/proc/cpuinfo") as f:
            return any(line.startswith("flags") and " fma " in line + " " for line in f)
    except OSError:
        return False


@pytest.mark.skipif(not _has_fma(), reason="the host CPU has no FMA: a contracted build cannot run here")
def test_the_planted_inputs_catch_a_contracted_build_and_random_ones_do_not(planted, node_shapes, tmp_path):
    fused, real = _fused_oracle(tmp_path), O.lib()
    points = {"obb": 0, "frustum2": 0}
    for sc in planted.values():
        for i, sh in enumerate(sc["shapes"]):
            differ = _cull_points(real, sh, sc["x"], sc["y"], sc["z"]) != _cull_points(fused, sh, sc["x"], sc["y"], sc["z"])
            points[sh[0]] += int(differ[sc["owner"] == i].sum())
    targets, (families, shapes) = node_shapes
    relations, seen, touching = {"obb": 0, "frustum2": 0}, set(), 0
    for (kind, corner, first), target in zip(families, [t for t in targets for _ in range(2)]):
        cubes = node_cubes(target)
        rows = []
        for j in range(13):
            a, b = _cull_cubes(real, shapes[first + j], cubes), _cull_cubes(fused, shapes[first + j], cubes)
            relations[kind] += int((a != b).sum())
            seen |= set(a.tolist())
            rows.append(a[-27])
        touching += len(set(rows)) > 1
    print(f"families in which the touching cube's Relation changes: {touching} of {len(families)}")
    rng = np.random.default_rng(1)
    random = 0
    for scale, sc in planted.items():
        for sh in sc["shapes"][::4]:
            x, y, z = (T.SCALES[scale][a] + rng.uniform(0.0, 64.0, 100_000) for a in range(3))
            random += int((_cull_points(real, sh, x, y, z) != _cull_points(fused, sh, x, y, z)).sum())
    print(f"fused != oracle: planted points {points}, planted relations {relations}, random points {random} of 1 000 000")
    assert points["obb"] > 0 and points["frustum2"] > 0
    assert relations["obb"] > 0 and relations["frustum2"] > 0 and seen == {0, 1, 2}
    assert random == 0  # the gap: nothing random ever sees the last bit
