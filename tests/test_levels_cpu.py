"""csrc/pcv_levels.cpp (the level table of a cube, the promotion arithmetic of a node table: standard C++, no HIP) and
tests/levels_driver.cpp as one stand-alone program with ASan and UBSan: tame, deep, degenerate, non-finite and untamed
boxes at three level caps, and a 9-node table with its broken variants. The sanitizers must stay silent; edges and
encodings of the finite boxes equal the oracle's table entry for entry, the promotion rows equal the loaded library's."""
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O
from point_cloud_viewer_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 0xFFFFFFFF

BIG = -2.0 ** 501  # |min| above 2^500: the table is not "tame" (no unguarded exact division)
BOXES = {  # name: (min, max, resolution, finite)
    "cube100_1e-3": ((-50.0, -50.0, -50.0), (50.0, 50.0, 50.0), 1e-3, True),
    "cube100_1e-4": ((-50.0, -50.0, -50.0), (50.0, 50.0, 50.0), 1e-4, True),
    "deep_2^30": ((0.0, 0.0, 0.0), (1024.0, 1024.0, 1024.0), 2.0 ** -20, True),  # edge / resolution = 2^30: levels beyond one key word
    "zero_extent": ((3.0, 4.0, 5.0), (3.0, 4.0, 5.0), 1e-3, True),
    "one_nan": ((0.0, 0.0, 0.0), (10.0, float("nan"), 10.0), 1e-3, False),
    "one_inf": ((0.0, 0.0, 0.0), (10.0, 10.0, float("inf")), 1e-3, False),
    "min_2^501": ((BIG, BIG, BIG), (BIG + 2.0 ** 460, BIG + 2.0 ** 459, BIG + 2.0 ** 455), 1e-3, True),
}
CAPS = (1, 40, 64)


def _node(first, count, level, parent, first_child=0, child_mask=0, is_leaf=1):
    return dict(id_high=level << 56, id_low=0, first=first, count=count, level=level, parent=parent, first_child=first_child,
                child_mask=child_mask, is_leaf=is_leaf)


def nine_nodes():
    """Breadth first, children consecutive: the root with three children, two of them split again; six leaves, 122 points."""
    return [
        _node(0, 122, 0, INVALID, 1, 0b00100101, 0),
        _node(0, 25, 1, 0, 4, 0b00000011, 0), _node(25, 1, 1, 0), _node(26, 96, 1, 0, 6, 0b10010001, 0),
        _node(0, 17, 2, 1), _node(17, 8, 2, 1),
        _node(26, 64, 2, 3), _node(90, 9, 2, 3), _node(99, 23, 2, 3),
    ]


def promote_cases():
    def changed(i, **kw):
        t = nine_nodes()
        t[i].update(kw)
        return t
    two = [_node(0, 10, 0, INVALID, 1, 0b11, 0), _node(0, 10, 1, 0)]  # test_stages_cpu: two children, one entry
    return {  # name: (nodes, n, with slots)
        "nine": (nine_nodes(), 122, True),
        "nine_lengths_only": (nine_nodes(), 0, False),
        "two_children_one_entry": (two, 10, False),
        "child_before_parent": (changed(1, first_child=1), 122, True),
        "inner_without_children": (changed(3, child_mask=0), 122, True),
        "children_past_the_table": (changed(3, first_child=7), 122, True),
        "leaf_range_outside_n": (nine_nodes(), 121, True),
        "parent_out_of_range": (changed(4, parent=99), 122, True),
    }


def _library_rows(nodes, n, with_slots):
    """What the loaded library's pcv_promote_assign returns, as the driver prints it."""
    lib = L.load_library()
    arr = (L.SplitNode * len(nodes))()
    for a, nd in zip(arr, nodes):
        for k, v in nd.items():
            setattr(a, k, v)
    per = (L.PromoteNode * len(nodes))()
    node_of = np.full(n if with_slots else 0, INVALID, dtype=np.uint32)
    slot_in = np.full(n if with_slots else 0, INVALID, dtype=np.uint32)
    rc = lib.pcv_promote_assign(arr, len(nodes), per, n, node_of.ctypes.data if with_slots else None,
                                slot_in.ctypes.data if with_slots else None)
    rows = ["promote %d" % rc]
    if rc == L.PCV_OK:
        rows += ["P %d %d %d %d" % (i, p.stream_len, p.num_points, p.child_offset) for i, p in enumerate(per)]
        rows += ["Q %d %d %d" % (j, node_of[j], slot_in[j]) for j in range(node_of.size)]
    return rows


@pytest.fixture(scope="module")
def driver_output(tmp_path_factory):
    """One build and one run of the sanitizer program over every case: {case name: printed lines}."""
    tmp = tmp_path_factory.mktemp("levels")
    lines = []
    for name, (bmin, bmax, res, _) in BOXES.items():
        for cap in CAPS:
            lines.append(" ".join(["levels", "%s@%d" % (name, cap)] + [float(v).hex() for v in (*bmin, *bmax, res)] + [str(cap)]))
    for name, (nodes, n, with_slots) in promote_cases().items():
        fields = ("id_high", "id_low", "first", "count", "level", "parent", "first_child", "child_mask", "is_leaf")
        lines.append(" ".join(["promote", name, str(n), str(int(with_slots)), str(len(nodes))] +
                              [str(nd[f]) for nd in nodes for f in fields]))
    (tmp / "cases.txt").write_text("\n".join(lines) + "\n")
    exe = tmp / "levels_driver"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan",  # the runtimes inside the program: nothing to preload
                           os.path.join(ROOT, "tests", "levels_driver.cpp"),
                           os.path.join(ROOT, "point_cloud_viewer_amd", "csrc", "pcv_levels.cpp"), "-o", str(exe)])
    p = subprocess.run([str(exe), str(tmp / "cases.txt")], capture_output=True, text=True)
    cases, name = {}, None
    for line in p.stdout.splitlines():
        if line.startswith("case "):
            name = line[5:]
            cases[name] = []
        else:
            cases[name].append(line)
    return p, cases


def test_sanitizer_build_of_the_level_code_runs_clean(driver_output):
    p, cases = driver_output
    assert p.returncode == 0, (p.stdout[-1000:] + p.stderr)[-3000:]
    assert "runtime error" not in p.stderr and "Sanitizer" not in p.stderr, p.stderr[-3000:]
    assert len(cases) == len(BOXES) * len(CAPS) + len(promote_cases())


@pytest.mark.parametrize("name", [k for k, v in BOXES.items() if v[3]])
@pytest.mark.parametrize("cap", CAPS)
def test_finite_boxes_equal_the_oracle_table(driver_output, name, cap):
    _, cases = driver_output
    bmin, bmax, res, _ = BOXES[name]
    ml, edge, enc = O.level_table(bmin, bmax, res, cap)
    rows = cases["%s@%d" % (name, cap)]
    assert rows[0] == "table %d" % ml
    got = [r.split() for r in rows if r.startswith("L ")]
    assert [int(g[1]) for g in got] == list(range(ml + 1))
    assert [float.fromhex(g[2]) for g in got] == [float(e) for e in edge]  # entry for entry, bit for bit (hex floats)
    assert [int(g[3]) for g in got] == [int(c) for c in enc]
    # the kernels' copy of the table (PcvLevels) holds the same edges and encodings as far as it goes
    kept = [r.split() for r in rows if r.startswith("M ")][:min(ml, 40) + 1]
    assert [float.fromhex(m[2]) for m in kept] == [float(e) for e in edge[:len(kept)]]
    assert [int(m[5]) for m in kept] == [int(c) for c in enc[:len(kept)]]
    if name == "deep_2^30" and cap >= 40:
        assert ml == 30  # past the 21 levels of one key word
    if name == "min_2^501":
        assert rows[[r.split()[0] for r in rows].index("lv")].split()[2] == "0"  # fast_ok: not tame


@pytest.mark.parametrize("name", list(promote_cases()))
def test_promote_rows_equal_the_loaded_library(driver_output, name):
    _, cases = driver_output
    nodes, n, with_slots = promote_cases()[name]
    want = _library_rows(nodes, n, with_slots)
    assert cases[name] == want
    assert (want[0] == "promote 0") == name.startswith("nine")  # every broken variant is refused, by both
