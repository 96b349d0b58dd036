"""The plan of the record sort's first pass where the records come without their colour (csrc/pcv_sort_plan.h: packed 8-byte
records from the chain pass; 12-byte records with color_in keep their plan) and the hand-over rule of the single-chain build, on
tests/sort_plan_packed_driver.cpp (one stand-alone program with ASan and UBSan, no HIP, no library).

The LDS of a workgroup is 163 840 bytes. The first pass needs its static part (tile of 8 192 records x 12 bytes + the digit state
of 16 waves: 107 584 bytes for 128 digit values, 116 800 for 256), the map as half words and the colours' buffer
(ceil((15 + 8 192 x stride) / 16) + 1 pieces of 16 bytes: 24 608 bytes at stride 3, 32 800 at stride 4). So a packed sort keeps the
map in LDS up to (163 840 - static - buffer) / 2 entries, rounded down to whole 16 bytes of map — 15 824 / 11 216 entries at
stride 3, 11 728 / 7 120 at stride 4 — and gathers it from global memory above; these figures are worked out here from the sizes,
not read back from the code under test."""
import json
import os
import subprocess

import pytest

from sort_plan_helper import CSRC, ROOT, SANITIZE, sanitizers_silent

LDS = 163840
STATIC = {128: 8192 * 12 + 128 * 4 * 18 + 64, 256: 8192 * 12 + 256 * 4 * 18 + 64}
STATIC_PLANE = {128: 8192 * 16 + 128 * 4 * 18 + 64, 256: 8192 * 16 + 256 * 4 * 18 + 64}
BUFFER = {s: (-(-(15 + 8192 * s) // 16) + 1) * 16 for s in (3, 4)}
N = 200_000


def staged_limit(R, stride):
    return min(16384, (LDS - STATIC[R] - BUFFER[stride]) // 16 * 8)


def line(bits, map_entries, plane=0, packed=1, stride=3, rows=1, n=N):
    return (n, bits, map_entries, plane, packed, stride, rows)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("sort_plan_packed") / "sort_plan_packed_driver"
    subprocess.check_call(SANITIZE + [os.path.join(ROOT, "tests", "sort_plan_packed_driver.cpp"), os.path.join(CSRC, "pcv_sort_plan.cpp"),
                                      "-o", str(out)])
    return out


def plans(exe, tmp_path, lines):
    path = tmp_path / "facts.txt"
    path.write_text("".join(" ".join(str(v) for v in l) + "\n" for l in lines))
    p = subprocess.run([str(exe), str(path)], capture_output=True, text=True)
    sanitizers_silent(p)
    rows = [json.loads(x) for x in p.stdout.splitlines()]
    assert len(rows) == len(lines)
    return rows


def test_the_figures_the_rule_rests_on(exe):
    p = subprocess.run([str(exe), "rule"], capture_output=True, text=True)
    sanitizers_silent(p)
    rows = [json.loads(x) for x in p.stdout.splitlines()]
    assert (STATIC[128], STATIC[256], BUFFER[3], BUFFER[4]) == (107584, 116800, 24608, 32800)
    for r in (r for r in rows if "R" in r):
        assert r["static"] == STATIC[r["R"]] and r["buffer"] == BUFFER[r["stride"]] and r["attr"] == LDS - STATIC[r["R"]], r
        assert r["staged_entries"] == staged_limit(r["R"], r["stride"]), r
    assert [staged_limit(R, s) for R in (128, 256) for s in (3, 4)] == [15824, 11728, 11216, 7120]
    # the hand-over: tried for 12-byte records of raw input without an intensity plane; packed up to 65 536 predicted nodes
    for r in (r for r in rows if "tried" in r):
        assert r["tried"] == int(r["switch"] and r["compact"] and not r["routed"] and not r["intensity"]), r
    assert {r["nodes"]: r["packed"] for r in rows if "nodes" in r} == {1: 1, 65535: 1, 65536: 1, 65537: 0, 1 << 20: 0}


@pytest.mark.parametrize("stride", (3, 4))
@pytest.mark.parametrize("bits", (13, 8))  # digits of 7 bits (128 digit values) and of 8 (256)
def test_packed_map_on_both_sides_of_the_lowered_limit(exe, tmp_path, stride, bits):
    R = 128 if bits == 13 else 256
    limit = staged_limit(R, stride)
    got = plans(exe, tmp_path, [line(bits, e, stride=stride) for e in (1, limit - 1, limit, limit + 1, 16384, 16385, 65536)])
    for r in got:
        in_lds = r["map_entries"] <= limit
        assert "error" not in r, r
        assert (r["R"], r["PL"], r["pass_packed"], r["MAP"]) == (R, 0, 1, 1 if in_lds else 2), r
        assert r["dyn_lds"] == ((2 * r["map_entries"] + 15) // 16 * 16 if in_lds else 0), r
        assert r["color_lds"] == BUFFER[stride] and r["later_color_lds"] == 0, r  # the packed form always stages its colours
        assert r["lds"] <= LDS, r
    at_limit = next(r for r in got if r["map_entries"] == limit)
    assert LDS - at_limit["lds"] < 16, at_limit  # the limit is the last map that fits


def test_packed_is_refused_outside_its_form(exe, tmp_path):
    got = plans(exe, tmp_path, [line(13, 65537), line(13, 9000, plane=1), line(13, 9000, rows=0), line(13, 65536), line(13, 9000)])
    assert ["error" in r for r in got] == [True, True, True, False, False], got
    assert all("packed records" in r["error"] for r in got[:3])


@pytest.mark.parametrize("stride", (3, 4))
def test_color_in_records_keep_their_plan_and_their_loads_per_lane(exe, tmp_path, stride):
    """12-byte records with color_in: the map's place is what it is without the colour (16 384 entries in LDS, which leaves no room
    for the colours' buffer: 107 584 + 32 768 + 24 608 > 163 840), so no buffer is planned for them, with or without the plane."""
    entries = (300, 9000, staged_limit(128, stride), staged_limit(128, stride) + 1, 16384, 16385)
    got = plans(exe, tmp_path, [line(13, e, packed=0, stride=stride) for e in entries] + [line(13, 9000, plane=1, packed=0, stride=stride)])
    assert STATIC[128] + 2 * 16384 + BUFFER[3] > LDS
    for r in got[:-1]:
        assert r["MAP"] == (1 if r["map_entries"] <= 16384 else 2) and r["pass_packed"] == 0, r
        assert r["dyn_lds"] == ((2 * r["map_entries"] + 15) // 16 * 16 if r["MAP"] == 1 else 0), r
        assert r["color_lds"] == 0 and r["lds"] <= LDS, r
    plane = got[-1]
    assert plane["PL"] == 1 and plane["color_lds"] == 0 and STATIC_PLANE[128] + BUFFER[stride] > LDS
