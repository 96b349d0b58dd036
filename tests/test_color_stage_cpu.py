"""csrc/pcv_color_stage.h — the address plan of the record sort's cooperative colour load — played on the CPU by
tests/color_stage_driver.cpp (one stand-alone program with ASan and UBSan, no HIP, no library). The kernel's guarantee that no
load touches a byte outside the caller's colour array rests on this plan: the driver fetches every piece exactly as the plan
says (one aligned 16-byte copy, or byte by byte) from an array with nothing readable behind its last byte, for strides 3 and 4,
every pointer offset 0..15, n = 1, 2, 5, 6, 8191, 8192, 8193, 16385 and tiles that start at tile multiples and at chunk starts
that are only 4-record-aligned, and reads every record's colour back out of the staged buffer."""
import json
import os
import subprocess

import pytest

from sort_plan_helper import ROOT, SANITIZE, sanitizers_silent

NS = (1, 2, 5, 6, 8191, 8192, 8193, 16385)
TILE = 8192
STARTS = (4, 8, 12, 8196, 8200, 8204)


@pytest.fixture(scope="module")
def played(tmp_path_factory):
    exe = tmp_path_factory.mktemp("color_stage") / "color_stage_driver"
    subprocess.check_call(SANITIZE + [os.path.join(ROOT, "tests", "color_stage_driver.cpp"), "-o", str(exe)])
    p = subprocess.run([str(exe)], capture_output=True, text=True)
    return p, [json.loads(line) for line in p.stdout.splitlines()]


def tile_bases(n):
    bases = list(range(0, n, TILE))
    for s in STARTS:
        bases += [b for b in (s, s + TILE) if b < n]
    return bases


def test_sanitizers_stay_silent_and_every_combination_ran(played):
    p, rows = played
    sanitizers_silent(p)
    assert {(r["stride"], r["offset"], r["n"]) for r in rows} == {(s, o, n) for s in (3, 4) for o in range(16) for n in NS}
    assert len(rows) == 2 * 16 * len(NS)


def test_no_byte_outside_the_array_and_every_colour_found(played):
    for r in played[1]:
        assert r["bad"] == "", r
        bases = tile_bases(r["n"])
        assert r["tiles"] == len(bases)
        assert r["records"] == sum(min(TILE, r["n"] - b) for b in bases)  # every record of every tile read back and compared


def test_the_residues_that_occur_are_covered(played):
    """base x stride mod 16 over 4-record-aligned chunk starts: 0, 4, 8, 12 at stride 3 and 0 alone at stride 4."""
    for r in played[1]:
        if r["n"] == 16385:
            assert r["residues"] == (0x1111 if r["stride"] == 3 else 0x0001), r


def test_partial_pieces_only_at_the_ends_of_the_array(played):
    """An aligned array that is a multiple of 16 bytes long has no partial piece at all; the one-record arrays are one partial
    piece (no byte in front of the first record, none behind the last); a full tile behind a skewed start needs the buffer's
    last piece."""
    for r in played[1]:
        whole = r["offset"] == 0 and (r["n"] * r["stride"]) % 16 == 0
        if whole:
            assert r["partial"] == 0, r
        if r["n"] == 1:
            assert (r["tiles"], r["full"], r["records"]) == (1, 0, 1), r
            assert r["partial_bytes"] == r["stride"] and r["partial"] in (1, 2), r  # (two pieces where the record straddles a boundary)
        if r["n"] == 16385:
            most = -(-(15 + TILE * r["stride"]) // 16)
            assert r["max_pieces"] == (most if (r["stride"] == 3 or r["offset"] != 0) else most - 1), r
