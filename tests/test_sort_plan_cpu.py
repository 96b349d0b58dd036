"""csrc/pcv_sort_plan.cpp (what a radix sort launches, from its facts: standard C++, no HIP) and tests/sort_plan_driver.cpp as
one stand-alone program with ASan and UBSan. The sanitizers must stay silent; the invariants of the plan hold over a sweep of
sizes, bit counts, payload shapes, map sizes and switches; the cases below are pinned value for value as the sort's host code
had them before the plan existed (radix_sort of csrc/pcv_sort.hip at the commit named in tests/golden/sort_launches.json)."""
import json
import subprocess

import pytest

from sort_plan_helper import (KEYS, REC12_CHUNKS, REC12_PIECES, REC_PLANES, REC_UINT2, REC_UINT4, ROWS, ROWS_TRUE, UPSWEEP, UPSWEEP_MAP,
                              build_driver, facts, run_facts)

SETTLE_512, SETTLE_1024_PLANE, SETTLE_1024_R256 = range(3)
NS = (1, 4095, 4096, 4097, 8209, 65535, 65536, 200000, 10 ** 8, 2 * 10 ** 8, 5 * 10 ** 8, 2 ** 32 - 2)
MAPS = (0, 1, 4999, 5000, 5001, 10000, 10001, 16384, 16385, 32768, 65536)


def rec12(n, bits, plane=0, map_entries=8000, **kw):
    """The single-chain build's record sort: 12-byte records, the rank in bits [8, 8 + bits), map, rows and second given."""
    return facts(n, 8, 8 + bits, vec_in=1, vec_bytes=8, nwords=plane, map=1, map_entries=map_entries, rows=1, second=1, **kw)


PINNED = {
    "u64_keys": facts(10 ** 6, 0, 63, key_bytes=8),
    "pairs_13_bits": facts(10 ** 6, 0, 13, nwords=1),
    "rec12": rec12(200_000, 13),
    "rec12_plane": rec12(200_000, 13, plane=1),
    "rec12_plane_map_12000": rec12(200_000, 13, plane=1, map_entries=12000),
    "rec12_50000": rec12(50_000, 13),
    "rec12_17_bits": rec12(200_000, 17),
    "rank15_default_bins": rec12(8 * 10 ** 6, 15),
    "rank15_bins_32768": rec12(8 * 10 ** 6, 15, bins=32768),
    "rank16_bins_65536": rec12(8 * 10 ** 6, 16, bins=65536),
    "rank16_bins_65536_plane": rec12(8 * 10 ** 6, 16, plane=1, bins=65536),
    "msd": rec12(200_000, 13, sort_msd=1),
    "rows2_off": rec12(200_000, 13, sort_rows2=0),
    "n_too_large": facts(2 ** 32 - 1, 0, 32),
    "records_with_u64_keys": facts(1000, 0, 40, key_bytes=8, nwords=1),
    "no_keys": facts(0, 0, 32),
    "no_bits": facts(1000, 12, 12),
}


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """One build of the sanitizer program, one run over the sweep and one over the pinned cases."""
    tmp = tmp_path_factory.mktemp("sort_plan")
    exe = build_driver(tmp)
    sweep = subprocess.run([str(exe), "sweep"], capture_output=True, text=True)
    pinned, rows = run_facts(exe, tmp, "pinned.txt", PINNED.values())
    return sweep, pinned, {name: (rows[2 * i], rows[2 * i + 1]) for i, name in enumerate(PINNED)} if len(rows) == 2 * len(PINNED) else {}


@pytest.fixture(scope="module")
def sweep_rows(driver):
    return [json.loads(line) for line in driver[0].stdout.splitlines()]


def test_sanitizer_build_of_the_plan_runs_clean(driver):
    for p in driver[:2]:
        assert p.returncode == 0, (p.stdout[-1000:] + p.stderr)[-3000:]
        assert "runtime error" not in p.stderr and "Sanitizer" not in p.stderr, p.stderr[-3000:]
    assert len(driver[2]) == len(PINNED)


def test_the_sweep_covers_what_it_says(sweep_rows):
    plans = [r for r in sweep_rows if "passes" in r]
    assert not [r for r in sweep_rows if "error" in r]
    assert {r["n"] for r in plans} == set(NS)
    assert {r["end"] for r in plans if r["key_bytes"] == 8} == set(range(1, 65))
    assert {r["end"] - r["begin"] for r in plans if r["key_bytes"] == 4 and not r["rec12"]} == set(range(1, 33))
    assert {r["map_entries"] for r in plans if r["rec12"] and r["rows"]} == set(MAPS)
    shapes = {(r["vec_in"], r["vec_bytes"] if r["vec_in"] else 0, r["nwords"]) for r in plans}
    assert shapes >= {(0, 0, 0), (0, 0, 1), (0, 0, 8), (1, 16, 0), (1, 16, 1), (1, 16, 4), (1, 8, 0), (1, 8, 1), (1, 8, 2), (1, 8, 4)}
    assert {(r["sort_rows2"], r["sort_msd"], r["bins"]) for r in plans} == {(1, 0, 0), (0, 0, 0), (1, 1, 0), (1, 0, 32768), (1, 0, 65536)}
    assert any(r["two_pass"] and r["held_back"] for r in plans) and any(r["two_pass"] and r["msd"] for r in plans)


def _bins(n, forced):
    return forced or (65536 if n >= 5 * 10 ** 8 else 32768 if n >= 2 * 10 ** 8 else 16384)


def check_plan(r):
    total = r["end"] - r["begin"]
    passes = r["passes"]
    records = bool(r["vec_in"] or r["nwords"])
    is_rec12 = bool(r["vec_in"] and r["vec_bytes"] == 8 and r["nwords"] <= 1)
    assert (r["records"], r["rec12"], r["with_plane"]) == (records, is_rec12, is_rec12 and r["nwords"] == 1)
    # the digits tile [begin, end) exactly; records: as few passes as 8-bit digits allow, of equal width except the last
    by_shift = sorted(passes, key=lambda p: p["shift"])
    at = r["begin"]
    count = -(-total // 8)
    width = -(-total // count) if records else 8
    for k, p in enumerate(by_shift):
        assert p["shift"] == at and 1 <= p["nbits"] <= 8
        assert p["nbits"] == (width if k + 1 < len(by_shift) else r["end"] - at)
        at += p["nbits"]
    assert at == r["end"] and len(passes) == count
    assert r["result_in_a"] == (len(passes) % 2 == 0)
    # geometry
    tile = 8192 if is_rec12 else 4096
    assert 1 <= r["groups"] <= 1024 and r["chunk"] % tile == 0 and r["chunk"] > 0
    assert r["groups"] * r["chunk"] >= r["n"] > (r["groups"] - 1) * r["chunk"]
    # the forms of the passes
    rows_form = bool(r["map"] and r["rows"] and is_rec12)
    two = bool(rows_form and r["sort_rows2"] and count == 2 and r["map_entries"] <= _bins(r["n"], r["bins"]) and
               (1 << total) <= _bins(r["n"], r["bins"]) and r["groups"] >= 8)
    assert r["two_pass"] == two and r["msd"] == (two and r["sort_msd"]) and r["held_back"] == (two and r["second"] and not r["sort_msd"])
    if not r["msd"]:
        assert passes == by_shift
    for k, p in enumerate(passes):
        if rows_form and (k == 0 or two):
            assert p["hist"] == (ROWS_TRUE if two else ROWS) and p["down"] == (REC12_PIECES if k else REC12_CHUNKS)
        elif k == 0 and r["map"] and r["vec_in"]:
            assert p["hist"] == UPSWEEP_MAP and p["map_lds"] == (0 < r["map_entries"] <= 15000)
        else:
            assert p["hist"] == UPSWEEP and p["plain_add"] == (records and k > 0) and not p["map_lds"]
        if not (rows_form and (k == 0 or two)):
            assert p["down"] == (REC12_CHUNKS if is_rec12 else KEYS if not records else
                                 REC_UINT2 if r["vec_in"] and r["vec_bytes"] == 8 else REC_UINT4 if r["vec_in"] else REC_PLANES)
        if p["down"] in (REC12_CHUNKS, REC12_PIECES):
            assert p["R"] == (128 if p["nbits"] <= 7 else 256) and p["PL"] == r["with_plane"]
        # the map: in LDS as half words where the kernel form admits it, inside what the form may ask for
        if rows_form and k == 0:
            assert p["MAP"] in (1, 2) and (p["MAP"] == 1) <= (r["map_entries"] <= p["lds_entries"])
            assert p["dyn_lds"] == ((2 * r["map_entries"] + 15) // 16 * 16 if p["MAP"] == 1 else 0)
            if not r["msd"]:
                assert (p["MAP"] == 1) == (r["map_entries"] <= p["lds_entries"])
        else:
            assert p["MAP"] == 0 and p["dyn_lds"] == 0
        assert p["dyn_lds"] <= p["lds_attr"]
    if two:
        assert r["pieces"] == (1 << passes[0]["nbits"]) * r["blocks"] <= 1024 and r["blocks"] >= 1 and r["gpb"] * r["blocks"] >= r["groups"]
        assert r["settles"] == (passes[1]["nbits"] <= 7 or not r["with_plane"]) and r["settles_without_blob"] == (not r["with_plane"])


def test_plan_invariants_over_the_sweep(sweep_rows):
    plans = [r for r in sweep_rows if "passes" in r]
    assert len(plans) > 100_000
    for r in plans:
        try:
            check_plan(r)
        except AssertionError:
            print(r)
            raise


def check_scratch(s):
    hist, totals, hist2, totals2, ranges, order, rows_true, end = s["scratch"]
    assert hist == 0
    assert [totals - hist, hist2 - totals, totals2 - hist2, ranges - totals2, order - ranges, rows_true - order] == \
        [256 * 1024 * 4, 256 * 4, 256 * 1024 * 4, 256 * 4, 1024 * 8, 1024 * 4]  # in the stated order, back to back: disjoint
    assert all(v % 4 == 0 for v in s["scratch"]) and ranges % 8 == 0
    assert end == s["bytes"] - 256
    bins = _bins(s["n"], s["bins"])
    assert s["rows_true_bins"] == bins
    assert end - rows_true == (bins * 1024 * 4 if s["groups8192"] >= 8 else 0)
    assert (s["groups8192"] >= 8) == (s["n"] > 7 * 8192)


def test_scratch_layout_over_the_sweep(sweep_rows, driver):
    rows = [r for r in sweep_rows if "scratch" in r]
    assert {(r["n"], r["bins"]) for r in rows} == {(n, b) for n in NS for b in (0, 32768, 65536)}
    for r in rows + [v[1] for v in driver[2].values()]:
        check_scratch(r)
    by = {(r["n"], r["bins"]): r["rows_true_bins"] for r in rows}
    assert [by[n, 0] for n in (10 ** 8, 2 * 10 ** 8, 5 * 10 ** 8)] == [16384, 32768, 65536]


def _passes(r, *keys):
    return [tuple(p[k] for k in keys) for p in r["passes"]]


def test_pinned_keys_only_and_generic_record_sorts(driver):
    r, _ = driver[2]["u64_keys"]
    check_plan(r)
    assert (r["groups"], r["chunk"], r["result_in_a"]) == (245, 4096, 1)
    assert _passes(r, "shift", "nbits", "hist", "plain_add", "down") == [(8 * k, 8, UPSWEEP, 0, KEYS) for k in range(7)] + [(56, 7, UPSWEEP, 0, KEYS)]
    r, _ = driver[2]["pairs_13_bits"]
    check_plan(r)
    assert _passes(r, "shift", "nbits", "hist", "plain_add", "down") == [(0, 7, UPSWEEP, 0, REC_PLANES), (7, 6, UPSWEEP, 1, REC_PLANES)]
    assert r["result_in_a"] == 1


def test_pinned_two_pass_rows_form(driver):
    r, s = driver[2]["rec12"]
    check_plan(r)
    assert (r["groups"], r["chunk"]) == (25, 8192)
    assert (r["two_pass"], r["msd"], r["held_back"], r["result_in_a"]) == (1, 0, 1, 1)
    assert _passes(r, "shift", "nbits", "hist", "down", "R", "PL", "MAP", "dyn_lds") == \
        [(8, 7, ROWS_TRUE, REC12_CHUNKS, 128, 0, 1, 16000), (15, 6, ROWS_TRUE, REC12_PIECES, 128, 0, 0, 0)]
    assert (r["blocks"], r["gpb"], r["pieces"]) == (8, 4, 1024)
    assert r["passes"][0]["nbits"] == 7  # PcvSortSecond::low_bits of the held-back pass
    assert (r["settles"], r["settle_form"]) == (1, SETTLE_512)
    assert s["bytes"] == 69_220_608
    r, _ = driver[2]["rec12_plane"]
    check_plan(r)
    assert _passes(r, "R", "PL", "MAP", "dyn_lds") == [(128, 1, 1, 16000), (128, 1, 0, 0)]  # 8 000 <= 10 000 entries
    assert (r["two_pass"], r["held_back"], r["settles"], r["settles_without_blob"], r["settle_form"]) == (1, 1, 1, 0, SETTLE_1024_PLANE)
    r, _ = driver[2]["rec12_plane_map_12000"]
    check_plan(r)
    assert _passes(r, "R", "PL", "MAP", "dyn_lds") == [(128, 1, 2, 0), (128, 1, 0, 0)]


def test_pinned_one_rows_pass_then_generic_passes(driver):
    r, s = driver[2]["rec12_50000"]
    check_plan(r)
    assert r["groups"] == 7 and not r["two_pass"] and not r["held_back"] and r["result_in_a"] == 1
    assert _passes(r, "shift", "nbits", "hist", "plain_add", "down", "R", "MAP") == \
        [(8, 7, ROWS, 0, REC12_CHUNKS, 128, 1), (15, 6, UPSWEEP, 1, REC12_CHUNKS, 128, 0)]
    assert s["bytes"] == 2_111_744
    r, _ = driver[2]["rec12_17_bits"]
    check_plan(r)
    assert not r["two_pass"] and r["result_in_a"] == 0
    assert _passes(r, "shift", "nbits", "hist", "down") == \
        [(8, 6, ROWS, REC12_CHUNKS), (14, 6, UPSWEEP, REC12_CHUNKS), (20, 5, UPSWEEP, REC12_CHUNKS)]


def test_pinned_wide_ranks_and_switches(driver):
    r, _ = driver[2]["rank15_default_bins"]
    check_plan(r)
    assert not r["two_pass"] and _passes(r, "shift", "nbits", "hist") == [(8, 8, ROWS), (16, 7, UPSWEEP)]  # 1 << 15 > 16 384
    r, _ = driver[2]["rank15_bins_32768"]
    check_plan(r)
    assert r["two_pass"] and _passes(r, "shift", "nbits", "R") == [(8, 8, 256), (16, 7, 128)]
    r, _ = driver[2]["rank16_bins_65536"]
    check_plan(r)
    assert r["two_pass"] and _passes(r, "shift", "nbits", "R") == [(8, 8, 256), (16, 8, 256)]
    assert (r["settles"], r["settle_form"]) == (1, SETTLE_1024_R256)
    r, _ = driver[2]["rank16_bins_65536_plane"]
    check_plan(r)
    assert r["two_pass"] and r["held_back"] and not r["settles"]  # no LDS for 256 digit values next to the plane
    r, _ = driver[2]["msd"]
    check_plan(r)
    assert (r["two_pass"], r["msd"], r["held_back"], r["result_in_a"]) == (1, 1, 0, 1)
    assert _passes(r, "shift", "nbits", "down") == [(15, 6, REC12_CHUNKS), (8, 7, REC12_PIECES)]  # p1 and p2 swapped
    r, _ = driver[2]["rows2_off"]
    check_plan(r)
    assert not r["two_pass"] and _passes(r, "shift", "nbits", "hist") == [(8, 7, ROWS), (15, 6, UPSWEEP)]


def test_pinned_refusals_and_empty_sorts(driver):
    assert driver[2]["n_too_large"][0]["error"] == "radix sort: n must be < 2^32 - 1"
    assert driver[2]["records_with_u64_keys"][0]["error"] == "record sort needs 32-bit keys"
    for name in ("no_keys", "no_bits"):
        r, _ = driver[2][name]
        assert r["passes"] == [] and r["result_in_a"] == 1 and not r["two_pass"]
