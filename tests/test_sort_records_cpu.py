"""The record-sort tests' own parts, checked without a GPU: the numpy truth (tests/sort_records_truth.py) on hand-written
records, and for every case of tests/sort_records_cases.py the plan it is written to reach — from the plan driver of
tests/test_sort_plan_cpu.py and from the host-only part of pcv_sort_records (csrc/pcv_sort_records_check.cpp with
tests/sort_records_driver.cpp), both stand-alone programs under ASan and UBSan."""
import json
import os
import subprocess

import numpy as np
import pytest

import sort_records_truth as T
from sort_plan_helper import CSRC, ROOT, SANITIZE, build_driver, facts, run_facts, sanitizers_silent
from sort_records_cases import (ALL_GENERIC, ALL_PIECES, ALL_REC12, CASES, IN_HOST_MEMORY, ROWS_ON_DEVICE, check_plan, groups_and_chunk,
                                instantiation_set)

REPLAY = T.REPLAY


# ---- the truth on a dozen records ------------------------------------------------------------------------------------
def test_truth_is_stable_among_equal_ranks():
    ranks = np.array([3, 1, 3, 0, 1, 3, 2, 0, 1, 3, 3, 0], dtype=np.uint32)
    blue = np.arange(12, dtype=np.uint32) + 100
    vec = np.stack([np.arange(12, dtype=np.uint32) ^ T.X_TAG, np.arange(12, dtype=np.uint32) * 7], axis=1).astype(np.uint32)
    plane = np.arange(12, dtype=np.uint32) * 1000
    t = T.sort_truth(ranks << 8 | blue, 2, vec, [plane])
    assert t["order"].tolist() == [3, 7, 11, 1, 4, 8, 6, 0, 2, 5, 9, 10]
    assert (t["keys"] >> 8).tolist() == [0, 0, 0, 1, 1, 1, 2, 3, 3, 3, 3, 3]
    assert (t["keys"] & 0xFF).tolist() == [103, 107, 111, 101, 104, 108, 106, 100, 102, 105, 109, 110]
    assert (t["vec"][:, 0] ^ T.X_TAG).tolist() == t["order"].tolist() and t["vec"][:, 1].tolist() == [7 * i for i in t["order"]]
    assert t["planes"][0].tolist() == [1000 * i for i in t["order"]]
    # without the colour byte (a 16-byte payload) the whole key is the rank
    vec4 = np.zeros((12, 4), dtype=np.uint32)
    vec4[:, 3] = np.arange(12)
    t = T.sort_truth(ranks, 2, vec4)
    assert t["keys"].tolist() == [0, 0, 0, 1, 1, 1, 2, 3, 3, 3, 3, 3] and t["vec"][:, 3].tolist() == [3, 7, 11, 1, 4, 8, 6, 0, 2, 5, 9, 10]
    # key + planes only
    t = T.sort_truth(ranks, 2, None, [plane, plane + 1])
    assert t["vec"] is None and t["planes"][1].tolist() == [1000 * i + 1 for i in [3, 7, 11, 1, 4, 8, 6, 0, 2, 5, 9, 10]]


def test_truth_applies_the_map_and_the_replay_word():
    # predicted ranks 0..4 -> true ranks 2, 0, 2, 1, (unused); entry 2 is marked for replay
    m = np.array([2, 0, 2 | REPLAY, 1, 3], dtype=np.uint32)
    pred = np.array([0, 1, 2, 3, 2, 0, 1, 3, 2, 0, 3, 1], dtype=np.uint32)
    blue = np.arange(12, dtype=np.uint32) + 1
    vec = np.stack([np.arange(12, dtype=np.uint32) ^ T.X_TAG, np.full(12, 9, dtype=np.uint32)], axis=1).astype(np.uint32)
    t = T.sort_truth(pred << 8 | blue, 2, vec, map=m)
    assert t["true"].tolist() == [2, 0, 2, 1, 2, 2, 0, 1, 2, 2, 1, 0]
    assert t["order"].tolist() == [1, 6, 11, 3, 7, 10, 0, 2, 4, 5, 8, 9]
    assert (t["keys"] >> 8).tolist() == [0, 0, 0, 1, 1, 1, 2, 2, 2, 2, 2, 2] and (t["keys"] & 0xFF).tolist() == [2, 7, 12, 4, 8, 11, 1, 3, 5, 6, 9, 10]
    # the records that went through entry 2 (inputs 2, 4, 8) carry their input index, the others their word
    assert t["vec"][:, 0].tolist() == [1 ^ T.X_TAG, 6 ^ T.X_TAG, 11 ^ T.X_TAG, 3 ^ T.X_TAG, 7 ^ T.X_TAG, 10 ^ T.X_TAG, 0 ^ T.X_TAG, 2, 4,
                                       5 ^ T.X_TAG, 8, 9 ^ T.X_TAG]
    assert [T.input_index_at(w, 12, True) for w in t["vec"][:, 0]] == t["order"].tolist()
    # 16-byte payloads: the key is the true rank alone
    vec4 = np.zeros((12, 4), dtype=np.uint32)
    vec4[:, 0] = np.arange(12) ^ T.X_TAG
    t = T.sort_truth(pred, 2, vec4, map=m)
    assert t["keys"].tolist() == [0, 0, 0, 1, 1, 1, 2, 2, 2, 2, 2, 2] and t["vec"][7, 0] == 2


def test_truth_joins_the_colour():
    m = np.array([1, 0], dtype=np.uint32)
    pred = np.array([0, 1, 1, 0, 1, 0, 0, 1, 1, 0, 0, 1], dtype=np.uint32)
    for stride in (3, 4):
        color = (np.arange(12 * stride, dtype=np.uint32) * 37 + 5).astype(np.uint8)
        vec = np.stack([np.arange(12, dtype=np.uint32) ^ T.X_TAG, np.arange(12, dtype=np.uint32) + 0x100], axis=1).astype(np.uint32)
        t = T.sort_truth(pred << 8, 1, vec, map=m, color=color, color_stride=stride)
        order = [1, 2, 4, 7, 8, 11, 0, 3, 5, 6, 9, 10]
        assert t["order"].tolist() == order
        rgb = color.reshape(12, stride)
        for slot, i in enumerate(order):
            assert int(t["keys"][slot]) == (int(m[pred[i]]) << 8) | int(rgb[i, 2])
            assert int(t["vec"][slot, 1]) == (i + 0x100) | int(rgb[i, 0]) << 16 | int(rgb[i, 1]) << 24


def test_truth_rows_and_geometry():
    assert T.geometry(1) == (1, 8192) and T.geometry(8192) == (1, 8192) and T.geometry(8193) == (2, 8192)
    assert T.geometry(57344) == (7, 8192) and T.geometry(57345) == (8, 8192) and T.geometry(8_388_608) == (1024, 8192)
    assert T.geometry(8_388_609) == (513, 16384) and T.geometry(8_388_608 + 8_192 + 17) == (513, 16384)
    n = 8192 + 12
    pred = np.zeros(n, dtype=np.uint32)
    pred[:8192] = np.arange(8192) % 3            # chunk 0: 2731, 2731, 2730 of ranks 0, 1, 2
    pred[8192:] = [4, 4, 1, 0, 4, 1, 1, 4, 4, 0, 1, 4]  # chunk 1: the dozen
    vec = np.zeros((n, 2), dtype=np.uint32)
    rows = T.rows_truth(pred << 8 | 0xAB, vec, 6)
    assert rows.shape == (2, 6) and rows.dtype == np.uint32
    assert rows.tolist() == [[2731, 2731, 2730, 0, 0, 0], [2, 4, 0, 0, 6, 0]]
    assert T.rows_truth(pred, None, 6).tolist() == rows.tolist()  # without the colour byte the key is the rank


def test_first_difference_names_slot_and_records():
    c = T.make_case(5, 12, 2, vec_words=2, nplanes=1, map_entries=6, replay=0.5)
    t = T.sort_truth(c["keys"], 2, c["vec"], c["planes"], c["map"])
    assert T.first_difference(t["keys"], t["keys"].copy(), "keys", t, t["vec"], t["planes"][0]) is None
    got = t["vec"].copy()
    got[[4, 7]] = got[[7, 4]]  # two records swapped
    if np.array_equal(got, t["vec"]):
        pytest.fail("the generator's payloads do not tell the records apart")
    msg = T.first_difference(t["vec"], got, "vec", t, got, t["planes"][0])
    assert f"slot 4 of 12: expected input index {int(t['order'][4])} " in msg and f"input index {int(t['order'][7])};" in msg


def test_generator_makes_what_it_says():
    c = T.make_case(3, 5000, 9, vec_words=2, nplanes=2, map_entries=700, replay=0.03)
    pred = c["keys"] >> 8
    m = c["map"]
    assert pred.max() < 700 and len(m) == 700
    true = m & T.INDEX_MASK
    assert true.max() < 512 and len(np.unique(true)) < len(m)              # many to one
    assert np.any(np.diff(true.astype(np.int64)) < 0)                       # not monotone
    assert len(np.unique(pred)) < 700                                       # predicted ranks nobody has
    assert len(np.unique(true[pred])) < 512                                 # true ranks without a record
    assert 0 < np.count_nonzero(m & REPLAY) < 70
    assert np.array_equal(c["vec"][:, 0] ^ T.X_TAG, np.arange(5000))        # the payload names its record
    for p in c["planes"]:
        assert len(np.unique(p)) == 5000
    again = T.make_case(3, 5000, 9, vec_words=2, nplanes=2, map_entries=700, replay=0.03)
    assert all(np.array_equal(c[k], again[k]) for k in ("keys", "vec", "map")) and np.array_equal(c["planes"][1], again["planes"][1])
    col = T.make_case(4, 100, 3, map_entries=20, color_stride=4)
    assert not np.any(col["keys"] & 0xFF) and not np.any(col["vec"][:, 1] >> 16) and col["color"].shape == (400,)


# ---- the plan of every case ------------------------------------------------------------------------------------------------
def case_facts(c):
    rec12 = c["vec_words"] == 2
    base = 8 if rec12 else 0
    return facts(c["n"], base, base + c["key_bits"], vec_in=int(c["vec_words"] != 0), vec_bytes=4 * c["vec_words"] or 16, nwords=c["nplanes"],
                 color_in=int(c["color_stride"] != 0), map=int(c["map_entries"] != 0), map_entries=c["map_entries"], rows=int(c["rows"] is not None),
                 second=int(c["hold_second"] and c["map_entries"] != 0))


def case_line(c, nulls=0, mem=1, **over):
    """One call of tests/sort_records_driver.cpp."""
    v = dict(n=c["n"], key_bits=c["key_bits"], vec_bytes=4 * c["vec_words"], nwords=c["nplanes"], map_entries=c["map_entries"],
             rows_mode={None: 0, "given": 1, "device": 2}[c["rows"]], hold_second=int(c["hold_second"]), color_stride=c["color_stride"],
             first_in0=int(c["first_in0"]))
    v.update(over)
    return (v["n"], v["key_bits"], v["vec_bytes"], v["nwords"], v["map_entries"], v["rows_mode"], v["hold_second"], v["color_stride"],
            v["first_in0"], nulls, mem)


REFUSED = {  # a call the entry must refuse -> a word of its message
    "keys_null": (case_line(CASES["edge_n63_b7"], nulls=1), "keys is null"),
    "vec_null": (case_line(CASES["edge_n63_b7"], nulls=2), "vec is null"),
    "plane_null": (case_line(CASES["gen_v0_p3_m0_n4097_b11"], nulls=4), "plane is null"),
    "rows_null": (case_line(CASES["edge_n63_b7"], nulls=8), "rows is null"),
    "nine_planes": (case_line(CASES["gen_v0_p8_m0_n4097_b11"], nwords=9), "nwords"),
    "vec_bytes_12": (case_line(CASES["edge_n63_b7"], vec_bytes=12), "vec_bytes"),
    "no_payload": (case_line(CASES["gen_v0_p2_m0_n4097_b11"], nwords=0), "payload or a plane"),
    "no_bits": (case_line(CASES["edge_n63_b7"], key_bits=0), "key_bits"),
    "25_bits_above_the_colour": (case_line(CASES["nomap"], key_bits=25), "key_bits"),
    "33_bits": (case_line(CASES["gen_v4_p0_m0_n4097_b32"], key_bits=33), "key_bits"),
    "n_too_large": (case_line(CASES["nomap"], n=2 ** 32 - 1), "n must be < 2^32 - 1"),
    "rows_without_map": (case_line(CASES["nomap"], rows_mode=1), "rows need a map"),
    "rows_with_two_planes": (case_line(CASES["edge_n63_b7"], nwords=2), "rows need a map"),
    "rows_mode_3": (case_line(CASES["edge_n63_b7"], rows_mode=3), "rows_mode"),
    "color_without_rows": (case_line(CASES["norows_15000"], color_stride=3), "color_in"),
    "color_stride_5": (case_line(CASES["color_s3_p0_n8193_one"], color_stride=5), "color_stride"),
    "map_without_payload": (case_line(CASES["gen_v0_p2_m0_n4097_b11"], map_entries=100), "payload word"),
    "first_in0_without_plane": (case_line(CASES["edge_n63_b7"], first_in0=1), "plane0_in"),
    "16_bits_through_a_map_in_lds": (case_line(CASES["wide_b16_p0"], map_entries=12000), "half words"),
    "bad_mem": (case_line(CASES["edge_n63_b7"], mem=2), "bad mem"),
}


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    """Both sanitizer programs, each run once over the case table."""
    tmp = tmp_path_factory.mktemp("sort_records")
    plan_exe = build_driver(tmp)
    plan_run, plan_rows = run_facts(plan_exe, tmp, "cases.txt", [case_facts(c) for c in CASES.values()])
    exe = tmp / "sort_records_driver"
    subprocess.check_call(SANITIZE + [os.path.join(ROOT, "tests", "sort_records_driver.cpp"), os.path.join(CSRC, "pcv_sort_records_check.cpp"),
                                      os.path.join(CSRC, "pcv_sort_plan.cpp"), "-o", str(exe)])
    lines = [case_line(c) for c in CASES.values()] + [case_line(c, mem=0, n=0) for c in CASES.values()] + [v[0] for v in REFUSED.values()]
    (tmp / "calls.txt").write_text("".join(" ".join(str(int(x)) for x in line) + "\n" for line in lines))
    run = subprocess.run([str(exe), str(tmp / "calls.txt")], capture_output=True, text=True)
    keys = subprocess.run([str(exe), "keys"], capture_output=True, text=True)
    return plan_run, plan_rows, run, [json.loads(line) for line in run.stdout.splitlines()], keys


def test_sanitizer_builds_run_clean(drivers):
    plan_run, plan_rows, run, rows, keys = drivers
    for p in (plan_run, run, keys):
        sanitizers_silent(p)
    assert len(plan_rows) == 2 * len(CASES) and len(rows) == 2 * len(CASES) + len(REFUSED) + 1
    assert json.loads(keys.stdout) == {"key_checks_failed": 0}
    assert rows[-1] == {"null_args": 1, "bad_mem": 1}


def as_plan_info(r):
    """A row of tests/sort_plan_driver.cpp in the shape of pcv_sort_plan_info."""
    return dict(two_pass=r["two_pass"], held_back=r["held_back"], pieces=r["pieces"], blocks=r["blocks"], gpb=r["gpb"], groups=r["groups"],
                chunk=r["chunk"], passes=r["passes"])


def test_every_case_reaches_the_plan_it_is_written_for(drivers):
    _, plan_rows, _, rows, _ = drivers
    for k, c in enumerate(CASES.values()):
        from_plan, from_entry = plan_rows[2 * k], rows[k]
        assert "error" not in from_plan and "error" not in from_entry, (c["name"], from_plan, from_entry)
        check_plan(c, as_plan_info(from_plan))
        check_plan(c, from_entry)
        # the entry's facts: the rank above a colour byte for 12-byte records; and it hands back the plan's own figures
        assert (from_entry["begin"], from_entry["end"]) == ((8, 8 + c["key_bits"]) if c["vec_words"] == 2 else (0, c["key_bits"]))
        for f in ("two_pass", "held_back", "pieces", "blocks", "gpb", "groups", "chunk"):
            assert from_entry[f] == from_plan[f], (c["name"], f)
        for p, q in zip(from_entry["passes"], from_plan["passes"]):
            assert all(p[f] == q[f] for f in ("shift", "nbits", "hist", "down", "R", "MAP", "PL", "map_lds", "dyn_lds")), (c["name"], p, q)
        # the same call without records has no passes
        empty = rows[len(CASES) + k]
        assert empty["npasses"] == 0 and empty["passes"] == [] and not empty["two_pass"], (c["name"], empty)
    big = [c for c in CASES.values() if c["big"]]
    assert len(big) == 2 and all(groups_and_chunk(c) == (513, 16384) for c in big)
    assert all(n in CASES for n in ROWS_ON_DEVICE + IN_HOST_MEMORY)


def test_the_case_table_covers_every_form(drivers):
    rec12, pieces, gen = instantiation_set(rows for rows in drivers[3][:len(CASES)])
    assert rec12 == ALL_REC12 and pieces == ALL_PIECES and gen == ALL_GENERIC


def test_bad_calls_are_refused_with_a_message(drivers):
    rows = drivers[3][2 * len(CASES):-1]
    for (name, (_, word)), row in zip(REFUSED.items(), rows):
        assert word in row.get("error", ""), (name, row)
