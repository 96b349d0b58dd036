"""The generator of the sharded-build fuzz proves its own coverage: from the oracle and the level table alone (no sharded code but
the pure plan), the 120 seeded cases and the named ones of tests/sharded_cases.py reach every branch the fuzz is there for. The
bounds are conditions: a change of the draw that loses one has to change the seeds or the draw, never the bound."""
import numpy as np

import oracle_lib as O
import sharded_cases as SC

IDS = SC.all_cases()


def _count(pred):
    return sum(1 for cid in IDS if pred(SC.get(cid), SC.facts(cid)))


def test_case_dicts_are_well_formed():
    assert len(SC.SEEDS) == 120 and len(set(SC.CONSTRUCTED)) == len(SC.CONSTRUCTED)
    keys = {"x", "y", "z", "rgb", "intensity", "bmin", "bmax", "res", "cap", "world", "shard_mode", "compress", "cuts", "views",
            "regime", "kind"}
    for cid in IDS:
        c = SC.get(cid)
        n = c["x"].size
        assert keys <= set(c), cid
        assert c["y"].size == n and c["z"].size == n and c["rgb"].shape == (n, 3), cid
        assert c["intensity"] is None or c["intensity"].shape == (n,), cid
        assert c["cuts"].size == c["world"] + 1 and c["cuts"][0] == 0 and c["cuts"][-1] == n and np.all(np.diff(c["cuts"]) >= 0), cid
        assert n <= 70_000 and c["world"] in SC.WORLDS and c["shard_mode"] in SC.SHARD_MODES, cid
    assert SC.get(3) is SC.get(3)  # one draw per case, shared by every test of a session
    again = SC.case.__wrapped__(3)
    assert all(np.array_equal(again[k], SC.get(3)[k]) for k in ("x", "y", "z", "rgb", "cuts")), "the draw is seeded"


def test_every_level_1_coding_and_both_unsplittable_cubes_occur():
    for enc in (1, 2, 3, 4):  # u8, u16, Float32, Float64 (codec.rs:31-40)
        assert _count(lambda c, f: f["enc1"] == enc and f["max_level"] >= 2) >= 5, enc
    # A cube whose level-1 nodes cannot split while an octant holds more than the capacity: once with a resolution of at least the
    # root edge and once with one in [edge / 2, edge). The level table has no max_level 0 (the root always gets its level-1 children,
    # make_level_table / generation.rs:128-150), so the coarsest cube there is shows as max_level 1 as well.
    assert min(SC.facts(cid)["max_level"] for cid in IDS) == 1

    def stuck(c, f):
        return f["max_level"] == 1 and not f["can_split"] and f["octant_max"] > c["cap"]

    edge = lambda c: float(np.max(c["bmax"] - c["bmin"]))
    assert _count(lambda c, f: stuck(c, f) and c["res"] >= edge(c)) >= 1
    assert _count(lambda c, f: stuck(c, f) and edge(c) / 2 <= c["res"] < edge(c)) >= 1
    # the raw exchange with a forced level-1 split under a global layout: a level 1 that is not Float32 coded, split by the plan
    for enc in (1, 2, 4):
        assert _count(lambda c, f: f["enc1"] == enc and f["split_mask"] != 0 and c["world"] > 1) >= 3, enc


def test_plans_spread_octants_leave_ranks_idle_and_slices_empty():
    def spread(c, f):
        return any(len(set(f["rank_of"][8 * o:8 * o + 8][f["counts"][8 * o:8 * o + 8] > 0].tolist())) > 1 for o in range(8))

    assert _count(spread) >= 10
    assert _count(lambda c, f: f["counts"].sum() > 0 and np.any(f["owned"] == 0)) >= 5
    assert _count(lambda c, f: f["ranks_without_input"] > 0) >= 10
    # an empty slice strictly between two that hold points
    def hole(c, f):
        full = np.nonzero(np.diff(c["cuts"]))[0]
        return full.size >= 2 and np.any(np.diff(c["cuts"])[full[0]:full[-1]] == 0)

    assert _count(hole) >= 10
    assert _count(lambda c, f: 0 < c["x"].size < c["world"]) >= 3          # fewer points than ranks
    assert _count(lambda c, f: f["ranks_with_input"] == 1 and c["world"] > 1) >= 5  # everything on one rank


def test_every_world_size_and_cut_kind_occurs():
    for world in SC.WORLDS:
        assert _count(lambda c, f: c["world"] == world) >= 5, world
    for kind in SC.CUT_KINDS:
        assert _count(lambda c, f: c["cut_kind"] == kind) >= 5, kind
    for mode in SC.SHARD_MODES:
        assert _count(lambda c, f: c["shard_mode"] == mode) >= 20, mode
    assert _count(lambda c, f: c["views"]) >= 20 and _count(lambda c, f: not c["views"]) >= 20
    assert _count(lambda c, f: c["intensity"] is not None) >= 20
    # slices that end inside a routing tile and inside a group of four, passed as views (the general kernels)
    assert _count(lambda c, f: c["views"] and np.any(c["cuts"][1:-1] % 4 != 0)) >= 10
    assert _count(lambda c, f: np.any(np.diff(c["cuts"]) > SC.TILE) and np.any(c["cuts"][1:-1] % SC.TILE != 0)) >= 10
    # the octants-only plan of a compressed exchange on slices whose first coordinate is not 16-byte aligned (pcv_route_plan's
    # general kernel) and on aligned ones (its streaming kernel)
    def octant_plans(c, f, odd):
        if not (f["compressed"] and c["shard_mode"] == "octants"):
            return False
        starts = c["cuts"][:-1][np.diff(c["cuts"]) > 0]
        return bool(np.any((starts % 2 == 1) & c["views"])) if odd else bool(np.any((starts % 2 == 0) | (not c["views"])))

    assert _count(lambda c, f: octant_plans(c, f, True)) >= 3 and _count(lambda c, f: octant_plans(c, f, False)) >= 5
    # several routing tiles on every one of 8 ranks
    assert _count(lambda c, f: c["world"] == 8 and np.all(np.diff(c["cuts"]) > 2 * SC.TILE)) >= 1


def test_points_lie_on_the_centre_planes():
    assert _count(lambda c, f: f["on_planes"] >= 100) >= 15


def test_one_tree_is_deeper_than_21_levels():
    c = SC.constructed("deep_tree")
    with O.max_points_per_node(c["cap"]):
        want = O.build_closed(c["res"], c["bmin"], c["bmax"], c["x"], c["y"], c["z"], c["rgb"], threads=4)
    assert max(nd["level"] for nd in want.nodes.values()) > 21 and c["x"].size <= 8_000


def test_the_branch_tally_has_its_lower_bounds():
    """What tests/test_gpu_sharded_fuzz.py must count at its end: the two-pass and the one-pass compressed routes, the raw exchange
    and plans that split a level-1 node all occur, many times."""
    t = SC.tally_expected(IDS)
    assert t["cases"] == len(IDS)
    assert t["compressed_cases"] >= SC.MIN_COMPRESSED_CASES and t["two_pass_ranks"] >= SC.MIN_TWO_PASS_RANKS, t
    assert t["one_pass_ranks"] >= SC.MIN_ONE_PASS_RANKS and t["raw_cases"] >= SC.MIN_RAW_CASES, t
    assert t["split_cases"] >= SC.MIN_SPLIT_CASES, t
