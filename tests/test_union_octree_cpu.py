"""Cell unions as locations over the octree, on the CPU: pcv_s2_union_intersects_cubes_host (the chain the device walks with)
against the independent truth of s2_region_truth.py, and every refusal of the host twin with its message. No device."""
import numpy as np
import pytest

import point_cloud_viewer_amd as pcv
import s2_region_truth as R
import s2_truth as T
import union_octree_cases as U


def test_host_twin_equals_the_truth_on_every_decided_pair():
    """4 681 cubes (find_bounding_cube to depth 4 over the scene's bounding cube) x the scene's unions and a level-8 cell. The
    truth alone gives, of 23 405 evaluated pairs, 0 undecided: union 0 173 yes, 1 825, 2 125, 3 (far) 0, 5 91."""
    cubes = U.scene_cubes()
    assert cubes.shape == (4681, 4)
    unions = U.unions()
    pairs = undecided = 0
    for u, cells in enumerate(unions):
        got = pcv.s2_union_intersects_cubes(cells, cubes)
        if not cells:
            assert not got.any(), "the empty union intersects nothing"
            continue
        bounds = R.cell_bounds(cells)
        truth = [U.truth_of_cube(cells, c, bounds) for c in cubes]
        decided = np.array([t is not None for t in truth])
        want = np.array([t or 0 for t in truth], dtype=np.uint8)
        pairs += len(truth)
        undecided += int((~decided).sum())
        yes, no = int((want[decided] == 1).sum()), int((want[decided] == 0).sum())
        print(f"union {u}: {len(cells)} cells, yes {yes}, no {no}, undecided {int((~decided).sum())}")
        assert np.array_equal(got[decided], want[decided]), (u, np.nonzero(got[decided] != want[decided])[0][:8])
        if u == len(unions) - 1:
            assert yes == len(truth), "the level-8 cell holds every cube"
        elif u == 3:
            assert yes == 0, "the far cell meets no cube"
        else:
            assert yes > 0 and no > 0, (u, yes, no)
    assert undecided * 100 <= pairs, (undecided, pairs)


def test_host_twin_refusals():
    cubes = U.scene_cubes()[:3]
    c = T.parent(U.centre_leaf(), 20)
    nxt = c + ((c & -c) << 1)
    for cells, message in (([nxt, c], "the cells of a union must ascend by id: cell 1 is below its predecessor"),
                           ([0], "cell 0 of the union is 0, which is no cell id"), ([c | 2], "cell 0 is no S2 cell id"),
                           ([T.parent(U.centre_leaf(), 0)], "a union with a level-0 cell has no geometry")):
        with pytest.raises(pcv.PcvError) as e:
            pcv.s2_union_intersects_cubes(cells, cubes)
        assert e.value.code == pcv.PCV_E_INVALID and str(e.value) == "PCV_E_INVALID: " + message, (cells, str(e.value))
    assert pcv.s2_union_intersects_cubes([c, c], cubes).tolist() == pcv.s2_union_intersects_cubes([c], cubes).tolist()  # not normalized, not refused
    assert pcv.s2_union_intersects_cubes([c], np.zeros((0, 4))).size == 0


def test_children_of_a_missed_cube_may_hit_but_the_walk_stops():
    """bfs() is the contract: a node is listed iff it and all its ancestors intersect."""
    flags = np.array([1, 0, 1, 1, 1], dtype=np.uint8)
    first_child = np.array([1, 3, 0, 0, 0], dtype=np.uint32)
    child_mask = np.array([0b101, 0b11, 0, 0, 0], dtype=np.uint8)
    assert U.bfs(flags, first_child, child_mask).tolist() == [0, 2]
