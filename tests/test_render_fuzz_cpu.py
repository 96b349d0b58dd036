"""What the inputs of test_gpu_render_fuzz.py reach, proved on the CPU from the oracle's node tables and the numpy frame of
tests/render_oracle.py alone: the oracle's windowed coverage against the predicate on every pixel, the planted f32 values, the
exact point counts at the chunk seams, and the chunk and pixel totals that send the stride loops round twice."""
import numpy as np
import pytest

import render_cases as RC
import render_oracle as R
import visible_cases as VC

F32 = np.float32
IDENTITY_LUT = np.arange(256, dtype=np.uint8)
CUS = 256  # the CU count the stride preconditions are stated for; the GPU test asserts them again for the device's own


@pytest.fixture(scope="module")
def planted():
    return RC.oracle_scene(RC.planted_cloud())


def test_planted_positions_decode_exactly(planted):
    tn = planted["tn"]
    assert sorted(planted["oracle"].nodes) == ["r", "r0"] and {tn.node(k)["encoding"] for k in ("r", "r0")} == {4}
    p = np.concatenate([RC.positions(tn, "r"), RC.positions(tn, "r0")])
    assert sorted(map(tuple, p.tolist())) == sorted(map(tuple, planted["pts"].tolist()))


@pytest.mark.parametrize("axis", [0, 1])
def test_windowed_coverage_equals_the_predicate_on_every_pixel(planted, axis):
    """draw_nodes tests the predicate in a window around each point; here it is tested on every pixel of the image, and for
    these dyadic positions in exact arithmetic too. Every view draws one point, whose window depth is 0.5."""
    tn = planted["tn"]
    p = np.concatenate([RC.positions(tn, k) for k in ("r", "r0")])
    views = RC.planted_views(axis)
    for W, H, ps in RC.PLANT_CASES[axis]:
        extent = (W, H)[axis]
        for j, m in enumerate(views):
            t = RC.PLANT_T[j]
            want = R.render_view(tn, m, W, H, ps, 1.0, 0, IDENTITY_LUT)
            assert want["status"] == 0 and want["drawn"] == ["r", "r0"] and want["points_drawn"] == 1, (W, H, ps, j)
            draw, xw, yw, zw = RC.window(m, p, W, H)
            assert draw.sum() == 1 and tuple(p[draw][0, :2]) == ((t, 32.0) if axis == 0 else (32.0, t))
            assert float((xw, yw)[axis][0]) == t * extent / 64.0 and float((xw, yw)[1 - axis][0]) == 0.5 * (H, W)[axis]
            assert ((zw >= 0) & (zw <= 1)).all() and float(zw[0]) == 0.5
            cov = want["depth"] < 1.0
            assert np.array_equal(cov, RC.brute_force_coverage(xw, yw, ps, W, H)), (W, H, ps, j)
            run = RC.exact_run(t, extent, ps)
            line = cov.any(axis=0) if axis == 0 else cov.any(axis=1)[::-1]
            assert np.nonzero(line)[0].tolist() == run and want["pixels_covered"] == len(run) * min(int(ps), (H, W)[axis]), (W, H, ps, j)
            # the half-open ends: the pixel whose centre is xw - h is covered, the one whose centre is xw + h is not
            lo_px, hi_px = t * extent / 64.0 - ps / 2.0 - 0.5, t * extent / 64.0 + ps / 2.0 - 0.5
            if lo_px == int(lo_px) and 0 <= lo_px < extent:
                assert int(lo_px) in run
            if hi_px == int(hi_px) and 0 <= hi_px < extent:
                assert int(hi_px) not in run


def test_planted_ends_are_reached():
    """Both kinds of window coordinate (whole and half-whole) have a pixel centre exactly on each end of the square at sizes 1, 2, 3
    and 64; xw == 0 covers nothing at size 1, xw == W the last column."""
    on_lo, on_hi = set(), set()
    for ps in (1.0, 2.0, 3.0, 64.0):
        for t in RC.PLANT_T:
            lo_px, hi_px = t - ps / 2.0 - 0.5, t + ps / 2.0 - 0.5
            if lo_px == int(lo_px) and 0 <= lo_px < 64:
                on_lo.add(ps)
            if hi_px == int(hi_px) and 0 <= hi_px < 64:
                on_hi.add(ps)
    assert on_lo == {1.0, 2.0, 3.0, 64.0} and on_hi == {1.0, 2.0, 3.0, 64.0}
    assert RC.exact_run(0.0, 64, 1.0) == [] and RC.exact_run(64.0, 64, 1.0) == [63]
    assert RC.exact_run(0.0, 16384, 64.0) == list(range(32)) and RC.exact_run(64.0, 16384, 64.0) == list(range(16352, 16384))
    assert RC.exact_run(32.0, 16384, 64.0) == list(range(8160, 8224))


def test_w_at_flt_max_and_one_step_into_infinity():
    s = RC.oracle_scene(RC.fltmax_cloud())
    tn = s["tn"]
    m1, m2 = RC.fltmax_views()
    p = np.concatenate([RC.positions(tn, k) for k in ("r", "r0")])
    assert p[:, 2].tolist() == [0.0, 1.0, 2.0, 3.0]
    w1, w2 = R.clip_f32(m1, p)[3], R.clip_f32(m2, p)[3]
    assert w1.tolist() == [RC.FLT_MAX, RC.FLT_MAX, np.inf, np.inf] and w2.tolist() == [RC.FLT_MAX, np.inf, np.inf, np.inf]
    # in f64 the pair of the first view is one step apart, on the two sides of the rounding limit
    w64 = (RC.W_STEP * p[:, 2]) + m1[15]
    assert w64[2] == RC.W_LIMIT and w64[2] - w64[1] == RC.W_STEP and np.nextafter(w64[1], np.inf) == w64[2]
    for m, drawn in ((m1, 2), (m2, 1)):
        names = tn.visible(m)
        assert names == ["r", "r0"]  # a list, not a panic: status 0
        want = R.render_view(tn, m, 5, 5, 1.0, 1.0, 0, IDENTITY_LUT)
        assert want["status"] == 0 and want["points_submitted"] == 4 and want["points_drawn"] == drawn
        _, _, _, zw = RC.window(m, p, 5, 5)
        assert ((zw >= 0) & (zw <= 1)).all()


@pytest.mark.parametrize("enc", [1, 2, 3, 4])
def test_leaf_clouds_hold_the_intended_counts(enc):
    per = RC.PER[enc]
    assert RC.leaf_counts(enc) == [per - 1, per, per + 1, 2 * per + 63, 2 * per + 64, 2 * per + 65]
    assert sorted({n % 64 for n in RC.leaf_counts(enc)}) == [0, 1, 63]
    for n in RC.leaf_counts(enc):
        cloud = RC.leaf_cloud(enc, n)
        s = RC.oracle_scene(cloud)
        tn, nodes = s["tn"], s["oracle"].nodes
        assert sorted(nodes) == ["r", "r0"] and nodes["r0"]["num_points"] == n and nodes["r0"]["encoding"] == enc
        assert nodes["r"]["num_points"] == cloud["total"] - n
        views = RC.leaf_views(cloud)
        for m in views:
            assert tn.visible(m) == ["r", "r0"]
        # point k lands on pixel k % 256, from the decoded positions
        ranks = RC.drawn_ranks(tn, ["r", "r0"])
        assert sorted(ranks.tolist()) == list(range(cloud["total"]))
        p = np.concatenate([RC.positions(tn, k) for k in ("r", "r0")])
        draw, xw, yw, zw = RC.window(views[0], p, RC.LEAF_W, RC.LEAF_H)
        assert draw.all()
        pix = (RC.LEAF_H - 1 - np.floor(yw).astype(np.int64)) * RC.LEAF_W + np.floor(xw).astype(np.int64)
        assert np.array_equal(pix, ranks % 256) and (xw != np.floor(xw)).all() and (yw != np.floor(yw)).all()
        # depth decreases with k from layer to layer
        order = np.argsort(ranks)
        layers = zw[order].reshape(-1)[:cloud["total"] // 256 * 256].reshape(-1, 256)
        assert (layers.max(axis=1)[1:] < layers.min(axis=1)[:-1]).all()
        real = R.render_view(tn, views[0], RC.LEAF_W, RC.LEAF_H, 1.0, 1.0, 0, IDENTITY_LUT)
        flat = R.render_view(tn, views[1], RC.LEAF_W, RC.LEAF_H, 1.0, 1.0, 0, IDENTITY_LUT)
        assert real["pixels_covered"] == flat["pixels_covered"] == 256 and len(np.unique(flat["depth"])) == 1
        k_real, k_flat = ranks[real["winner"]], ranks[flat["winner"]]
        top = np.arange(256) + (cloud["total"] - 1 - np.arange(256)) // 256 * 256  # the largest k of every pixel
        assert np.array_equal(k_real.ravel(), top) and np.array_equal(k_flat.ravel(), np.arange(256))
        # the winners of the real view sit in the leaf's last chunks, those of the flat view in the first chunk of both nodes
        assert (real["winner"] >= nodes["r"]["num_points"]).sum() >= 200
        assert not np.array_equal(real["image"], flat["image"])


@pytest.mark.parametrize("enc", [1, 2, 3, 4])
def test_multi_node_trees_cut_behind_a_ragged_multi_chunk_node(enc):
    cloud = RC.multi_cloud(enc)
    s = RC.oracle_scene(cloud)
    tn, m, per = s["tn"], RC.multi_view(cloud), RC.PER[enc]
    names = tn.visible(m)
    i, max_nodes = RC.multi_cut(tn, enc, m)
    nd = tn.node(names[i])
    assert 0 < i < max_nodes - 1 and max_nodes < len(names)
    assert nd["encoding"] == enc and nd["num_points"] > per and nd["num_points"] % per != 0
    want = R.render_view(tn, m, 33, 17, 2.0, 1.0, max_nodes, IDENTITY_LUT)
    assert want["drawn"] == names[:max_nodes] and want["pixels_covered"] > 100
    # pixels won by points of that node's last chunk, and by points of the nodes behind it
    before = sum(tn.node(k)["num_points"] for k in names[:i])
    last_chunk = before + nd["num_points"] // per * per
    win = want["winner"][want["winner"] >= 0]
    assert ((win >= last_chunk) & (win < before + nd["num_points"])).any() and (win >= before + nd["num_points"]).any()


def test_seam_views_cover_pixels_at_every_odd_size():
    tn = RC.tree("A")["tn"]
    views = RC.seam_views()
    assert sum(w * h % 64 != 0 for w, h in RC.ODD_SIZES) >= 4
    assert [tn.visible(m) is None for m in views] == [False, False, True, False, False]
    for w, h in RC.ODD_SIZES:
        covered = [R.render_view(tn, m, w, h, 1.0, 1.0, 0, IDENTITY_LUT)["pixels_covered"] for m in views]
        assert covered[2] == 0 and all(covered[v] > 0 for v in (0, 1, 3, 4)), ((w, h), covered)


def test_stride_cases_exceed_a_resident_grid_of_256_cus():
    a, b = RC.tree("A")["tn"], RC.tree("B")["tn"]
    w, h = RC.RESOLVE_SIZE
    views = RC.resolve_stride_views(CUS)
    assert len(views) * w * h >= 1.2 * RC.pixel_threshold(CUS) and all(a.visible(m) for m in views)
    per_view = RC.drawn_chunks(b, b.visible(VC.ortho()))
    assert 5000 < per_view <= VC.NODES["B"]  # every node that holds points, one chunk each
    views = RC.splat_stride_views(CUS, per_view)
    chunks = sum(RC.drawn_chunks(b, b.visible(m)) for m in views)
    assert chunks >= 2 * RC.chunk_threshold(CUS), (chunks, len(views))


def test_random_plan_draws_at_least_40_views():
    tn = RC.tree("A")["tn"]
    plan = RC.random_plan()
    assert [len(mats) for mats, _, _ in plan] == [16, 16, 16, 16, 4]
    assert all(size in RC.ODD_SIZES[1:] for _, size, _ in plan) and sum(len(mats) for mats, _, ps in plan if ps == 64.0) <= 4
    drawn = panics = 0
    for mats, (w, h), ps in plan[:4]:
        for m in mats:
            want = R.render_view(tn, m, w, h, ps, 1.0, 0, IDENTITY_LUT)
            drawn += want["status"] == 0 and want["pixels_covered"] > 0
            panics += want["status"] is None
    assert drawn >= 40 and panics >= 1, (drawn, panics)
