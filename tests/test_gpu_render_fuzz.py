"""pcv_render_views where its three kernels take the branches the first tests never reached: waves that hold pixels
of two views, planes and groups that are no multiple of a wave, the second trip of the grid-stride loops, chunks and 64-lane
tails of exact sizes in every encoding, and points planted on the f32 edges of the clip and coverage rules. The inputs are
those of tests/render_cases.py; test_render_fuzz_cpu.py proves on the CPU that they reach those places. Every comparison goes
through test_gpu_render.check_views: images, depth bits and every info field against tests/render_oracle.py, byte for byte."""
import numpy as np
import pytest
import torch

import point_cloud_viewer_amd as pcv
import render_cases as RC
import render_oracle as R
import visible_cases as VC
from test_gpu_render import check_views

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = pcv.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def trees(ctx):
    out = {key: dict(RC.tree(key), tree=RC.gpu_tree(ctx, key)) for key in "AB"}
    for s in out.values():
        assert sorted(s["tree"].node_names()) == sorted(s["oracle"].nodes)
    yield out
    for s in out.values():
        s["tree"].free()


@pytest.fixture(scope="module")
def planted(ctx):
    s = RC.gpu_scene(ctx, RC.planted_cloud())
    yield s
    s["tree"].free()


def frusta(ctx, mats):
    return ctx.shapes([("frustum", m) for m in mats])


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def test_odd_planes_and_view_seams(ctx, trees):
    """Planes of 1 .. 4095 pixels: with all five views in one group the waves of render_resolve hold pixels of two (at 1 x 1, of
    all five) views; with groups of 1 and of 2, 2, 1 views the groups end inside a wave."""
    s = trees["A"]
    tree, tn, views = s["tree"], s["tn"], RC.seam_views()
    shapes = frusta(ctx, views)
    assert sum(w * h % 64 != 0 for w, h in RC.ODD_SIZES) >= 4
    for w, h in RC.ODD_SIZES:
        runs = []
        for k in (None, 1, 2):
            rv = tree.render(shapes, w, h, depth=True, max_workspace_bytes=None if k is None else 8 * w * h * k)
            wants = check_views(rv, tree, tn, views, w, h, shapes=shapes)
            runs.append((rv.images().cpu().numpy(), rv.depth().cpu().numpy(), [rv.info(v) for v in range(5)]))
            # a range that starts at an odd view
            assert np.array_equal(rv.images(1, 3).cpu().numpy(), runs[-1][0][1:4])
            assert np.array_equal(rv.depth(3, 2).cpu().numpy().view(np.uint32), runs[-1][1][3:5].view(np.uint32))
            rv.close()
        for img, dep, infos in runs[1:]:
            assert np.array_equal(img, runs[0][0]) and np.array_equal(dep.view(np.uint32), runs[0][1].view(np.uint32)) and infos == runs[0][2]
        covered = [x["pixels_covered"] for x in wants]
        # views 0 | 1 and 3 | 4 meet at a seam with pixels covered on both of its sides; view 2 is the singular matrix
        assert covered[2] == 0 and wants[2]["status"] is None and all(covered[v] > 0 for v in (0, 1, 3, 4)), ((w, h), covered)


def test_resolve_takes_its_stride_loop_twice(ctx, trees):
    s = trees["A"]
    w, h = RC.RESOLVE_SIZE
    views = RC.resolve_stride_views(cus())
    assert len(views) * w * h > RC.pixel_threshold(cus()) == 8 * cus() * 256  # one group: the default workspace holds them all
    assert 8 * w * h * len(views) <= 2 << 30
    rv = s["tree"].render(frusta(ctx, views), w, h)
    wants = check_views(rv, s["tree"], s["tn"], views, w, h)
    assert all(x["pixels_covered"] > 1000 for x in wants)
    rv.close()


def test_splat_takes_its_stride_loop_twice(ctx, trees):
    s = trees["B"]
    tn = s["tn"]
    per_view = RC.drawn_chunks(tn, tn.visible(VC.ortho()))
    views = RC.splat_stride_views(cus(), per_view)
    chunks = sum(RC.drawn_chunks(tn, tn.visible(m)) for m in views)
    assert chunks > RC.chunk_threshold(cus()) == 8 * cus() * 4
    rv = s["tree"].render(frusta(ctx, views), 33, 17, point_size=1.0)
    wants = check_views(rv, s["tree"], tn, views, 33, 17)
    assert all(x["points_drawn"] == 60_000 and x["pixels_covered"] > 100 for x in wants)
    rv.close()


@pytest.mark.parametrize("enc", [1, 2, 3, 4])
def test_chunk_seams_in_a_single_leaf(ctx, enc):
    """A leaf of per - 1 .. 2 per + 65 points whose colours carry the point's index: the winner of every pixel, decoded from the
    device's image, is the oracle's; with real depth it comes from the leaf's last chunk and 64-lane tail, with the depth
    flattened from the head of both nodes."""
    for n in RC.leaf_counts(enc):
        s = RC.gpu_scene(ctx, RC.leaf_cloud(enc, n))
        tree, tn = s["tree"], s["tn"]
        assert tn.node("r0")["num_points"] == n and tn.node("r0")["encoding"] == enc
        views = RC.leaf_views(s)
        rv = tree.render(frusta(ctx, views), RC.LEAF_W, RC.LEAF_H)
        wants = check_views(rv, tree, tn, views, RC.LEAF_W, RC.LEAF_H)
        imgs = rv.images().cpu().numpy()
        assert not np.array_equal(imgs[0], imgs[1])
        ranks = RC.drawn_ranks(tn, ["r", "r0"])
        for v in range(2):
            assert wants[v]["drawn"] == ["r", "r0"] and wants[v]["pixels_covered"] == 256 and wants[v]["points_drawn"] == s["total"]
            assert np.array_equal(RC.colour_rank(imgs[v][..., :3]), ranks[wants[v]["winner"]]), (n, v)
        top = np.arange(256) + (s["total"] - 1 - np.arange(256)) // 256 * 256
        assert np.array_equal(RC.colour_rank(imgs[0][..., :3]).ravel(), top)
        assert np.array_equal(RC.colour_rank(imgs[1][..., :3]).ravel(), np.arange(256))
        rv.close()
        tree.free()


@pytest.mark.parametrize("enc", [1, 2, 3, 4])
def test_chunk_seams_inside_a_draw_list(ctx, enc):
    """A node in the middle of the draw list with several chunks, the last of them ragged; max_nodes cuts the list behind it."""
    s = RC.gpu_scene(ctx, RC.multi_cloud(enc))
    tree, tn, m = s["tree"], s["tn"], RC.multi_view(s)
    i, max_nodes = RC.multi_cut(tn, enc, m)
    shapes = frusta(ctx, [m, m])
    for cut in (max_nodes, 0):
        rv = tree.render(shapes, 33, 17, point_size=2.0, max_nodes=cut)
        wants = check_views(rv, tree, tn, [m, m], 33, 17, point_size=2.0, max_nodes=cut, shapes=shapes)
        assert len(wants[0]["drawn"]) == (cut or wants[0]["nodes_visible"]) > i + 1 and wants[0]["pixels_covered"] > 100
        rv.close()
    tree.free()


def test_w_at_flt_max_is_drawn_and_infinity_is_not(ctx):
    s = RC.gpu_scene(ctx, RC.fltmax_cloud())
    tree, tn = s["tree"], s["tn"]
    views = RC.fltmax_views()
    p = np.concatenate([RC.positions(tn, k) for k in ("r", "r0")])
    w = [R.clip_f32(m, p)[3].tolist() for m in views]
    assert w[0] == [RC.FLT_MAX, RC.FLT_MAX, np.inf, np.inf] and w[1] == [RC.FLT_MAX, np.inf, np.inf, np.inf]
    rv = tree.render(frusta(ctx, views), 5, 5, depth=True)
    wants = check_views(rv, tree, tn, views, 5, 5)
    assert [x["status"] for x in wants] == [0, 0] and [x["points_submitted"] for x in wants] == [4, 4]
    assert wants[0]["points_drawn"] == 2 and wants[1]["points_drawn"] == 1
    assert rv.info(0)["points_drawn"] == rv.info(1)["points_drawn"] + 1
    rv.close()
    tree.free()


@pytest.mark.parametrize("axis", [0, 1])
def test_exact_pixel_centres_and_border_clamps(ctx, planted, axis):
    """One planted point per view, at whole and half-whole window coordinates, at 0 and at the extent: the covered run of the
    device's image equals the run of the predicate in exact arithmetic — the pixel whose centre is xw - h in, the one whose
    centre is xw + h out — at point sizes 1, 2, 3 and 64, on a 64-pixel axis and at the 16384 extent limit."""
    tree, tn = planted["tree"], planted["tn"]
    views = RC.planted_views(axis)
    shapes = frusta(ctx, views)
    p = np.concatenate([RC.positions(tn, k) for k in ("r", "r0")])
    for W, H, ps in RC.PLANT_CASES[axis]:
        extent = (W, H)[axis]
        rv = tree.render(shapes, W, H, point_size=ps, depth=True)
        wants = check_views(rv, tree, tn, views, W, H, point_size=ps)
        dep = rv.depth().cpu().numpy()
        for j, t in enumerate(RC.PLANT_T):
            draw, xw, yw, _ = RC.window(views[j], p, W, H)
            assert draw.sum() == 1 and float((xw, yw)[axis][0]) == t * extent / 64.0  # the planted f32 value
            info = rv.info(j)
            cov = dep[j] < 1.0
            line = cov.any(axis=0) if axis == 0 else cov.any(axis=1)[::-1]
            run = RC.exact_run(t, extent, ps)
            assert info["points_drawn"] == 1 and np.nonzero(line)[0].tolist() == run, (W, H, ps, t)
            assert info["pixels_covered"] == len(run) * min(int(ps), (H, W)[axis]) == wants[j]["pixels_covered"]
        if ps == 1.0:  # xw == 0: drawn, covers nothing; x == w: the last column (row)
            assert rv.info(0)["pixels_covered"] == 0 and rv.info(len(views) - 1)["pixels_covered"] == 1
            assert (dep[-1] < 1.0).any(axis=0)[-1] if axis == 0 else (dep[-1] < 1.0).any(axis=1)[0]
        rv.close()


def test_point_size_64_covers_a_3_by_5_image(ctx, trees):
    s = trees["A"]
    views = RC.seam_views()
    rv = s["tree"].render(frusta(ctx, views), 3, 5, point_size=64.0)
    wants = check_views(rv, s["tree"], s["tn"], views, 3, 5, point_size=64.0)
    assert [x["pixels_covered"] for x in wants] == [15, 15, 0, 15, 15] and all(wants[v]["points_drawn"] > 0 for v in (0, 1, 3, 4))
    rv.close()


def test_seeded_random_views(ctx, trees):
    s = trees["A"]
    drawn = panics = 0
    for call, (mats, (w, h), ps) in enumerate(RC.random_plan()):
        shapes = frusta(ctx, mats)
        rv = s["tree"].render(shapes, w, h, point_size=ps)
        wants = check_views(rv, s["tree"], s["tn"], mats, w, h, point_size=ps, shapes=shapes)
        if call < 4:
            drawn += sum(x["status"] == 0 and x["pixels_covered"] > 0 for x in wants)
            panics += sum(x["status"] is None for x in wants)
        rv.close()
    assert drawn >= 40 and panics >= 1, (drawn, panics)
