"""pcv_xray_inpaint on the device against the numpy restatement of DESIGN 9a (xray_inpaint_oracle): every node image, leaves
and parents, byte for byte, and the three counters. Inputs are tile directories written here with exact hole patterns and
opened with xray_open; one case is a small cloud built with the transparent background."""
import functools
import os
import subprocess

import numpy as np
import pytest

import point_cloud_viewer_amd as pcv
import xray_inpaint_oracle as IO
import xray_merge_oracle as MO
import xray_oracle as X
import xray_pyramid_oracle as P
from test_gpu_query import ctx  # noqa: F401  (module fixture)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECT = (0.0, 0.0, 64.0)
HOLE = np.array(X.TRANSPARENT, np.uint8)


# ---- inputs ---------------------------------------------------------------------------------------------------------------
def canvas(G, W, d, seed, partial_alpha=False, blank=None):
    """A (G W)^2 RGBA image of random opaque colours with holes: single pixels, a gap 2 d wide across a tile edge (all of
    it closes), one 2 d wide from the middle column of a tile on (the tile to the right sees only its right bank, so the
    two enlarged tiles disagree and the blend makes partial alpha), one 2 d + 1 wide (its middle stays open), a hole on a
    tile corner; tiles below 8 pixels get random holes only; blank: a cell left all transparent."""
    rng = np.random.default_rng(seed)
    n = G * W
    img = rng.integers(0, 256, (n, n, 4), dtype=np.uint8)
    img[..., 3] = 255
    hole = rng.random((n, n)) < (0.08 if W >= 8 else 0.35)  # single pixels and small clusters
    if W >= 8:
        at = W - d                                      # a vertical gap across the first tile edge
        hole[:, at:at + 2 * d] = True
        if G >= 2:
            at = W + W // 2                             # and one from the middle column of the second tile on
            hole[:, at:at + 2 * d] = True
        at = n // 2 + 1                                 # a horizontal gap, one pixel too wide to close
        hole[at:at + 2 * d + 1, :] = True
        hole[W - 1:W + 1, W - 1:W + 1] = True           # the corner shared by four tiles
    if partial_alpha:
        for a, (y, x) in zip((1, 127, 128, 254) * 4, rng.integers(0, n, (16, 2))):
            img[y, x, 3] = a
            hole[y, x] = False
    img[hole] = HOLE
    if blank is not None:
        cx, cy = blank
        img[(G - 1 - cy) * W:(G - cy) * W, cx * W:(cx + 1) * W] = HOLE
    return img


def cut(img, G, W, level, x0=0, y0=0, missing=()):
    """{leaf index: tile} of the G x G cells of the canvas, cell (0, 0) at the bottom left = quadtree cell (x0, y0)."""
    return {IO.node_index(level, x0 + cx, y0 + cy): np.ascontiguousarray(img[(G - 1 - cy) * W:(G - cy) * W, cx * W:(cx + 1) * W])
            for cx in range(G) for cy in range(G) if (cx, cy) not in missing}


def write_quadtree(directory, root, leaves, deepest, W):
    """Leaf tiles through the library's PNG encoder and the meta file of the quadtree below `root` (a node name)."""
    os.makedirs(directory, exist_ok=True)
    nodes = {(deepest, i) for i in leaves}
    for i in leaves:
        for level in range(deepest - 1, len(root) - 2, -1):
            nodes.add((level, i >> (2 * (deepest - level))))
    nodes.add(X.node_id(root))
    for i, tile in leaves.items():
        with open(os.path.join(directory, X.node_name(deepest, i) + ".png"), "wb") as f:
            f.write(pcv.xray_png_encode(tile))
    with open(os.path.join(directory, P.meta_file_name(root)), "wb") as f:
        f.write(MO.encode_meta(RECT, deepest, W, sorted(nodes)))


MISSING = ((1, 2), (3, 0), (2, 2), (0, 1))
# name: (W, d, G, deepest, missing cells, partial alpha, blank cell, background)
CASES = {
    "w8_d1_2x2": (8, 1, 2, 1, (), False, None, "white"),
    "w8_d2_4x4_missing": (8, 2, 4, 2, MISSING, False, None, "white"),
    "w16_d3_2x2_blank_leaf": (16, 3, 2, 1, (), False, (1, 0), "transparent"),
    "w16_d7_4x4_missing_alpha": (16, 7, 4, 2, MISSING, True, None, "white"),
    "w2_d1_4x4_missing": (2, 1, 4, 2, MISSING, False, None, "white"),
    "w2_d3_2x2_window_clips": (2, 3, 2, 1, (), False, None, "transparent"),
    "w8_d9_2x2_window_clips": (8, 9, 2, 1, ((1, 1),), True, None, "white"),
    "w8_d2_1x1": (8, 2, 1, 0, (), False, None, "white"),
}
W2 = "W = 2: the ramp is (0, 1) and a final tile's pixels sit where it keeps the tile's own value"
DEGENERATE = {"w8_d2_1x1": "a lone leaf has nothing to blend with", "w2_d1_4x4_missing": W2, "w2_d3_2x2_window_clips": W2}


@functools.lru_cache(maxsize=None)
def case(name):
    W, d, G, deepest, missing, alpha, blank, bg = CASES[name]
    leaves = cut(canvas(G, W, d, len(name) + W + d, alpha, blank), G, W, deepest, missing=missing)
    images, counters, pre, unblended = IO.inpaint(leaves, deepest, (0, 0), W, d, bg)
    return leaves, images, counters, pre, unblended


def assert_equals_oracle(xt, images, counters, leaf_order):
    got = dict(zip(xt.node_ids, xt.node_images()))
    assert set(got) == {X.node_name(*k) for k in images} and len(xt.node_ids) == len(got)
    for k, img in images.items():
        g = got[X.node_name(*k)]
        assert np.array_equal(g, img), (X.node_name(*k), int((g != img).any(-1).sum()), np.argwhere((g != img).any(-1))[:4].tolist())
    info = xt.inpaint_info()
    want = np.array([counters[int(i)] for i in leaf_order], dtype=np.uint64).reshape(-1, 3)
    assert [int(i) for i in xt.leaf_index] == [int(i) for i in leaf_order]
    for col, key in enumerate(("target_pixels", "filled_pixels", "blended_pixels")):
        assert np.array_equal(info[key], want[:, col]), key


@pytest.mark.parametrize("name", list(CASES))
def test_opened_quadtree_equals_the_oracle(ctx, tmp_path, name):  # noqa: F811
    W, d, G, deepest, missing, alpha, blank, bg = CASES[name]
    leaves, images, counters, _, _ = case(name)
    write_quadtree(tmp_path / "in", "r", leaves, deepest, W)
    (x,) = ctx.xray_open(tmp_path / "in")
    out = x.inpaint(d, background=bg)
    x.free()  # the result owns its images
    assert_equals_oracle(out, images, counters, sorted(leaves))
    total = {k: int(v.sum()) for k, v in out.inpaint_info().items()}
    print(name, total)
    assert total["target_pixels"] > 0 and total["filled_pixels"] > 0
    if name in DEGENERATE:
        assert total["blended_pixels"] == 0, DEGENERATE[name]
    else:
        assert total["blended_pixels"] > 0
    # the written directory reopens to the same images in both PNG modes
    for png in ("stored", "deflate"):
        out.write(tmp_path / png, png=png)
        (back,) = ctx.xray_open(tmp_path / png)
        assert back.node_ids == out.node_ids and np.array_equal(back.node_images(), out.node_images()), png
        assert back.bounding_rect == RECT and P.decode_meta((tmp_path / png / "meta.pb").read_bytes())["tile_size"] == W
    assert [a for a in out.node_pngs(png="stored")] == [(tmp_path / "stored" / (n + ".png")).read_bytes() for n in out.node_ids]
    for call in (out.images, out.build_parents):
        with pytest.raises(pcv.PcvError, match="PCV_E_INVALID"):
            call()


def test_the_cases_cover_partial_alpha_on_both_sides_of_the_threshold():
    """On the oracle's output: final-tile pixels whose blended alpha is in 1..127 (they become background) and in 128..254
    (they stay), and the hole patterns behave as named."""
    low = high = 0
    for name in CASES:
        _, _, _, pre, unblended = case(name)
        for i, tile in pre.items():
            alpha = tile[..., 3][(tile != unblended[i]).any(-1)]  # of the pixels the blend changed
            low += int(((alpha >= 1) & (alpha <= 127)).sum())
            high += int(((alpha >= 128) & (alpha <= 254)).sum())
    assert low > 0 and high > 0, (low, high)
    # the 2 d gap closes entirely, the middle of the 2 d + 1 gap stays open (w8_d2: d = 2, W = 8, 32 x 32 canvas)
    W, d, G = 8, 2, 4
    img = canvas(G, W, d, 0)
    known = img[..., 3] != 0
    closed = IO.close(known, d)
    assert closed[:W, W - d:W + d].all() and not closed[G * W // 2 + 1 + d, :].any()


def test_small_chunks_give_the_same_tiles(ctx, tmp_path):  # noqa: F811
    name = "w8_d2_4x4_missing"
    W, d, G, deepest, *_ = CASES[name]
    leaves, images, counters, _, _ = case(name)
    write_quadtree(tmp_path / "in", "r", leaves, deepest, W)
    (x,) = ctx.xray_open(tmp_path / "in")
    ctx.set_xray_chunk_bytes(1)  # groups of at most nine enlarged tiles: several groups, each stitches its neighbours again
    try:
        out = x.inpaint(d)
    finally:
        ctx.set_xray_chunk_bytes(0)
    assert_equals_oracle(out, images, counters, sorted(leaves))


def test_distance_zero_is_the_rebackgrounded_quadtree(ctx, tmp_path):  # noqa: F811
    W, d, G, deepest, *_ = CASES["w16_d7_4x4_missing_alpha"]
    leaves = case("w16_d7_4x4_missing_alpha")[0]
    write_quadtree(tmp_path / "in", "r", leaves, deepest, W)
    (x,) = ctx.xray_open(tmp_path / "in")
    for bg in ("white", "transparent"):
        out = x.inpaint(0, background=bg)
        final = {i: np.where(t[..., 3:4] < 128, P.background(bg), t) for i, t in leaves.items()}
        want, _ = P.pyramid(final, deepest, 0, W, bg)
        assert_equals_oracle(out, want, {i: (0, 0, 0) for i in leaves}, sorted(leaves))
    assert any(((t[..., 3] > 0) & (t[..., 3] < 128)).any() for t in leaves.values())  # alpha 1 and 127 went to the background


@pytest.fixture(scope="module")
def partial(tmp_path_factory):
    """x = r03 (cell (1, 1) of level 2) with its four edge neighbours and one diagonal quadtree in one directory; 2 x 2
    leaves per part at level 3, cut from one 6 x 6 canvas so that holes straddle the parts' borders."""
    W, d, deepest = 8, 2, 3
    base = tmp_path_factory.mktemp("partial")
    img = canvas(6, W, d, 77)
    img[:, 2 * W + W // 2:2 * W + W // 2 + 2 * d] = HOLE  # a 2 d gap from the middle column of x's left leaves on: the blend has work
    all_leaves = cut(img, 6, W, deepest)  # canvas cell (cx, cy) = quadtree cell (cx, cy) of the 8 x 8 level-3 grid
    parts = {}
    for cx, cy in ((1, 1), (0, 1), (1, 2), (2, 1), (1, 0), (2, 2)):
        root = X.node_name(2, IO.node_index(2, cx, cy))
        mine = {i: t for i, t in all_leaves.items() if (i >> 2) == IO.node_index(2, cx, cy)}
        if (cx, cy) == (1, 1):
            mine.pop(IO.node_index(deepest, 2, 3))   # x misses its top left leaf: the Left leaf (1, 3) is not taken
        if (cx, cy) == (1, 2):
            mine.pop(IO.node_index(deepest, 3, 4))   # the Top part misses a leaf that would have been taken
        parts[root] = mine
        write_quadtree(base, root, mine, deepest, W)
    return dict(W=W, d=d, deepest=deepest, dir=base, parts=parts, x=X.node_name(2, IO.node_index(2, 1, 1)))


def test_partial_quadtree_with_four_neighbours(ctx, partial, tmp_path, capfd):  # noqa: F811
    W, d, deepest, xname = partial["W"], partial["d"], partial["deepest"], partial["x"]
    opened = {p.node_ids[-1]: p for p in ctx.xray_open(partial["dir"])}
    assert len(opened) == 6
    order = [X.node_name(2, IO.node_index(2, cx, cy)) for cx, cy in ((0, 1), (1, 2), (2, 1), (1, 0))]
    nbs = [(X.node_id(n), partial["parts"][n]) for n in order]
    images, counters, _, _ = IO.inpaint(partial["parts"][xname], deepest, X.node_id(xname), W, d, "white", nbs)
    out = opened[xname].inpaint(d, neighbors=[opened[n] for n in order])
    assert_equals_oracle(out, images, counters, sorted(partial["parts"][xname]))
    assert out.node_ids[-1] == xname and out.inpaint_info()["blended_pixels"].sum() > 0
    # without the neighbours the tiles differ: the adjacent leaves did feed the stitch
    alone = opened[xname].inpaint(d)
    assert not np.array_equal(alone.node_images(), out.node_images())
    # the directory tool picks the same parts, and the C example writes the same files
    tool = pcv.inpaint_xray_quadtree(ctx, partial["dir"], tmp_path / "py", d, root_node_id=xname)
    assert np.array_equal(tool.node_images(), out.node_images()) and "No adjacent leaf nodes" not in capfd.readouterr().err
    assert set(os.listdir(tmp_path / "py")) == {n + ".png" for n in out.node_ids} | {P.meta_file_name(xname)}
    exe = os.path.join(ROOT, "examples", "bin", "inpaint_xray_quadtree")
    subprocess.check_call([exe, str(partial["dir"]), "--output-directory", str(tmp_path / "c"), "--inpaint-distance-px", str(d),
                           "--root-node-id", xname])
    files = sorted(os.listdir(tmp_path / "py"))
    assert files == sorted(os.listdir(tmp_path / "c"))
    for f in files:
        assert (tmp_path / "py" / f).read_bytes() == (tmp_path / "c" / f).read_bytes(), f
    # a partial quadtree on its own: the reference's warning
    lonely = tmp_path / "lonely"
    write_quadtree(lonely, xname, partial["parts"][xname], deepest, W)
    pcv.inpaint_xray_quadtree(ctx, lonely, tmp_path / "lonely_out", d, root_node_id=xname, png="deflate")
    assert "No adjacent leaf nodes found in neighboring quadtrees" in capfd.readouterr().err
    # the inpainted partial quadtree merges like any part
    merged = ctx.xray_merge([out], "white")
    assert merged.node_ids[-1] == "r" and merged.node_ids[:len(out.node_ids)] == out.node_ids
    got = dict(zip(merged.node_ids, merged.node_images()))
    assert np.array_equal(got[xname], images[X.node_id(xname)])
    want, _ = P.pyramid({X.node_id(xname)[1]: got[xname]}, 2, 0, W, "white")
    assert np.array_equal(got["r"], want[(0, 0)])


def test_a_built_cloud_and_the_refusals(ctx):  # noqa: F811
    rng = np.random.default_rng(9)
    n = 6000
    x, y, z = rng.random(n) * 32.0, rng.random(n) * 32.0, rng.random(n) * 4.0
    x[:2], y[:2], z[:2] = (0.0, 32.0), (0.0, 32.0), (0.0, 4.0)
    rgb = rng.integers(0, 256, (n, 3), dtype=np.uint8)
    tree = ctx.build(0.001, pcv.Aabb(np.zeros(3), np.array([32.0, 32.0, 4.0])), x, y, z, rgb, max_points_per_node=2000)
    W, d = 16, 2
    xt = tree.xray_tiles(W, 0.5, "colored", background="transparent")  # 64 x 64 pixels over 6000 points: speckled
    assert xt.deepest_level == 2 and xt.num_created >= 4
    leaves = {int(xt.leaf_index[int(c)]): img for c, img in zip(xt.created, xt.images())}
    images, counters, _, _ = IO.inpaint(leaves, 2, (0, 0), W, d, "white")
    out = xt.inpaint(d)
    assert_equals_oracle(out, images, counters, [int(xt.leaf_index[int(c)]) for c in xt.created])
    info = out.inpaint_info()
    assert info["target_pixels"].sum() > 0 and info["blended_pixels"].sum() > 0
    # an inpainted result with the transparent background can be inpainted again; with the white one it cannot
    again = xt.inpaint(d, background="transparent").inpaint(1)
    assert again.node_ids == out.node_ids
    # refusals allocate nothing
    import torch
    white = tree.xray_tiles(W, 0.5, "colored", background="white")
    merged = ctx.xray_merge([out], "white")
    other = tree.xray_tiles(8, 1.0, "colored", background="transparent")
    odd = tree.xray_tiles(6, 1.0, "colored", background="transparent")
    ctx.synchronize()
    ctx.trim()
    torch.cuda.synchronize()
    before = torch.cuda.mem_get_info()[0]
    for who, dist, nbs, message in ((xt, 255, (), "saturates"), (white, 2, (), "white background"), (out, 2, (), "white background"),
                                    (odd, 2, (), "power of two"), (xt, 2, (other,), "tile size 8"), (xt, 2, (xt,), "not the Left, Top"),
                                    (merged, 2, (), "merged")):
        with pytest.raises(pcv.PcvError, match=message) as e:
            who.inpaint(dist, neighbors=nbs)
        assert e.value.code == pcv.PCV_E_INVALID
        with pytest.raises(pcv.PcvError, match=message):
            pcv.xray_inpaint_check(who, dist, nbs)
    with pytest.raises(ValueError):
        xt.inpaint(2, background="grey")
    ctx.trim()
    torch.cuda.synchronize()
    assert torch.cuda.mem_get_info()[0] >= before - (1 << 20)  # a refusal comes before any allocation; the margin is the runtime's own
    other_ctx = pcv.Context(0)
    try:
        with pytest.raises(pcv.PcvError, match="another context"):
            xt.inpaint(2, ctx=other_ctx)
    finally:
        other_ctx.close()
