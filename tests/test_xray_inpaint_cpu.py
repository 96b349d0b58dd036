"""The host side of pcv_xray_inpaint without a GPU: the oracle's own steps against independent restatements (scipy's filters
for the close, a double loop for the fill, hand-computed pixels for the blend), and pcv_xray_inpaint_plan / _check on
quadtree directories written by the test and opened host only."""
import itertools

import numpy as np
import pytest
import scipy.ndimage as ndi

import point_cloud_viewer_amd as pcv
import xray_inpaint_oracle as IO
import xray_merge_oracle as MO
import xray_oracle as X
from point_cloud_viewer_amd import _lib as L

RECT = (0.0, 0.0, 64.0)


# ---- the oracle's steps against independent restatements -----------------------------------------------------------------
@pytest.mark.parametrize("d", [1, 2, 3, 7, 20])
def test_close_is_scipys_max_then_min_filter(d):
    rng = np.random.default_rng(d)
    for shape, density in (((16, 16), 0.1), ((16, 16), 0.5), ((4, 4), 0.3), ((32, 32), 0.03), ((8, 8), 0.0), ((8, 8), 1.0)):
        mask = rng.random(shape) < density
        size = 2 * d + 1
        want = ndi.minimum_filter(ndi.maximum_filter(mask.astype(np.uint8), size=size, mode="constant", cval=0), size=size,
                                  mode="constant", cval=1).astype(bool)
        assert np.array_equal(IO.close(mask, d), want), (shape, density)
        assert (IO.close(mask, d) | ~mask).all()  # closing is extensive: the target mask is closed & !known


def fill_double_loop(img, known, target, d):
    out = img.copy()
    n = known.shape[0]
    for y in range(n):
        for x in range(n):
            if not target[y, x]:
                continue
            r = None
            for t in range(1, d + 1):
                if any(known[v, u] for v in range(max(y - t, 0), min(y + t, n - 1) + 1) for u in range(max(x - t, 0), min(x + t, n - 1) + 1)):
                    r = t
                    break
            s, total = [0, 0, 0], 0
            for v in range(max(y - 2 * r, 0), min(y + 2 * r, n - 1) + 1):
                for u in range(max(x - 2 * r, 0), min(x + 2 * r, n - 1) + 1):
                    if known[v, u]:
                        wq = 2 * r + 1 - max(abs(v - y), abs(u - x))
                        total += wq
                        for c in range(3):
                            s[c] += wq * int(img[v, u, c])
            out[y, x] = [(s[c] + total // 2) // total for c in range(3)] + [255]
    return out


@pytest.mark.parametrize("d", [1, 3])
def test_fill_against_a_double_loop(d):
    rng = np.random.default_rng(10 + d)
    img = rng.integers(0, 256, (16, 16, 4), dtype=np.uint8)
    img[..., 3] = np.where(rng.random((16, 16)) < 0.6, 255, 0)
    img[..., 3][3, 4] = 1  # foreign partial alpha is known
    img[img[..., 3] == 0] = X.TRANSPARENT
    known, target = IO.masks(img, d)
    assert target.sum() > 10
    got = IO.fill(img, known, target, d)
    assert np.array_equal(got, fill_double_loop(img, known, target, d))
    assert np.array_equal(got[~target], img[~target]) and (got[target][:, 3] == 255).all()


def test_fill_by_hand():
    # one hole between two known pixels of a row, d = 1: r = 1, sources within distance 2, weights 3 - distance
    img = np.empty((8, 8, 4), np.uint8)
    img[:] = X.TRANSPARENT
    img[3, 2], img[3, 4], img[3, 5] = (10, 0, 200, 255), (40, 100, 0, 255), (250, 250, 250, 255)
    known, target = IO.masks(img, 1)
    assert target[3, 3] and not target[6, 6] and not target[3, 2]
    got = IO.fill(img, known, target, 1)
    # (3, 3): sources (3, 2) w 2, (3, 4) w 2, (3, 5) w 1: W_sum 5 -> r = (20 + 80 + 250 + 2) // 5, ...
    assert tuple(got[3, 3]) == ((20 + 80 + 250 + 2) // 5, (0 + 200 + 250 + 2) // 5, (400 + 0 + 250 + 2) // 5, 255)


def test_blend_weights_and_rounding_by_hand():
    px = lambda *v: np.array(v, np.uint8)  # noqa: E731
    # ties round away from zero, not to even
    assert IO.interpolate(px(1, 3, 5, 255), px(0, 0, 0, 255), 0.5).tolist() == [1, 2, 3, 255]
    # width 4 (W = 2): weights i / 3 in f32. A colour against the transparent border (255, 255, 255, 0), the colour being
    # `this` (the neighbour's side): alpha 255 / 3 = 85 < 128 and 510 / 3 = 170 >= 128
    third, two_thirds = np.float32(1) / np.float32(3), np.float32(2) / np.float32(3)
    assert IO.interpolate(px(10, 20, 30, 255), px(255, 255, 255, 0), third).tolist() == [173, 177, 180, 85]
    assert IO.interpolate(px(10, 20, 30, 255), px(255, 255, 255, 0), two_thirds).tolist() == [92, 98, 105, 170]
    # the ends of the ramp keep one side exactly
    assert IO.interpolate(px(7, 8, 9, 255), px(200, 100, 50, 0), 0.0).tolist() == [200, 100, 50, 0]
    assert IO.interpolate(px(7, 8, 9, 255), px(200, 100, 50, 0), 1.0).tolist() == [7, 8, 9, 255]
    # width 16: the alpha of colour against border crosses 128 between i = 7 (119) and i = 8 (136)
    ramp = np.arange(16, dtype=np.float32) / np.float32(15)
    alpha = IO.interpolate(np.full(16, 255, np.uint8), np.zeros(16, np.uint8), ramp)
    assert alpha.tolist() == [0, 17, 34, 51, 68, 85, 102, 119, 136, 153, 170, 187, 204, 221, 238, 255]


def test_blend_in_place_order():
    # three tiles in a row at level 2: the middle one blends its left half with the left tile and its right half with the
    # right tile; the vertical phase then works on those results
    rng = np.random.default_rng(5)
    en = {IO.node_index(2, x, 1): rng.integers(0, 256, (8, 8, 4), dtype=np.uint8) for x in range(3)}
    en[IO.node_index(2, 1, 0)] = rng.integers(0, 256, (8, 8, 4), dtype=np.uint8)
    before = {k: v.copy() for k, v in en.items()}
    IO.blend(en, 2)
    a, b, c, below = (IO.node_index(2, 0, 1), IO.node_index(2, 1, 1), IO.node_index(2, 2, 1), IO.node_index(2, 1, 0))
    ramp = (np.arange(4, dtype=np.float32) / np.float32(3))
    h_ab = IO.interpolate(before[b][:, :4], before[a][:, 4:], ramp[None, :, None])
    h_bc = IO.interpolate(before[c][:, :4], before[b][:, 4:], ramp[None, :, None])
    assert np.array_equal(en[a][:, 4:], h_ab) and np.array_equal(en[c][:, :4], h_bc) and np.array_equal(en[a][:, :4], before[a][:, :4])
    h_b = np.concatenate([h_ab, h_bc], axis=1)
    v = IO.interpolate(before[below][:4], h_b[4:], ramp[:, None, None])  # `below` has no horizontal neighbour
    assert np.array_equal(en[b][4:], v) and np.array_equal(en[below][:4], v) and np.array_equal(en[b][:4], h_b[:4])


# ---- pcv_xray_inpaint_plan / _check on opened directories -----------------------------------------------------------------
def write_part(directory, root, leaves, deepest, tile=4, rect=RECT):
    """A meta file with the root, every level between and the leaves (node ids as names); no tiles: the plan reads none."""
    directory.mkdir(parents=True, exist_ok=True)
    nodes = {X.node_id(n) for n in leaves}
    for n in leaves:
        for k in range(len(root), len(n)):
            nodes.add(X.node_id(n[:k]))
    nodes.add(X.node_id(root))
    (directory / ("meta" + root[1:] + ".pb")).write_bytes(MO.encode_meta(rect, deepest, tile, sorted(nodes)))


def opened(directory):
    return pcv.xray_open_host(directory)


def leaf_names(level, cells):
    return [X.node_name(level, IO.node_index(level, x, y)) for x, y in cells]


def oracle_plan(x, neighbours):
    def root_of(p):
        lv, ix = p.nodes()
        at = int(np.argmin(lv))
        return int(lv[at]), int(ix[at])
    return IO.plan([int(i) for i in x.leaf_index], x.deepest_level, root_of(x), [(root_of(p), [int(i) for i in p.leaf_index]) for p in neighbours])


def test_plan_every_absent_pattern_on_a_4x4_level(tmp_path):
    cells = [(x, y) for x in range(4) for y in range(4)]
    seen = set()
    rng = np.random.default_rng(3)
    subsets = [cells, [(1, 1)], [(0, 0), (3, 3)]] + [[c for c in cells if rng.random() < p] or [(2, 2)] for p in (0.3, 0.5, 0.5, 0.7, 0.7, 0.85)]
    # the eight neighbours of (1, 1) and of (2, 2) in every combination, spread over the two centres
    for mask in range(256):
        ring = [(dx, dy) for dx, dy in itertools.product((-1, 0, 1), repeat=2) if (dx, dy) != (0, 0)]
        subsets.append([(1, 1)] + [(1 + dx, 1 + dy) for k, (dx, dy) in enumerate(ring) if mask >> k & 1])
    for k, sub in enumerate(subsets):
        d = tmp_path / f"s{k}"
        write_part(d, "r", leaf_names(2, sub), 2)
        (x,) = opened(d)
        slots, na = pcv.xray_inpaint_plan(x)
        want, adjacent = oracle_plan(x, [])
        assert na == 0 and not adjacent and np.array_equal(slots, want), sub
        assert (slots[:, 4, 0] == 0).all() and (slots[:, 4, 1] == np.arange(len(sub))).all()
        for row in slots:
            seen.add(tuple(int(v) != L.XRAY_INPAINT_ABSENT for v in row[:, 0]))
    assert len({s for s in seen}) >= 256  # every presence pattern of the eight neighbours occurred


def test_plan_partial_quadtree_with_four_neighbours(tmp_path):
    # level-1 roots: x = r2 (cell (1, 0)); a level-1 cell has only two edge neighbours inside the root, so the four-sided
    # case sits one level down: x = r03 (cell (1, 1) of the 4 x 4 grid of level 2), leaves at level 4 (4 x 4 per part)
    deepest = 4

    def part_cells(cx, cy, keep):
        return [(4 * cx + x, 4 * cy + y) for x in range(4) for y in range(4) if keep(x, y)]
    root = X.node_name(2, IO.node_index(2, 1, 1))
    x_cells = part_cells(1, 1, lambda x, y: (x, y) not in ((0, 2), (3, 3), (1, 0)))  # holes on the Left, Top / Right and Bottom edges
    write_part(tmp_path / "d", root, leaf_names(deepest, x_cells), deepest)
    sides = {"left": (0, 1), "top": (1, 2), "right": (2, 1), "bottom": (1, 0)}
    for name, (cx, cy) in sides.items():
        write_part(tmp_path / "d", X.node_name(2, IO.node_index(2, cx, cy)), leaf_names(deepest, part_cells(cx, cy, lambda x, y: (x + y) % 5 != 4)), deepest)
    # a diagonal quadtree is in the directory too and must never be read
    write_part(tmp_path / "d", X.node_name(2, IO.node_index(2, 2, 2)), leaf_names(deepest, part_cells(2, 2, lambda x, y: True)), deepest)
    parts = {p.node_ids[-1]: p for p in opened(tmp_path / "d")}
    x = parts[root]
    nbs = [parts[X.node_name(2, IO.node_index(2, cx, cy))] for cx, cy in sides.values()]
    for order in (nbs, nbs[::-1], nbs[1:3], []):
        slots, na = pcv.xray_inpaint_plan(x, order)
        want, adjacent = oracle_plan(x, order)
        assert np.array_equal(slots, want) and na == len(adjacent)
    slots, na = pcv.xray_inpaint_plan(x, nbs)
    _, adjacent = oracle_plan(x, nbs)
    # the Left neighbour's leaf (3, 4 + 2) faces the missing leaf (4, 6) of x: it is a leaf of that part and is not taken
    skipped = IO.node_index(deepest, 3, 6)
    assert skipped in [int(i) for i in nbs[0].leaf_index] and skipped not in adjacent
    assert IO.node_index(deepest, 3, 4) in adjacent and na == len(adjacent) and 0 < na < 16
    # every side contributes, and a corner slot of an edge leaf can hold a leaf of a side neighbour
    assert {p for p, _ in adjacent.values()} == {1, 2, 3, 4}
    assert ((slots[:, :, 0] != 0) & (slots[:, :, 0] != L.XRAY_INPAINT_ABSENT)).sum() > na
    diag = pcv.xray_inpaint_plan(x, [])[0]
    assert ((diag[:, :, 0] == 0) | (diag[:, :, 0] == L.XRAY_INPAINT_ABSENT)).all()


def test_check_messages(tmp_path):
    def part(name, root, cells, deepest=3, tile=4):
        write_part(tmp_path / name, root, leaf_names(deepest, cells), deepest, tile)
        return opened(tmp_path / name)[0]

    def refused(x, d, nbs, message):
        with pytest.raises(pcv.PcvError, match=message) as e:
            pcv.xray_inpaint_check(x, d, nbs)
        assert e.value.code == pcv.PCV_E_INVALID
        if d == 0:  # the plan makes the same checks
            with pytest.raises(pcv.PcvError, match=message):
                pcv.xray_inpaint_plan(x, nbs)
    x = part("x", "r2", [(4, 0), (5, 1)])        # r2: cell (1, 0) of level 1
    left = part("left", "r0", [(3, 0), (3, 1)])   # r0: cell (0, 0)
    top = part("top", "r3", [(4, 4)])             # r3: cell (1, 1)
    diag = part("diag", "r1", [(3, 4)])           # r1: cell (0, 1)
    pcv.xray_inpaint_check(x, 3, [left, top])
    pcv.xray_inpaint_check(x, 254, [])
    pcv.xray_inpaint_check(x, 0, [top, left])
    refused(x, 255, [], "255.*saturates")
    refused(x, 256, [], "u8")
    refused(x, 0, [diag], "r1.*not the Left, Top, Right or Bottom neighbour of r2")
    refused(x, 0, [x], "not the Left, Top, Right or Bottom neighbour")
    refused(x, 0, [left, left], "two Left neighbours")
    refused(x, 0, [part("deep", "r0", [(7, 0)], deepest=4)], "neighbour 0 has deepest level 4, not 3")
    refused(x, 0, [left, part("tile", "r3", [(4, 4)], tile=8)], "neighbour 1 has tile size 8, not 4")
    refused(part("odd", "r", [(0, 0)], tile=6), 0, [], "tile size 6 is not a power of two")
    refused(part("one", "r", [(0, 0)], tile=1), 0, [], "tile size 1 is not a power of two")
    refused(x, 0, [part("lower", "r00", [(0, 0)])], "not the Left, Top, Right or Bottom neighbour")
    refused(x, 0, [left, top, left, top, left], "more than 4")
    (tmp_path / "empty").mkdir()
    (tmp_path / "empty" / "meta.pb").write_bytes(MO.encode_meta(RECT, 3, 4, []))
    refused(opened(tmp_path / "empty")[0], 0, [], "has no nodes")
    freed = part("freed", "r0", [(0, 0)])
    handle = freed.handle
    freed.free()
    freed.handle = handle  # the address is only looked up in the registry of live handles, never read
    try:
        refused(x, 0, [freed], "not a live pcv_xray")
    finally:
        freed.handle = None
