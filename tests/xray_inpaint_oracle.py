"""Numpy restatement of the inpainting contract, written from the contract and from
xray/src/bin/inpaint_xray_quadtree.rs, xray/src/inpaint.rs and xray/src/utils.rs, not from the kernels: the enlarged tiles are
real images that the blend rewrites in place, phase after phase, as the reference rewrites its *.inpaint.png files; the close
is brute force over clipped windows. Step 4, the fill, is this project's own (the reference calls texture synthesis there)."""
import numpy as np

import xray_oracle as X
import xray_pyramid_oracle as P

F32 = np.float32
ABSENT = 0xFFFFFFFF
DIRECTIONS = (("Left", -1, 0), ("Top", 0, 1), ("Right", 1, 0), ("Bottom", 0, -1))  # get_adjacent_leaf_node_ids' order
# stitched_image's regions, rows top to bottom (Top is y + 1): (dx, dy) of the neighbour that fills the slot
SLOTS = ((-1, 1), (0, 1), (1, 1), (-1, 0), (0, 0), (1, 0), (-1, -1), (0, -1), (1, -1))


# ---- quadtree ids (quadtree/src/lib.rs:290-349) ---------------------------------------------------------------------------
def spatial(level, index):
    x = y = 0
    for i in range(1, level + 1):
        mask = 1 << (level - i)
        digit = index >> ((level - i) * 2)
        if digit & 1:
            y |= mask
        if digit & 2:
            x |= mask
    return x, y


def node_index(level, x, y):
    index = 0
    for i in range(1, level + 1):
        index <<= 2
        mask = 1 << (level - i)
        index += (1 if y & mask else 0) + (2 if x & mask else 0)
    return index


def neighbor(level, index, dx, dy):
    """NodeId::neighbor: the index of the neighbour at the same level, or None outside the grid."""
    x, y = spatial(level, index)
    x, y = x + dx, y + dy
    return node_index(level, x, y) if 0 <= x < (1 << level) and 0 <= y < (1 << level) else None


# ---- steps 1 and 2 as a table --------------------------------------------------------------------------------------------
def plan(leaves, deepest, root, neighbours):
    """leaves: x's leaf indices in node order; root: (level, index); neighbours: [(root, leaf indices in node order)].
    Returns (slots (n, 9, 2) uint32 of (part, node), adjacent {leaf index: (part, node)})."""
    own = {int(i): c for c, i in enumerate(leaves)}
    adjacent = {}
    for _, dx, dy in DIRECTIONS:
        want = neighbor(root[0], root[1], dx, dy)
        for k, (nroot, nleaves) in enumerate(neighbours):
            if want is None or nroot != (root[0], want):
                continue
            for c, i in enumerate(nleaves):
                back = neighbor(deepest, int(i), -dx, -dy)
                if back is not None and back in own:
                    adjacent.setdefault(int(i), (k + 1, c))
    slots = np.full((len(leaves), 9, 2), ABSENT, dtype=np.uint32)
    for c, i in enumerate(leaves):
        for s, (dx, dy) in enumerate(SLOTS):
            j = neighbor(deepest, int(i), dx, dy)
            if j is None:
                continue
            if j in own:
                slots[c, s] = (0, own[j])
            elif j in adjacent:
                slots[c, s] = adjacent[j]
    return slots, adjacent


# ---- step 2 ---------------------------------------------------------------------------------------------------------------
def stitched(idx, deepest, tiles, W):
    """stitched_image :90-121 for leaf idx; tiles: {leaf index: (W, W, 4) image} of every tile that may contribute."""
    w = h = W // 2
    img = np.empty((4 * h, 4 * w, 4), np.uint8)
    img[:] = X.TRANSPARENT
    img[h:h + W, w:w + W] = tiles[idx]

    def copy(dx, dy, fx, fy, cw, ch, tx, ty):
        j = neighbor(deepest, idx, dx, dy)
        if j is not None and j in tiles:
            img[ty:ty + ch, tx:tx + cw] = tiles[j][fy:fy + ch, fx:fx + cw]
    copy(-1, 1, w, h, w, h, 0, 0)             # TopLeft
    copy(0, 1, 0, h, 2 * w, h, w, 0)          # Top
    copy(1, 1, 0, h, w, h, 3 * w, 0)          # TopRight
    copy(1, 0, 0, 0, w, 2 * h, 3 * w, h)      # Right
    copy(1, -1, 0, 0, w, h, 3 * w, 3 * h)     # BottomRight
    copy(0, -1, 0, 0, 2 * w, h, w, 3 * h)     # Bottom
    copy(-1, -1, w, 0, w, h, 0, 3 * h)        # BottomLeft
    copy(-1, 0, w, 0, w, 2 * h, 0, h)         # Left
    return img


# ---- step 3 ---------------------------------------------------------------------------------------------------------------
def dilate(mask, d):
    n, m = mask.shape
    out = np.zeros_like(mask)
    for y in range(n):
        for x in range(m):
            out[y, x] = mask[max(y - d, 0):y + d + 1, max(x - d, 0):x + d + 1].any()
    return out


def erode(mask, d):
    n, m = mask.shape
    out = np.zeros_like(mask)
    for y in range(n):
        for x in range(m):
            out[y, x] = mask[max(y - d, 0):y + d + 1, max(x - d, 0):x + d + 1].all()
    return out


def close(mask, d):
    """erode(dilate(mask, d), d) in the Chebyshev norm; windows clipped to the image."""
    return erode(dilate(mask, d), d)


def masks(img, d):
    known = img[..., 3] != 0
    return known, close(known, d) & ~known


# ---- step 4 ---------------------------------------------------------------------------------------------------------------
def fill(img, known, target, d):
    out = img.copy()
    n, m = known.shape
    for y, x in zip(*np.nonzero(target)):
        r = next(t for t in range(1, d + 1) if known[max(y - t, 0):y + t + 1, max(x - t, 0):x + t + 1].any())
        y0, y1, x0, x1 = max(y - 2 * r, 0), min(y + 2 * r, n - 1), max(x - 2 * r, 0), min(x + 2 * r, m - 1)
        yy, xx = np.mgrid[y0:y1 + 1, x0:x1 + 1]
        wgt = (2 * r + 1 - np.maximum(np.abs(yy - y), np.abs(xx - x))).astype(np.int64) * known[y0:y1 + 1, x0:x1 + 1]
        total = int(wgt.sum())
        for c in range(3):
            out[y, x, c] = (int((wgt * img[y0:y1 + 1, x0:x1 + 1, c].astype(np.int64)).sum()) + total // 2) // total
        out[y, x, 3] = 255
    return out


# ---- step 5 ---------------------------------------------------------------------------------------------------------------
def round_half_away(v):
    """f32::round for v >= 0: the fraction of an f32 is exact, so no sum decides the tie."""
    v = np.asarray(v, F32)
    t = np.trunc(v)
    return t + ((v - t) >= F32(0.5))


def interpolate(this, other, wt):
    """interpolate_pixels (utils.rs:46-60) on uint8 arrays: (this * wt + other * (1 - wt)).round() as u8, every operation
    an f32 operation of its own."""
    wt = np.asarray(wt, F32)
    a = this.astype(F32) * wt
    b = other.astype(F32) * (F32(1.0) - wt)
    return np.minimum(round_half_away(a + b), F32(255)).astype(np.uint8)


def blend(enlarged, deepest):
    """interpolate_inpaint_image_with for Right over every leaf, then for Bottom, on the images in place."""
    some = next(iter(enlarged.values()))
    size = some.shape[0]
    half = size // 2
    ramp = (np.arange(half, dtype=F32) / F32(half - 1)).astype(F32)
    for parity in (0, 1):  # interleaved by x as in the reference; the regions of a phase are disjoint anyway
        for idx in enlarged:
            if spatial(deepest, idx)[0] % 2 != parity:
                continue
            j = neighbor(deepest, idx, 1, 0)
            if j is None or j not in enlarged:
                continue
            v = interpolate(enlarged[j][:, :half], enlarged[idx][:, half:], ramp[None, :, None])
            enlarged[j][:, :half] = v
            enlarged[idx][:, half:] = v
    for parity in (0, 1):
        for idx in enlarged:
            if spatial(deepest, idx)[1] % 2 != parity:
                continue
            j = neighbor(deepest, idx, 0, -1)
            if j is None or j not in enlarged:
                continue
            v = interpolate(enlarged[j][:half], enlarged[idx][half:], ramp[:, None, None])
            enlarged[j][:half] = v
            enlarged[idx][half:] = v


# ---- the whole ------------------------------------------------------------------------------------------------------------
def inpaint(leaves, deepest, root, W, d, bg_name, neighbours=()):
    """leaves: {leaf index: image} of x (transparent background); root: (level, index) of x's root; neighbours:
    [(root, {leaf index: image})]. Returns (images {(level, index): image} of the leaves and every parent up to the root,
    counters {leaf index: (target, filled, blended)}, {leaf index: final tile before the background}, {leaf index: the
    same before the blend})."""
    bg = P.background(bg_name)
    order = list(leaves)
    final, counters, pre, unblended = {}, {}, {}, {}
    if d == 0:
        for i in order:
            final[i] = np.where(leaves[i][..., 3:4] < 128, bg, leaves[i])
            counters[i] = (0, 0, 0)
            pre[i] = unblended[i] = leaves[i]
    else:
        _, adjacent = plan(order, deepest, root, [(r, list(t)) for r, t in neighbours])
        tiles = dict(leaves)
        for i, (part, _) in adjacent.items():
            tiles[i] = neighbours[part - 1][1][i]
        w = W // 2
        enlarged, known, target, filled = {}, {}, {}, {}
        for i in order:
            st = stitched(i, deepest, tiles, W)
            known[i], target[i] = masks(st, d)
            enlarged[i] = fill(st, known[i], target[i], d)
            filled[i] = enlarged[i].copy()
        blend(enlarged, deepest)
        c = slice(w, w + W)
        for i in order:
            out = enlarged[i][c, c]
            pre[i], unblended[i] = out, filled[i][c, c]
            counters[i] = (int(target[i][c, c].sum()), int(((out[..., 3] >= 128) & ~known[i][c, c]).sum()),
                           int((out != filled[i][c, c]).any(-1).sum()))
            final[i] = np.where(out[..., 3:4] < 128, bg, out)
    images, _ = P.pyramid(final, deepest, root[0], W, bg_name)
    return images, counters, pre, unblended
