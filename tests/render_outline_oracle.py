"""numpy restatement of the node outlines of the viewer's frame on top of tests/render_oracle.py.

Written from the contract and the reference's box drawer (sdl_viewer/src/box_drawer.rs: the corner table and the 12 index
pairs; lib.rs:202-208: a node's outline right after the node's points, under the same depth test), not from the kernel.
Every f32 step is one operation on np.float32 values; the clip parameters are found segment by segment with scalars, the
pixel centres of a segment are found by testing the predicate on every pixel of the major axis."""
import numpy as np

import render_oracle as R

F32 = np.float32
YELLOW = (255, 255, 0, 255)
# box_drawer.rs:63-72 as (x, y, z) picks: 0 takes min, 1 takes min + edge (the table's -1 / +1)
CORNERS = ((0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1), (0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0))
# box_drawer.rs:85-98
EDGES = ((0, 1), (1, 2), (2, 3), (3, 0), (4, 5), (5, 6), (6, 7), (7, 4), (1, 5), (6, 2), (4, 0), (3, 7))


def box_segments(cube_min, cube_edge, matrix):
    """Step 9: the 12 edges of a cube as pairs of f32 clip-space points: (12, 2, 4)."""
    mn = np.asarray(cube_min, np.float64)
    far = mn + np.float64(cube_edge)  # one f64 add per axis
    corners = np.array([[far[a] if pick[a] else mn[a] for a in range(3)] for pick in CORNERS], np.float64)
    clip = np.stack(R.clip_f32(matrix, corners), axis=1)  # (8, 4) f32
    return np.array([[clip[a], clip[b]] for a, b in EDGES], F32)


def clip_segment(a, b):
    """Step 10 for one segment of f32 clip points a, b: the clipped endpoints, or None when the segment is dropped."""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    if not (np.isfinite(a).all() and np.isfinite(b).all()):
        return None
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        def dist(p):
            x, y, z, w = p
            return [w, w + x, w - x, w + y, w - y, w + z, w - z]
        t_in, t_out = F32(0.0), F32(1.0)
        for k, (d0, d1) in enumerate(zip(dist(a), dist(b))):
            in0, in1 = (d0 > 0, d1 > 0) if k == 0 else (d0 >= 0, d1 >= 0)
            if not in0 and not in1:
                return None
            if in0 != in1:
                t = d0 / (d0 - d1)
                if in0:
                    if t < t_out:
                        t_out = t
                elif t > t_in:
                    t_in = t
        if t_in > t_out:
            return None
        p = a + t_in * (b - a) if t_in > 0 else a
        q = a + t_out * (b - a) if t_out < 1 else b
    for e in (p, q):
        if not (e[3] > 0 and e[3] < np.inf):
            return None
    return p.astype(F32), q.astype(F32)


def window(p, W, H):
    """Step 4 of §9b for one clip point."""
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        x, y, z, w = p
        xd, yd, zd = x / w, y / w, z / w
        return (xd + F32(1.0)) * (F32(0.5) * F32(W)), (yd + F32(1.0)) * (F32(0.5) * F32(H)), zd * F32(0.5) + F32(0.5)


def raster(p0, p1, W, H):
    """Step 11 for one segment between two window points: (image pixel index, zw) of its fragments."""
    x0, y0, z0 = p0
    x1, y1, z1 = p1
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        x_major = np.abs(x1 - x0) >= np.abs(y1 - y0)
        m0, m1, n0, n1, size_m, size_n = (x0, x1, y0, y1, W, H) if x_major else (y0, y1, x0, x1, H, W)
        lo, hi = min(m0, m1), max(m0, m1)
        i = np.arange(size_m, dtype=np.int64)
        c = i.astype(F32) + F32(0.5)
        i = i[(lo <= c) & (c < hi)]
        if i.size == 0:
            return np.zeros(0, np.int64), np.zeros(0, F32)
        c = i.astype(F32) + F32(0.5)
        t = (c - m0) / (m1 - m0)
        n = n0 + t * (n1 - n0)
        zw = z0 + t * (z1 - z0)
        zw = np.where(zw > 0, zw, F32(0.0))  # (a NaN and -0.0 become +0.0)
        zw = np.where(zw > 1, F32(1.0), zw).astype(F32)
        ok = (n >= 0) & (n < F32(size_n))
        i, n, zw = i[ok], n[ok], zw[ok]
        j = np.floor(n).astype(np.int64)
    gx, gy = (i, j) if x_major else (j, i)
    return (H - 1 - gy) * W + gx, zw


def outline_fragments(cube_min, cube_edge, matrix, W, H):
    """All fragments of one node's outline: (pixel indices, zw, segments drawn)."""
    pix, zws, drawn = [], [], 0
    for a, b in box_segments(cube_min, cube_edge, matrix):
        ends = clip_segment(a, b)
        if ends is None:
            continue
        w0, w1 = window(ends[0], W, H), window(ends[1], W, H)
        if not np.isfinite(np.array(w0 + w1, F32)).all():
            continue
        drawn += 1
        p, z = raster(w0, w1, W, H)
        pix.append(p)
        zws.append(z)
    if not pix:
        return np.zeros(0, np.int64), np.zeros(0, F32), drawn
    return np.concatenate(pix), np.concatenate(zws), drawn


def draw_nodes(nodes, matrix, W, H, point_size, lut, color=YELLOW):
    """render_oracle.draw_nodes with every node's outline drawn right after the node's points (step 12): the same dict, with
    `winner` in the ranks of step 12 (node k owns n_k + 1 ranks, the last one is its outline), pixels_covered counting every
    pixel that is not background, plus segments_submitted, segments_drawn, outline_pixels, and for the tests' own bookkeeping
    `fragments` (per node the image pixel indices and zw of its outline's fragments) and `outline_rank` (per node)."""
    out = R.draw_nodes(nodes, matrix, W, H, point_size, lut)
    counts = np.array([np.frombuffer(nd["rgb"], np.uint8).size // 3 for nd in nodes], np.int64)
    first = np.concatenate([[0], np.cumsum(counts)])  # points before node k: its first rank is first[k] + k
    assert int(first[-1]) + len(nodes) < 2 ** 32 - 1
    # the points' winners keep their order under the new ranks, so the winner among the points of a pixel is the same point
    old = out["winner"].reshape(-1)
    key = np.full(W * H, np.uint64(0xffffffffffffffff))
    has = old >= 0
    node_of = np.searchsorted(first, old[has], side="right") - 1
    key[has] = (out["depth"].reshape(-1)[has].view(np.uint32).astype(np.uint64) << np.uint64(32)) | (old[has] + node_of).astype(np.uint64)
    outline_rank = first[1:] + np.arange(len(nodes))
    submitted = drawn = 0
    fragments = []
    for k, nd in enumerate(nodes):
        pix, zw, n = outline_fragments(nd["cube_min"], nd["cube_edge"], matrix, W, H)
        fragments.append((pix, zw))
        submitted += 12
        drawn += n
        if pix.size:
            np.minimum.at(key, pix, (zw.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(outline_rank[k]))
    covered = key != np.uint64(0xffffffffffffffff)
    rank = (key & np.uint64(0xffffffff)).astype(np.int64)
    is_outline = covered & np.isin(rank, outline_rank)
    image, depth, winner = out["image"].reshape(-1, 4), out["depth"].reshape(-1), out["winner"].reshape(-1)
    winner[covered] = rank[covered]
    depth[covered] = (key[covered] >> np.uint64(32)).astype(np.uint32).view(F32)
    image[is_outline] = np.asarray(color, np.uint8)
    out.update(pixels_covered=int(covered.sum()), outline_pixels=int(is_outline.sum()), segments_submitted=submitted, segments_drawn=drawn,
               fragments=fragments, outline_rank=outline_rank, first_rank=first[:-1] + np.arange(len(nodes)))
    return out


def render_view(tn, matrix, W, H, point_size=1.0, gamma=1.0, max_nodes=0, lut=None, color=YELLOW):
    """render_oracle.render_view with show_octree_nodes on (step 8: the boxes of the view's cut visible list)."""
    lut = R.gamma_lut(gamma) if lut is None else lut
    names = tn.visible(matrix)
    if names is None:
        out = draw_nodes([], matrix, W, H, point_size, lut, color)
        out.update(status=None, nodes_visible=None, drawn=[])
        return out
    drawn = names[:max_nodes] if max_nodes else names
    out = draw_nodes([tn.node(k) for k in drawn], matrix, W, H, point_size, lut, color)
    out.update(status=0, nodes_visible=len(names), drawn=drawn)
    return out
