"""Numpy restatement of xray's leaf level (xray/src/generation.rs) — the CPU oracle of pcv_xray_*.

Geometry: find_quadtree_bounding_rect_and_levels :515, get_nodes_at_level :534, get_bounding_box :550, Node::get_child
(quadtree/src/lib.rs:80-97), Obb::from(Aabb).transformed (obb.rs:20-47). Points: oracle_lib's nodes_in_location,
decode_positions, cull_points and iso_transform_points, node by node in nodes_in_location order — one valid order of the
reference's single-threaded ParallelIterator. Strategies: :159-199 (xray), :294-345 (colored, f32 sums in that order),
:365-408 (height_stddev: streaming_stats::OnlineStats restated as Welford with variance = q / n; the crate is not vendored,
so this restatement is unpinned), colormap.rs, color.rs:29-36; background :684.
"""
import math

import numpy as np

import oracle_lib as O

F32 = np.float32
WHITE, TRANSPARENT = (255, 255, 255, 255), (255, 255, 255, 0)


# ---- geometry (Python floats are IEEE f64; every expression keeps the reference's operation order) ------------------
def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def quat_rotate(q, v):
    """UnitQuaternion * Vector3 as nalgebra computes it: t = 2 (q.v x v); v + w t + q.v x t."""
    qv = (q[0], q[1], q[2])
    t = tuple(c * 2.0 for c in _cross(qv, v))
    c = _cross(qv, t)
    return tuple((t[i] * q[3] + c[i]) + v[i] for i in range(3))


def iso_point(iso, p):
    r = quat_rotate(iso[3:7], p)
    return (r[0] + iso[0], r[1] + iso[1], r[2] + iso[2])


def bounding_box(bmin, bmax, iso=None):
    if iso is None:
        return tuple(float(v) for v in bmin), tuple(float(v) for v in bmax)
    corners = [(bmax[0] if ix else bmin[0], bmax[1] if iy else bmin[1], bmax[2] if iz else bmin[2])
               for ix in (0, 1) for iy in (0, 1) for iz in (0, 1)]
    pts = [iso_point(iso, tuple(float(c) for c in k)) for k in corners]
    lo, hi = list(pts[0]), list(pts[0])
    for p in pts[1:]:
        for a in range(3):
            lo[a] = p[a] if p[a] < lo[a] else lo[a]
            hi[a] = p[a] if p[a] > hi[a] else hi[a]
    return tuple(lo), tuple(hi)


def node_id(name):
    return len(name) - 1, (int(name[1:], 4) if len(name) > 1 else 0)


def node_name(level, index):
    return "r" + "".join(str((index >> (2 * l)) & 3) for l in range(level - 1, -1, -1))


def parent_id(level, index):
    return None if level == 0 else (level - 1, index >> 2)


def child_index(level, index):
    return None if level == 0 else index & 3


def get_child(node, ci):
    (level, index), (mx, my), edge = node
    half = edge / 2.0
    if ci & 1:
        my += half
    if ci & 2:
        mx += half
    return ((level + 1, (index << 2) + ci), (mx, my), half)


def leaf_geometry(tile_size_px, pixel_size_m, bmin, bmax, iso=None, root="r"):
    lo, hi = bounding_box(bmin, bmax, iso)
    dx, dy = hi[0] - lo[0], hi[1] - lo[1]
    cur, levels = float(tile_size_px) * pixel_size_m, 0
    while cur < dx or cur < dy:
        cur *= 2.0
        levels += 1
    rl, ri = node_id(root)
    node = ((0, 0), (lo[0], lo[1]), cur)
    for l in range(rl - 1, -1, -1):
        node = get_child(node, (ri >> (2 * l)) & 3)
    leaves, stack = [], [node]
    while stack:
        nd = stack.pop()
        if nd[0][0] == levels:
            leaves.append(nd)
        else:
            stack.extend(get_child(nd, i) for i in range(4))
    tiles = [((mx, my, lo[2]), (mx + e, my + e, hi[2])) for _, (mx, my), e in leaves]
    return dict(rect=(lo[0], lo[1], cur), deepest_level=levels, leaf_index=[l[0][1] for l in leaves],
                leaf_ids=[node_name(*l[0]) for l in leaves], tile_bbox=tiles, bbox=(lo, hi))


def tile_obb(iso, mn, mx):
    """Obb::from(tile).transformed(&query_from_global.inverse()) as pcv_shape OBB params."""
    qi = (-iso[3], -iso[4], -iso[5], iso[6])
    ti = quat_rotate(qi, (-iso[0], -iso[1], -iso[2]))
    c = tuple((mn[a] + mx[a]) * 0.5 for a in range(3))
    rc = quat_rotate(qi, c)
    t = tuple(ti[a] + rc[a] for a in range(3))
    w = qi[3] * 1.0 - ((qi[0] * 0.0 + qi[1] * 0.0) + qi[2] * 0.0)
    q = (qi[3] * 0.0 + qi[0] * 1.0 + (qi[1] * 0.0 - qi[2] * 0.0), qi[3] * 0.0 + qi[1] * 1.0 + (qi[2] * 0.0 - qi[0] * 0.0),
         qi[3] * 0.0 + qi[2] * 1.0 + (qi[0] * 0.0 - qi[1] * 0.0), w)
    return list(t) + list(q) + [(mx[a] - mn[a]) * 0.5 for a in range(3)]


# ---- colour functions -------------------------------------------------------------------------------------------------
def sat_u8(v):
    v = np.asarray(v, dtype=F32)
    out = np.where(~(v > 0), F32(0), np.where(v >= F32(255), F32(255), np.trunc(v)))
    return out.astype(np.uint8)


def to_u8(r, g, b, a):
    f = lambda c: sat_u8(np.asarray(c, dtype=F32) * F32(255))
    return np.stack(np.broadcast_arrays(f(r), f(g), f(b), f(a)), axis=-1)


def xray_value(n):
    v = (1.0 - math.log(n) / math.log(1024.0)) * 255.0
    return 0 if not v > 0 else (255 if v >= 255 else int(v))


def _interp(v, y0, x0, y1, x1):
    return (v - F32(x0)) * (F32(y1) - F32(y0)) / (F32(x1) - F32(x0)) + F32(y0)


def jet_base(val):
    val = np.asarray(val, dtype=F32)
    return np.where(val <= F32(-0.75), F32(0), np.where(val <= F32(-0.25), _interp(val, 0.0, -0.75, 1.0, -0.25),
                    np.where(val <= F32(0.25), F32(1), np.where(val <= F32(0.75), _interp(val, 1.0, 0.25, 0.0, 0.75), F32(0)))))


def jet(val):
    val = np.asarray(val, dtype=F32)
    return to_u8(jet_base(val - F32(0.5)), jet_base(val), jet_base(val + F32(0.5)), F32(1))


def purplish(val):
    val = np.asarray(val, dtype=F32)
    return to_u8((F32(1) - val) * F32(0.8), (F32(1) - val) * F32(0.8), (F32(1) - val) * F32(1.0), F32(1))


# ---- points and raster --------------------------------------------------------------------------------------------------
class TreePoints:
    """Decoded node positions of an oracle octree, cached per node."""

    def __init__(self, oracle_nodes, cube_of, bmin, bmax):
        self.nodes, self.cube_of, self.bmin, self.bmax, self.cache = oracle_nodes, cube_of, bmin, bmax, {}

    def node(self, name):
        if name not in self.cache:
            nd = self.nodes[name]
            cmin, edge = self.cube_of(name)
            x, y, z = O.decode_positions(nd["encoding"], cmin, edge, nd["xyz"])
            inten = np.frombuffer(nd["intensity"], dtype=np.float32) if nd["intensity"] else None
            self.cache[name] = (x, y, z, np.frombuffer(nd["rgb"], dtype=np.uint8).reshape(-1, 3), inten)
        return self.cache[name]

    def query(self, kind, params, interval=None):
        xs, ys, zs, cs = [], [], [], []
        for name in O.nodes_in_location(self.bmin, self.bmax, self.nodes, kind, params):
            if self.nodes[name]["num_points"] == 0:
                continue
            x, y, z, rgb, inten = self.node(name)
            keep = O.cull_points(kind, params, x, y, z, inten if interval is not None else None, interval).astype(bool)
            xs.append(x[keep]), ys.append(y[keep]), zs.append(z[keep]), cs.append(rgb[keep])
        if not xs:
            return np.zeros(0), np.zeros(0), np.zeros(0), np.zeros((0, 3), np.uint8)
        return np.concatenate(xs), np.concatenate(ys), np.concatenate(zs), np.concatenate(cs)


def sat_u32(v):
    v = np.asarray(v, dtype=np.float64)
    out = np.where(~(v > 0), 0.0, np.where(v >= 4294967295.0, 4294967295.0, np.trunc(np.where(np.isfinite(v), v, 0.0))))
    return out.astype(np.uint64)


def discretise(x, y, z, mn, mx, W):
    d = [mx[a] - mn[a] for a in range(3)]
    px = sat_u32(((x - mn[0]) / d[0]) * float(W))
    py = sat_u32((1.0 - ((y - mn[1]) / d[1])) * float(W))
    pz = sat_u32(((z - mn[2]) / d[2]) * 1024.0)
    return px, py, pz


def _groups(pix):
    """Stable sort by pixel: (order, unique pixels, starts, counts)."""
    order = np.argsort(pix, kind="stable")
    u, starts, counts = np.unique(pix[order], return_index=True, return_counts=True)
    return order, u, starts, counts


def tile_image(x, y, z, rgb, mn, mx, W, strategy, background="white"):
    """RGBA (W, W, 4) of one created tile and the number of drawn points."""
    px, py, pz = discretise(x, y, z, mn, mx, W)
    draw = (px < W) & (py < W)
    img = np.empty((W, W, 4), dtype=np.uint8)
    img[:] = TRANSPARENT
    pix = (py[draw] * W + px[draw]).astype(np.int64)
    if pix.size:
        order, u, starts, counts = _groups(pix)
        if strategy == "xray":
            key = np.unique(pix * 2048 + pz[draw].astype(np.int64))
            n = np.bincount(np.searchsorted(u, key // 2048), minlength=u.size)
            v = np.array([255] + [xray_value(c) for c in range(1, 1026)], dtype=np.uint8)[n]
            col = np.stack([v, v, v, np.full_like(v, 255)], axis=-1)
        elif strategy == "colored":
            c = (rgb[draw][order].astype(F32) / F32(255))
            sums = np.zeros((u.size, 3), dtype=F32)
            for k in range(int(counts.max())):
                live = counts > k
                sums[live] = sums[live] + c[starts[live] + k]
            cnt = counts.astype(F32)
            mean = sums / cnt[:, None]
            alpha = np.minimum(counts, 1 << 24).astype(F32) / cnt
            col = to_u8(mean[:, 0], mean[:, 1], mean[:, 2], alpha)
        else:
            _, max_stddev, cmap = strategy
            zz = z[draw][order]
            mean, q = np.zeros(u.size), np.zeros(u.size)
            for k in range(int(counts.max())):
                live = counts > k
                xk = zz[starts[live] + k]
                old = mean[live]
                mean[live] = old + (xk - old) / float(k + 1)
                q[live] = q[live] + (xk - old) * (xk - mean[live])
            sd = np.sqrt(q / counts).astype(F32)
            m = F32(max_stddev)
            s = np.where(sd < F32(0), F32(0), np.where(sd > m, m, sd)) / m
            col = jet(s) if cmap == "jet" else purplish(s)
        img.reshape(-1, 4)[u] = col
    bg = WHITE if background == "white" else TRANSPARENT
    img[img[..., 3] < 128] = bg
    return img, int(draw.sum())


def xray_tiles(tp, tile_size_px, pixel_size_m, strategy, iso=None, interval=None, background="white", root="r"):
    """{leaf id: (image, drawn)} for every created tile, and the geometry."""
    g = leaf_geometry(tile_size_px, pixel_size_m, tp.bmin, tp.bmax, iso, root)
    out = {}
    for name, (mn, mx) in zip(g["leaf_ids"], g["tile_bbox"]):
        if iso is None:
            kind, params = O.SHAPE_AABB, list(mn) + list(mx)
        else:
            kind, params = O.SHAPE_OBB, tile_obb(iso, mn, mx)
        x, y, z, rgb = tp.query(kind, params, interval)
        if x.size == 0:
            continue
        if iso is not None:
            x, y, z = O.iso_transform_points(iso, x, y, z)
        out[name] = tile_image(x, y, z, rgb, mn, mx, tile_size_px, strategy, background)
    return out, g
