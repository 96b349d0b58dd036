"""The terrain layer's reduction restated in numpy: the f64 chain with one ufunc call per operation, np.rint,
exact integer sums, the total-order key; and a checker of the geometry shader's whole requirement that knows nothing of how
quad ids are coded. Written from the contract, not from the C code.

params: dict(tile_size, resolution_m, origin[3], world_from_terrain[7] = translation xyz + quaternion ijkw, statistic
"max" | "min" | "mean", min_points)."""
import numpy as np

IDENTITY = [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0]


def params(tile_size=4, resolution_m=1.0, origin=(0.0, 0.0, 0.0), world_from_terrain=None, statistic="max", min_points=1):
    return dict(tile_size=int(tile_size), resolution_m=float(resolution_m), origin=[float(v) for v in origin],
                world_from_terrain=list(IDENTITY if world_from_terrain is None else world_from_terrain), statistic=statistic,
                min_points=int(min_points))


def frame(world_from_terrain):
    """terrain_from_world as (M [3, 3], t [3]): M = R^T / |q|^2 with R written out, every product and sum on its own."""
    t = np.array(world_from_terrain[:3], dtype=np.float64)
    i, j, k, w = (np.float64(v) for v in world_from_terrain[3:])
    ii, jj, kk, ww = i * i, j * j, k * k, w * w
    ij, ik, jk, wi, wj, wk = i * j, i * k, j * k, w * i, w * j, w * k
    s = ((ii + jj) + kk) + ww
    two = np.float64(2.0)
    r = np.array([[((ww + ii) - jj) - kk, two * (ij - wk), two * (ik + wj)],
                  [two * (ij + wk), ((ww - ii) + jj) - kk, two * (jk - wi)],
                  [two * (ik - wj), two * (jk + wi), ((ww - ii) - jj) + kk]], dtype=np.float64)
    return r.T / s, t


def chain(p, x, y, z):
    """dict(u, v, i, j (int64; 0 where not ok), h (float32), dz, ok) of every point."""
    x, y, z = (np.asarray(a, dtype=np.float64) for a in (x, y, z))
    m, t = frame(p["world_from_terrain"])
    o, res = np.array(p["origin"], dtype=np.float64), np.float64(p["resolution_m"])
    with np.errstate(all="ignore"):
        dx, dy, dz = np.subtract(x, t[0]), np.subtract(y, t[1]), np.subtract(z, t[2])
        row = lambda r: np.add(np.add(np.multiply(m[r, 0], dx), np.multiply(m[r, 1], dy)), np.multiply(m[r, 2], dz))
        lx, ly, lz = row(0), row(1), row(2)
        u = np.divide(np.subtract(lx, o[0]), res)
        v = np.divide(np.subtract(ly, o[1]), res)
        fi = np.floor(np.add(u, 0.5))
        fj = np.floor(np.add(v, 0.5))
        hz = np.subtract(lz, o[2])
        h = hz.astype(np.float32)  # round to nearest even
        ok_uv = np.isfinite(u) & np.isfinite(v) & (np.abs(fi) < 2.0 ** 62) & (np.abs(fj) < 2.0 ** 62)
        ok = ok_uv & np.isfinite(h)
        i = np.where(ok_uv, fi, 0.0).astype(np.int64)
        j = np.where(ok_uv, fj, 0.0).astype(np.int64)
    return dict(u=u, v=v, i=np.where(ok, i, 0), j=np.where(ok, j, 0), h=np.where(ok, h, np.float32(0)).astype(np.float32), dz=hz, ok=ok,
                ok_uv=ok_uv, i_uv=i, j_uv=j)


def declared_range(p, bbox_min, bbox_max):
    """(imin, imax, jmin, jmax): the (i, j) hull of the box's eight corners, widened by one vertex."""
    lo, hi = np.asarray(bbox_min, dtype=np.float64), np.asarray(bbox_max, dtype=np.float64)
    cx = np.array([[hi[0] if c & 1 else lo[0], hi[1] if c & 2 else lo[1], hi[2] if c & 4 else lo[2]] for c in range(8)])
    c = chain(p, cx[:, 0], cx[:, 1], cx[:, 2])  # only u and v make the range: a corner's height may overflow f32
    assert c["ok_uv"].all(), "a corner of the box has no grid vertex"
    return int(c["i_uv"].min()) - 1, int(c["i_uv"].max()) + 1, int(c["j_uv"].min()) - 1, int(c["j_uv"].max()) + 1


def ord32(h):
    """The monotone map of f32 bits onto u32: total order, -0 < +0."""
    b = np.asarray(h, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return np.where(b & 0x80000000, ~b & 0xFFFFFFFF, b | 0x80000000).astype(np.uint64)


def unord32(k):
    k = np.asarray(k, dtype=np.uint64)
    b = np.where(k & 0x80000000, k & 0x7FFFFFFF, ~k & 0xFFFFFFFF).astype(np.uint32)
    return b.view(np.float32)


def quad_masks(is_set, i0=0, j0=0):
    """uint32 [h, w] masks of a window of set flags [h, w] (row = j - j0, column = i - i0); outside it nothing is set."""
    s = np.asarray(is_set, dtype=bool)
    h, w = s.shape
    out = np.zeros((h, w), dtype=np.uint32)
    if h < 2 or w < 2:
        return out
    q = s[:-1, :-1] & s[:-1, 1:] & s[1:, :-1] & s[1:, 1:]  # q[r, c]: the quad whose lower corner is (c, r)
    bit = (np.uint32(1) << (((np.arange(w - 1) + i0) % 3)[None, :] + 3 * ((np.arange(h - 1) + j0) % 3)[:, None]).astype(np.uint32))
    qb = np.where(q, bit, np.uint32(0)).astype(np.uint32)
    out[:-1, :-1] |= qb
    out[:-1, 1:] |= qb
    out[1:, :-1] |= qb
    out[1:, 1:] |= qb
    return out


def check_property(masks, is_set):
    """The geometry shader's requirement over a window: for the triangles of every quad — under either diagonal, all four —
    the AND of the three vertices' masks is nonzero iff the quad's four corners are set. Returns the list of violations
    (quad column, quad row, triangle, AND, rendered)."""
    m, s = np.asarray(masks).astype(np.uint32), np.asarray(is_set, dtype=bool)
    ll, lr, ul, ur = m[:-1, :-1], m[:-1, 1:], m[1:, :-1], m[1:, 1:]
    rendered = s[:-1, :-1] & s[:-1, 1:] & s[1:, :-1] & s[1:, 1:]
    bad = []
    for name, tri in (("ll-lr-ur", ll & lr & ur), ("ll-ur-ul", ll & ur & ul), ("ll-lr-ul", ll & lr & ul), ("lr-ur-ul", lr & ur & ul)):
        for r, c in zip(*np.nonzero((tri != 0) != rendered)):
            bad.append((int(c), int(r), name, int(tri[r, c]), bool(rendered[r, c])))
    return bad


def reduce(p, bbox_min, bbox_max, x, y, z, rgb, vertices=None):
    """The whole reduction -> dict(tiles int32 [n, 2] ascending by (x, y), heights f32 [n, T, T, 2], colors u8 [n, T, T, 4],
    counts u32 [n, T, T], outside, set_vertices, rendered_quads, window = (i0, j0, set flags) of the declared range).
    vertices: the points' dict(i, j, h, dz, ok) from elsewhere (the host twin), in place of this file's chain."""
    T, stat, minp = p["tile_size"], p["statistic"], p["min_points"]
    rgb = np.asarray(rgb, dtype=np.uint8).reshape(-1, 3)
    c = chain(p, x, y, z) if vertices is None else vertices
    imin, imax, jmin, jmax = declared_range(p, bbox_min, bbox_max)
    keep = c["ok"] & (c["i"] >= imin) & (c["i"] <= imax) & (c["j"] >= jmin) & (c["j"] <= jmax)
    if stat == "mean":
        with np.errstate(all="ignore"):
            keep &= np.abs(c["dz"]) < 2.0 ** 21
    outside = int(keep.size - keep.sum())
    i, j, h, dz, col = c["i"][keep], c["j"][keep], c["h"][keep], c["dz"][keep], rgb[keep].astype(np.uint64)
    w, hgt = imax - imin + 1, jmax - jmin + 1
    assert w * hgt <= 1 << 26, "the truth keeps the declared range dense: choose a smaller box"
    flat = (j - jmin) * w + (i - imin)
    count = np.bincount(flat, minlength=w * hgt).astype(np.int64)
    height = np.zeros(w * hgt, dtype=np.float32)
    color = np.zeros((w * hgt, 4), dtype=np.uint8)
    is_set = count >= minp
    if stat in ("max", "min"):
        o = ord32(h)
        if stat == "min":
            o = ~o & np.uint64(0xFFFFFFFF)
        key = (o << np.uint64(32)) | (col[:, 0] << np.uint64(16)) | (col[:, 1] << np.uint64(8)) | col[:, 2]
        best = np.zeros(w * hgt, dtype=np.uint64)
        np.maximum.at(best, flat, key)
        bo = best >> np.uint64(32)
        if stat == "min":
            bo = ~bo & np.uint64(0xFFFFFFFF)
        height = np.where(is_set, unord32(bo), np.float32(0)).astype(np.float32)
        for ch, sh in enumerate((16, 8, 0)):
            color[:, ch] = np.where(is_set, (best >> np.uint64(sh)) & np.uint64(255), 0)
    else:
        hq = np.rint(dz * 1024.0).astype(np.int64)
        sum_h = np.zeros(w * hgt, dtype=np.int64)
        np.add.at(sum_h, flat, hq)
        n = np.maximum(count, 1)
        height = np.where(is_set, ((sum_h.astype(np.float64) / n.astype(np.float64)) / 1024.0).astype(np.float32), np.float32(0)).astype(np.float32)
        for ch in range(3):
            sc = np.zeros(w * hgt, dtype=np.int64)
            np.add.at(sc, flat, col[:, ch].astype(np.int64))
            color[:, ch] = np.where(is_set, (sc + n // 2) // n, 0)
    color[:, 3] = np.where(is_set, 255, 0)
    set2 = is_set.reshape(hgt, w)
    masks = quad_masks(set2, imin, jmin)
    rendered = int((set2[:-1, :-1] & set2[:-1, 1:] & set2[1:, :-1] & set2[1:, 1:]).sum()) if hgt > 1 and w > 1 else 0
    # cut into tiles: the tiles with a set vertex, ascending by (x, y)
    sj, si = np.nonzero(set2)
    tiles = np.unique(np.stack([(si + imin) // T, (sj + jmin) // T], axis=1), axis=0).astype(np.int32).reshape(-1, 2)
    n = tiles.shape[0]
    heights, colors, counts = np.zeros((n, T, T, 2), np.float32), np.zeros((n, T, T, 4), np.uint8), np.zeros((n, T, T), np.uint32)
    h2, c2, n2 = height.reshape(hgt, w), color.reshape(hgt, w, 4), count.reshape(hgt, w)
    for k, (tx, ty) in enumerate(tiles):
        # the part of the tile inside the declared range
        a0, a1 = max(int(tx) * T, imin), min(int(tx) * T + T - 1, imax)
        b0, b1 = max(int(ty) * T, jmin), min(int(ty) * T + T - 1, jmax)
        dst = (slice(b0 - int(ty) * T, b1 - int(ty) * T + 1), slice(a0 - int(tx) * T, a1 - int(tx) * T + 1))
        src = (slice(b0 - jmin, b1 - jmin + 1), slice(a0 - imin, a1 - imin + 1))
        heights[k][dst + (0,)] = h2[src]
        heights[k][dst + (1,)] = masks[src].astype(np.float32)
        colors[k][dst] = c2[src]
        counts[k][dst] = n2[src]
    return dict(tiles=tiles, heights=heights, colors=colors, counts=counts, outside=outside, set_vertices=int(is_set.sum()),
                rendered_quads=rendered, window=(imin, jmin, set2))


def assemble(tiles, plane, T):
    """Tiles [n, T, T, ...] laid out as one window: (i0, j0, array [rows, columns, ...]), zeros where no tile is."""
    tiles = np.asarray(tiles).reshape(-1, 2)
    x0, x1, y0, y1 = tiles[:, 0].min(), tiles[:, 0].max(), tiles[:, 1].min(), tiles[:, 1].max()
    out = np.zeros(((y1 - y0 + 1) * T, (x1 - x0 + 1) * T) + plane.shape[3:], dtype=plane.dtype)
    for k, (tx, ty) in enumerate(tiles):
        out[(ty - y0) * T:(ty - y0 + 1) * T, (tx - x0) * T:(tx - x0 + 1) * T] = plane[k]
    return int(x0) * T, int(y0) * T, out
