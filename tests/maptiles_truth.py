"""A numpy truth for the map-tile product (csrc/pcv_maptiles.hip).

    pixel    (u, v) from pcv_wmr_project (the host twin of the kernels' chain; its distance to a long-double / mpmath truth is
             test_wmr_cpu's and test_maptiles_cpu's subject), S = 256 * 2^zoom, gx = floor(u S), gy = floor(v S): exact in
             f64 because S is a power of two. Drawn iff u S and v S are finite, >= 0 and < S.
    value    integer sums per pixel via np.add.at, xray_truth.colored_rgba, then pixels with alpha < 128 (and pixels
             without a point) take the background
    parents  xray_pyramid_oracle.resize_half(build_parent(children)): child digit c = 2 xbit + (1 - ybit)
    json     tiles.json, with Python's own repr of a double (shortest round trip) and math for the bounds
"""
import math

import numpy as np

import point_cloud_viewer_amd as pcv

import xray_pyramid_oracle as XP
import xray_truth as XT

T = 256


def main_cloud(seed=7, sites=2000, per_site=10):
    """The GPU tests' cloud: `sites` sites uniform in the config-1 box (200 x 200 x 20 m at lat 37.407204, lon -122.147604),
    `per_site` points within 2 cm of each, random colours. At zoom 19 it covers 4 x 4 tiles."""
    from point_cloud_viewer_amd import synthetic
    rng = np.random.default_rng(seed)
    local = np.empty((sites, 3))
    local[:, 0], local[:, 1], local[:, 2] = rng.uniform(-100, 100, sites), rng.uniform(-100, 100, sites), rng.uniform(-10, 10, sites)
    local = np.repeat(local, per_site, axis=0) + rng.uniform(-0.02, 0.02, (sites * per_site, 3))
    rot, t = synthetic.ecef_from_local(37.407204, -122.147604)
    p = local @ rot.T + t
    rgb = rng.integers(0, 256, (len(p), 3), dtype=np.uint8)
    return np.ascontiguousarray(p[:, 0]), np.ascontiguousarray(p[:, 1]), np.ascontiguousarray(p[:, 2]), rgb


def ecef_from_lat_lng(lat, lng, h=0.0):
    """WGS84 (radians, metres) -> ECEF, the prime-vertical radius form."""
    lat, lng = np.asarray(lat, dtype=np.float64), np.asarray(lng, dtype=np.float64)
    a, e2 = 6378137.0, 0.006694379990141317
    n = a / np.sqrt(1.0 - e2 * np.sin(lat) ** 2)
    return (n + h) * np.cos(lat) * np.cos(lng), (n + h) * np.cos(lat) * np.sin(lng), (n * (1.0 - e2) + h) * np.sin(lat)


def edge_points(zoom):
    """(x, y, z) of the edge set: NaN and infinite coordinates, the origin, the -x axis with y = +0.0 (u = 1, dropped) and
    y = -0.0 (u = 0, drawn at gx = 0), latitudes beyond +-85.06 degrees, the poles, and the corners of wmr_oracle.grid's
    rectangles laid on the tile seams of `zoom` around the config-1 site, each nudged by +-1 ulp per axis."""
    import wmr_oracle as W
    pts = [(np.nan, 1.0, 2.0), (1.0, np.nan, 2.0), (1.0, 2.0, np.nan), (np.inf, 1.0, 2.0), (-np.inf, 1.0, 2.0), (1.0, np.inf, 2.0),
           (1.0, 2.0, -np.inf), (np.inf, np.inf, np.inf), (0.0, 0.0, 0.0), (-0.0, -0.0, -0.0)]
    for r in (6378137.0, 6378100.0, 1.0, 7.0e6):
        for zz in (0.0, 1000.0, -2.5e6):
            pts += [(-r, 0.0, zz), (-r, -0.0, zz)]
    for lat in (85.06, 85.0511287798066, 85.0512, 86.0, 89.9, 89.999999, -85.06, -85.0511287798066, -85.0512, -86.0, -89.9):
        for lng in (-122.147604, 0.0, 179.9999, -180.0, 180.0, 45.0):
            for h in (0.0, 9000.0):
                pts.append(tuple(float(c) for c in ecef_from_lat_lng(math.radians(lat), math.radians(lng), h)))
    pts += [(0.0, 0.0, 6356752.314245179), (0.0, 0.0, -6356752.314245179), (1e-9, 0.0, 6356752.3), (0.0, -1e-9, -6356752.3)]
    x, y, z = (np.array([p[a] for p in pts], dtype=np.float64) for a in range(3))
    # the seams: a 3 x 3 grid of tile-sized rectangles whose corners are tile corners of `zoom`
    side = 1.0 / (1 << zoom)
    cu, cv = pcv.wmr_project(*(np.array([c]) for c in ecef_from_lat_lng(math.radians(37.407204), math.radians(-122.147604))))
    tx, ty = math.floor(float(cu[0]) / side), math.floor(float(cv[0]) / side)
    rects = W.grid((tx + 1.5) * side, (ty + 1.5) * side, 3, side)
    su = np.array(sorted({r[0] for r in rects} | {r[2] for r in rects}))
    sv = np.array(sorted({r[1] for r in rects} | {r[3] for r in rects}))
    assert np.array_equal(su, (tx + np.arange(4)) * side) and np.array_equal(sv, (ty + np.arange(4)) * side)
    uu, vv = (a.ravel() for a in np.meshgrid(su, sv))
    lat, lng = pcv.wmr_to_lat_lng(uu, vv)
    seams = []
    for h in (0.0, 35.0):
        sx, sy, sz = ecef_from_lat_lng(lat, lng, h)
        for dx in (-1, 0, 1):
            for dy in (-1, 0, 1):
                for dz in (-1, 0, 1):
                    nudge = lambda a, d: a if d == 0 else np.nextafter(a, np.inf * d)
                    seams.append((nudge(sx, dx), nudge(sy, dy), nudge(sz, dz)))
    x = np.concatenate([x] + [s[0] for s in seams])
    y = np.concatenate([y] + [s[1] for s in seams])
    z = np.concatenate([z] + [s[2] for s in seams])
    return np.ascontiguousarray(x), np.ascontiguousarray(y), np.ascontiguousarray(z)


def pixels(zoom, x, y, z):
    """(gx, gy as int64, ok): the pixel rule over pcv_wmr_project's (u, v); gx = gy = 0 where dropped."""
    x, y, z = (np.asarray(a, dtype=np.float64) for a in (x, y, z))
    u, v = pcv.wmr_project(x, y, z)
    S = float(T << zoom)
    with np.errstate(invalid="ignore", over="ignore"):
        us, vs = u * S, v * S
        ok = (us >= 0.0) & (us < S) & (vs >= 0.0) & (vs < S)
    # some infinite coordinates come out of the chain with a finite (u, v): a coordinate that is not finite drops the point
    ok &= np.isfinite(x) & np.isfinite(y) & np.isfinite(z)
    gx = np.where(ok, np.floor(np.where(ok, us, 0.0)), 0.0).astype(np.int64)
    gy = np.where(ok, np.floor(np.where(ok, vs, 0.0)), 0.0).astype(np.int64)
    return gx, gy, ok


def pack_background(background):
    return np.array([int(v) & 255 for v in background], dtype=np.uint8)


def reduce(zoom, x, y, z, rgb, background=(0, 0, 0, 0)):
    """dict(tiles uint32 [n, 2] ascending by (x, y), images uint8 [n, 256, 256, 4], counts uint32 [n, 256, 256], dropped,
    drawn, over: pixels with more than 2^24 points)."""
    gx, gy, ok = pixels(zoom, x, y, z)
    rgb = np.asarray(rgb, dtype=np.uint8).reshape(-1, 3)
    gx, gy, c = gx[ok], gy[ok], rgb[ok].astype(np.int64)
    key = ((gx >> 8) << 32) | (gy >> 8)
    keys = np.unique(key)  # ascending by (x, y)
    slot = np.searchsorted(keys, key)
    pix = slot * (T * T) + (gy & 255) * T + (gx & 255)
    n = np.bincount(pix, minlength=len(keys) * T * T).astype(np.int64)
    sums = np.zeros((3, len(keys) * T * T), dtype=np.int64)
    for k in range(3):
        np.add.at(sums[k], pix, c[:, k])
    bg = pack_background(background)
    img = np.empty((len(keys) * T * T, 4), dtype=np.uint8)
    img[:] = bg
    hit = np.flatnonzero(n)
    if hit.size:
        px = XT.colored_rgba(sums[0][hit], sums[1][hit], sums[2][hit], n[hit])
        px[px[:, 3] < 128] = bg
        img[hit] = px
    tiles = np.stack([keys >> 32, keys & 0xffffffff], axis=1).astype(np.uint32).reshape(-1, 2)
    return dict(tiles=tiles, images=img.reshape(-1, T, T, 4), counts=n.astype(np.uint32).reshape(-1, T, T), dropped=int((~ok).sum()),
                drawn=int(ok.sum()), over=int((n > (1 << 24)).sum()))


def quad_index(zoom, x, y):
    index = 0
    for b in range(zoom - 1, -1, -1):
        index = (index << 2) | (2 * ((x >> b) & 1) + (1 - ((y >> b) & 1)))
    return index


def parents(zoom, min_zoom, tiles, images, background=(0, 0, 0, 0)):
    """{z: (tiles uint32 [n, 2] ascending by (x, y), images)} for z = zoom down to min_zoom."""
    bg = pack_background(background)
    tp = XP.taps(T)
    out = {zoom: (np.asarray(tiles, dtype=np.uint32).reshape(-1, 2), np.asarray(images))}
    for z in range(zoom - 1, min_zoom - 1, -1):
        ct, ci = out[z + 1]
        have = {(int(x), int(y)): ci[k] for k, (x, y) in enumerate(ct)}
        up = sorted({(x >> 1, y >> 1) for x, y in have})
        imgs = np.empty((len(up), T, T, 4), dtype=np.uint8)
        for k, (px, py) in enumerate(up):
            children = [None] * 4
            for dx in (0, 1):
                for dy in (0, 1):
                    children[2 * dx + (1 - dy)] = have.get((2 * px + dx, 2 * py + dy))
            imgs[k] = XP.resize_half(XP.build_parent(children, T, bg), tp)
        out[z] = (np.array(up, dtype=np.uint32).reshape(-1, 2), imgs)
    return out


def lat_lng_deg(u, v):
    """WebMercatorCoord::to_lat_lng (web_mercator.rs:55-64) with Python's math, in degrees."""
    sin_y = 1.0 / ((math.exp(-(v - 0.5) * 4.0 * math.pi) + 1.0) * -0.5) + 1.0
    return math.degrees(math.asin(sin_y)), math.degrees((u - 0.5) * 2.0 * math.pi)


def bounds(zoom, tiles):
    """[west, south, east, north] in degrees of the hull of the tiles' corners; zeros without a tile."""
    t = np.asarray(tiles, dtype=np.int64).reshape(-1, 2)
    if len(t) == 0:
        return [0.0, 0.0, 0.0, 0.0]
    s = float(1 << zoom)
    north, west = lat_lng_deg(t[:, 0].min() / s, t[:, 1].min() / s)
    south, east = lat_lng_deg((t[:, 0].max() + 1) / s, (t[:, 1].max() + 1) / s)
    return [west, south, east, north]


def json_text(tiles_by_zoom, bounds_of=None):
    """tiles.json for {z: [[x, y], ...]} over a contiguous range of zooms; bounds_of: the four doubles to print (default: this
    module's own evaluation)."""
    zooms = sorted(tiles_by_zoom)
    f = lambda v: repr(float(v))
    b = bounds(zooms[-1], tiles_by_zoom[zooms[-1]]) if bounds_of is None else bounds_of
    lists = ",".join('"%d":[%s]' % (z, ",".join("[%d,%d]" % (int(x), int(y)) for x, y in tiles_by_zoom[z])) for z in zooms)
    return ('{"scheme":"xyz","format":"png","tile_size":256,"minzoom":%d,"maxzoom":%d,"bounds":[%s],"tiles":{%s}}'
            % (zooms[0], zooms[-1], ",".join(f(v) for v in b), lists))
