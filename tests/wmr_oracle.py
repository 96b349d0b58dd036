"""Oracle of the web-mercator rectangle (reference src/geometry/web_mercator_rect.rs, src/math/web_mercator.rs, src/math/sat.rs).

Truth of a point's normalised map coordinates (u, v): an ITERATED geodetic inverse (not the closed form the library restates)
followed by the projection, in mpmath at 40 digits (`truth_uv_mp`). mpmath costs about a millisecond per point, so a cloud of
200 000 points goes through the same iteration in numpy long double first (`truth_uv_ld`, 64-bit mantissa on x86: a few 1e-19
per operation); `truth_uv` keeps that value for every point farther than 1e-13 + delta from each bound it is tested against
and recomputes the others — the only ones whose classification the long-double error could touch — with mpmath. The caller
checks the long-double values against mpmath on a sample (test_wmr_cpu.py asserts < 1e-15, two orders below the 1e-13 guard).

The SAT side is a literal numpy restatement: intersector() (web_mercator_rect.rs:85-116), cache_separating_axes_for_aabb
(sat.rs:111-143) and the Relation of sat.rs:174-205, in plain f64 with left-to-right dot products as nalgebra evaluates them."""
import math

import numpy as np

A = 6378137.0
F = 1.0 / 298.257223563
E2 = F * (2.0 - F)
LAT_BOUND_RAD = 1.4844222297453324
REL_IN, REL_CROSS, REL_OUT = 0, 1, 2


# ---- truth ---------------------------------------------------------------------------------------------------------------
def truth_uv_ld(x, y, z, iterations=12):
    """(u, v) as long double arrays: geodetic latitude by fixed-point iteration on the exact relation
    tan(lat) = z / (p (1 - e^2 N / (N + h))), which contracts by about e^2 per step at terrestrial heights."""
    ld = np.longdouble
    x, y, z = (np.asarray(a, dtype=ld) for a in (x, y, z))
    a, f = ld(A), ld(1) / ld("298.257223563")
    e2 = f * (2 - f)
    p = np.sqrt(x * x + y * y)
    lat = np.arctan2(z, p * (1 - e2))
    for _ in range(iterations):
        s = np.sin(lat)
        n = a / np.sqrt(1 - e2 * s * s)
        h = p / np.cos(lat) - n
        lat = np.arctan2(z, p * (1 - e2 * n / (n + h)))
    lng = np.arctan2(y, x)
    pi = ld("3.14159265358979323846264338327950288")
    lat = np.clip(lat, -ld(LAT_BOUND_RAD), ld(LAT_BOUND_RAD))
    s = np.sin(lat)
    return ld(0.5) + lng / (2 * pi), ld(0.5) - np.log((1 + s) / (1 - s)) / (4 * pi)


def truth_uv_mp(x, y, z, iterations=30):
    """(u, v) of ONE point as mpmath numbers at 40 digits, same iteration."""
    import mpmath as mp
    with mp.workdps(40):
        x, y, z = mp.mpf(float(x)), mp.mpf(float(y)), mp.mpf(float(z))
        a, f = mp.mpf(A), 1 / mp.mpf("298.257223563")
        e2 = f * (2 - f)
        p = mp.sqrt(x * x + y * y)
        lat = mp.atan2(z, p * (1 - e2))
        for _ in range(iterations):
            s = mp.sin(lat)
            n = a / mp.sqrt(1 - e2 * s * s)
            h = p / mp.cos(lat) - n
            lat = mp.atan2(z, p * (1 - e2 * n / (n + h)))
        lng = mp.atan2(y, x)
        lat = min(max(lat, -mp.mpf(LAT_BOUND_RAD)), mp.mpf(LAT_BOUND_RAD))
        s = mp.sin(lat)
        return +(mp.mpf(0.5) + lng / (2 * mp.pi)), +(mp.mpf(0.5) - mp.log((1 + s) / (1 - s)) / (4 * mp.pi))


def truth_uv(x, y, z, ubounds, vbounds, delta):
    """(u, v) as long double arrays; points within delta + 1e-13 of any of the given bounds are recomputed with mpmath.
    Returns (u, v, number of points recomputed)."""
    u, v = truth_uv_ld(x, y, z)
    guard = np.longdouble(delta) + np.longdouble(1e-13)
    near = np.zeros(u.shape, dtype=bool)
    for b in ubounds:
        near |= np.abs(u - np.longdouble(b)) <= guard
    for b in vbounds:
        near |= np.abs(v - np.longdouble(b)) <= guard
    idx = np.nonzero(near)[0]
    for i in idx:
        mu, mv = truth_uv_mp(x[i], y[i], z[i])
        u[i], v[i] = _mp_to_ld(mu), _mp_to_ld(mv)
    return u, v, idx.size


def _mp_to_ld(m):
    import mpmath as mp
    hi = float(m)
    return np.longdouble(hi) + np.longdouble(float(m - mp.mpf(hi)))


def classify(u, v, rect, delta):
    """(truth flag, ambiguous) of WebMercatorRect::contains per point: nw.x <= u && nw.y <= v && u < se.x && v < se.y.
    Ambiguous: u or v within delta of a bound it is tested against."""
    ld = np.longdouble
    nwx, nwy, sex, sey = (ld(float(c)) for c in rect)
    flag = (nwx <= u) & (nwy <= v) & (u < sex) & (v < sey)
    d = ld(delta)
    amb = (np.abs(u - nwx) <= d) | (np.abs(u - sex) <= d) | (np.abs(v - nwy) <= d) | (np.abs(v - sey) <= d)
    return flag, amb


# ---- corners in mpmath ---------------------------------------------------------------------------------------------------
def corners_mp(rect):
    """compute_corners (web_mercator_rect.rs:61-83) at 40 digits: (8, 3) list of mpmath numbers."""
    import mpmath as mp
    with mp.workdps(40):
        a, f = mp.mpf(A), 1 / mp.mpf("298.257223563")
        e2 = f * (2 - f)

        def to_lat_lng(u, v):
            cx, cy = mp.mpf(float(u)) - mp.mpf(0.5), mp.mpf(float(v)) - mp.mpf(0.5)
            sin_term = mp.exp(-cy * 4 * mp.pi)
            sin_y = 1 / ((sin_term + 1) * mp.mpf(-0.5)) + 1
            bound = mp.mpf(0.99627207622075)
            sin_y = min(max(sin_y, -bound), bound)
            lng = min(max(cx * 2 * mp.pi, -mp.pi), mp.pi)
            return mp.asin(sin_y), lng

        def ecef(lat, lng, h):
            n = a / mp.sqrt(1 - e2 * mp.sin(lat) ** 2)
            return [+((n + h) * mp.cos(lat) * mp.cos(lng)), +((n + h) * mp.cos(lat) * mp.sin(lng)), +((n * (1 - e2) + h) * mp.sin(lat))]

        nlat, wlng = to_lat_lng(rect[0], rect[1])
        slat, elng = to_lat_lng(rect[2], rect[3])
        out = []
        for h in (mp.mpf(-500), mp.mpf(10000)):
            out += [ecef(nlat, wlng, h), ecef(nlat, elng, h), ecef(slat, elng, h), ecef(slat, wlng, h)]
        return out


def corners_np(rect):
    """The same formulas in plain numpy / math f64 (the yardstick of the library's tolerance)."""
    def to_lat_lng(u, v):
        cx, cy = u - 0.5, v - 0.5
        sin_term = math.exp(-cy * (4.0 * math.pi))
        sin_y = 1.0 / ((sin_term + 1.0) * -0.5) + 1.0
        sin_y = min(max(sin_y, -0.99627207622075), 0.99627207622075)
        return math.asin(sin_y), min(max(cx * (2.0 * math.pi), -math.pi), math.pi)

    def ecef(lat, lng, h):
        n = A / math.sqrt(1.0 - E2 * math.sin(lat) ** 2)
        return [(n + h) * math.cos(lat) * math.cos(lng), (n + h) * math.cos(lat) * math.sin(lng), (n * (1.0 - E2) + h) * math.sin(lat)]

    nlat, wlng = to_lat_lng(float(rect[0]), float(rect[1]))
    slat, elng = to_lat_lng(float(rect[2]), float(rect[3]))
    out = []
    for h in (-500.0, 10000.0):
        out += [ecef(nlat, wlng, h), ecef(nlat, elng, h), ecef(slat, elng, h), ecef(slat, wlng, h)]
    return np.array(out)


# ---- SAT -----------------------------------------------------------------------------------------------------------------
def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _cross(a, b):
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])


def _normalize(v):
    with np.errstate(all="ignore"):
        return v / np.sqrt(np.float64(_dot(v, v)))


def intersector(corners):
    """(edges (12, 3), face normals (6, 3)) in web_mercator_rect.rs:85-116 order."""
    c = np.asarray(corners, dtype=np.float64)
    e = [_normalize(c[(i + 1) & 3] - c[i]) for i in range(4)]
    e += [_normalize(c[4 + ((i + 1) & 3)] - c[4 + i]) for i in range(4)]
    e += [_normalize(c[4 + i] - c[i]) for i in range(4)]
    n = [_normalize(_cross(e[i], e[8 + i])) for i in range(4)]
    n += [_normalize(_cross(e[1], e[0])), _normalize(_cross(e[5], e[4]))]
    return np.array(e), np.array(n)


def _dedup(axes):
    out = []
    for a in axes:
        dupe = False
        for b in out:
            dm, dp = a - b, a + b
            if min(_dot(dm, dm), _dot(dp, dp)) < 2.220446049250313e-16:
                dupe = True
                break
        if not dupe:
            out.append(a)
    return np.array(out)


def separating_axes(edges_a, normals_a, edges_b, normals_b):
    """cache_separating_axes (sat.rs:111-143): normals of both, then every finite normalised edge cross product, deduplicated."""
    axes = [np.asarray(n, dtype=np.float64) for n in normals_a] + [np.asarray(n, dtype=np.float64) for n in normals_b]
    for ea in edges_a:
        for eb in edges_b:
            c = _normalize(_cross(ea, eb))
            if np.all(np.isfinite(c)):
                axes.append(c)
    return _dedup(axes)


UNIT = np.eye(3)


def axes_for_aabb(corners):
    """cache_separating_axes_for_aabb (sat.rs:111-143) of a rectangle's polyhedron: up to 45 axes."""
    e, n = intersector(corners)
    return separating_axes(e, n, UNIT, UNIT)


def _project(corners, axis):
    p = [_dot(c, axis) for c in np.asarray(corners, dtype=np.float64)]
    return min(p), max(p)


def relation(axes, corners_a, corners_b):
    """sat.rs:174-205: Out if an axis separates, else Cross if b sticks out of a on any axis, else In."""
    rel = REL_IN
    for ax in axes:
        amin, amax = _project(corners_a, ax)
        bmin, bmax = _project(corners_b, ax)
        if bmin > amax or bmax < amin:
            return REL_OUT
        if amin > bmin or bmax > amax:
            rel = REL_CROSS
    return rel


def intersect(corners_a, corners_b):
    """Intersector::intersect of two rectangles' polyhedra (the reference's intersection_test)."""
    ea, na = intersector(corners_a)
    eb, nb = intersector(corners_b)
    return relation(separating_axes(ea, na, eb, nb), corners_a, corners_b)


def relations_for_cubes(corners, cubes):
    """Relation of every cube (rows: min xyz, edge) against the rectangle with these corners, vectorised; the arithmetic is
    `relation`'s (left-to-right dot products, min / max over the cube's 8 corners)."""
    axes = axes_for_aabb(corners)
    cubes = np.asarray(cubes, dtype=np.float64).reshape(-1, 4)
    mn, mx = cubes[:, :3], cubes[:, :3] + cubes[:, 3:4]
    lo, hi = np.minimum(mn, mx), np.maximum(mn, mx)
    out = np.zeros(len(cubes), dtype=np.uint8)
    sep = np.zeros(len(cubes), dtype=bool)
    cross = np.zeros(len(cubes), dtype=bool)
    c = np.asarray(corners, dtype=np.float64)
    for ax in axes:
        pa = (c[:, 0] * ax[0] + c[:, 1] * ax[1]) + c[:, 2] * ax[2]
        amin, amax = pa.min(), pa.max()
        pb = []
        for i in range(8):
            px = (hi if i & 1 else lo)[:, 0] * ax[0]
            py = (hi if i & 2 else lo)[:, 1] * ax[1]
            pz = (hi if i & 4 else lo)[:, 2] * ax[2]
            pb.append((px + py) + pz)
        pb = np.array(pb)
        bmin, bmax = pb.min(axis=0), pb.max(axis=0)
        sep |= (bmin > amax) | (bmax < amin)
        cross |= (amin > bmin) | (bmax > amax)
    out[cross] = REL_CROSS
    out[sep] = REL_OUT
    return out


# ---- rectangles ----------------------------------------------------------------------------------------------------------
def grid(cu, cv, n, side):
    """n x n rectangles of side `side` (normalised units) centred on (cu, cv): list of (nw.x, nw.y, se.x, se.y)."""
    u0, v0 = cu - n * side / 2.0, cv - n * side / 2.0
    return [(u0 + i * side, v0 + j * side, u0 + (i + 1) * side, v0 + (j + 1) * side) for j in range(n) for i in range(n)]
