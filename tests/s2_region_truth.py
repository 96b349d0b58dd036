"""An independent restatement of the S2 region chain of DESIGN §9d in plain Python: a cell from its id, Cell::rect_bound,
CellUnion::normalize / rect_bound / intersects_cellid and Rect::intersects_cell, with math.atan2 / sin / cos / sqrt. It takes
cell ids from s2_truth.py and never calls the library; test_s2_query_cpu.py and test_gpu_s2_query.py compare the library
against it.

Where the library walks one list (normalize) or searches one (intersects_cellid), this file states the property instead:
normalize is a fixed point of "drop what another cell contains, replace four siblings by their parent", intersects_cellid is
"some cell of the union shares a leaf with the id".

The library's transcendentals are not libm's, so a decision within rounding of equality may differ. `decided_lists`
evaluates every (location, cell) pair with the rect as it is, grown by DELTA and shrunk by DELTA; only pairs on which all
three agree are compared ("ties")."""
import functools
import math

import numpy as np

import s2_truth as T

PI = math.pi
TWO_PI = 2.0 * math.pi
EPS = 2.220446049250313e-16
DELTA = 1e-12  # rad: about 6 um on the ground
EMPTY = (1.0, 0.0, PI, -PI)


# ---- cell ids ------------------------------------------------------------------------------------------------------------
def level(cell):
    return T.MAX_LEVEL - ((cell & -cell).bit_length() - 1) // 2


def children(cell):
    lsb = cell & -cell
    return [cell - lsb + (2 * k + 1) * (lsb >> 2) for k in range(4)]


def parent_of(cell):
    return T.parent(cell, level(cell) - 1)


def leaves_overlap(a, b):
    return T.range_min(a) <= T.range_max(b) and T.range_min(b) <= T.range_max(a)


def normalize(cells):
    """CellUnion::normalize as a fixed point; ascending."""
    cur = set(int(c) for c in cells)
    while True:
        kept = {c for c in cur if not any(o != c and T.range_min(o) <= c <= T.range_max(o) for o in cur)}
        merged = set(kept)
        for c in kept:
            if level(c) == 0:
                continue
            p = parent_of(c)
            kids = children(p)
            if all(k in kept for k in kids):
                merged.difference_update(kids)
                merged.add(p)
        if merged == cur:
            return sorted(merged)
        cur = merged


def union_intersects(cells, cell):
    return any(leaves_overlap(int(c), int(cell)) for c in cells)


# ---- projections ---------------------------------------------------------------------------------------------------------
def st_to_uv(s):
    if s >= 0.5:
        return (1.0 / 3.0) * (4.0 * s * s - 1.0)
    return (1.0 / 3.0) * (1.0 - 4.0 * (1.0 - s) * (1.0 - s))


def face_uv_to_xyz(face, u, v):
    return ((1.0, u, v), (-u, 1.0, v), (-u, -v, 1.0), (-1.0, -v, -u), (v, -1.0, -u), (v, u, -1.0))[face]


# the u and v axes of each face: does the axis have a z component
U_HAS_Z = (False, False, False, True, True, False)
V_HAS_Z = (True, True, False, False, False, False)


def lat_of(p):
    return math.atan2(p[2], math.sqrt(p[0] * p[0] + p[1] * p[1]))


def lng_of(p):
    return math.atan2(p[1], p[0])


def unit(p):
    n2 = p[0] * p[0] + p[1] * p[1] + p[2] * p[2]
    if n2 == 0.0:
        return p
    r = 1.0 / math.sqrt(n2)
    return (p[0] * r, p[1] * r, p[2] * r)


def point_of(lat, lng):
    c = math.cos(lat)
    return (math.cos(lng) * c, math.sin(lng) * c, math.sin(lat))


# ---- intervals on the circle: (lo, hi), inverted when lo > hi, empty (pi, -pi), full (-pi, pi) --------------------------------
def s1_is_empty(i):
    return i[0] == PI and i[1] == -PI


def s1_has(i, p):
    if i[0] > i[1]:
        return (p >= i[0] or p <= i[1]) and not s1_is_empty(i)
    return i[0] <= p <= i[1]


def s1_contains(i, p):
    return s1_has(i, PI if p == -PI else p)


def pos_dist(a, b):
    d = b - a
    return d if d >= 0.0 else (b + PI) - (a - PI)


def s1_add(i, p):
    if p == -PI:
        p = PI
    if s1_has(i, p):
        return i
    if s1_is_empty(i):
        return (p, p)
    return (p, i[1]) if pos_dist(p, i[0]) < pos_dist(i[1], p) else (i[0], p)


def s1_pair(a, b):
    a = PI if a == -PI else a
    b = PI if b == -PI else b
    return (a, b) if pos_dist(a, b) <= PI else (b, a)


def s1_covers(i, o):
    if i[0] > i[1]:
        if o[0] > o[1]:
            return o[0] >= i[0] and o[1] <= i[1]
        return (o[0] >= i[0] or o[1] <= i[1]) and not s1_is_empty(i)
    if o[0] > o[1]:
        return i == (-PI, PI) or s1_is_empty(o)
    return o[0] >= i[0] and o[1] <= i[1]


def s1_meets(i, o):
    if s1_is_empty(i) or s1_is_empty(o):
        return False
    if i[0] > i[1]:
        return o[0] > o[1] or o[0] <= i[1] or o[1] >= i[0]
    if o[0] > o[1]:
        return o[0] <= i[1] or o[1] >= i[0]
    return o[0] <= i[1] and o[1] >= i[0]


def s1_union(i, o):
    """The union rule of DESIGN §9d."""
    if s1_is_empty(o):
        return i
    if s1_has(i, o[0]):
        if s1_has(i, o[1]):
            return i if s1_covers(i, o) else (-PI, PI)
        return (i[0], o[1])
    if s1_has(i, o[1]):
        return (o[0], i[1])
    if s1_is_empty(i) or s1_has(o, i[0]):
        return o
    return (o[0], i[1]) if pos_dist(o[1], i[0]) < pos_dist(i[1], o[0]) else (i[0], o[1])


def s1_length(i):
    ln = i[1] - i[0]
    if ln >= 0.0:
        return ln
    ln += TWO_PI
    return ln if ln > 0.0 else -1.0


def s1_center(i):
    c = 0.5 * (i[0] + i[1])
    if not i[0] > i[1]:
        return c
    return c + PI if c <= 0.0 else c - PI


def wrap(x):
    return x - TWO_PI if x > PI else (x + TWO_PI if x < -PI else x)


def s1_grow(i, margin):
    """Interval::expanded for margin >= 0."""
    if s1_is_empty(i):
        return i
    if s1_length(i) + 2.0 * margin + 2.0 * EPS >= TWO_PI:
        return (-PI, PI)
    lo, hi = wrap(i[0] - margin), wrap(i[1] + margin)
    if lo == -PI and hi != PI:
        lo = PI
    if hi == -PI and lo != PI:
        hi = PI
    if lo <= -PI:
        lo = PI
    return (lo, hi)


# ---- a cell --------------------------------------------------------------------------------------------------------------
class Cell:
    __slots__ = ("id", "face", "uv", "rect", "center", "vertices", "vertex_ll")


def rect_bound(face, uv):
    u, v = uv[0] + uv[1], uv[2] + uv[3]
    i = int(u > 0.0) if U_HAS_Z[face] else int(u < 0.0)
    j = int(v > 0.0) if V_HAS_Z[face] else int(v < 0.0)
    us, vs = (uv[0], uv[1]), (uv[2], uv[3])
    la = lat_of(face_uv_to_xyz(face, us[i], vs[j]))
    lb = lat_of(face_uv_to_xyz(face, us[1 - i], vs[1 - j]))
    lat = (min(la, lb), max(la, lb))
    lng = s1_add((PI, -PI), lng_of(face_uv_to_xyz(face, us[i], vs[1 - j])))
    lng = s1_add(lng, lng_of(face_uv_to_xyz(face, us[1 - i], vs[j])))
    margin = 2.0 * EPS
    lat = (max(lat[0] - margin, -0.5 * PI), min(lat[1] + margin, 0.5 * PI))
    lng = s1_grow(lng, margin)
    if lat[0] == -0.5 * PI or lat[1] == 0.5 * PI:
        lng = (-PI, PI)
    return (lat[0], lat[1], lng[0], lng[1])


@functools.lru_cache(maxsize=1 << 17)
def cell(cell_id):
    """Cell::from(id) for level >= 1."""
    cell_id = int(cell_id)
    lv = level(cell_id)
    assert lv >= 1
    face, i, j = T.face_ij(T.range_min(cell_id))
    size = 1 << (T.MAX_LEVEL - lv)
    i, j = i & ~(size - 1), j & ~(size - 1)
    c = Cell()
    c.id, c.face = cell_id, face
    c.uv = (st_to_uv(i / T.MAX_SIZE), st_to_uv((i + size) / T.MAX_SIZE), st_to_uv(j / T.MAX_SIZE), st_to_uv((j + size) / T.MAX_SIZE))
    c.rect = rect_bound(face, c.uv)
    raw = face_uv_to_xyz(face, st_to_uv((2 * i + size) / (2 * T.MAX_SIZE)), st_to_uv((2 * j + size) / (2 * T.MAX_SIZE)))
    c.center = (lat_of(raw), lng_of(raw))
    c.vertices = tuple(unit(face_uv_to_xyz(face, c.uv[a], c.uv[2 + b])) for a, b in ((0, 0), (1, 0), (1, 1), (0, 1)))
    c.vertex_ll = tuple((lat_of(p), lng_of(p)) for p in c.vertices)
    return c


def rect_union(r, o):
    if o[0] > o[1]:
        lat = (r[0], r[1])
    elif r[0] > r[1]:
        lat = (o[0], o[1])
    else:
        lat = (min(r[0], o[0]), max(r[1], o[1]))
    lng = s1_union((r[2], r[3]), (o[2], o[3]))
    return (lat[0], lat[1], lng[0], lng[1])


def union_rect(cells):
    r = EMPTY
    for c in cells:
        r = rect_union(r, cell(c).rect)
    return r


def corners_rect(corners):
    """cells_in_convex_polyhedron's region: leaf cells of the corners, normalized, the union's rect bound."""
    return union_rect(normalize(T.leaf_id(float(p[0]), float(p[1]), float(p[2])) for p in np.asarray(corners).reshape(8, 3)))


# ---- Rect::intersects_cell -------------------------------------------------------------------------------------------------
def rect_has(r, ll):
    return r[0] <= ll[0] <= r[1] and s1_contains((r[2], r[3]), ll[1])


def rects_meet(r, o):
    if r[0] <= o[0]:
        lat = o[0] <= r[1] and o[0] <= o[1]
    else:
        lat = r[0] <= o[1] and r[0] <= r[1]
    return lat and s1_meets((r[2], r[3]), (o[2], o[3]))


def cell_has_point(c, p):
    f = c.face
    major = p[f % 3]
    if (f < 3 and not major > 0.0) or (f >= 3 and not major < 0.0):
        return False
    num = ((p[1], p[2]), (-p[0], p[2]), (-p[0], -p[1]), (p[2], p[1]), (p[2], -p[0]), (-p[1], -p[0]))[f]
    u, v = num[0] / major, num[1] / major
    return c.uv[0] - EPS <= u <= c.uv[1] + EPS and c.uv[2] - EPS <= v <= c.uv[3] + EPS


def cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def edges_cross(a, b, c, d):
    ab = cross(a, b)
    acb, bda = -dot(ab, c), dot(ab, d)
    if not acb * bda > 0.0:
        return False
    cd = cross(c, d)
    cbd, dac = -dot(cd, b), dot(cd, a)
    return acb * cbd > 0.0 and acb * dac > 0.0


def meridian_meets_edge(a, b, lat_lo, lat_hi, lng):
    return edges_cross(a, b, point_of(lat_lo, lng), point_of(lat_hi, lng))


def parallel_meets_edge(a, b, lat, lng):
    z = unit(cross((a[0] + b[0], a[1] + b[1], a[2] + b[2]), (b[0] - a[0], b[1] - a[1], b[2] - a[2])))
    if z[2] < 0.0:
        z = (-z[0], -z[1], -z[2])
    y = unit((z[1], -z[0], 0.0))
    x = cross(y, z)
    sin_lat = math.sin(lat)
    if not abs(sin_lat) < x[2]:
        return False
    cos_t = sin_lat / x[2]
    sin_t = math.sqrt(1.0 - cos_t * cos_t)
    theta = math.atan2(sin_t, cos_t)
    span = s1_pair(math.atan2(dot(a, y), dot(a, x)), math.atan2(dot(b, y), dot(b, x)))
    for sign, t in ((1.0, theta), (-1.0, -theta)):
        if s1_contains(span, t):
            ix = x[0] * cos_t + sign * (y[0] * sin_t)
            iy = x[1] * cos_t + sign * (y[1] * sin_t)
            if s1_contains(lng, math.atan2(iy, ix)):
                return True
    return False


def intersects_cell(r, c):
    """Rect::intersects_cell in the order of DESIGN §9d."""
    if r[0] > r[1]:
        return False
    if rect_has(r, c.center):
        return True
    lng = (r[2], r[3])
    if cell_has_point(c, point_of(0.5 * (r[0] + r[1]), s1_center(lng))):
        return True
    if not rects_meet(r, c.rect):
        return False
    if any(rect_has(r, ll) for ll in c.vertex_ll):
        return True
    for k in range(4):
        n = (k + 1) & 3
        span = s1_pair(c.vertex_ll[k][1], c.vertex_ll[n][1])
        if not s1_meets(lng, span):
            continue
        a, b = c.vertices[k], c.vertices[n]
        if s1_contains(span, r[2]) and meridian_meets_edge(a, b, r[0], r[1], r[2]):
            return True
        if s1_contains(span, r[3]) and meridian_meets_edge(a, b, r[0], r[1], r[3]):
            return True
        if parallel_meets_edge(a, b, r[0], lng) or parallel_meets_edge(a, b, r[1], lng):
            return True
    return False


# ---- ties ------------------------------------------------------------------------------------------------------------------
def grown(r, d=DELTA):
    if r[0] > r[1]:
        return r
    lng = s1_grow((r[2], r[3]), d)
    return (r[0] - d, r[1] + d, lng[0], lng[1])


def shrunk(r, d=DELTA):
    if r[0] > r[1] or r[1] - r[0] < 2.0 * d:
        return EMPTY
    lng = (r[2], r[3])
    if lng != (-PI, PI):
        if s1_length(lng) < 2.0 * d:
            return EMPTY
        lng = (wrap(r[2] + d), wrap(r[3] - d))
    return (r[0] + d, r[1] - d, lng[0], lng[1])


def _np_meet(r, bounds):
    """rects_meet of one rect against an (n, 4) array of cell bounds (exact comparisons only)."""
    if r[0] > r[1]:
        return np.zeros(len(bounds), dtype=bool)
    lo, hi, a, b = bounds[:, 0], bounds[:, 1], bounds[:, 2], bounds[:, 3]
    lat = np.where(r[0] <= lo, (lo <= r[1]) & (lo <= hi), (r[0] <= hi))
    o_inv, o_empty = a > b, (a == PI) & (b == -PI)
    if r[2] > r[3]:
        lng = o_inv | (a <= r[3]) | (b >= r[2])
    else:
        lng = np.where(o_inv, (a <= r[3]) | (b >= r[2]), (a <= r[3]) & (b >= r[2]))
    if s1_is_empty((r[2], r[3])):
        lng = np.zeros(len(bounds), dtype=bool)
    return lat & lng & ~o_empty


def cell_bounds(cell_ids):
    return np.array([cell(int(c)).rect for c in cell_ids]).reshape(-1, 4)


def decided_lists(cell_ids, rect, delta=DELTA, bounds=None):
    """For one rect over a cloud's cells: (yes, undecided, tested) — the indices of the cells that intersect under all three of
    rect / grown / shrunk, the indices on which the three disagree, and the number of pairs that the bound rejection let
    through. Every other cell does not intersect under all three."""
    bounds = cell_bounds(cell_ids) if bounds is None else bounds
    variants = (rect, grown(rect, delta), shrunk(rect, delta))
    near = np.zeros(len(bounds), dtype=bool)
    for v in variants:
        near |= _np_meet(v, bounds)
    # steps 2 and 3 come before the rejection; a cell whose bound a rect misses by more than rounding passes neither
    yes, undecided = [], []
    for k in np.nonzero(near)[0]:
        c = cell(int(cell_ids[k]))
        votes = [intersects_cell(v, c) for v in variants]
        if all(votes):
            yes.append(int(k))
        elif any(votes):
            undecided.append(int(k))
    return yes, undecided, int(_np_meet(rect, bounds).sum())


# ---- inputs shared by the CPU and the GPU tests --------------------------------------------------------------------------
def quat_rotate(q, v):
    """Unit quaternion (i, j, k, w) times a vector."""
    u = np.asarray(q[:3], dtype=np.float64)
    v = np.asarray(v, dtype=np.float64)
    return v + 2.0 * np.cross(u, np.cross(u, v) + q[3] * v)


def aabb_corners(lo, hi):
    return np.array([[(lo, hi)[a][0], (lo, hi)[b][1], (lo, hi)[c][2]] for a in (0, 1) for b in (0, 1) for c in (0, 1)], dtype=np.float64)


def obb_corners(translation, quat, half):
    return np.array([np.asarray(translation) + quat_rotate(quat, [sx * half[0], sy * half[1], sz * half[2]])
                     for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)])


def frustum_corners(query_from_clip):
    """The clip cube's corners through query_from_clip (16 doubles, column-major), after the perspective division."""
    m = np.asarray(query_from_clip, dtype=np.float64).reshape(4, 4).T
    out = []
    for x in (-1.0, 1.0):
        for y in (-1.0, 1.0):
            for z in (-1.0, 1.0):
                p = m @ np.array([x, y, z, 1.0])
                out.append(p[:3] / p[3])
    return np.array(out)


def spec_corners(spec):
    """The (8, 3) corners of a Context.shapes entry, on the CPU (the device computes its own: Shapes.get)."""
    import point_cloud_viewer_amd as pcv
    kind = spec[0]
    if kind == "aabb":
        return aabb_corners(np.asarray(spec[1], dtype=np.float64), np.asarray(spec[2], dtype=np.float64))
    if kind == "obb":
        return obb_corners(spec[1], spec[2], spec[3])
    if kind == "frustum2":
        return frustum_corners(spec[2])
    if kind == "web_mercator_rect":
        return pcv.wmr_corners(spec)
    return np.zeros((8, 3))


KINDS = {"all": 0, "aabb": 1, "frustum": 2, "obb": 3, "frustum2": 4, "web_mercator_rect": 5}


@functools.lru_cache(maxsize=None)
def scene():
    """The 20 000-point uniform ECEF cloud (200 m x 200 m x 20 m) and about 40 locations of every kind over it:
    (x, y, z, rgb, bmin, bmax, specs) — specs are Context.shapes entries; a ("frustum", zeros) stands for the frustum whose
    matrix has no inverse."""
    import oracle_lib as O
    import point_cloud_viewer_amd as pcv
    from point_cloud_viewer_amd import synthetic
    x, y, z, rgb, bmin, bmax = synthetic.uniform_ecef(20000)
    rot, centre = synthetic.ecef_from_local(37.407204, -122.147604)
    rng = np.random.Generator(np.random.PCG64(2024))
    diag = bmax - bmin
    specs = [("all",), ("aabb", bmin - 1.0, bmax + 1.0), ("aabb", bmin + 0.2 * diag, bmin + 0.8 * diag)]
    for a in range(4):  # tiles
        for b in range(4):
            lo = bmin + diag * np.array([a / 4.0, b / 4.0, 0.0])
            specs.append(("aabb", lo, lo + diag * np.array([0.25, 0.25, 1.0])))
    def unit_quat():
        q = rng.standard_normal(4)
        return list(q / np.linalg.norm(q))
    for _ in range(8):  # random OBBs inside and across the cloud's edge
        t = centre + rot @ (rng.uniform(-1.0, 1.0, 3) * np.array([110.0, 110.0, 10.0]))
        specs.append(("obb", t, unit_quat(), rng.uniform(0.5, 40.0, 3)))
    specs.append(("obb", centre, [0.0, 0.0, 0.0, 1.0], [50.0, 50.0, 5.0]))
    for far in (10.0, 100.0):  # frusta that look out from inside the cloud
        for _ in range(2):
            eye = centre + rot @ (rng.uniform(-1.0, 1.0, 3) * np.array([60.0, 60.0, 5.0]))
            c, q = O.frustum_new(list(eye), unit_quat(), O.perspective3_new(1.0, 1.2, 0.1, far))
            specs.append(("frustum2", c, q))
    specs.append(("frustum", np.zeros(16)))
    # zoom-21 map tiles around the centre: the reference's rectangle (queries.rs:59-68) and its neighbours
    lat, lng = math.radians(37.407204), math.radians(-122.147604)
    u, v = pcv.wmr_from_lat_lng([lat], [lng])
    px, py = float(u[0]) * 256.0 * 2.0 ** 21, float(v[0]) * 256.0 * 2.0 ** 21
    for dx, dy in ((0, 0), (-256, 0), (256, 0), (0, -256), (0, 256), (512, 512), (-4096, 0)):
        specs.append(pcv.web_mercator_rect_from_zoomed([px + dx - 128.0, py + dy - 128.0], [px + dx + 128.0, py + dy + 128.0], 21))
    assert all(s is not None for s in specs)
    return x, y, z, rgb, bmin, bmax, tuple(specs)


def scene_unions(level_):
    """Cell unions over the scene's cloud: the reference's [cell, cell.next()] at the cloud's centre (queries.rs:49-53), a
    coarser cell, finer cells, a far-away cell and the empty union; each ascending."""
    from point_cloud_viewer_amd import synthetic
    _, centre = synthetic.ecef_from_local(37.407204, -122.147604)
    leaf = T.leaf_id(*[float(v) for v in centre])
    c = T.parent(leaf, level_)
    nxt = c + ((c & -c) << 1)
    far = T.parent(T.leaf_id(0.0, 0.0, 6.371e6), 12)
    return [sorted([c, nxt]), [T.parent(leaf, max(1, level_ - 3))], sorted(children(c)[1:3]) if level_ < 30 else [c], [far], [],
            sorted([T.parent(leaf, min(30, level_ + 4)), far])]
