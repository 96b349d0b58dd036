"""Truths and planted inputs for `contains` of oriented boxes (obb.rs:83-90) and frusta (frustum.rs:120-125), and for the
node relation of those two kinds. Pure python: numpy, `fractions`, `mpmath`. Imports neither the oracle nor the library; where
a construction needs the reference's `Frustum::new` matrix, the caller hands the function in (`frustum_new`): the matrix is an
input there, never a verdict.

Four things:

* exact rules — `obb_contains_exact`, `frustum_contains_exact`: the reference's formulas in `Fraction`s on the f64 inputs taken
  as exact rationals; `obb_exact`, `frustum_exact`: the same rules over arrays in scaled python integers, with the exact margin
  to the nearest face. A non-finite input has no rational: there the rules evaluate the same formula in IEEE arithmetic (python
  floats, nothing fused, min / max ignoring a NaN as f64::min / f64::max do) — on the exact scenes every finite intermediate is
  exact anyway;
* exact scenes — `obb_exact_scene`, `frustum_exact_scene`: inputs on which the f64 chain rounds nowhere (quaternions with
  components in {0, +-1/2, +-1}, everything else a small multiple of 1/4; a perspective matrix with dyadic entries), so the flags
  of any correct f64 evaluation equal the exact rule with no exception; `exact_pair` for positions that are not dyadic (the
  four rotations that are exact on any double, one IEEE addition);
* planted points — `plant_on_box`, `plant_on_frustum`, `with_neighbours`: positions on the six faces of a general shape, mapped
  at 200 bits and rounded to f64, and their neighbours 1-3 `nextafter` steps away along each axis;
* planted shapes — `boxes_through`, `frusta_through`: the reverse, for things that cannot be moved (node cube corners, stored
  points): the box centre / the frustum eye is moved, at 200 bits, so that a face passes through the target; plus that centre's /
  eye's neighbours 1-2 steps away per axis.

Forward error bounds of the f64 chains (used to leave out the bulk points no evaluation order is bound to decide alike), with
u = 2^-53 and gamma_k = k u / (1 - k u):

* oriented box: `b = (t w + qv x t) + v + t'`, `t = 2 (qv x v)`, `t' = -(q^-1 c)` computed by the same chain. The longest path
  from an input to `b_a` is mul, sub, mul, sub, add, add, add = 7 roundings (the scaling by 2 is exact); the absolute values of
  the expanded terms sum to at most 13 |v|_inf for |q components| <= 1 (|v| + 4 |v| + 8 |v|), and the same for c. So
  `|fl(b_a) - b_a| <= gamma_7 * 13 * (|p|_inf + |c|_inf)` — 8.7e-8 m at ECEF magnitudes, 1.3e-12 m in a 64 m scene;
* frustum: `r_i = ((m_i0 x + m_i1 y) + m_i2 z) + m_i3` and `w` alike: 4 roundings deep, then one division. With
  `A_i = sum |m_ij| |p_j| + |m_i3|`: `|fl(r_i) - r_i| <= gamma_4 A_i`; the comparison of `r_i / w` with +-1 is decided like
  `|r_i|` against `|w|`, so a point counts as decided when `||r_i| - |w|| > gamma_5 (A_i + A_w)` for the three i and
  `|w| > gamma_5 A_w`.
"""
import math
from fractions import Fraction

import numpy as np
from mpmath import mp, mpf

BITS = 200
U = 2.0 ** -53


def gamma(k):
    return k * U / (1.0 - k * U)


# a 64 m scene at the origin, and one on the ellipsoid (radius 6 372 km: a valid ECEF point, so that S2 clouds take it too)
SCALES = {"local": np.zeros(3), "ecef": np.array([-2.7e6, -4.3e6, 3.85e6])}

# ---- the quaternions (i, j, k, w) whose rotation chain is exact -------------------------------------------------------------
# components in {0, +-1/2, +-1}: products with multiples of 1/4 stay short dyadic numbers
EXACT_QUATS = [(1.0, 0.0, 0.0, 0.0), (0.0, 1.0, 0.0, 0.0), (0.0, 0.0, 1.0, 0.0), (0.0, 0.0, 0.0, 1.0)] + \
              [(a, b, c, d) for a in (0.5, -0.5) for b in (0.5, -0.5) for c in (0.5, -0.5) for d in (0.5, -0.5)]
# exact on ANY double: identity and the half turns about x, y, z (every product is 0 * v or 1 * v, every sum has a zero term or
# is -2 v + v); the signs s_a with R p = (s_x p_x, s_y p_y, s_z p_z)
EXACT_ROTATIONS = [((0.0, 0.0, 0.0, 1.0), (1.0, 1.0, 1.0)), ((1.0, 0.0, 0.0, 0.0), (1.0, -1.0, -1.0)),
                   ((0.0, 1.0, 0.0, 0.0), (-1.0, 1.0, -1.0)), ((0.0, 0.0, 1.0, 0.0), (-1.0, -1.0, 1.0))]


# ---- exact rules, one point ------------------------------------------------------------------------------------------------
def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _rotate(q, v):
    """UnitQuaternion * Vector3 as nalgebra writes it: t = 2 (qv x v); v + w t + qv x t. Any number type."""
    qv = (q[0], q[1], q[2])
    t = tuple(2 * c for c in _cross(qv, v))
    c = _cross(qv, t)
    return tuple(v[a] + q[3] * t[a] + c[a] for a in range(3))


def _nanmin(a, b):
    return b if a != a else (a if b != b else min(a, b))


def _nanmax(a, b):
    return b if a != a else (a if b != b else max(a, b))


def _finite(*vals):
    return all(math.isfinite(float(v)) for v in vals)


def obb_contains_exact(centre, quat, half, p):
    """Obb::contains: obb_from_query = (conjugate quaternion, -(q^-1 c)); |q_a| <= half_a, closed on both sides."""
    if any(float(h) != float(h) for h in half):
        return False  # a NaN half extent: no comparison holds
    if _finite(*centre, *quat, *half, *p):
        N = Fraction
    else:
        N = float  # see the module docstring
    with np.errstate(all="ignore"):
        q = tuple(N(float(v)) for v in quat)
        inv = (-q[0], -q[1], -q[2], q[3])
        t = tuple(-c for c in _rotate(inv, tuple(N(float(v)) for v in centre)))
        b = _rotate(inv, tuple(N(float(v)) for v in p))
        return all(abs(b[a] + t[a]) <= N(float(half[a])) for a in range(3))


def frustum_contains_exact(m, p):
    """Frustum::contains: column-major clip_from_query, divided by w unless w == 0; min > -1 and max < 1."""
    m = [float(v) for v in np.asarray(m, dtype=np.float64).ravel()]
    N = Fraction if _finite(*m, *p) else float
    v = [N(float(c)) for c in p]
    row = lambda i: N(m[i]) * v[0] + N(m[4 + i]) * v[1] + N(m[8 + i]) * v[2] + N(m[12 + i])
    r, w = [row(0), row(1), row(2)], row(3)
    if w != 0:
        r = [c / w for c in r]
    mn, mx = _nanmin(_nanmin(r[0], r[1]), r[2]), _nanmax(_nanmax(r[0], r[1]), r[2])
    return bool(mn > -1 and mx < 1)


# ---- exact rules over arrays: scaled integers ------------------------------------------------------------------------------
def _scale_exp(*arrays):
    e = 0
    for a in arrays:
        a = np.asarray(a, dtype=np.float64).ravel()
        a = a[a != 0]
        if a.size:
            e = max(e, 53 - int(np.frexp(a)[1].min()))
    return e


def _ints(a, E):
    """a * 2^E as an object array of python ints (exact: E comes from _scale_exp over a)."""
    a = np.asarray(a, dtype=np.float64)
    if not np.all(np.isfinite(a)):
        raise ValueError("no rational for a non-finite value")
    m, ex = np.frexp(a)
    mi = (m * 2.0 ** 53).astype(np.int64).ravel().tolist()
    sh = (ex.astype(np.int64) - 53 + E).ravel().tolist()
    out = np.empty(len(mi), dtype=object)
    for k, (v, s) in enumerate(zip(mi, sh)):
        if v == 0:
            out[k] = 0
        else:
            assert s >= 0
            out[k] = v << s
    return out.reshape(a.shape)


def _to_float(num, den):
    return np.array([float(Fraction(int(v), den)) for v in num], dtype=np.float64)


def obb_exact(centre, quat, half, x, y, z):
    """The exact rule over arrays -> (inside, on_face, margin): on_face = on the box's surface (the smallest of
    half_a - |b_a| is 0), margin = the exact distance min_a |half_a - |b_a|| (metres, rounded to f64 once). The rotation chain
    is linear in v, so b = L(p - c)."""
    x, y, z = (np.asarray(v, dtype=np.float64) for v in (x, y, z))
    if any(float(h) != float(h) for h in half):
        return np.zeros(x.size, bool), np.zeros(x.size, bool), np.full(x.size, np.nan)
    Ep, Eq = _scale_exp(x, y, z, centre, half), _scale_exp(quat)
    P = [_ints(v, Ep) for v in (x, y, z)]
    Cn, H, Q = _ints(centre, Ep), _ints(half, Ep), _ints(quat, Eq)
    D = [P[a] - Cn[a] for a in range(3)]
    u, w = (-Q[0], -Q[1], -Q[2]), Q[3]
    ud = _cross(u, D)
    uud = _cross(u, ud)
    s2 = 1 << (2 * Eq)
    B = [D[a] * s2 + 2 * w * ud[a] + 2 * uud[a] for a in range(3)]
    gaps = [H[a] * s2 - abs(B[a]) for a in range(3)]
    inside = np.array([(g0 >= 0 and g1 >= 0 and g2 >= 0) for g0, g1, g2 in zip(*gaps)], dtype=bool)
    on_face = np.array([(min(g0, g1, g2) == 0) for g0, g1, g2 in zip(*gaps)], dtype=bool)
    margin = _to_float([min(abs(g0), abs(g1), abs(g2)) for g0, g1, g2 in zip(*gaps)], 1 << (Ep + 2 * Eq))
    return inside, on_face, margin


def frustum_exact(m, x, y, z):
    """The exact rule over arrays -> (inside, on_plane, gap, w): |r_i| < s with s = |w|, or 1 where w == 0 (no division);
    on_plane = on the frustum's surface (the smallest of s - |r_i| is 0); gap[:, i] = ||r_i| - s| and w, exact values rounded to f64 once."""
    m = np.asarray(m, dtype=np.float64).ravel()
    x, y, z = (np.asarray(v, dtype=np.float64) for v in (x, y, z))
    Ep, Em = _scale_exp(x, y, z), _scale_exp(m)
    P = [_ints(v, Ep) for v in (x, y, z)]
    M = _ints(m, Em)
    one_p, one = 1 << Ep, 1 << (Ep + Em)
    row = lambda i: M[i] * P[0] + M[4 + i] * P[1] + M[8 + i] * P[2] + M[12 + i] * one_p
    R, W = [row(0), row(1), row(2)], row(3)
    S = np.array([abs(v) if v != 0 else one for v in W], dtype=object)
    gaps = [S - abs(R[i]) for i in range(3)]
    inside = np.array([(g0 > 0 and g1 > 0 and g2 > 0) for g0, g1, g2 in zip(*gaps)], dtype=bool)
    on_plane = np.array([(min(g0, g1, g2) == 0) for g0, g1, g2 in zip(*gaps)], dtype=bool)
    gap = np.stack([_to_float([abs(g) for g in gaps[i]], one) for i in range(3)], axis=1)
    return inside, on_plane, gap, _to_float(W, one)


def obb_error_bound(centre, x, y, z):
    """gamma_7 * 13 * (|p|_inf + |c|_inf) per point (module docstring)."""
    pmax = np.maximum(np.maximum(np.abs(x), np.abs(y)), np.abs(z))
    return gamma(7) * 13.0 * (pmax + float(np.max(np.abs(centre)))) * (1.0 + 1e-9)


def frustum_decided(m, x, y, z, gap, w):
    """Per point: does the exact margin exceed the chain's forward error bound (module docstring)?"""
    m = np.abs(np.asarray(m, dtype=np.float64).ravel())
    A = [m[i] * np.abs(x) + m[4 + i] * np.abs(y) + m[8 + i] * np.abs(z) + m[12 + i] for i in range(4)]
    g = gamma(5) * (1.0 + 1e-9)
    ok = np.abs(w) > g * A[3]
    for i in range(3):
        ok &= gap[:, i] > g * (A[i] + A[3])
    return ok


# ---- exact scenes ----------------------------------------------------------------------------------------------------------
def non_finite_points():
    """NaN, +inf and -inf in each axis, the other two coordinates small multiples of 1/4."""
    pts = []
    for bad in (math.nan, math.inf, -math.inf):
        for a in range(3):
            p = [0.25, -0.5, 0.75]
            p[a] = bad
            pts.append(p)
    return np.array(pts)


def _truth(rule, shapes, x, y, z):
    return [np.array([rule(*sh, (x[k], y[k], z[k])) for k in range(x.size)], dtype=bool) for sh in shapes]


def obb_exact_scene():
    """20 exact quaternions at centre (0.25, -0.5, 0.75), half extents (1, 0.5, 1.25), then a zero, a negative and a NaN half
    extent; a 17^3 grid of multiples of 1/4 and the non-finite points. -> dict(shapes, x, y, z, finite (count of grid points),
    want (flags per shape, exact rule), on_face (kept-on-a-face counts per shape))."""
    centre, half = (0.25, -0.5, 0.75), (1.0, 0.5, 1.25)
    shapes = [(centre, q, half) for q in EXACT_QUATS]
    shapes += [(centre, EXACT_QUATS[5], (1.0, 0.0, 1.25)), (centre, EXACT_QUATS[9], (1.0, -0.5, 1.25)),
               (centre, EXACT_QUATS[14], (1.0, 0.5, math.nan))]
    g = np.arange(-8, 9) * 0.25
    gx, gy, gz = (v.ravel() for v in np.meshgrid(g, g, g, indexing="ij"))
    nf = non_finite_points()
    x, y, z = np.concatenate([gx, nf[:, 0]]), np.concatenate([gy, nf[:, 1]]), np.concatenate([gz, nf[:, 2]])
    want, on_face = [], []
    for sh in shapes:
        inside, face, _ = obb_exact(*sh, gx, gy, gz)
        tail = np.array([obb_contains_exact(*sh, p) for p in nf], dtype=bool)
        want.append(np.concatenate([inside, tail]))
        on_face.append(int((inside & face).sum()))
    for a in (x, y, z, *want):
        a.setflags(write=False)
    return dict(shapes=shapes, x=x, y=y, z=z, finite=gx.size, want=want, on_face=on_face)


def perspective_exact():
    """Perspective::new(-1, 1, -0.5, 0.5, 1, 3) (frustum.rs:16-45), column-major: every entry dyadic."""
    m = np.zeros(16)
    m[0], m[5], m[10], m[14], m[11] = 1.0, 2.0, -2.0, -3.0, -1.0
    return m


def _rotation_matrix4(signs):
    m = np.zeros(16)
    m[0], m[5], m[10], m[15] = signs[0], signs[1], signs[2], 1.0
    return m


def _mat4_mul(a, b):
    a, b = np.asarray(a).reshape(4, 4).T, np.asarray(b).reshape(4, 4).T
    return (a @ b).T.ravel().copy()


def frustum_exact_scene():
    """The dyadic perspective matrix, the same pre-multiplied by the four exact rotations, a matrix whose bottom row is zero;
    a 1/4-grid over x in [-4, 4], y in [-2, 2], z in [-4, 1] (the eye plane w == 0 and points behind the eye included) and the
    non-finite points. -> dict(shapes (matrices), x, y, z, finite, want, on_plane, kept)."""
    p = perspective_exact()
    shapes = [p] + [_mat4_mul(_rotation_matrix4(s), p) for _, s in EXACT_ROTATIONS]
    shapes += [_mat4_mul(p, _rotation_matrix4(s)) for _, s in EXACT_ROTATIONS[1:]]  # ... and the rotated query space
    flat = p.copy()
    flat[3::4] = 0.0
    shapes.append(flat)
    gx, gy, gz = (v.ravel() for v in np.meshgrid(np.arange(-16, 17) * 0.25, np.arange(-8, 9) * 0.25, np.arange(-16, 5) * 0.25,
                                                 indexing="ij"))
    nf = non_finite_points()
    x, y, z = np.concatenate([gx, nf[:, 0]]), np.concatenate([gy, nf[:, 1]]), np.concatenate([gz, nf[:, 2]])
    want, on_plane, kept = [], [], []
    for m in shapes:
        inside, plane, _, _ = frustum_exact(m, gx, gy, gz)
        tail = np.array([frustum_contains_exact(m, q) for q in nf], dtype=bool)
        want.append(np.concatenate([inside, tail]))
        on_plane.append(int(plane.sum()))
        kept.append(int(inside.sum()))
    for a in (x, y, z, *want):
        a.setflags(write=False)
    return dict(shapes=shapes, x=x, y=y, z=z, finite=gx.size, want=want, on_plane=on_plane, kept=kept)


def exact_pair(p, rotation, axis, reach=8.0):
    """For a position p that is no dyadic number (a decoded stored point): a box under one of EXACT_ROTATIONS whose face along
    `axis` is closed exactly on p, and the same box with that half extent one `nextafter` lower. b_a = fl(s_a p_a + t_a) is one
    IEEE addition, half_a := |b_a|. -> (closed shape, open shape, exact) with exact = the addition rounded nothing, i.e. the
    exact rule and the f64 chain agree (the caller asserts it)."""
    quat, s = EXACT_ROTATIONS[rotation]
    p = [float(v) for v in p]
    centre = [p[a] - (0.375 * reach + 0.03125 * a) for a in range(3)]  # one rounding here; the centre is an input
    t = [-(s[a] * centre[a]) for a in range(3)]  # obb_from_query's translation: R^-1 (-c), exact for these rotations
    b = [s[a] * p[a] + t[a] for a in range(3)]
    half = [reach, reach, reach]
    half[axis] = abs(b[axis])
    lower = list(half)
    lower[axis] = float(np.nextafter(half[axis], -math.inf))
    exact = Fraction(s[axis]) * Fraction(p[axis]) + Fraction(t[axis]) == Fraction(b[axis])
    return (centre, list(quat), half), (centre, list(quat), lower), exact


# ---- general shapes (parameters only) --------------------------------------------------------------------------------------
def unit_quat(rng):
    q = rng.normal(size=4)
    return q / math.sqrt(float(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]))


def general_boxes(scale, n, seed):
    """n oriented boxes inside a 64 m scene at SCALES[scale]: [(centre, quat, half)]."""
    rng = np.random.default_rng(seed)
    return [(SCALES[scale] + rng.uniform(16.0, 48.0, 3), unit_quat(rng), rng.uniform(2.0, 12.0, 3)) for _ in range(n)]


def general_frusta(scale, n, seed):
    """n frusta looking into that scene: [(eye, quat, (aspect, fovy, near, far))], for Perspective3 + Frustum::new."""
    rng = np.random.default_rng(seed)
    return [(SCALES[scale] + rng.uniform(8.0, 56.0, 3), unit_quat(rng),
             (float(rng.choice([0.75, 1.0, 1.7777])), float(rng.uniform(0.4, 1.6)), float(rng.uniform(0.5, 2.0)), float(rng.uniform(20.0, 60.0))))
            for _ in range(n)]


# ---- 200-bit maps ----------------------------------------------------------------------------------------------------------
def _mpv(v):
    return [mpf(float(c)) for c in v]


def _box_map(quat):
    """The 3 x 3 matrix of v -> L(v), the rotation chain of the CONJUGATE quaternion (what contains applies), and its inverse."""
    inv = _mpv((-quat[0], -quat[1], -quat[2], quat[3]))
    cols = [_rotate(inv, tuple(mpf(1 if a == k else 0) for a in range(3))) for k in range(3)]
    L = mp.matrix(3, 3)
    for k in range(3):
        for a in range(3):
            L[a, k] = cols[k][a]
    return L, mp.inverse(L)


def plant_on_box(centre, quat, half, rng, per_face):
    """per_face positions on each of the six faces: box-frame points with b_a = +-half_a, the others uniform inside, mapped to
    the world (c + L^-1 b) at 200 bits and rounded to f64 -> ((6 * per_face, 3) positions, face index 0..5 per position)."""
    out, face = [], []
    with mp.workprec(BITS):
        _, Linv = _box_map(quat)
        c = _mpv(centre)
        for f in range(6):
            a, sign = f // 2, (1.0 if f % 2 else -1.0)
            for _ in range(per_face):
                b = [mpf(float(half[k])) * mpf(float(rng.uniform(-0.95, 0.95))) for k in range(3)]
                b[a] = mpf(float(half[a])) * sign
                wv = Linv * mp.matrix(b)
                out.append([float(wv[k] + c[k]) for k in range(3)])
                face.append(f)
    return np.array(out), np.array(face)


def plant_on_frustum(m, rng, per_face):
    """per_face positions on each of the six clip planes: clip-space points with one coordinate +-1, the others uniform
    inside, through the 200-bit inverse of the f64 clip matrix -> (positions, face index per position)."""
    out, face = [], []
    with mp.workprec(BITS):
        M = mp.matrix(4, 4)
        mm = np.asarray(m, dtype=np.float64).ravel()
        for r in range(4):
            for c in range(4):
                M[r, c] = mpf(float(mm[4 * c + r]))
        Minv = mp.inverse(M)
        for f in range(6):
            a, sign = f // 2, (1 if f % 2 else -1)
            for _ in range(per_face):
                cl = [mpf(float(rng.uniform(-0.9, 0.9))) for _ in range(3)] + [mpf(1)]
                cl[a] = mpf(sign)
                h = Minv * mp.matrix(cl)
                out.append([float(h[k] / h[3]) for k in range(3)])
                face.append(f)
    return np.array(out), np.array(face)


def neighbour_offsets(steps):
    """(axis, signed step count) of a position's neighbours: 1..steps `nextafter` steps both ways along each axis."""
    return [(a, k * d) for a in range(3) for k in range(1, steps + 1) for d in (1, -1)]


def step(v, k):
    """v moved k `nextafter` steps (k may be negative)."""
    v = np.array(v, dtype=np.float64)
    for _ in range(abs(k)):
        v = np.nextafter(v, math.inf if k > 0 else -math.inf)
    return v


def with_neighbours(pos, face=None, steps=3):
    """Every position followed by its neighbours -> ((n * (1 + 6 steps), 3), face repeated likewise)."""
    pos = np.asarray(pos, dtype=np.float64)
    blocks = [pos]
    for a, k in neighbour_offsets(steps):
        q = pos.copy()
        q[:, a] = step(q[:, a], k)
        blocks.append(q)
    out = np.stack(blocks, axis=1).reshape(-1, 3)
    return (out, np.repeat(face, len(blocks))) if face is not None else out


# ---- planted shapes --------------------------------------------------------------------------------------------------------
def _family(v, steps=2):
    """v and its neighbours 1..steps steps away per axis: (1 + 6 steps, 3)."""
    return with_neighbours(np.asarray(v, dtype=np.float64).reshape(1, 3), steps=steps)


def obb_contains_f64(centre, quat, half, p):
    """Obb::contains in python floats, operation for operation as the reference evaluates it (nothing fused):
    cross = a.y b.z - a.z b.y ...; rotate = ((t w) + qv x t) + v with t = 2 (qv x v); obb_from_query = (conjugate, rotate(-c))."""
    def rotate(q, v):
        t = [2.0 * c for c in _cross(q[:3], v)]
        c = _cross(q[:3], t)
        return [(t[a] * q[3] + c[a]) + v[a] for a in range(3)]
    q = [float(v) for v in quat]
    inv = [-q[0], -q[1], -q[2], q[3]]
    t = rotate(inv, [-float(c) for c in centre])
    b = rotate(inv, [float(v) for v in p])
    return all(abs(b[a] + t[a]) <= float(half[a]) for a in range(3))


def frustum_contains_f64(m, p):
    """Frustum::contains in python floats: r_i = ((m_i0 x + m_i1 y) + m_i2 z) + m_i3, divided by w unless w == 0."""
    m = [float(v) for v in np.asarray(m, dtype=np.float64).ravel()]
    x, y, z = (float(v) for v in p)
    row = lambda i: ((m[i] * x + m[4 + i] * y) + m[8 + i] * z) + m[12 + i]
    r, w = [row(0), row(1), row(2)], row(3)
    if w != 0.0:
        r = [c / w for c in r]
    return min(r) > -1.0 and max(r) < 1.0


def _walk_to_flip(v, axis, flag_of, reach=1 << 16):
    """v moved along `axis` by whole `nextafter` steps to a position whose flag differs from that of its neighbour one step
    back towards v: the f64 chain's own error puts the 200-bit position a few steps from where the chain's verdict changes
    (a far plane, whose clip depth hardly moves with the eye, some hundreds). Doubling strides both ways, then bisection."""
    def at(k):
        w = np.array(v, dtype=np.float64)
        w[axis] = step(w[axis], k)
        return w
    first, n, hit = flag_of(at(0)), 1, None
    while hit is None and n <= reach:
        hit = next((k for k in (n, -n) if flag_of(at(k)) != first), None)
        n *= 2
    if hit is None:
        raise AssertionError("no flip within reach: the target is not near the face")
    lo = 0
    while abs(hit - lo) > 1:
        mid = (lo + hit) // 2
        if flag_of(at(mid)) == first:
            lo = mid
        else:
            hit = mid
    return at(hit)


def boxes_through(target, quat, half, face, rng):
    """Boxes (centre, quat, half) whose face `face` (0..5) passes through `target`: the centre c = K - L^-1 b with b_a = +-half_a
    at 200 bits, rounded, walked to where the f64 chain's flag for the target changes (a few steps: the chain's own rounding),
    and that centre's neighbours 1-2 steps away per axis: 13 boxes, the target kept by some and dropped by others."""
    a, sign = face // 2, (1.0 if face % 2 else -1.0)
    with mp.workprec(BITS):
        L, Linv = _box_map(quat)
        b = [mpf(float(half[k])) * mpf(float(rng.uniform(-0.9, 0.9))) for k in range(3)]
        b[a] = mpf(float(half[a])) * sign
        wv = Linv * mp.matrix(b)
        centre = [float(mpf(float(target[k])) - wv[k]) for k in range(3)]
        axis = int(np.argmax([abs(float(L[a, k])) for k in range(3)]))
    centre = _walk_to_flip(centre, axis, lambda c: obb_contains_f64(c, quat, half, target))
    return [(c, np.asarray(quat, dtype=np.float64), np.asarray(half, dtype=np.float64)) for c in _family(centre)]


def plane_distance(m, face, target):
    """Signed distance (world units, mpf) of `target` from clip plane `face` of the f64 clip matrix m, and the plane's unit
    normal: the plane is row_a - sign * row_w = 0."""
    mm = np.asarray(m, dtype=np.float64).ravel()
    a, sign = face // 2, (1 if face % 2 else -1)
    coef = [mpf(float(mm[4 * c + a])) - sign * mpf(float(mm[4 * c + 3])) for c in range(4)]
    norm = mp.sqrt(coef[0] ** 2 + coef[1] ** 2 + coef[2] ** 2)
    k = _mpv(target)
    return (coef[0] * k[0] + coef[1] * k[1] + coef[2] * k[2] + coef[3]) / norm, [c / norm for c in coef[:3]]


def frusta_through(target, quat, perspective, face, frustum_new, rng):
    """Frusta whose clip plane `face` passes through `target`: a clip-space point with that coordinate +-1 (the others inside)
    goes through the 200-bit inverse of the perspective matrix to eye space, k_e; the eye is K - R k_e, then moved along the
    plane's normal by the target's exact distance from the plane of the matrix `frustum_new(eye, quat, perspective)` returns
    (three rounds: the matrix is rebuilt in f64 every time), then walked to where the f64 chain's flag changes, then that eye's
    neighbours 1-2 steps per axis. -> [(eye, clip_from_query, query_from_clip)], 13 of them."""
    a, sign = face // 2, (1 if face % 2 else -1)
    flag_of = lambda e: frustum_contains_f64(frustum_new(e, quat, perspective)[0], target)
    with mp.workprec(BITS):
        P = mp.matrix(4, 4)
        pp = np.asarray(perspective, dtype=np.float64).ravel()
        for r in range(4):
            for c in range(4):
                P[r, c] = mpf(float(pp[4 * c + r]))
        cl = [mpf(float(rng.uniform(-0.8, 0.8))) for _ in range(3)] + [mpf(1)]
        cl[a] = mpf(sign)
        h = mp.inverse(P) * mp.matrix(cl)
        ke = _rotate(_mpv(quat), tuple(h[k] / h[3] for k in range(3)))
        eye = [float(mpf(float(target[k])) - ke[k]) for k in range(3)]
        for _ in range(3):
            c, _ = frustum_new(eye, quat, perspective)
            d, n = plane_distance(c, face, target)
            eye = [float(mpf(eye[k]) + d * n[k]) for k in range(3)]
        axis = int(np.argmax([abs(float(v)) for v in n]))
    eye = _walk_to_flip(eye, axis, flag_of)
    out = []
    for e in _family(eye):
        c, qi = frustum_new(e, quat, perspective)
        out.append((e, np.asarray(c, dtype=np.float64).copy(), np.asarray(qi, dtype=np.float64).copy()))
    return out


# ---- the planted sets the tests share --------------------------------------------------------------------------------------
def planted_points_scene(scale, make_frustum, boxes=10, frusta=10, per_face=10, seed=77):
    """General boxes and frusta at SCALES[scale], and per shape per_face positions on each face with their neighbours 1-3 steps
    away (6 * per_face * 19 points a shape), one array for all. make_frustum(eye, quat, (aspect, fovy, near, far)) ->
    (clip_from_query, query_from_clip). -> dict(shapes [("obb", c, q, h) | ("frustum2", c, qi)], x, y, z, owner, face)."""
    rng = np.random.default_rng(seed + (0 if scale == "local" else 1000))
    shapes, pts, owner, face = [], [], [], []
    for c, q, h in general_boxes(scale, boxes, seed + 1):
        pos, f = with_neighbours(*plant_on_box(c, q, h, rng, per_face))
        shapes.append(("obb", np.asarray(c), np.asarray(q), np.asarray(h)))
        pts.append(pos), face.append(f), owner.append(np.full(f.size, len(shapes) - 1))
    for eye, q, persp in general_frusta(scale, frusta, seed + 2):
        c, qi = make_frustum(eye, q, persp)
        pos, f = with_neighbours(*plant_on_frustum(c, rng, per_face))
        shapes.append(("frustum2", np.asarray(c, dtype=np.float64).copy(), np.asarray(qi, dtype=np.float64).copy()))
        pts.append(pos), face.append(f), owner.append(np.full(f.size, len(shapes) - 1))
    pts = np.concatenate(pts)
    out = dict(shapes=shapes, x=np.ascontiguousarray(pts[:, 0]), y=np.ascontiguousarray(pts[:, 1]), z=np.ascontiguousarray(pts[:, 2]),
               owner=np.concatenate(owner), face=np.concatenate(face))
    for k in ("x", "y", "z", "owner", "face"):
        out[k].setflags(write=False)
    return out


def node_cube_targets(count, seed=5, extent=64.0):
    """Node cubes of the power-of-two scene [0, extent]^3 at levels 1..5: (level, min xyz, edge)."""
    rng = np.random.default_rng(seed)
    out = []
    for k in range(count):
        level = 1 + k % 5
        edge = extent / 2 ** level
        out.append((level, rng.integers(0, 2 ** level, 3).astype(np.float64) * edge, edge))
    return out


def _touching_corner(cube_min, edge, outward):
    """The corner of the cube that a plane with this outward normal, coming from inside the shape, touches first: the cube then
    lies outside the face and meets it in that corner alone — the tie of `bmin > amax` (sat.rs:174-194)."""
    return np.array([cube_min[k] if float(outward[k]) > 0 else cube_min[k] + edge for k in range(3)], dtype=np.float64)


def planted_node_shapes(make_frustum, cubes, seed=9):
    """Per node cube (min xyz, edge) one box family and one frustum family (13 shapes each) with a face through the cube's corner
    that faces the shape, so that the cube touches the shape in that corner; general rotations, faces in turn.
    -> (families [(kind, corner, first shape index)], shapes as planted_points_scene lists them)."""
    rng = np.random.default_rng(seed)
    families, shapes = [], []
    for k, (cube_min, edge) in enumerate(cubes):
        quat, half, face = unit_quat(rng), rng.uniform(1.0, 20.0, 3), k % 6
        with mp.workprec(BITS):
            L, _ = _box_map(quat)
            outward = [(1 if face % 2 else -1) * L[face // 2, c] for c in range(3)]
        corner = _touching_corner(cube_min, edge, outward)
        families.append(("obb", corner, len(shapes)))
        shapes += [("obb", *b) for b in boxes_through(corner, quat, half, face, rng)]
        quat, face = unit_quat(rng), (k // 2) % 6
        persp = make_frustum.perspective(float(rng.choice([0.75, 1.0, 1.7777])), float(rng.uniform(0.4, 1.6)), 0.5, 40.0)
        with mp.workprec(BITS):  # the plane's normal does not depend on where the eye is
            _, normal = plane_distance(make_frustum.from_perspective([0.0, 0.0, 0.0], quat, persp)[0], face, [0.0, 0.0, 0.0])
            outward = [(1 if face % 2 else -1) * c for c in normal]
        corner = _touching_corner(cube_min, edge, outward)
        families.append(("frustum2", corner, len(shapes)))
        shapes += [("frustum2", c, qi) for _, c, qi in frusta_through(corner, quat, persp, face, make_frustum.from_perspective, rng)]
    return families, shapes


def planted_stored_shapes(make_frustum, targets, seed=21):
    """Per stored (decoded) position: a box family and a frustum family through it under general rotations (13 shapes each), and
    under each of EXACT_ROTATIONS and along each axis the exact pair (closed on the point, one step inside it).
    -> (families [dict(kind "obb" | "frustum2" | "pair", target, first, count, exact)], shapes)."""
    rng = np.random.default_rng(seed)
    families, shapes = [], []
    for t, p in enumerate(targets):
        fam = [("obb", *b) for b in boxes_through(p, unit_quat(rng), rng.uniform(1.0, 20.0, 3), t % 6, rng)]
        families.append(dict(kind="obb", target=t, first=len(shapes), count=len(fam), exact=False))
        shapes += fam
        persp = make_frustum.perspective(float(rng.choice([0.75, 1.0, 1.7777])), float(rng.uniform(0.4, 1.6)), 0.5, 40.0)
        fam = [("frustum2", c, qi) for _, c, qi in frusta_through(p, unit_quat(rng), persp, (t + 3) % 6, make_frustum.from_perspective, rng)]
        families.append(dict(kind="frustum2", target=t, first=len(shapes), count=len(fam), exact=False))
        shapes += fam
        for r in range(len(EXACT_ROTATIONS)):
            for axis in range(3):
                closed, lower, exact = exact_pair(p, r, axis)
                families.append(dict(kind="pair", target=t, first=len(shapes), count=2, exact=exact))
                shapes += [("obb", *closed), ("obb", *lower)]
    return families, shapes
