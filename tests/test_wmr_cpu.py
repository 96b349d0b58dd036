"""Web-mercator rectangles on the host: the constructor, the corners, the per-point chain and its transcendentals
(include/pcv_hip.h pcv_wmr_*; reference src/geometry/web_mercator_rect.rs, src/math/web_mercator.rs). No GPU."""
import math

import numpy as np
import pytest

import point_cloud_viewer_amd as pcv
from point_cloud_viewer_amd import _lib as L
from point_cloud_viewer_amd import synthetic

import wmr_oracle as W

DELTA = 1e-10        # normalised map units (about 4 mm on the ground): the band in which a flag may differ from the truth
MAX_AMBIGUOUS = 0.005


def rect_of(mn, mx, z):
    r = pcv.web_mercator_rect_from_zoomed(mn, mx, z)
    return None if r is None else tuple(r[1]) + tuple(r[2])


# ---- 1. the reference's own unit tests ------------------------------------------------------------------------------------
def test_wraparound_test():
    """web_mercator_rect.rs:198-221."""
    assert rect_of((255.5, 128.0), (0.5, 128.8), 0) is not None   # wraparound in x works
    assert rect_of((255.5, 128.0), (1.5, 128.8), 0) is None       # size is still checked
    assert rect_of((128.8, 255.5), (128.8, 0.5), 0) is None       # no wraparound in y


def test_from_zoomed_rejects_what_the_reference_rejects():
    """web_mercator.rs:84-97, web_mercator_rect.rs:40-53."""
    assert rect_of((1.0, 1.0), (2.0, 2.0), 24) is None
    assert rect_of((1.0, 1.0), (2.0, 2.0), 23) is not None
    assert rect_of((-0.5, 1.0), (0.5, 2.0), 3) is None
    assert rect_of((1.0, 1.0), (2.0, 256.0 * 8), 3) is None       # == 256 * 2^z is out of bounds
    assert rect_of((8.0, 8.0), (16.5, 9.0), 3) is None            # wider than one zoom-0 pixel
    assert rect_of((8.0, 8.0), (16.0, 16.0), 3) == (8.0 / 2048, 8.0 / 2048, 16.0 / 2048, 16.0 / 2048)
    assert rect_of((8.0, 9.0), (9.0, 8.0), 3) is None             # diff.y < 0
    wrap = rect_of((255.5, 128.0), (0.5, 128.8), 0)
    assert wrap[0] > wrap[2]                                      # passes the constructor ...
    x, y, z = synthetic.uniform_ecef(1000, lat=0.5, lon=-179.9999)[:3]
    assert pcv.wmr_contains(wrap, x, y, z).sum() == 0             # ... and contains nothing (web_mercator_rect.rs:121-127)


def test_projection_corners():
    """web_mercator.rs:107-128: the corners of the map, 1e-9 px at zoom 0."""
    u, v = pcv.wmr_from_lat_lng([W.LAT_BOUND_RAD, -W.LAT_BOUND_RAD], [-math.pi, math.pi])
    assert abs(256.0 * u[0]) <= 10e-10 and abs(256.0 * v[0]) <= 10e-10
    assert abs(256.0 * u[1] - 256.0) <= 10e-10 and abs(256.0 * v[1] - 256.0) <= 10e-10


def test_projection_roundtrip():
    """web_mercator.rs:130-146 (assert_relative_eq!'s default: max_relative = f64::EPSILON, epsilon = f64::EPSILON)."""
    lat, lng = math.radians(37.407204), math.radians(-122.147604)
    u, v = pcv.wmr_from_lat_lng([lat], [lng])
    lat2, lng2 = pcv.wmr_to_lat_lng(u, v)
    eps = 2.220446049250313e-16
    for a, b in ((lng, lng2[0]), (lat, lat2[0])):
        assert abs(a - b) <= eps or abs(a - b) <= max(abs(a), abs(b)) * eps, (a, b)


def test_projection_ground_truth():
    """web_mercator.rs:148-165: 20 px at zoom 19 — through from_lat_lng and through the ECEF chain."""
    lat, lng = math.radians(37.407204), math.radians(-122.147604)
    truth = np.array([84253.0 * 256.0 + 165.0, 203324.0 * 256.0 + 18.0])
    zoom = float(256 << 19)
    u, v = pcv.wmr_from_lat_lng([lat], [lng])
    assert np.all(np.abs(zoom * np.array([u[0], v[0]]) - truth) <= 20.0)
    p = synthetic._ecef_from_lat_lng(37.407204, -122.147604)
    u, v = pcv.wmr_project([p[0]], [p[1]], [p[2]])
    assert np.all(np.abs(zoom * np.array([u[0], v[0]]) - truth) <= 20.0)


def test_sagitta_test():
    """web_mercator_rect.rs:172-196."""
    lat, lng = pcv.wmr_to_lat_lng([127.5 / 256.0, 128.5 / 256.0], [127.5 / 256.0, 128.5 / 256.0])
    lat_diff, lng_diff = abs(lat[1] - lat[0]), abs(lng[1] - lng[0])
    assert 6335439.32 * (1.0 - math.cos(lat_diff / 2.0)) < 500.0
    assert 6378137.0 * (1.0 - math.cos(lng_diff / 2.0)) < 500.0


def test_intersection_test():
    """web_mercator_rect.rs:134-170: Out, Cross, Cross — pcv_wmr_corners + the numpy Intersector::intersect."""
    c1 = pcv.wmr_corners(rect_of((0.1, 0.1), (0.3, 0.3), 1))
    c2 = pcv.wmr_corners(rect_of((0.4, 0.4), (0.5, 0.5), 1))
    c3 = pcv.wmr_corners(rect_of((0.2, 0.2), (0.6, 0.6), 1))
    assert W.intersect(c1, c2) == W.REL_OUT
    assert W.intersect(c1, c3) == W.REL_CROSS
    assert W.intersect(c3, c2) == W.REL_CROSS


# ---- 2. corners against mpmath --------------------------------------------------------------------------------------------
def corner_cases():
    cases = []
    for z in range(0, 24):
        zoom = float(256 << z)
        for fy in (0.5, 0.35, 0.2, 0.05, 0.0005, 0.93, 0.9999):      # equator ... the clamp at 85.05 degrees, both hemispheres
            for fx in (0.0, 0.3, 0.75, 0.9999):
                mn = (min(fx * zoom, zoom - 2.0), min(fy * zoom, zoom - 2.0))
                r = rect_of(mn, (mn[0] + 1.0, mn[1] + 1.0), z)
                assert r is not None, (z, fx, fy)
                cases.append(r)
    cases.append(rect_of((255.5, 128.0), (0.5, 128.8), 0))             # across the antimeridian
    cases.append(rect_of((255.0, 0.0), (255.99, 1.0), 0))
    cases.append(rect_of((0.0, 255.0), (1.0, 255.99), 0))
    return cases


def test_corners_against_mpmath():
    """pcv_wmr_corners against the same formulas at 40 digits, zoom 0-23, equator to the clamp, both sides of the antimeridian.
    Tolerance: four times the largest error of a plain numpy f64 evaluation of the same formulas over the same cases.
    Measured (675 rectangles): numpy 2.274e-8 m, the library 2.274e-8 m (the same arithmetic on the same libm; the largest
    errors are at the clamp, where asin is steep)."""
    import mpmath as mp
    e_np = e_lib = 0.0
    cases = corner_cases()
    for r in cases:
        want = W.corners_mp(r)
        got_np, got = W.corners_np(r), pcv.wmr_corners(r)
        for i in range(8):
            for k in range(3):
                e_np = max(e_np, abs(float(mp.mpf(float(got_np[i, k])) - want[i][k])))
                e_lib = max(e_lib, abs(float(mp.mpf(float(got[i, k])) - want[i][k])))
    print(f"corners: {len(cases)} rectangles, largest error numpy {e_np:.3e} m, library {e_lib:.3e} m")
    assert e_np > 0.0
    assert e_lib <= 4.0 * e_np, (e_lib, e_np)


# ---- 3. the per-point chain against the truth -----------------------------------------------------------------------------
CLOUDS = [("config1", 37.407204, -122.147604), ("lat0", 0.0, 11.0), ("lat60", 60.0, 25.0), ("lat-80", -80.0, -60.0),
          ("antimeridian", -17.0, 180.0)]


def check_cloud(name, lat, lon, n_grid, side, n=200_000):
    x, y, z = synthetic.uniform_ecef(n, lat=lat, lon=lon)[:3]
    c = synthetic._ecef_from_lat_lng(lat, lon)
    cu, cv = (float(a[0]) for a in W.truth_uv_ld([c[0]], [c[1]], [c[2]]))
    if name == "antimeridian":
        cu = 1.0 - 0.5 * n_grid * side      # the grid ends at the map's right edge: the cloud's other half projects to u ~ 0
    rects = W.grid(cu, cv, n_grid, side)
    ub = sorted({r[0] for r in rects} | {r[2] for r in rects})
    vb = sorted({r[1] for r in rects} | {r[3] for r in rects})
    u, v, redone = W.truth_uv(x, y, z, ub, vb, DELTA)
    gu, gv = pcv.wmr_project(x, y, z)
    worst = max(float(np.abs(gu - u).max()), float(np.abs(gv - v).max()))
    ambiguous = np.zeros(n, dtype=bool)
    inside = 0
    for r in rects:
        flag, amb = W.classify(u, v, r, DELTA)
        got = pcv.wmr_contains(r, x, y, z).astype(bool)
        bad = (got != flag) & ~amb
        assert not bad.any(), (name, r, int(bad.sum()), float(u[bad][0]), float(v[bad][0]))
        ambiguous |= amb
        inside += int(got.sum())
    share = float(ambiguous.mean())
    print(f"{name}: {n_grid} x {n_grid} of side {side:g}: {inside} points inside, ambiguous {100 * share:.3f} %, "
          f"|uv - truth| <= {worst:.2e}, {redone} points through mpmath")
    assert share <= MAX_AMBIGUOUS, (name, share)
    return share, worst


def test_long_double_truth_agrees_with_mpmath():
    """The guard of wmr_oracle.truth_uv (1e-13) stands on this: the long-double iteration is within 1e-15 of mpmath."""
    worst = 0.0
    for name, lat, lon in CLOUDS:
        x, y, z = synthetic.uniform_ecef(40, seed=5, lat=lat, lon=lon)[:3]
        u, v = W.truth_uv_ld(x, y, z)
        for i in range(x.size):
            mu, mv = W.truth_uv_mp(x[i], y[i], z[i])
            worst = max(worst, abs(float(u[i] - W._mp_to_ld(mu))), abs(float(v[i] - W._mp_to_ld(mv))))
    print(f"long double vs mpmath: {worst:.2e}")
    assert worst < 1e-15


@pytest.mark.parametrize("name,lat,lon", CLOUDS)
@pytest.mark.parametrize("n_grid,side", [(7, 1e-6), (26, 2.5e-7)])
def test_contains_against_truth(name, lat, lon, n_grid, side):
    """pcv_wmr_contains against the iterated inverse: every flag outside the 1e-10 band equals the truth's, and at most 0.5 % of
    a case's points are in the band. Measured shares (7 x 7 of side 1e-6 / 26 x 26 of side 2.5e-7): config1 0.034 % / 0.143 %, lat0
    0.040 % / 0.163 %, lat60 0.032 % / 0.118 %, lat-80 0.015 % / 0.039 %, antimeridian 0.032 % / 0.125 % (the grids cover a part
    of the clouds at high latitude, where a metre is more map, and half of the one at the antimeridian);
    |(u, v) - truth| <= 9.9e-17, 6.7e-17, 1.9e-16, 5.5e-16, 1.2e-16."""
    check_cloud(name, lat, lon, n_grid, side)


# ---- 4. the transcendentals -----------------------------------------------------------------------------------------------
def ulps(got, want_mp):
    import mpmath as mp
    worst = 0.0
    for g, w in zip(got, want_mp):
        if w == 0:
            assert g == 0.0
            continue
        ulp = math.ldexp(1.0, math.frexp(float(w))[1] - 53)
        worst = max(worst, abs(float((mp.mpf(float(g)) - w) / ulp)))
    return worst


def test_transcendentals_against_mpmath():
    """atan2, sin, cos and ln of the chain on 10^5 arguments each over the ranges the chain feeds them (DESIGN §5 holds the
    figures; no threshold of its own beyond sanity — the flags of test_contains_against_truth are the check).
    Measured: atan2 2.29 ulp, sin 1.02 ulp, cos 1.40 ulp, ln 0.77 ulp (glibc on the same arguments: 0.79, 0.51, 0.51, 0.59)."""
    import mpmath as mp
    rng = np.random.default_rng(7)
    n = 100_000
    with mp.workdps(40):
        # atan2: (z a, p b) and (y, x) of ECEF points in every octant; latitudes' second atan2 has the same range
        lat, lon = rng.uniform(-1.55, 1.55, n), rng.uniform(-math.pi, math.pi, n)
        r = rng.uniform(6.3e6, 6.4e6, n)
        a, b = r * np.sin(lat), r * np.cos(lat) * np.where(rng.random(n) < 0.5, 1.0, np.cos(lon))
        got = pcv.wmr_math(L.WMR_FN_ATAN2, a, b)
        e_atan2 = ulps(got, [mp.atan2(mp.mpf(float(p)), mp.mpf(float(q))) for p, q in zip(a, b)])
        e_atan2_libm = ulps(np.arctan2(a, b), [mp.atan2(mp.mpf(float(p)), mp.mpf(float(q))) for p, q in zip(a, b)])
        # sin / cos: the parametric latitude and the clamped geodetic latitude, |x| <= pi / 2
        t = rng.uniform(-math.pi / 2, math.pi / 2, n)
        s, c = pcv.wmr_math(L.WMR_FN_SINCOS, t)
        want_s, want_c = [mp.sin(mp.mpf(float(v))) for v in t], [mp.cos(mp.mpf(float(v))) for v in t]
        e_sin, e_cos = ulps(s, want_s), ulps(c, want_c)
        e_sin_libm, e_cos_libm = ulps(np.sin(t), want_s), ulps(np.cos(t), want_c)
        # ln: (1 + s) / (1 - s) for |s| <= LAT_BOUND_SIN
        sy = rng.uniform(-0.99627207622075, 0.99627207622075, n)
        q = (1.0 + sy) / (1.0 - sy)
        want_l = [mp.log(mp.mpf(float(v))) for v in q]
        e_ln, e_ln_libm = ulps(pcv.wmr_math(L.WMR_FN_LN, q), want_l), ulps(np.log(q), want_l)
    print(f"ulps: atan2 {e_atan2:.2f} (libm {e_atan2_libm:.2f}), sin {e_sin:.2f} ({e_sin_libm:.2f}), cos {e_cos:.2f} ({e_cos_libm:.2f}), "
          f"ln {e_ln:.2f} ({e_ln_libm:.2f})")
    assert max(e_atan2, e_sin, e_cos, e_ln) < 4.0   # sanity: a wrong coefficient is thousands of ulps
