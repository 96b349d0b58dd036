"""CPU oracle of pcv_xray_run_s2: xray's leaf level over S2 cell clouds (PointClouds::S2Cells, point_cloud_client/src/lib.rs).

S2Points is what xray_many_oracle.tile_points / xray_tiles need of a cloud: bmin / bmax (S2Splitter's exact min / max) and
query(kind, params, interval). A location's points are those of the cells that S2Cells::nodes_in_location lists for it — the
host twin pcv.s2_cells_in_location over the shape's corners — cells ascending, the points of a cell in file (input) order,
filtered by oracle_lib.cull_points. The corners are a shape's own (s2_region_truth.spec_corners on the CPU; the device
tests hand in Shapes.get's, so that the lists are the device's lists).

brute_force is the independent layer for one tile: the filter over ALL input points, and the precondition under which the
listing cannot matter — every cell that holds a passing point is in s2_region_truth.decided_lists' `yes` list for the
corners' rect (the truth's own rect, not the product's).
"""
import math

import numpy as np

import oracle_lib as O
import point_cloud_viewer_amd as pcv
import s2_region_truth as R
import xray_intensity_oracle as I
import xray_many_oracle as M
import xray_oracle as X

F32 = np.float32
LAT, LNG = 37.407204, -122.147604  # s2_region_truth.scene()'s place


def quat_of(m):
    """Unit quaternion (i, j, k, w) of a rotation matrix."""
    t = m[0, 0] + m[1, 1] + m[2, 2]
    if t > 0.0:
        s = math.sqrt(t + 1.0) * 2.0
        q = [(m[2, 1] - m[1, 2]) / s, (m[0, 2] - m[2, 0]) / s, (m[1, 0] - m[0, 1]) / s, 0.25 * s]
    elif m[0, 0] > m[1, 1] and m[0, 0] > m[2, 2]:
        s = math.sqrt(1.0 + m[0, 0] - m[1, 1] - m[2, 2]) * 2.0
        q = [0.25 * s, (m[0, 1] + m[1, 0]) / s, (m[0, 2] + m[2, 0]) / s, (m[2, 1] - m[1, 2]) / s]
    elif m[1, 1] > m[2, 2]:
        s = math.sqrt(1.0 + m[1, 1] - m[0, 0] - m[2, 2]) * 2.0
        q = [(m[0, 1] + m[1, 0]) / s, 0.25 * s, (m[1, 2] + m[2, 1]) / s, (m[0, 2] - m[2, 0]) / s]
    else:
        s = math.sqrt(1.0 + m[2, 2] - m[0, 0] - m[1, 1]) * 2.0
        q = [(m[0, 2] + m[2, 0]) / s, (m[1, 2] + m[2, 1]) / s, 0.25 * s, (m[1, 0] - m[0, 1]) / s]
    q = np.array(q, dtype=np.float64)
    return [float(v) for v in q / np.linalg.norm(q)]


def local_from_ecef():
    """query_from_global into the scene's local frame: the inverse of synthetic.ecef_from_local — the quaternion of rot.T and
    the translation -(rot.T @ centre); translation xyz + quaternion ijkw."""
    from point_cloud_viewer_amd import synthetic
    rot, centre = synthetic.ecef_from_local(LAT, LNG)
    return [float(v) for v in -(rot.T @ centre)] + quat_of(rot.T)


def shape_spec(kind, params):
    """The Context.shapes entry of a tile's (kind, params) as xray_many_oracle makes them."""
    p = [float(v) for v in params]
    if kind == O.SHAPE_AABB:
        return ("aabb", p[0:3], p[3:6])
    assert kind == O.SHAPE_OBB
    return ("obb", p[0:3], p[3:7], p[7:10])


class S2Points:
    def __init__(self, x, y, z, rgb, intensity, split_level, corners_of=None):
        self.x, self.y, self.z = (np.ascontiguousarray(a, dtype=np.float64) for a in (x, y, z))
        self.rgb = np.ascontiguousarray(rgb, dtype=np.uint8)
        self.intensity = None if intensity is None else np.ascontiguousarray(intensity, dtype=np.float32)
        self.bmin = np.array([self.x.min(), self.y.min(), self.z.min()])
        self.bmax = np.array([self.x.max(), self.y.max(), self.z.max()])
        self.point_cell = pcv.s2_cell_ids(self.x, self.y, self.z, split_level)
        self.cell_ids = np.unique(self.point_cell)  # ascending
        order = np.argsort(self.point_cell, kind="stable")  # a cell's points in input order
        first = np.searchsorted(self.point_cell[order], self.cell_ids)
        self.cell_points = np.split(order, first[1:])
        self.corners_of = corners_of if corners_of is not None else (lambda kind, params: R.spec_corners(shape_spec(kind, params)))

    def listed_cells(self, kind, corners):
        """indices into cell_ids, ascending: S2Cells::nodes_in_location by the host twin"""
        return pcv.s2_cells_in_location(self.cell_ids, [int(kind)], [1], np.asarray(corners, dtype=np.float64).reshape(1, 8, 3))[0]

    def query_indices(self, kind, params, interval=None, corners=None):
        """input indices of the location's points: listed cells ascending, file order within a cell, culled"""
        corners = self.corners_of(kind, params) if corners is None else corners
        cells = self.listed_cells(kind, corners)
        if len(cells) == 0:
            return np.zeros(0, dtype=np.int64)
        idx = np.concatenate([self.cell_points[int(c)] for c in cells])
        return idx[self._keep(kind, params, interval, idx)]

    def _keep(self, kind, params, interval, idx):
        attr = self.intensity[idx] if interval is not None else None
        return O.cull_points(kind, params, self.x[idx], self.y[idx], self.z[idx], attr, interval).astype(bool)

    def query(self, kind, params, interval=None, corners=None):
        idx = self.query_indices(kind, params, interval, corners)
        return self.x[idx], self.y[idx], self.z[idx], self.rgb[idx]

    def brute_indices(self, kind, params, interval=None):
        """the filter over all input points, sorted input indices"""
        idx = np.arange(self.x.size)
        return idx[self._keep(kind, params, interval, idx)]


def brute_force(sp, kind, params, interval=None, corners=None, bounds=None):
    """(sorted input indices that pass the filter, cells that hold a passing point but are not decided `yes` for the corners'
    rect). The second list empty is the precondition: then no listing that agrees with the truth can miss a passing point."""
    idx = sp.brute_indices(kind, params, interval)
    corners = sp.corners_of(kind, params) if corners is None else corners
    rect = R.corners_rect([tuple(float(v) for v in c) for c in np.asarray(corners).reshape(8, 3)])
    yes = set(R.decided_lists(sp.cell_ids, rect, bounds=bounds)[0]) if rect is not None else set()
    holding = np.unique(np.searchsorted(sp.cell_ids, sp.point_cell[idx]))
    return idx, [int(c) for c in holding if int(c) not in yes]


def tile_shapes(g, iso=None):
    """[(kind, params)] per leaf tile of an xray_oracle.leaf_geometry, as xray_from_points makes its locations"""
    out = []
    for mn, mx in g["tile_bbox"]:
        if iso is None:
            out.append((O.SHAPE_AABB, list(mn) + list(mx)))
        else:
            out.append((O.SHAPE_OBB, X.tile_obb(iso, mn, mx)))
    return out


def geometry(sps, tile_size_px, pixel_size_m, iso=None, root="r"):
    lo, hi = M.union_box(sps)
    return X.leaf_geometry(tile_size_px, pixel_size_m, lo, hi, iso, root)


def brute_tile_points(sps, tile_size_px, pixel_size_m, iso=None, interval=None):
    """xray_many_oracle.tile_points' (geometry, points) from the brute-force filter (points in input order per cloud), and the
    list of (leaf id, cloud, cells) that fail the precondition."""
    g = geometry(sps, tile_size_px, pixel_size_m, iso)
    bounds = [R.cell_bounds(sp.cell_ids) for sp in sps]
    pts, failures = {}, []
    for name, (kind, params) in zip(g["leaf_ids"], tile_shapes(g, iso)):
        parts = []
        for k, sp in enumerate(sps):
            idx, bad = brute_force(sp, kind, params, interval, bounds=bounds[k])
            if bad:
                failures.append((name, k, bad))
            parts.append(idx)
        if sum(p.size for p in parts) == 0:
            continue
        x, y, z = (np.concatenate([getattr(sp, a)[p] for sp, p in zip(sps, parts)]) for a in "xyz")
        rgb = np.concatenate([sp.rgb[p] for sp, p in zip(sps, parts)])
        if iso is not None:
            x, y, z = O.iso_transform_points(iso, x, y, z)
        pts[name] = (x, y, z, rgb)
    return (g, pts), failures


def intensity_tiles(sps, tile_size_px, pixel_size_m, strategy, lo=0.0, hi=1.0, bin_size=None, background="white", interval=None,
                    iso=None):
    """xray_intensity_oracle.xray_tiles over S2Points: {leaf id: (image, drawn, negative, kept)} and the geometry."""
    g = geometry(sps, tile_size_px, pixel_size_m, iso)
    out = {}
    for name, (mn, mx), (kind, params) in zip(g["leaf_ids"], g["tile_bbox"], tile_shapes(g, iso)):
        parts = [(sp, sp.query_indices(kind, params, interval)) for sp in sps]
        if sum(p.size for _, p in parts) == 0:
            continue
        x, y, z = (np.concatenate([getattr(sp, a)[p] for sp, p in parts]) for a in "xyz")
        rgb = np.concatenate([sp.rgb[p] for sp, p in parts])
        inten = np.concatenate([sp.intensity[p] for sp, p in parts])
        if iso is not None:
            x, y, z = O.iso_transform_points(iso, x, y, z)
        out[name] = I.tile_image(x, y, z, rgb, inten, mn, mx, tile_size_px, strategy, lo, hi, bin_size, background) + (int(x.size),)
    return out, g
