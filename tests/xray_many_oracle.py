"""CPU oracle of pcv_xray_run_many: xray's leaf level over several octrees, as build_xray_quadtree runs with several
point_cloud_locations through one PointCloudClient (point_cloud_client/src/lib.rs).

Bounding box: PointCloudClientBuilder::build's union (:101-125), the first octree's meta box grown by every octree's min and
then its max in list order (Aabb::grow: per-component min / max). Leaf geometry: xray_oracle.leaf_geometry on that union.
Points of a tile: TreePoints.query per octree, concatenated in list order (try_for_each_batch's jobs are a flat_map over
the clouds, src/iterator.rs:262-270). Raster: xray_oracle.tile_image.
"""
import numpy as np

import oracle_lib as O
import xray_oracle as X


def union_box(tps):
    lo = [float(v) for v in tps[0].bmin]
    hi = [float(v) for v in tps[0].bmax]
    for tp in tps:
        for q in (tp.bmin, tp.bmax):
            for a in range(3):
                v = float(q[a])
                lo[a] = v if v < lo[a] else lo[a]
                hi[a] = v if v > hi[a] else hi[a]
    return tuple(lo), tuple(hi)


def tile_points(tps, tile_size_px, pixel_size_m, iso=None, interval=None, root="r"):
    """(geometry, {leaf id: (x, y, z, rgb)} for every tile with a kept point). Positions are in the query frame; the
    geometry's "kept_per_octree" holds each such tile's kept points per octree."""
    lo, hi = union_box(tps)
    g = X.leaf_geometry(tile_size_px, pixel_size_m, lo, hi, iso, root)
    g["kept_per_octree"] = {}
    pts = {}
    for name, (mn, mx) in zip(g["leaf_ids"], g["tile_bbox"]):
        if iso is None:
            kind, params = O.SHAPE_AABB, list(mn) + list(mx)
        else:
            kind, params = O.SHAPE_OBB, X.tile_obb(iso, mn, mx)
        parts = [tp.query(kind, params, interval) for tp in tps]
        x, y, z = (np.concatenate([p[a] for p in parts]) for a in range(3))
        if x.size == 0:
            continue
        rgb = np.concatenate([p[3] for p in parts])
        g["kept_per_octree"][name] = [int(p[0].size) for p in parts]
        if iso is not None:
            x, y, z = O.iso_transform_points(iso, x, y, z)
        pts[name] = (x, y, z, rgb)
    return g, pts


def xray_tiles(tps, tile_size_px, strategy, background="white", pixel_size_m=None, iso=None, interval=None, root="r",
               points=None):
    """{leaf id: (image, drawn, kept)} for every created tile, and the geometry. points: tile_points' result, reused."""
    g, pts = points if points is not None else tile_points(tps, tile_size_px, pixel_size_m, iso, interval, root)
    out = {}
    for name, (mn, mx) in zip(g["leaf_ids"], g["tile_bbox"]):
        if name in pts:
            x, y, z, rgb = pts[name]
            img, drawn = X.tile_image(x, y, z, rgb, mn, mx, tile_size_px, strategy, background)
            out[name] = (img, drawn, int(x.size))
    return out, g
