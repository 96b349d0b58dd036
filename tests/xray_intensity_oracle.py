"""Numpy restatement of xray's colored_with_intensity (IntensityColoringStrategy, xray/src/generation.rs:210-292) and of
binning (BinnedColoringStrategy::bins :138-157, PointColorColoringStrategy with bins :294-362): the CPU oracle of
pcv_xray_run_ex.

Points: xray_oracle's TreePoints and node order, with the intensity the octree carries. Per pixel and bin the f32 sum is
taken over the bin's points sorted by their value bits (any order is one the reference may take; this one is the device's),
the bin means are added in ascending bin order. Every kept point with intensity < 0 is counted; the tile is drawn from the
others (the documented rule of pcv_xray_run_ex). ln is the kernel's own f32 ln (an f64 series), restated operation by
operation; `ln_ref` is numpy's f32 log for comparison.
"""
import numpy as np

import oracle_lib as O
import xray_oracle as X

F32 = np.float32
_LN2 = 0.6931471805599453


def ln_f32(x):
    x = np.asarray(x, dtype=F32)
    d = x.astype(np.float64)
    ok = np.isfinite(d) & (d > 0)
    fr, ex = np.frexp(np.where(ok, d, 1.0))
    m, e = fr * 2.0, ex.astype(np.int64) - 1
    big = m > 1.4142135623730951
    m = np.where(big, m * 0.5, m)
    e = np.where(big, e + 1, e)
    s = (m - 1.0) / (m + 1.0)
    s2 = s * s
    poly = s2 * (1.0 / 3.0 + s2 * (1.0 / 5.0 + s2 * (1.0 / 7.0 + s2 * (1.0 / 9.0 + s2 * (1.0 / 11.0 + s2 * (1.0 / 13.0 + s2 * (
        1.0 / 15.0 + s2 * (1.0 / 17.0))))))))
    lnm = 2.0 * s + 2.0 * s * poly
    r = (e.astype(np.float64) * _LN2 + lnm).astype(F32)
    r = np.where(x == F32(0), F32(-np.inf), r)
    r = np.where(x == F32(np.inf), F32(np.inf), r)
    r = np.where((x < F32(0)) | np.isnan(x), F32(np.nan), r)
    return r.astype(F32)


def rust_max(a, b):
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    return np.where(np.isnan(a), b, np.where(np.isnan(b), a, np.where(a > b, a, b))).astype(F32)


def rust_min(a, b):
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    return np.where(np.isnan(a), b, np.where(np.isnan(b), a, np.where(a < b, a, b))).astype(F32)


def intensity_color(mean, lo, hi, ln=ln_f32):
    """get_pixel_color after the mean (:270-284): RGBA rows."""
    with np.errstate(all="ignore"):
        m = rust_min(rust_max(np.asarray(mean, F32), F32(lo)), F32(hi))
        b = (ln(m - F32(lo)) / ln(np.asarray(F32(hi) - F32(lo)))).astype(F32)
    return X.to_u8(b, b, b, F32(1))


def bins_of(inten, size):
    """(intensity as f64 / size) as i64: truncating, saturating, NaN -> 0."""
    with np.errstate(all="ignore"):
        v = inten.astype(np.float64) / float(size)
    out = np.zeros(v.shape, dtype=np.int64)
    fin = np.isfinite(v) & (v < 9223372036854775808.0) & (v >= -9223372036854775808.0)
    out[fin] = np.trunc(v[fin]).astype(np.int64)
    out[~np.isnan(v) & (v >= 9223372036854775808.0)] = np.iinfo(np.int64).max
    out[~np.isnan(v) & (v < -9223372036854775808.0)] = np.iinfo(np.int64).min
    return out


def query(tp, kind, params, interval=None):
    """TreePoints.query with the intensity of every kept point."""
    xs, ys, zs, cs, fs = [], [], [], [], []
    for name in O.nodes_in_location(tp.bmin, tp.bmax, tp.nodes, kind, params):
        if tp.nodes[name]["num_points"] == 0:
            continue
        x, y, z, rgb, inten = tp.node(name)
        keep = O.cull_points(kind, params, x, y, z, inten if interval is not None else None, interval).astype(bool)
        xs.append(x[keep]), ys.append(y[keep]), zs.append(z[keep]), cs.append(rgb[keep]), fs.append(inten[keep])
    if not xs:
        return np.zeros(0), np.zeros(0), np.zeros(0), np.zeros((0, 3), np.uint8), np.zeros(0, F32)
    return tuple(np.concatenate(a) for a in (xs, ys, zs, cs, fs))


def _seq_sum(vals, starts, counts):
    """f32 sums of vals[starts[i] : starts[i] + counts[i]], each left to right."""
    sums = np.zeros(starts.size, dtype=F32)
    for k in range(int(counts.max()) if counts.size else 0):
        live = counts > k
        sums[live] = (sums[live] + vals[starts[live] + k]).astype(F32)
    return sums


def tile_image(x, y, z, rgb, inten, mn, mx, W, strategy, lo=0.0, hi=1.0, bin_size=None, background="white"):
    """(image, drawn, negative) of one created tile. strategy: "colored_with_intensity" or "colored"."""
    neg = inten < F32(0) if strategy == "colored_with_intensity" else np.zeros(inten.shape, bool)
    keep = ~neg
    x, y, z, rgb, inten = x[keep], y[keep], z[keep], rgb[keep], inten[keep]
    px, py, _ = X.discretise(x, y, z, mn, mx, W)
    draw = (px < W) & (py < W)
    img = np.empty((W, W, 4), dtype=np.uint8)
    img[:] = X.TRANSPARENT
    pix = (py[draw] * W + px[draw]).astype(np.int64)
    if pix.size:
        f = inten[draw]
        b = bins_of(f, bin_size) if bin_size is not None else np.zeros(pix.size, np.int64)
        c = rgb[draw]
        value = f.view(np.uint32).astype(np.uint64) if strategy == "colored_with_intensity" else \
            (c[:, 0].astype(np.uint64) | c[:, 1].astype(np.uint64) << 8 | c[:, 2].astype(np.uint64) << 16)
        order = np.lexsort((value, b, pix))
        pix, b, f, c = pix[order], b[order], f[order], c[order]
        # (pixel, bin) segments
        head = np.ones(pix.size, bool)
        head[1:] = (pix[1:] != pix[:-1]) | (b[1:] != b[:-1])
        seg = np.flatnonzero(head)
        cnt = np.diff(np.append(seg, pix.size))
        seg_pix = pix[seg]
        if strategy == "colored_with_intensity":
            means = [(_seq_sum(f, seg, cnt) / cnt.astype(F32)).astype(F32)]
        else:
            csum = [np.add.reduceat(c[:, k].astype(np.uint64), seg) for k in range(3)]
            dn = 255.0 * cnt.astype(np.float64)
            means = [(s.astype(np.float64) / dn).astype(F32) for s in csum]
            means.append((np.minimum(cnt, 1 << 24).astype(F32) / cnt.astype(F32)).astype(F32))
        # per pixel: bin means in ascending bin order
        u, pstart, pcount = np.unique(seg_pix, return_index=True, return_counts=True)
        acc = [_seq_sum(m, pstart, pcount) for m in means]
        nb = pcount.astype(F32)
        if strategy == "colored_with_intensity":
            col = intensity_color((acc[0] / nb).astype(F32), lo, hi)
        else:
            col = X.to_u8(*[(a / nb).astype(F32) for a in acc])
        img.reshape(-1, 4)[u] = col
    bg = X.WHITE if background == "white" else X.TRANSPARENT
    img[img[..., 3] < 128] = bg
    return img, int(draw.sum()), int(neg.sum())


def xray_tiles(tps, tile_size_px, pixel_size_m, strategy, lo=0.0, hi=1.0, bin_size=None, background="white", interval=None):
    """{leaf id: (image, drawn, negative)} over the union of the octrees (TreePoints list, concatenated in list order),
    and the geometry."""
    import xray_many_oracle as M
    blo, bhi = M.union_box(tps)
    g = X.leaf_geometry(tile_size_px, pixel_size_m, blo, bhi)
    out = {}
    for name, (mn, mx) in zip(g["leaf_ids"], g["tile_bbox"]):
        parts = [query(tp, O.SHAPE_AABB, list(mn) + list(mx), interval) for tp in tps]
        if sum(p[0].size for p in parts) == 0:
            continue
        x, y, z, rgb, inten = (np.concatenate([p[a] for p in parts]) for a in range(5))
        out[name] = tile_image(x, y, z, rgb, inten, mn, mx, tile_size_px, strategy, lo, hi, bin_size, background)
    return out, g
