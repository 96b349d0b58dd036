"""CPU oracle of pcv_xray_run_s2_ex: xray's leaf level over S2 cell clouds with --filter-interval on any scalar attribute
(FilteredIterator over filter_intervals, xray/src/generation.rs:478-487) and --binning on any scalar attribute
(BinnedColoringStrategy::bins, :138-157).

A tile's points are xray_s2_oracle's (the listed cells ascending, file order within a cell, culled by the tile's shape and the
intensity interval) with the filter masks applied by numpy: `column.astype(f64)` in the closed interval, NaN failing. The
image is xray_intensity_oracle.tile_image with the bins passed in as an array: every cloud's bins come from its own column,
of its own data type, through xray_intensity_oracle.bins_of.
"""
import numpy as np

import oracle_lib as O
import xray_intensity_oracle as I
import xray_oracle as X
import xray_s2_oracle as S

F32 = np.float32


class AttrPoints(S.S2Points):
    """S2Points with the cloud's extra columns, in input order."""

    def __init__(self, x, y, z, rgb, intensity, split_level, extras, corners_of=None):
        super().__init__(x, y, z, rgb, intensity, split_level, corners_of)
        self.extras = {k: np.ascontiguousarray(v) for k, v in extras.items()}

    def column(self, name):
        return self.intensity if name == "intensity" else self.extras[name]


def filter_mask(sp, idx, filters):
    keep = np.ones(idx.size, dtype=bool)
    for name, (lo, hi) in (filters or {}).items():
        a = sp.column(name)[idx].astype(np.float64)
        with np.errstate(invalid="ignore"):
            keep &= (np.float64(lo) <= a) & (a <= np.float64(hi))
    return keep


def tile_indices(sps, kind, params, interval=None, filters=None):
    """per cloud: the input indices of the tile's kept points"""
    out = []
    for sp in sps:
        idx = sp.query_indices(kind, params, interval)
        out.append(idx[filter_mask(sp, idx, filters)])
    return out


def tile_image(x, y, z, rgb, inten, bins, mn, mx, W, strategy, lo=0.0, hi=1.0, background="white"):
    """xray_intensity_oracle.tile_image with the bin of every point given: (image, drawn, negative)."""
    neg = inten < F32(0) if strategy == "colored_with_intensity" else np.zeros(x.shape, bool)
    keep = ~neg
    x, y, z, rgb, inten, bins = x[keep], y[keep], z[keep], rgb[keep], inten[keep], bins[keep]
    px, py, _ = X.discretise(x, y, z, mn, mx, W)
    draw = (px < W) & (py < W)
    img = np.empty((W, W, 4), dtype=np.uint8)
    img[:] = X.TRANSPARENT
    pix = (py[draw] * W + px[draw]).astype(np.int64)
    if pix.size:
        f, b, c = inten[draw], bins[draw].astype(np.int64), rgb[draw]
        value = f.view(np.uint32).astype(np.uint64) if strategy == "colored_with_intensity" else \
            (c[:, 0].astype(np.uint64) | c[:, 1].astype(np.uint64) << 8 | c[:, 2].astype(np.uint64) << 16)
        order = np.lexsort((value, b, pix))
        pix, b, f, c = pix[order], b[order], f[order], c[order]
        head = np.ones(pix.size, bool)
        head[1:] = (pix[1:] != pix[:-1]) | (b[1:] != b[:-1])
        seg = np.flatnonzero(head)
        cnt = np.diff(np.append(seg, pix.size))
        seg_pix = pix[seg]
        if strategy == "colored_with_intensity":
            means = [(I._seq_sum(f, seg, cnt) / cnt.astype(F32)).astype(F32)]
        else:
            csum = [np.add.reduceat(c[:, k].astype(np.uint64), seg) for k in range(3)]
            dn = 255.0 * cnt.astype(np.float64)
            means = [(s.astype(np.float64) / dn).astype(F32) for s in csum]
            means.append((np.minimum(cnt, 1 << 24).astype(F32) / cnt.astype(F32)).astype(F32))
        u, pstart, pcount = np.unique(seg_pix, return_index=True, return_counts=True)
        acc = [I._seq_sum(m, pstart, pcount) for m in means]
        nb = pcount.astype(F32)
        if strategy == "colored_with_intensity":
            col = I.intensity_color((acc[0] / nb).astype(F32), lo, hi)
        else:
            col = X.to_u8(*[(a / nb).astype(F32) for a in acc])
        img.reshape(-1, 4)[u] = col
    bg = X.WHITE if background == "white" else X.TRANSPARENT
    img[img[..., 3] < 128] = bg
    return img, int(draw.sum()), int(neg.sum())


def tiles(sps, tile_size_px, pixel_size_m, strategy, binning=None, filters=None, lo=0.0, hi=1.0, background="white", interval=None,
          iso=None):
    """({leaf id: (image, drawn, negative, kept)}, geometry, {leaf id: [kept input indices per cloud]}) of the created tiles.
    strategy: "colored" or "colored_with_intensity" (binning: None or (attribute, size)), or "xray" (which reads no bins)."""
    g = S.geometry(sps, tile_size_px, pixel_size_m, iso)
    out, kept = {}, {}
    for name, (mn, mx), (kind, params) in zip(g["leaf_ids"], g["tile_bbox"], S.tile_shapes(g, iso)):
        parts = tile_indices(sps, kind, params, interval, filters)
        n = sum(p.size for p in parts)
        if n == 0:
            continue
        kept[name] = parts
        x, y, z = (np.concatenate([getattr(sp, a)[p] for sp, p in zip(sps, parts)]) for a in "xyz")
        rgb = np.concatenate([sp.rgb[p] for sp, p in zip(sps, parts)])
        if iso is not None:
            x, y, z = O.iso_transform_points(iso, x, y, z)
        if strategy == "xray":
            img, drawn = X.tile_image(x, y, z, rgb, mn, mx, tile_size_px, "xray", background)
            out[name] = (img, drawn, 0, n)
            continue
        inten = np.concatenate([sp.intensity[p] if sp.intensity is not None else np.zeros(p.size, F32) for sp, p in zip(sps, parts)])
        if binning is None:
            bins = np.zeros(n, dtype=np.int64)
        else:  # every cloud converts with its own data type (match_1d_attr_data per batch)
            bins = np.concatenate([I.bins_of(sp.column(binning[0])[p], binning[1]) for sp, p in zip(sps, parts)])
        out[name] = tile_image(x, y, z, rgb, inten, bins, mn, mx, tile_size_px, strategy, lo, hi, background) + (n,)
    return out, g, kept
