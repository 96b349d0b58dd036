"""Numpy restatement of xray's parent levels and quadtree directory — the CPU oracle of pcv_xray_build_parents,
pcv_xray_nodes, pcv_xray_write_dir and pcv_xray_png_encode.

create_non_leaf_nodes (xray/src/generation.rs:656-682): the parent ids of the level below. build_parent (:410-450): the
children in a 2W x 2W image over the background. build_node (:726-759): DynamicImage::resize(W, W, Lanczos3) of image
0.23.10 (sample.rs), restated from the pinned version: f32 taps with libm's sinf (what f32::sin calls on linux-gnu), the
vertical pass into an unclamped f32 intermediate, then the horizontal pass, clamp and round half away from zero. Every
pass is numpy float32 `*` and `+` (separate ufuncs: nothing is fused) in tap order.
Also: a PNG reader (chunk CRCs, zlib with its Adler-32, stored blocks, filter 0) and a decoder of xray_proto's Meta.
"""
import ctypes
import ctypes.util
import struct
import zlib

import numpy as np

import xray_oracle as X  # noqa: F401  (node names, backgrounds)

F32 = np.float32
_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.sinf.restype = ctypes.c_float
_libm.sinf.argtypes = [ctypes.c_float]
PI = F32(np.pi)  # f32::consts::PI


def sinf(x):
    return F32(_libm.sinf(float(F32(x))))


def sinc(t):
    t = F32(t)
    if t == F32(0):
        return F32(1)
    a = F32(t * PI)
    return F32(sinf(a) / a)


def lanczos3(x):
    x = F32(x)
    return F32(sinc(x) * sinc(F32(x / F32(3)))) if abs(x) < F32(3) else F32(0)


def taps(W):
    """(left, count, weights (W, 12)) of the 2W -> W resize: ratio 2, support 3 x 2."""
    n = 2 * W
    ratio, sratio = F32(2), F32(2)
    support = F32(F32(3) * sratio)
    left, count, weights = np.zeros(W, np.int64), np.zeros(W, np.int64), np.zeros((W, 12), F32)
    for o in range(W):
        c = F32(F32(F32(o) + F32(0.5)) * ratio)
        lo = min(max(int(np.floor(F32(c - support))), 0), n - 1)
        hi = min(max(int(np.ceil(F32(c + support))), lo + 1), n)
        ci = F32(c - F32(0.5))
        ws, s = [], F32(0)
        for i in range(lo, hi):
            w = lanczos3(F32(F32(F32(i) - ci) / sratio))
            ws.append(w)
            s = F32(s + w)
        left[o], count[o] = lo, hi - lo
        weights[o, :hi - lo] = [F32(w / s) for w in ws]
    return left, count, weights


def _pass(src, left, count, weights):
    """out[o] = sum_k src[left[o] + k] * w[o, k] along axis 0, f32, tap order; src is f32."""
    W = left.size
    out = np.zeros((W,) + src.shape[1:], F32)
    for k in range(int(count.max())):
        live = np.flatnonzero(count > k)
        w = weights[live, k].reshape((-1,) + (1,) * (src.ndim - 1))
        out[live] = out[live] + src[left[live] + k] * w
    return out


def resize_half(img, tp=None):
    """(2W, 2W, 4) uint8 -> (W, W, 4) uint8: vertical pass (rows), then horizontal pass (columns), clamp, round."""
    W = img.shape[0] // 2
    left, count, weights = tp if tp is not None else taps(W)
    mid = _pass(img.astype(F32), left, count, weights)                  # (W rows, 2W columns, 4), unclamped
    out = _pass(np.swapaxes(mid, 0, 1), left, count, weights)            # (W columns, W rows, 4)
    t = np.swapaxes(out, 0, 1)
    t = np.where(t < F32(0), F32(0), np.where(t > F32(255), F32(255), t))
    r = np.trunc(t)
    r = r + (t - r >= F32(0.5)).astype(F32)                             # half away from zero (t >= 0 here)
    return r.astype(np.uint8)


def background(name):
    return np.array(X.WHITE if name == "white" else X.TRANSPARENT, dtype=np.uint8)


def build_parent(children, W, bg):
    """children: 4 images or None (child c = index (parent << 2) + c); rows top to bottom."""
    big = np.empty((2 * W, 2 * W, 4), np.uint8)
    big[:] = bg
    for c, x0, y0 in ((1, 0, 0), (0, 0, W), (3, W, 0), (2, W, W)):
        if children[c] is not None:
            big[y0:y0 + W, x0:x0 + W] = children[c]
    return big


def parent_levels(leaf_index, deepest, root_level):
    """create_non_leaf_nodes: [(level, sorted parent indices)] from deepest - 1 up to root_level."""
    out, cur = [], sorted(set(int(i) for i in leaf_index))
    for level in range(deepest - 1, root_level - 1, -1):
        if not cur:
            break
        cur = sorted(set(i >> 2 for i in cur))
        out.append((level, cur))
    return out


def node_list(leaf_index, deepest, root_level):
    """pcv_xray_nodes' order: the leaves as given, then each parent level ascending."""
    nodes = [(deepest, int(i)) for i in leaf_index]
    for level, idx in parent_levels(leaf_index, deepest, root_level):
        nodes += [(level, i) for i in idx]
    return nodes


def pyramid(leaves, deepest, root_level, W, bg_name):
    """leaves: {leaf index: image}. Returns {(level, index): image} for leaves and every parent, and the children
    count of each parent."""
    bg = background(bg_name)
    tp = taps(W)
    imgs = {(deepest, int(i)): im for i, im in leaves.items()}
    nchildren = {}
    for level, idx in parent_levels(list(leaves), deepest, root_level):
        for p in idx:
            ch = [imgs.get((level + 1, (p << 2) + c)) for c in range(4)]
            nchildren[(level, p)] = sum(c is not None for c in ch)
            imgs[(level, p)] = resize_half(build_parent(ch, W, bg), tp)
    return imgs, nchildren


# ---- PNG reader --------------------------------------------------------------------------------------------------------
def read_png(data, stats=None):
    """RGBA8 PNG -> (h, w, 4) uint8. Checks the signature, every chunk CRC, colour type 6 / depth 8, the zlib stream
    (stored blocks parsed here, and zlib's own inflate with its Adler-32 check must agree) and filter byte 0 on every row."""
    assert data[:8] == b"\x89PNG\r\n\x1a\n", "signature"
    pos, ihdr, idat, chunks = 8, None, b"", []
    while pos < len(data):
        (n,) = struct.unpack(">I", data[pos:pos + 4])
        typ, body = data[pos + 4:pos + 8], data[pos + 8:pos + 8 + n]
        (crc,) = struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])
        assert zlib.crc32(typ + body) & 0xffffffff == crc, f"CRC of {typ}"
        chunks.append(typ)
        if typ == b"IHDR":
            ihdr = struct.unpack(">IIBBBBB", body)
        elif typ == b"IDAT":
            idat += body
        pos += 12 + n
    assert chunks[0] == b"IHDR" and chunks[-1] == b"IEND" and chunks.count(b"IDAT") == 1, chunks
    w, h, depth, ctype, comp, filt, inter = ihdr
    assert (depth, ctype, comp, filt, inter) == (8, 6, 0, 0, 0), ihdr
    raw = zlib.decompress(idat)
    # the stored blocks themselves
    assert idat[0] & 0x0f == 8 and ((idat[0] << 8) | idat[1]) % 31 == 0, "zlib header"
    p, blocks, out = 2, 0, b""
    while True:
        hdr = idat[p]
        assert hdr & 0x06 == 0, "not a stored block"
        ln, nln = struct.unpack("<HH", idat[p + 1:p + 5])
        assert ln ^ 0xffff == nln
        out += idat[p + 5:p + 5 + ln]
        p += 5 + ln
        blocks += 1
        if hdr & 1:
            break
    assert out == raw and struct.unpack(">I", idat[p:p + 4])[0] == zlib.adler32(raw) & 0xffffffff and p + 4 == len(idat)
    if stats is not None:
        stats["blocks"] = blocks
    rows = np.frombuffer(raw, np.uint8).reshape(h, 1 + 4 * w)
    assert (rows[:, 0] == 0).all(), "filter byte"
    return rows[:, 1:].reshape(h, w, 4).copy()


# ---- xray_proto Meta ---------------------------------------------------------------------------------------------------
def _varint(b, p):
    v, s = 0, 0
    while True:
        c = b[p]
        p += 1
        v |= (c & 0x7f) << s
        s += 7
        if c < 0x80:
            return v, p


def _fields(b):
    p, out = 0, []
    while p < len(b):
        key, p = _varint(b, p)
        f, wt = key >> 3, key & 7
        if wt == 0:
            v, p = _varint(b, p)
        elif wt == 1:
            (v,) = struct.unpack("<d", b[p:p + 8])
            p += 8
        elif wt == 2:
            n, p = _varint(b, p)
            v = bytes(b[p:p + n])
            p += n
        else:
            raise ValueError(f"wire type {wt}")
        out.append((f, wt, v))
    return out


def decode_meta(data):
    """Meta -> dict(version, rect=(min x, min y, edge), deepest_level, tile_size, nodes=[(level, index)]); fields must
    come in number order (rust-protobuf writes them so)."""
    m = dict(version=0, rect=(0.0, 0.0, 0.0), deepest_level=0, tile_size=0, nodes=[])
    fs = _fields(data)
    assert [f for f, _, _ in fs] == sorted(f for f, _, _ in fs), "field order"
    for f, wt, v in fs:
        if f == 1:
            m["version"] = v
        elif f == 2:
            mx = my = edge = 0.0
            for g, _, u in _fields(v):
                if g == 3:
                    for h, _, d in _fields(u):
                        if h == 1:
                            mx = d
                        elif h == 2:
                            my = d
                elif g == 4:
                    edge = u
            m["rect"] = (mx, my, edge)
        elif f == 3:
            m["deepest_level"] = v
        elif f == 4:
            m["tile_size"] = v
        elif f == 5:
            lv = ix = 0
            for g, _, u in _fields(v):
                if g == 1:
                    lv = u
                elif g == 2:
                    ix = u
            m["nodes"].append((lv, ix))
    return m


def meta_file_name(root="r"):
    """get_meta_pb_path: the root id with "r" replaced by "meta", + ".pb"."""
    return "meta" + root[1:] + ".pb"


def root_rect(rect, root="r"):
    """Node::from_node_id_and_root_bounding_rect(root, rect).bounding_rect as (min x, min y, edge)."""
    level, index = X.node_id(root)
    node = ((0, 0), (rect[0], rect[1]), rect[2])
    for l in range(level - 1, -1, -1):
        node = X.get_child(node, (index >> (2 * l)) & 3)
    return (node[1][0], node[1][1], node[2])
