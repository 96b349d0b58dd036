"""Numpy restatement of what merge_xray_quadtrees (xray/src/bin/merge_xray_quadtrees.rs) adds to the pyramid oracle: the
bounding rect walked up with Node::parent (quadtree/src/lib.rs:100-120), an encoder of xray_proto's Meta (version 3 and the
version-2 form with the deprecated f32 fields) and a PNG writer that can do what other encoders do to a tile: zlib levels,
fixed-Huffman blocks, the five row filters, split IDAT chunks and ancillary chunks."""
import struct
import zlib

import numpy as np

SIGNATURE = b"\x89PNG\r\n\x1a\n"


# ---- Node::parent ---------------------------------------------------------------------------------------------------
def node_parent(level, index, rect):
    """Node::parent: ((level - 1, index >> 2), rect of the parent); f64 `-` and `*` in the reference's order."""
    mx, my, edge = (np.float64(v) for v in rect)
    ci = index & 3
    if ci & 1:
        my = my - edge
    if ci & 2:
        mx = mx - edge
    return level - 1, index >> 2, (mx, my, edge * np.float64(2.0))


def merged_rect(level, index, rect):
    """validate_and_merge_metadata :162-169: the first root's rect under Node::parent until the root."""
    while level > 0:
        level, index, rect = node_parent(level, index, rect)
    return tuple(float(v) for v in rect)


# ---- xray_proto Meta ------------------------------------------------------------------------------------------------
def _varint(v):
    out = b""
    while v >= 0x80:
        out += bytes([(v & 0x7f) | 0x80])
        v >>= 7
    return out + bytes([v])


def _ld(field, body):
    return _varint(field << 3 | 2) + _varint(len(body)) + body


def encode_meta(rect, deepest_level, tile_size, nodes, version=3, deprecated=False):
    """Meta as rust-protobuf writes it; deprecated=True: Rect with deprecated_min (Vector2f, field 1) and
    deprecated_edge_length (float, field 2) only, as a version-2 writer did."""
    if deprecated:
        vec = _varint(1 << 3 | 5) + struct.pack("<f", rect[0]) + _varint(2 << 3 | 5) + struct.pack("<f", rect[1])
        r = _ld(1, vec) + _varint(2 << 3 | 5) + struct.pack("<f", rect[2])
    else:
        vec = _varint(1 << 3 | 1) + struct.pack("<d", rect[0]) + _varint(2 << 3 | 1) + struct.pack("<d", rect[1])
        r = _ld(3, vec) + _varint(4 << 3 | 1) + struct.pack("<d", rect[2])
    out = _varint(1 << 3) + _varint(version) + _ld(2, r) + _varint(3 << 3) + _varint(deepest_level) + _varint(4 << 3) + _varint(tile_size)
    for level, index in nodes:
        body = (_varint(1 << 3) + _varint(level) if level else b"") + (_varint(2 << 3) + _varint(index) if index else b"")
        out += _ld(5, body)
    return out


# ---- PNG writer -----------------------------------------------------------------------------------------------------
def chunk(kind, body):
    return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body) & 0xffffffff)


def _paeth(a, b, c):
    p = a + b - c
    pa, pb, pc = np.abs(p - a), np.abs(p - b), np.abs(p - c)
    return np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, b, c))


def filter_rows(img, filters):
    """Scanlines of an (h, w, 4) uint8 image, row y filtered with filters[y % len(filters)] (RFC 2083 6)."""
    h, w, _ = img.shape
    rows = img.reshape(h, 4 * w).astype(np.int64)
    out = bytearray()
    zero = np.zeros(4 * w, np.int64)
    for y in range(h):
        f = filters[y % len(filters)]
        cur, up = rows[y], rows[y - 1] if y else zero
        left = np.concatenate([zero[:4], cur[:-4]])
        upleft = np.concatenate([zero[:4], up[:-4]])
        if f == 0:
            line = cur
        elif f == 1:
            line = cur - left
        elif f == 2:
            line = cur - up
        elif f == 3:
            line = cur - (left + up) // 2
        else:
            line = cur - _paeth(left, up, upleft)
        out += bytes([f]) + (line & 255).astype(np.uint8).tobytes()
    return bytes(out)


def make_png(img, level=6, filters=(0,), fixed=False, idat_pieces=1, ancillary=False, header=None):
    """An RGBA8 PNG of img. fixed: deflate forced to fixed-Huffman blocks (Z_FIXED); idat_pieces: the zlib stream split into
    that many IDAT chunks (0: one chunk per byte); ancillary: gAMA, tEXt and tIME chunks around the data; header:
    (depth, colour type, interlace) to lie in IHDR."""
    h, w, _ = img.shape
    raw = filter_rows(img, filters)
    if fixed:
        co = zlib.compressobj(level, zlib.DEFLATED, 15, 8, zlib.Z_FIXED)
        z = co.compress(raw) + co.flush()
    else:
        z = zlib.compress(raw, level)
    depth, ctype, interlace = header or (8, 6, 0)
    out = SIGNATURE + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, ctype, 0, 0, interlace))
    if ancillary:
        out += chunk(b"gAMA", struct.pack(">I", 45455)) + chunk(b"tEXt", b"Software\0xray")
    n = len(z) if idat_pieces == 0 else idat_pieces
    cuts = [len(z) * k // n for k in range(n + 1)]
    for a, b in zip(cuts[:-1], cuts[1:]):
        out += chunk(b"IDAT", z[a:b])
    if ancillary:
        out += chunk(b"tIME", struct.pack(">HBBBBB", 2020, 1, 2, 3, 4, 5))
    return out + chunk(b"IEND", b"")
