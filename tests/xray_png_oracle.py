"""The run-length deflate stream of compressed xray tiles (PCV_XRAY_PNG_DEFLATE, include/pcv_hip.h), restated in plain
Python: filter, bands, tokens, bit packing, Adler-32 and the PNG wrapper; and a checker that reads any PNG back with
Python's zlib (an inflater this project did not write) and numpy. Also the hand-made tiles the CPU and GPU tests share."""
import struct
import zlib

import numpy as np

BAND_BYTES = 40960
MAX_EDGE = 8192
SIG = b"\x89PNG\r\n\x1a\n"

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]


def band_rows(w):
    return max(1, min(8, BAND_BYTES // (1 + 4 * w)))


def band_bound(n):
    return -(-(3 + 9 * n + 7) // 8) + 5


def stream_bound(w, h):
    r, row = band_rows(w), 1 + 4 * w
    return 2 + sum(band_bound(min(r, h - y) * row) for y in range(0, h, r)) + 4


def filtered(img):
    """(h, 1 + 4 w) u8: row 0 Sub with 4 bytes per pixel, every other row Up."""
    h, w = img.shape[:2]
    px = img.reshape(h, 4 * w).astype(np.int16)
    out = np.empty((h, 1 + 4 * w), np.uint8)
    out[0, 0] = 1
    first = px[0].copy()
    first[4:] -= px[0, :-4]
    out[0, 1:] = first.astype(np.uint8)
    out[1:, 0] = 2
    out[1:, 1:] = (px[1:] - px[:-1]).astype(np.uint8)
    return out


class Bits:
    def __init__(self):
        self.out, self.acc, self.cnt = bytearray(), 0, 0

    def put(self, value, n):  # LSB first
        self.acc |= value << self.cnt
        self.cnt += n
        while self.cnt >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.cnt -= 8

    def huff(self, code, n):  # Huffman codes go in MSB first
        self.put(int(format(code, "0%db" % n)[::-1], 2), n)

    def symbol(self, s):
        if s < 144:
            self.huff(0x30 + s, 8)
        elif s < 256:
            self.huff(0x190 + s - 144, 9)
        elif s < 280:
            self.huff(s - 256, 7)
        else:
            self.huff(0xC0 + s - 280, 8)

    def match(self, length):  # distance 1
        k = max(i for i in range(29) if LEN_BASE[i] <= length)
        self.symbol(257 + k)
        self.put(length - LEN_BASE[k], LEN_EXTRA[k])
        self.huff(0, 5)

    def pad(self):
        if self.cnt:
            self.put(0, 8 - self.cnt)


def band_block(data, last):
    """One band: fixed-Huffman block of run tokens, then the empty stored block."""
    b = Bits()
    b.put(0, 1)
    b.put(1, 2)
    n, j = len(data), 0
    while j < n:
        e = j + 1
        while e < n and data[e] == data[j]:
            e += 1
        v, r = int(data[j]), e - j - 1
        b.symbol(v)
        while r >= 3:
            m = min(r, 258)
            b.match(m)
            r -= m
        for _ in range(r):
            b.symbol(v)
        j = e
    b.symbol(256)
    block_bits = 8 * len(b.out) + b.cnt
    b.put(1 if last else 0, 1)
    b.put(0, 2)
    b.pad()
    b.out += b"\x00\x00\xff\xff"
    return bytes(b.out), block_bits


def zlib_stream(img):
    h, w = img.shape[:2]
    f = filtered(img)
    r = band_rows(w)
    out = bytearray(b"\x78\x01")
    for y in range(0, h, r):
        out += band_block(f[y:y + r].tobytes(), y + r >= h)[0]
    s1, s2 = 1, 0
    for v in f.tobytes():  # the definition, byte by byte
        s1 = (s1 + v) % 65521
        s2 = (s2 + s1) % 65521
    return bytes(out) + struct.pack(">I", s2 << 16 | s1)


def chunk(kind, body):
    return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body))


def png(img):
    h, w = img.shape[:2]
    return SIG + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 6, 0, 0, 0)) + chunk(b"IDAT", zlib_stream(img)) + chunk(b"IEND", b"")


def idat(file):
    """The concatenated IDAT payload of a PNG, every chunk CRC checked."""
    assert file[:8] == SIG
    pos, z = 8, b""
    while pos < len(file):
        n, kind = struct.unpack(">I4s", file[pos:pos + 8])
        body = file[pos + 8:pos + 8 + n]
        assert struct.unpack(">I", file[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(kind + body), kind
        if kind == b"IDAT":
            z += body
        pos += 12 + n
    assert kind == b"IEND" and pos == len(file)
    return z


def decode(file):
    """Any RGBA8 PNG -> (h, w, 4) u8 through zlib.decompress and numpy (filters 0, 1, 2 only: what this project writes)."""
    w, h, depth, colour, comp, flt, lace = struct.unpack(">IIBBBBB", file[16:29])
    assert file[12:16] == b"IHDR" and (depth, colour, comp, flt, lace) == (8, 6, 0, 0, 0)
    raw = np.frombuffer(zlib.decompress(idat(file)), np.uint8)
    assert raw.size == h * (1 + 4 * w)
    rows = raw.reshape(h, 1 + 4 * w)
    out = np.zeros((h, 4 * w), np.uint8)
    for y in range(h):
        t, line = rows[y, 0], rows[y, 1:]
        if t == 0:
            out[y] = line
        elif t == 1:
            out[y] = np.cumsum(line.reshape(w, 4).astype(np.uint64), axis=0).astype(np.uint8).reshape(-1)
        elif t == 2:
            out[y] = line + (out[y - 1] if y else 0)
        else:
            raise AssertionError("filter %d" % t)
    return out.reshape(h, w, 4)


# ---- hand-made tiles ------------------------------------------------------------------------------------------------
def from_filtered(f):
    """The w x w tile whose filtered scanlines are f ((w, 1 + 4 w) u8 with the right filter bytes)."""
    w = f.shape[0]
    out = np.zeros((w, 4 * w), np.uint8)
    out[0] = np.cumsum(f[0, 1:].reshape(w, 4).astype(np.uint64), axis=0).astype(np.uint8).reshape(-1)
    for y in range(1, w):
        out[y] = f[y, 1:] + out[y - 1]
    return out.reshape(w, w, 4)


def tile_with_runs(w, runs, start_row=1, start_col=1):
    """A tile whose filtered bytes are zero except for the runs (length, value) laid one after another, separated by a
    single byte of value + 1, beginning at (start_row, start_col) of the filtered rows and skipping filter bytes."""
    f = np.zeros((w, 1 + 4 * w), np.uint8)
    f[0, 0], f[1:, 0] = 1, 2
    y, x = start_row, start_col
    for length, value in runs:
        for k in range(length + 1):
            if x == 1 + 4 * w:
                y, x = y + 1, 1
            assert y < w, "runs do not fit the tile"
            f[y, x] = value if k < length else (value + 1) & 255
            x += 1
    return from_filtered(f)


RUN_LENGTHS = [1, 2, 3, 4, 258, 259, 260, 261, 262, 517, 10, 11, 18, 19, 34, 35, 66, 67, 130, 131, 257, 258]


def hand_made_tiles():
    """name -> (w, w, 4) u8: the smallest tiles at which the stream can still go wrong."""
    t = {}
    rng = np.random.default_rng(20261018)
    for w in (1, 7, 16):
        t["white_%d" % w] = np.full((w, w, 4), 255, np.uint8)
        t["transparent_%d" % w] = np.zeros((w, w, 4), np.uint8)
        t["noise_%d" % w] = rng.integers(0, 256, (w, w, 4), dtype=np.uint8)
    t["white_256"] = np.full((256, 256, 4), 255, np.uint8)
    sparse = np.full((256, 256, 4), 255, np.uint8)
    hit = rng.random((256, 256)) < 0.02
    sparse[hit] = rng.integers(0, 256, (int(hit.sum()), 4), dtype=np.uint8)
    t["sparse_256"] = sparse
    # run lengths, each run followed by one byte of another value; values on both sides of the 8- / 9-bit literal border
    for value in (7, 143, 144, 200):
        t["runs_16_v%d" % value] = tile_with_runs(16, [(n, value) for n in RUN_LENGTHS if n < 200], start_row=0, start_col=6)
    for value in (7, 200):
        t["long_runs_64_v%d" % value] = tile_with_runs(64, [(n, value) for n in RUN_LENGTHS], start_row=0, start_col=9)
    # w = 16 (band = rows 0 .. 7, 65 bytes each). A row starts with its filter byte, so only a run of 2s goes on across a
    # row end: one does inside the band (rows 3 -> 4, one run of 15 + 1 + 19 bytes), one across the band end (rows 7 -> 8),
    # where it has to be cut; a run of 9s ends exactly at a row end
    f = np.zeros((16, 65), np.uint8)
    f[0, 0], f[1:, 0] = 1, 2
    f[3, 50:] = 2
    f[4, 1:20] = 2
    f[7, 40:] = 2
    f[8, 1:30] = 2
    f[5, 30:] = 9
    t["band_end_16"] = from_filtered(f)
    # block ends on every bit position: k extra 8-bit literals move the end of the band's block by k bits mod 8
    for k in range(8):
        f = np.zeros((7, 29), np.uint8)
        f[0, 0], f[1:, 0] = 1, 2
        f[3, 1:1 + 2 * k:2] = 5
        t["bit_end_7_%d" % k] = from_filtered(f)
    return t


def block_end_bits(img):
    """Bit position (mod 8) at which the Huffman block of each band ends."""
    f = filtered(img)
    r = band_rows(img.shape[1])
    return [band_block(f[y:y + r].tobytes(), False)[1] % 8 for y in range(0, img.shape[0], r)]
