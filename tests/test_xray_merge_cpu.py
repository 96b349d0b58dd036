"""The host side of merge_xray_quadtrees, no GPU: pcv_png_decode against PNGs made with numpy and zlib (every block type,
filter and chunk layout an encoder may choose) and against its bad inputs, a sanitizer build of the decoder under a
stand-alone driver, the Meta reader of pcv_xray_open_dir, the rect walk-up of Node::parent, and every message of
validate_and_merge_metadata through handles opened (without a context) from hand-written directories."""
import os
import shutil
import struct
import subprocess
import zlib

import numpy as np
import pytest

import point_cloud_viewer_amd as pcv
import xray_merge_oracle as MO
import xray_pyramid_oracle as P
from point_cloud_viewer_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def random_image(w, seed, smooth=False):
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (w, w, 4), dtype=np.uint8)
    if smooth:  # long matches and a skewed alphabet: dynamic-Huffman blocks with distances
        img[w // 4:] = img[w // 4 - 1]
        img[..., 3] = 255
    return img


def decode_raw(data, capacity=None, fill=0xa5):
    """(status, w, h, buffer) of pcv_png_decode into a buffer `capacity` bytes long inside a guarded, pre-filled array."""
    lib = pcv.load_library()
    buf = np.frombuffer(bytes(data) + b"\0", dtype=np.uint8)[:len(data)]  # never a null pointer, also for no bytes
    w, h = L.C.c_uint32(), L.C.c_uint32()
    guard = 64
    out = np.full((capacity or 0) + guard, fill, dtype=np.uint8)
    rc = lib.pcv_png_decode(buf.ctypes.data, buf.size, L.C.byref(w), L.C.byref(h),
                            out.ctypes.data if capacity else None, capacity or 0)
    assert (out[capacity or 0:] == fill).all(), "written past capacity"
    return rc, w.value, h.value, out[:capacity or 0]


SIZES = [1, 7, 16, 256]


@pytest.mark.parametrize("w", SIZES)
def test_zlib_levels_and_fixed_huffman(w):
    for seed, smooth in ((w, False), (w + 1, True)):
        img = random_image(w, seed, smooth)
        for level in (0, 1, 9):
            assert np.array_equal(pcv.png_decode(MO.make_png(img, level)), img), (level, smooth)
        assert np.array_equal(pcv.png_decode(MO.make_png(img, 6, fixed=True)), img)


@pytest.mark.parametrize("w", SIZES)
def test_every_filter_and_a_mix(w):
    img = random_image(w, 10 + w, smooth=w > 7)
    for filters in ((0,), (1,), (2,), (3,), (4,), (4, 1, 3, 0, 2), (2, 4, 4, 3)):
        assert np.array_equal(pcv.png_decode(MO.make_png(img, 9, filters=filters)), img), filters


def test_split_idat_and_ancillary_chunks():
    img = random_image(16, 5, smooth=True)
    for pieces in (0, 3):  # one IDAT per byte of the stream; three pieces
        png = MO.make_png(img, 9, filters=(4, 1), idat_pieces=pieces, ancillary=True)
        assert png.count(b"IDAT") == (pieces or len(zlib.compress(MO.filter_rows(img, (4, 1)), 9)))
        assert np.array_equal(pcv.png_decode(png), img)


@pytest.mark.parametrize("w", SIZES + [129])
def test_round_trip_through_the_librarys_encoder(w):
    img = random_image(w, 20 + w)
    png = bytes(pcv.xray_png_encode(img))
    assert np.array_equal(pcv.png_decode(png), img) and np.array_equal(P.read_png(png), img)


def _status(data, capacity=4 * 16 * 16):
    rc, _, _, out = decode_raw(data, capacity)
    if rc != L.PCV_OK:
        assert (out == 0xa5).all(), "a failed decode wrote its output"
        assert pcv.load_library().pcv_host_last_error().startswith(b"png:")
    return rc


def test_bad_inputs():
    img = random_image(16, 7, smooth=True)
    good = MO.make_png(img, 9, filters=(4, 2, 1))
    assert _status(good) == L.PCV_OK and _status(good, 4 * 16 * 16 - 1) == L.PCV_E_INVALID
    at = good.index(b"IDAT")
    (n,) = struct.unpack(">I", good[at - 4:at])
    crc_at, adler_at = at + 4 + n, at + 4 + n - 4
    flipped = bytearray(good)
    flipped[crc_at] ^= 1
    assert _status(flipped) == L.PCV_E_IO
    # the Adler-32 flipped and the chunk CRC made right again: only the zlib check can see it
    body = bytearray(good[at + 4:at + 4 + n])
    body[-1] ^= 0x10
    assert adler_at == at + 4 + len(body) - 4
    bad_adler = good[:at - 4] + MO.chunk(b"IDAT", bytes(body)) + good[crc_at + 4:]
    assert _status(bad_adler) == L.PCV_E_IO and b"Adler" in pcv.load_library().pcv_host_last_error()
    for cut in range(len(good)):  # truncation at every byte
        assert _status(good[:cut]) == L.PCV_E_IO, cut
    for header in ((8, 2, 0), (16, 6, 0), (8, 6, 1)):  # RGB8, RGBA16, interlaced
        assert _status(MO.make_png(img, 9, header=header)) == L.PCV_E_INVALID, header

    def with_stream(z):
        return MO.SIGNATURE + good[8:at - 4] + MO.chunk(b"IDAT", z) + MO.chunk(b"IEND", b"")
    # a fixed-Huffman block whose first symbol is a match of length 3 at distance 1: before the start of the output.
    # bits, LSB first: BFINAL 1, BTYPE 01, length code 257 = 0000001 (7 bits, MSB first), distance code 0 = 00000
    bits = "1" + "10" + "0000001" + "00000"
    word = sum(1 << i for i, b in enumerate(bits) if b == "1")
    far = b"\x78\x01" + word.to_bytes(2, "little") + b"\0" * 8
    assert _status(with_stream(far)) == L.PCV_E_IO and b"distance" in pcv.load_library().pcv_host_last_error()
    raw = MO.filter_rows(img, (0,))
    assert _status(with_stream(zlib.compress(raw + b"\0", 9))) == L.PCV_E_IO  # longer than h * (1 + 4 w)
    assert _status(with_stream(zlib.compress(raw[:-1], 9))) == L.PCV_E_IO      # shorter
    assert _status(with_stream(zlib.compress(b"\x05" + raw[1:], 9))) == L.PCV_E_IO  # filter byte 5
    assert _status(with_stream(b"\x78\x01\x07" + b"\0" * 8)) == L.PCV_E_IO  # reserved block type 3
    assert _status(b"") == L.PCV_E_IO and _status(b"\0" * 64) == L.PCV_E_IO


def test_sanitizer_build_of_the_decoder_runs_clean(tmp_path):
    """The decoder and tests/png_decode_driver.cpp as one stand-alone program with ASan and UBSan: truncations, byte flips
    and 1 000 seeded mutations of a valid file."""
    img = random_image(16, 3, smooth=True)
    (tmp_path / "good.png").write_bytes(MO.make_png(img, 9, filters=(0, 1, 2, 3, 4), idat_pieces=3, ancillary=True))
    exe = tmp_path / "png_decode_driver"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan",  # the runtimes inside the program: nothing to preload
                           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "png_decode_driver.cpp"),
                           os.path.join(ROOT, "point_cloud_viewer_amd", "csrc", "pcv_png.cpp"), "-o", str(exe)])
    p = subprocess.run([str(exe), str(tmp_path / "good.png")], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    decodes, accepted = (int(t) for t in p.stdout.split() if t.isdigit())
    assert decodes > 1000 + 3 * len((tmp_path / "good.png").read_bytes()) and 0 < accepted < decodes


def test_sanitizer_build_of_the_meta_code_runs_clean(tmp_path):
    """csrc/pcv_xray_meta.cpp and tests/xray_meta_driver.cpp as one stand-alone program with ASan and UBSan: a Meta of 20
    nodes encoded equal to the protobuf runtime's bytes (tests/meta_proto.py) and parsed back, then every truncation and
    every single-byte change of that file and of a version-2 file with the deprecated f32 fields: each fails or gives a
    Meta inside the ranges."""
    import meta_proto
    X = meta_proto.xray_classes()
    nodes = [(i % 6, (i * 2654435761) % 4 ** (i % 6)) for i in range(20)]
    files = []
    for version in (3, 2):
        m = X["Meta"](version=version, deepest_level=5, tile_size=256)
        if version == 3:
            m.bounding_rect.min.x, m.bounding_rect.min.y, m.bounding_rect.edge_length = 0.1, -333333.25, 0.3
        else:
            r = m.bounding_rect
            r.deprecated_min.x, r.deprecated_min.y, r.deprecated_edge_length = 0.5, -1024.25, 2048.0
        for level, index in nodes:
            m.nodes.add(level=level, index=index)
        files.append(m.SerializeToString(deterministic=True))
        (tmp_path / ("v%d.pb" % version)).write_bytes(files[-1])
    # the hand-written test encoder of the directories below agrees with the runtime too
    assert files[0] == MO.encode_meta((0.1, -333333.25, 0.3), 5, 256, nodes)
    assert files[1] == MO.encode_meta((0.5, -1024.25, 2048.0), 5, 256, nodes, version=2, deprecated=True)
    exe = tmp_path / "xray_meta_driver"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan",  # the runtimes inside the program: nothing to preload
                           os.path.join(ROOT, "tests", "xray_meta_driver.cpp"),
                           os.path.join(ROOT, "point_cloud_viewer_amd", "csrc", "pcv_xray_meta.cpp"), "-o", str(exe)])
    p = subprocess.run([str(exe), str(tmp_path / "v3.pb"), str(tmp_path / "v2.pb")], capture_output=True, text=True)
    assert p.returncode == 0, (p.stdout + p.stderr)[-2000:]
    parses, accepted = (int(t) for t in p.stdout.split())
    assert parses == sum(len(f) + 1 + 255 * len(f) for f in files) and 0 < accepted < parses


# ---- directories ---------------------------------------------------------------------------------------------------
RECT = (0.1, -1e6 / 3, 0.3)


def write_part(directory, root, nodes, rect=RECT, deepest=5, tile=4, name=None, **kw):
    os.makedirs(directory, exist_ok=True)
    ids = [P.X.node_id(n) for n in nodes]
    with open(os.path.join(directory, name or P.meta_file_name(root)), "wb") as f:
        f.write(MO.encode_meta(rect, deepest, tile, ids, **kw))
    return ids


def test_meta_reader(tmp_path):
    # what the library's own writer lays out (version 3, fields in order) and a shuffled node list
    ids = write_part(tmp_path / "a", "r2", ["r213", "r2", "r21", "r20", "r211"], deepest=3, tile=16)
    (xt,) = pcv.xray_open_host(tmp_path / "a")
    assert P.decode_meta((tmp_path / "a" / "meta2.pb").read_bytes())["nodes"] == ids
    assert xt.deepest_level == 3 and xt.tile_size_px == 16 and xt.bounding_rect == RECT
    # descending level, then ascending index
    assert xt.node_ids == ["r211", "r213", "r20", "r21", "r2"] and xt.leaf_ids == ["r211", "r213"] and xt.num_created == 2
    assert pcv.xray_merge_check([xt])[0] == 1
    for call in (xt.images, xt.build_parents):
        with pytest.raises(pcv.PcvError, match="PCV_E_INVALID"):
            call()
    with pytest.raises(pcv.PcvError, match="PCV_E_IO"):  # no PNG in the directory
        xt.node_images(0, 1)
    # version 2: the deprecated f32 min and edge, widened
    write_part(tmp_path / "v2", "r", ["r"], rect=(0.1, -7.3, 0.3), version=2, deprecated=True)
    (v2,) = pcv.xray_open_host(tmp_path / "v2")
    assert v2.bounding_rect == tuple(float(np.float32(v)) for v in (0.1, -7.3, 0.3))
    # version 2 that already carries the f64 fields takes those
    write_part(tmp_path / "v2d", "r", ["r"], version=2)
    assert pcv.xray_open_host(tmp_path / "v2d")[0].bounding_rect == RECT
    for bad, body in (("v4", MO.encode_meta(RECT, 5, 4, [(0, 0)], version=4)), ("garbage", b"\xff" * 40),
                      ("cut", MO.encode_meta(RECT, 5, 4, [(2, 7)])[:-1]), ("outside", MO.encode_meta(RECT, 5, 4, [(1, 4)]))):
        os.makedirs(tmp_path / bad)
        (tmp_path / bad / "meta.pb").write_bytes(body)
        with pytest.raises(pcv.PcvError, match="PCV_E_INVALID"):
            pcv.xray_open_host(tmp_path / bad)
    # several meta files: ascending file name order; a directory without any: nothing
    for root in ("r3", "r0", "r12"):
        write_part(tmp_path / "many", root, [root])
    assert [x.node_ids for x in pcv.xray_open_host(tmp_path / "many")] == [["r0"], ["r12"], ["r3"]]
    os.makedirs(tmp_path / "none")
    assert pcv.xray_open_host(tmp_path / "none") == []
    with pytest.raises(pcv.PcvError, match="PCV_E_IO"):
        pcv.xray_open_host(tmp_path / "missing")


def test_a_tile_of_another_size_and_a_corrupt_tile(tmp_path):
    write_part(tmp_path, "r1", ["r1", "r10"], deepest=2, tile=4)
    img = random_image(4, 1)
    (tmp_path / "r10.png").write_bytes(MO.make_png(img, 9, filters=(4,)))
    (tmp_path / "r1.png").write_bytes(MO.make_png(random_image(7, 1), 9))
    (xt,) = pcv.xray_open_host(tmp_path)
    assert np.array_equal(xt.node_images(0, 1)[0], img)
    with pytest.raises(pcv.PcvError, match="PCV_E_INVALID.*7 x 7"):
        xt.node_images(1, 1)
    (tmp_path / "r1.png").write_bytes(MO.make_png(img, 9)[:-20])
    with pytest.raises(pcv.PcvError, match="PCV_E_IO"):
        xt.node_images(1, 1)
    with pytest.raises(pcv.PcvError, match="PCV_E_INVALID"):
        xt.node_images(1, 2)


@pytest.mark.parametrize("level", [1, 2, 3, 4, 5])
def test_rect_walk_up_is_node_parent_bit_for_bit(tmp_path, level):
    rng = np.random.default_rng(level)
    for k in range(8):
        index = int(rng.integers(0, 4 ** level)) if k else 4 ** level - 1
        root = P.X.node_name(level, index)
        d = tmp_path / f"{k}"
        write_part(d, root, [root])
        got_level, got = pcv.xray_merge_check(pcv.xray_open_host(d))
        want = MO.merged_rect(level, index, RECT)
        assert got_level == level
        assert struct.pack("<3d", *got) == struct.pack("<3d", *want), (root, got, want)
        assert got[2] == 0.3 * 2 ** level


def test_validation_messages(tmp_path):
    def parts(*specs):
        shutil.rmtree(tmp_path / "d", ignore_errors=True)
        for k, (root, nodes, kw) in enumerate(specs):
            write_part(tmp_path / "d", root, nodes, name=f"meta_{k}.pb", **kw)
        return pcv.xray_open_host(tmp_path / "d")

    def refused(ps, message):
        with pytest.raises(pcv.PcvError) as e:
            pcv.xray_merge_check(ps)
        assert e.value.code == L.PCV_E_INVALID and message in str(e.value), str(e.value)

    refused([], "No subquadtrees meta files found.")
    refused(parts(("r0", [], {}), ("r1", [], {})), "All subquadtress are empty.")
    refused(parts(("r0", ["r0", "r00"], {}), ("r0", ["r0", "r01"], {})), "Not all roots are unique.")
    refused(parts(("r0", ["r0"], {}), ("r12", ["r12"], {})), "Not all roots have the same level.")
    refused(parts(("r0", ["r0"], {}), ("r1", ["r1"], dict(deepest=4))), "Not all meta files have the same deepest level.")
    refused(parts(("r0", ["r0"], {}), ("r1", ["r1"], dict(tile=8))), "Not all meta files have the same tile size.")
    # an empty part is skipped for the roots, but its deepest_level and tile_size still count
    refused(parts(("r0", ["r0"], {}), ("r1", [], dict(deepest=4))), "Not all meta files have the same deepest level.")
    refused(parts(("r0", ["r0"], {}), ("r1", [], dict(tile=8))), "Not all meta files have the same tile size.")
    refused(parts(("r0", ["r00", "r01"], {})), "root is not defined")
    ok = parts(("r2", [], {}), ("r1", ["r1", "r13"], {}), ("r0", ["r0"], {}))
    level, rect = pcv.xray_merge_check(ok)
    assert level == 1 and rect == MO.merged_rect(1, 1, RECT)  # the first non-empty part in argument order
    assert pcv.xray_merge_check(ok[::-1])[1] == MO.merged_rect(1, 0, RECT)
    assert pcv.xray_merge_check(parts(("r", ["r", "r3"], {}))) == (0, RECT)  # L == 0
