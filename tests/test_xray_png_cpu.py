"""Compressed xray tiles on the host, no GPU: pcv_xray_png_encode_ex in deflate mode against the plain Python restatement
of the stream (tests/xray_png_oracle.py) byte for byte, back through Python's zlib and through pcv_png_decode, the stored
mode against pcv_xray_png_encode, the capacity bound, and a sanitizer build of the encoder under a stand-alone driver."""
import os
import struct
import subprocess

import numpy as np
import pytest

import point_cloud_viewer_amd as pcv
import xray_png_oracle as PO
from point_cloud_viewer_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILES = PO.hand_made_tiles()


def encode_raw(img, mode, capacity, fill=0xa5):
    """(status, needed, buffer) of pcv_xray_png_encode_ex into `capacity` bytes inside a guarded, pre-filled array."""
    lib = pcv.load_library()
    img = np.ascontiguousarray(img)
    out = np.full(capacity + 64, fill, dtype=np.uint8)
    need = L.C.c_uint64()
    rc = lib.pcv_xray_png_encode_ex(img.ctypes.data, img.shape[1], img.shape[0], mode, out.ctypes.data if capacity else None, capacity,
                                    L.C.byref(need))
    assert (out[capacity:] == fill).all(), "written past capacity"
    return rc, need.value, out[:capacity]


@pytest.mark.parametrize("name", sorted(TILES))
def test_deflate_equals_the_oracle_and_decodes(name):
    img = TILES[name]
    want = PO.png(img)
    got = pcv.xray_png_encode(img, png="deflate")
    assert got == want, (name, len(got), len(want))
    assert np.array_equal(PO.decode(got), img)          # Python's zlib
    assert np.array_equal(pcv.png_decode(got), img)     # the project's own reader
    w = img.shape[1]
    assert len(PO.idat(got)) <= PO.stream_bound(w, w)
    assert len(got) <= pcv.load_library().pcv_xray_png_bound(w, w, L.XRAY_PNG_DEFLATE) == 57 + PO.stream_bound(w, w)


@pytest.mark.parametrize("name", ["white_1", "noise_7", "runs_16_v200", "sparse_256"])
def test_stored_mode_is_pcv_xray_png_encode(name):
    img = TILES[name]
    old = pcv.xray_png_encode(img)
    rc, need, buf = encode_raw(img, L.XRAY_PNG_STORED, len(old))
    assert rc == L.PCV_OK and need == len(old) and buf.tobytes() == old
    assert np.array_equal(PO.decode(old), img)


def test_the_hand_made_tiles_reach_what_they_are_for():
    """The oracle's own view of the tiles: every block-end bit position occurs, runs are cut at the band end, the sizes of
    the issue's table hold."""
    ends = set()
    for name, img in TILES.items():
        ends.update(PO.block_end_bits(img))
    assert ends == set(range(8)), ends
    assert len(PO.zlib_stream(TILES["white_256"])) == 2537
    f = PO.filtered(TILES["band_end_16"]).reshape(-1)
    assert (f[3 * 65 + 50:4 * 65 + 20] == 2).all() and (f[7 * 65 + 40:8 * 65 + 30] == 2).all()  # across a row end, a band end
    # cut at the band end: the first band ends with a run of 25, the second starts with one of 30 (and is not one of 55)
    first, _ = PO.band_block(f[:8 * 65].tobytes(), False)
    whole, _ = PO.band_block(f[:9 * 65].tobytes(), False)
    assert PO.zlib_stream(TILES["band_end_16"])[2:2 + len(first)] == first != whole[:len(first)]
    assert PO.band_rows(256) == 8 and PO.band_rows(2048) == 4 and PO.band_rows(8192) == 1 and PO.band_rows(1) == 8


def test_noise_fits_the_bound_and_needs_more_than_raw():
    img = np.random.default_rng(5).integers(0, 256, (64, 64, 4), dtype=np.uint8)
    z = PO.idat(pcv.xray_png_encode(img, png="deflate"))
    assert 64 * 257 < len(z) <= PO.stream_bound(64, 64)
    assert np.array_equal(pcv.png_decode(pcv.xray_png_encode(img, png="deflate")), img)


def test_needed_is_reported_and_a_short_buffer_is_left_alone():
    img = TILES["runs_16_v144"]
    want = PO.png(img)
    rc, need, _ = encode_raw(img, L.XRAY_PNG_DEFLATE, 0)
    assert rc == L.PCV_OK and need == len(want)
    rc, need, buf = encode_raw(img, L.XRAY_PNG_DEFLATE, len(want) - 1)
    assert rc == L.PCV_OK and need == len(want) and (buf == 0xa5).all()
    rc, need, buf = encode_raw(img, L.XRAY_PNG_DEFLATE, len(want))
    assert rc == L.PCV_OK and buf.tobytes() == want
    lib = pcv.load_library()
    assert lib.pcv_xray_png_encode_ex(img.ctypes.data, 16, 16, 2, None, 0, None) == L.PCV_E_INVALID
    assert lib.pcv_xray_png_encode_ex(img.ctypes.data, 0, 16, L.XRAY_PNG_DEFLATE, None, 0, None) == L.PCV_E_INVALID
    assert lib.pcv_xray_png_bound(8193, 8193, L.XRAY_PNG_DEFLATE) == 0


def test_non_square_images_follow_the_same_stream():
    rng = np.random.default_rng(9)
    for h, w in ((3, 11), (17, 5), (9, 1)):
        img = np.where(rng.random((h, w, 1)) < 0.2, rng.integers(0, 256, (h, w, 4)), 255).astype(np.uint8)
        assert pcv.xray_png_encode(img, png="deflate") == PO.png(img), (h, w)


def test_sanitizer_build_of_the_encoder_runs_clean(tmp_path):
    """The host encoder and tests/png_encode_driver.cpp as one stand-alone program with ASan and UBSan: the hand-made
    tiles and 1 000 seeded ones, both modes, exact and short buffers."""
    with open(tmp_path / "tiles.bin", "wb") as f:
        f.write(struct.pack("<I", len(TILES)))
        for name in sorted(TILES):
            f.write(struct.pack("<I", TILES[name].shape[1]) + TILES[name].tobytes())
    exe = tmp_path / "png_encode_driver"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-static-libasan", "-static-libubsan",  # the runtimes inside the program: nothing to preload
                           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "png_encode_driver.cpp"),
                           os.path.join(ROOT, "point_cloud_viewer_amd", "csrc", "pcv_png.cpp"), "-o", str(exe)])
    p = subprocess.run([str(exe), str(tmp_path / "tiles.bin")], capture_output=True, text=True)
    assert p.returncode == 0, (p.stdout + p.stderr)[-2000:]
    assert int(p.stdout.split()[0]) == 2 * (len(TILES) + 1000)
