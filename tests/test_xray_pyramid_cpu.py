"""Host-only parts of xray's parent levels against tests/xray_pyramid_oracle.py: the 2:1 Lanczos3 taps bit for bit, the
resize's invariants, the PNG encoder through an independent reader, and the C example's usage line."""
import os
import subprocess

import numpy as np
import pytest

import point_cloud_viewer_amd as pcv
import xray_pyramid_oracle as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [1, 2, 3, 5, 6, 7, 16, 33, 64, 256]


@pytest.mark.parametrize("W", SIZES)
def test_lanczos_taps_equal_the_restatement_bit_for_bit(W):
    left, count, w = pcv.xray_lanczos_taps(W)
    wl, wc, ww = P.taps(W)
    assert np.array_equal(left, wl) and np.array_equal(count, wc)
    assert np.array_equal(w.view(np.uint32), ww.view(np.uint32))
    assert count.max() <= 12 and (count >= min(2 * W, 2)).all()
    if W == 1:
        assert list(left) == [0] and list(count) == [2] and w[0, 0] == w[0, 1] == np.float32(0.5)


@pytest.mark.parametrize("W", [16, 33, 64, 256])
def test_interior_taps_are_shared_and_mirror_symmetric(W):
    left, count, w = pcv.xray_lanczos_taps(W)
    interior = range(3, W - 3)
    assert all(count[o] == 12 for o in interior) and all(count[o] < 12 for o in (0, 1, 2, W - 3, W - 2, W - 1))
    for o in interior:
        assert left[o] == 2 * o - 5
        assert np.array_equal(w[o].view(np.uint32), w[3].view(np.uint32)), o
    assert np.array_equal(w[3], w[3][::-1])
    # the edges mirror each other: output o from the left is output W - 1 - o from the right, taps reversed (equal up to
    # the order of the normalising sum)
    for o in range(3):
        c = count[o]
        assert count[W - 1 - o] == c and np.allclose(w[o, :c], w[W - 1 - o, :c][::-1], rtol=0, atol=1e-7), o
    s = np.float32(0)
    for v in w[3]:
        s = np.float32(s + v)
    assert abs(float(s) - 1.0) < 1e-6


@pytest.mark.parametrize("W", [1, 2, 7, 33])
def test_constant_image_resizes_to_itself(W):
    tp = pcv.xray_lanczos_taps(W)
    for c in ((0, 0, 0, 0), (255, 255, 255, 255), (255, 255, 255, 0), (17, 128, 254, 1), (200, 3, 99, 255)):
        img = np.empty((2 * W, 2 * W, 4), np.uint8)
        img[:] = c
        out = P.resize_half(img, (tp[0].astype(np.int64), tp[1].astype(np.int64), tp[2]))
        assert out.shape == (W, W, 4) and (out == np.array(c, np.uint8)).all(), (W, c)


def test_resize_halves_a_checkerboard_to_grey_and_keeps_edges():
    W = 16
    img = np.zeros((2 * W, 2 * W, 4), np.uint8)
    img[..., 3] = 255
    img[::2, ::2, :3] = 255
    img[1::2, 1::2, :3] = 255
    out = P.resize_half(img)
    assert (out[3:-3, 3:-3, :3].astype(int) - 128).__abs__().max() <= 1 and (out[..., 3] == 255).all()


@pytest.mark.parametrize("shape", [(1, 1), (3, 2), (64, 64), (100, 200), (300, 300)])
def test_png_round_trip(shape):
    h, w = shape
    rng = np.random.default_rng(h * 1000 + w)
    img = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    data = pcv.xray_png_encode(img)
    stats = {}
    got = P.read_png(data, stats)
    assert np.array_equal(got, img)
    scan = h * (1 + 4 * w)
    assert stats["blocks"] == (scan + 65534) // 65535
    if scan > 65535:
        assert stats["blocks"] >= 2
    # the size the encoder reports is what it writes
    lib = pcv.load_library()
    import ctypes as C
    need = C.c_uint64()
    assert lib.pcv_xray_png_encode(img.ctypes.data, w, h, None, 0, C.byref(need)) == pcv.PCV_OK and need.value == len(data)
    small = np.zeros(len(data) - 1, np.uint8)  # too small: nothing written
    assert lib.pcv_xray_png_encode(img.ctypes.data, w, h, small.ctypes.data, small.nbytes, C.byref(need)) == pcv.PCV_OK
    assert not small.any()


def test_png_and_taps_refuse_bad_sizes():
    import ctypes as C
    lib = pcv.load_library()
    need = C.c_uint64()
    px = np.zeros(4, np.uint8)
    assert lib.pcv_xray_png_encode(px.ctypes.data, 0, 1, None, 0, C.byref(need)) == pcv.PCV_E_INVALID
    assert lib.pcv_xray_png_encode(px.ctypes.data, 1, 0, None, 0, C.byref(need)) == pcv.PCV_E_INVALID
    assert lib.pcv_xray_lanczos_taps(0, None, None, None) == pcv.PCV_E_INVALID
    assert lib.pcv_xray_lanczos_taps(32769, None, None, None) == pcv.PCV_E_INVALID


def test_new_entry_points_are_bound():
    names = set(pcv._lib.exported_symbols())
    for n in ("pcv_xray_build_parents", "pcv_xray_nodes", "pcv_xray_node_images", "pcv_xray_write_dir", "pcv_xray_lanczos_taps",
              "pcv_xray_png_encode"):
        assert n in names and getattr(pcv.load_library(), n)


def test_oracle_parent_sets_and_assembly():
    # create_non_leaf_nodes: leaves r000, r003, r330 under r -> r00, r33 -> r0, r3 -> r
    leaves = [int("000", 4), int("003", 4), int("330", 4)]
    assert P.parent_levels(leaves, 3, 0) == [(2, [0, int("33", 4)]), (1, [0, 3]), (0, [0])]
    assert P.parent_levels(leaves, 3, 3) == [] and P.parent_levels([], 3, 0) == []
    W = 2
    kids = [np.full((W, W, 4), c, np.uint8) for c in (10, 20, 30, 40)]
    big = P.build_parent([kids[0], kids[1], None, kids[3]], W, P.background("transparent"))
    assert (big[:W, :W] == 20).all() and (big[W:, :W] == 10).all() and (big[:W, W:] == 40).all()
    assert (big[W:, W:] == np.array([255, 255, 255, 0], np.uint8)).all()
    assert P.meta_file_name("r") == "meta.pb" and P.meta_file_name("r01") == "meta01.pb"


def test_build_xray_quadtree_example_prints_usage():
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "examples")])
    p = subprocess.run([os.path.join(ROOT, "examples", "bin", "build_xray_quadtree")], capture_output=True, text=True)
    assert p.returncode == 2 and "usage" in p.stderr
