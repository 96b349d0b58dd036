"""show_octree_nodes on the host (no GPU): pcv_render_check_overlay, and the numpy oracle of the node outlines
(tests/render_outline_oracle.py) on cases whose pixels are worked out by hand here."""
import ctypes as C

import numpy as np
import pytest

import point_cloud_viewer_amd as pcv
import render_outline_oracle as RO

F32 = np.float32
LUT = np.arange(256, dtype=np.uint8)
# x, y pass through, z is halved, w = 1: zw = z / 4 + 1 / 2 (as tests/test_render_cpu.py)
MATRIX = np.diag([1.0, 1.0, 0.5, 1.0]).ravel(order="F")


def check(overlay):
    msg = C.create_string_buffer(b"x" * 199, 200)
    rc = pcv.load_library().pcv_render_check_overlay(C.byref(overlay) if overlay is not None else None, msg, 200)
    return rc, msg.value.decode()


def test_check_overlay_accepts_what_is_defined():
    assert check(None) == (pcv.PCV_OK, "")
    assert check(pcv.render_overlay()) == (pcv.PCV_OK, "")
    assert check(pcv.render_overlay(True)) == (pcv.PCV_OK, "")
    assert check(pcv.render_overlay(True, (1, 2, 3, 4))) == (pcv.PCV_OK, "")
    o = pcv.render_overlay(True)
    assert o.flags == 1 and list(o.outline_rgba) == [255, 255, 0, 255] and C.sizeof(o) == 8
    assert pcv.render_overlay(False).flags == 0
    pcv.render_check_overlay(o)
    pcv.render_check_overlay(None)


@pytest.mark.parametrize("flags", [2, 3, 0x80000000, 0xfffffffe])
def test_check_overlay_refuses_unknown_flag_bits(flags):
    rc, msg = check(pcv.render_overlay(flags=flags))
    assert rc == pcv.PCV_E_INVALID and "unknown overlay flag" in msg and "PCV_RENDER_OUTLINE_NODES" in msg
    with pytest.raises(pcv.PcvError) as e:
        pcv.render_check_overlay(pcv.render_overlay(flags=flags))
    assert e.value.code == pcv.PCV_E_INVALID and "unknown overlay flag" in str(e.value)
    # a short buffer gets a cut, terminated message; none at all is allowed
    small = C.create_string_buffer(8)
    assert pcv.load_library().pcv_render_check_overlay(C.byref(pcv.render_overlay(flags=flags)), small, 8) == pcv.PCV_E_INVALID
    assert small.value == b"render:"
    assert pcv.load_library().pcv_render_check_overlay(C.byref(pcv.render_overlay(flags=flags)), None, 0) == pcv.PCV_E_INVALID


def test_python_refuses_a_bad_colour():
    for bad in ((1, 2, 3), (0, 0, 0, 256), (-1, 0, 0, 0)):
        with pytest.raises(pcv.PcvError):
            pcv.render_overlay(True, bad)


def node(points, colors, cube_min=(-0.5, -0.5, -0.5), cube_edge=1.0):
    """A Float64 node: position = attribute * edge + min."""
    return dict(encoding=4, xyz=np.asarray(points, "<f8").tobytes(), rgb=np.asarray(colors, np.uint8).tobytes(),
                cube_min=np.asarray(cube_min, np.float64), cube_edge=cube_edge)


def gl_pixels(pairs, W=16, H=16):
    """Image-plane mask of GL pixels (i, j): image row 0 is the top."""
    m = np.zeros((H, W), bool)
    for i, j in pairs:
        m[H - 1 - j, i] = True
    return m


# the cube [-0.5, 0.5]^3 head-on at 16 x 16: its corners are at window x, y in {4, 12}; the quad at z = -0.5 has zw = 0.375,
# the one at z = +0.5 has zw = 0.625, and both project to the same square. A horizontal edge covers the centres 4.5 .. 11.5
# of its row (4 or 12), a vertical one those of its column; the four edges along z project to a point and draw nothing.
SQUARE = ([(i, 4) for i in range(4, 12)] + [(i, 12) for i in range(4, 12)] + [(4, j) for j in range(4, 12)] + [(12, j) for j in range(4, 12)])


def test_oracle_axis_aligned_cube_head_on():
    assert len(set(SQUARE)) == 31  # (4, 4) is on two edges; (12, 12) on none: the ranges are half open
    yellow, grey = [255, 255, 0, 255], [90, 90, 90]
    out = RO.draw_nodes([node([[0.5, 0.5, 0.5]], [grey])], MATRIX, 16, 16, 1.0, LUT)
    want = gl_pixels(SQUARE)
    assert (out["image"][want] == yellow).all() and (out["depth"][want] == F32(0.375)).all()  # the nearer quad wins
    centre = gl_pixels([(7, 7)])  # the point is at window (8, 8): of the centres, 7.5 lies in [7.5, 8.5)
    assert (out["image"][centre] == grey + [255]).all() and (out["depth"][centre] == F32(0.5)).all()
    rest = ~(want | centre)
    assert (out["image"][rest] == [0, 0, 0, 255]).all() and (out["depth"][rest] == 1.0).all()
    assert out["segments_submitted"] == 12 and out["segments_drawn"] == 12 and out["outline_pixels"] == 31
    assert out["pixels_covered"] == 32 and out["points_drawn"] == 1
    # ranks: the point is 0, the outline 1
    assert out["winner"][centre][0] == 0 and (out["winner"][want] == 1).all()
    # another colour is stored as given, the gamma table does not touch it
    out = RO.draw_nodes([node([[0.5, 0.5, 0.5]], [grey])], MATRIX, 16, 16, 1.0, LUT[::-1].copy(), color=(7, 8, 9, 10))
    assert (out["image"][want] == [7, 8, 9, 10]).all() and (out["image"][centre] == [165, 165, 165, 255]).all()


def test_oracle_order_at_equal_depth():
    """A point on a cube corner has the zw of the outline fragments around it: the node's own point and an earlier node's
    point win, a later node's point loses. point_size 2: a point at window (4, 4) covers the centres 3.5 and 4.5 (at size 1
    only 3.5, beside the outline)."""
    red, green, blue = [200, 10, 10], [10, 200, 10], [10, 10, 200]
    # node A: a point on the corner (-0.5, -0.5, -0.5) -> GL pixels {3, 4} x {3, 4}, zw 0.375: (4, 4) is on the outline.
    # Node B, the same cube, drawn after A: a point on (0.5, -0.5, -0.5) -> {11, 12} x {3, 4}: (11, 4) and (12, 4) are.
    a, b = node([[0.0, 0.0, 0.0]], [red]), node([[1.0, 0.0, 0.0]], [green])
    out = RO.draw_nodes([a, b], MATRIX, 16, 16, 2.0, LUT)
    own, later, below = gl_pixels([(4, 4)]), gl_pixels([(11, 4), (12, 4)]), gl_pixels([(11, 3), (12, 3)])
    assert (out["image"][own] == red + [255]).all() and out["winner"][own][0] == 0 and out["depth"][own][0] == F32(0.375)
    assert (out["image"][later] == [255, 255, 0, 255]).all() and (out["winner"][later] == 1).all()  # A's outline (rank 1), B's point (rank 2)
    assert (out["image"][below] == green + [255]).all() and (out["depth"][later] == F32(0.375)).all()
    assert out["outline_pixels"] == 30 and out["pixels_covered"] == 31 + 3 + 2 and out["segments_submitted"] == 24
    # B first: its point now precedes A's outline and B's own; A's point comes after B's outline
    out = RO.draw_nodes([b, a], MATRIX, 16, 16, 2.0, LUT)
    assert (out["image"][later] == green + [255]).all() and (out["image"][own] == [255, 255, 0, 255]).all()
    # a point behind the outline's depth is hidden by it, one in front hides it
    far, near = node([[0.0, 0.0, 0.5]], [blue]), node([[0.0, 0.0, -1.0]], [blue])
    assert (RO.draw_nodes([far], MATRIX, 16, 16, 2.0, LUT)["image"][own] == [255, 255, 0, 255]).all()
    out = RO.draw_nodes([near], MATRIX, 16, 16, 2.0, LUT)
    assert (out["image"][own] == blue + [255]).all() and out["depth"][own][0] == F32(0.125)


def fragments(a, b, W=16, H=16):
    """Clip, window and raster of one clip-space segment: (set of GL (i, j), {(i, j): zw}) or None when it is dropped."""
    ends = RO.clip_segment(np.array(a, F32), np.array(b, F32))
    if ends is None:
        return None
    pix, zw = RO.raster(RO.window(ends[0], W, H), RO.window(ends[1], W, H), W, H)
    return {(int(p % W), H - 1 - int(p // W)): float(z) for p, z in zip(pix, zw)}


def test_oracle_edge_across_the_near_plane():
    # w + z: -2 at a, 2 at b -> t = 0.5: the clipped end is (0, 0.25, -1, 1), window (8, 10, 0); b is at window (12, 10, 1)
    ends = RO.clip_segment(np.array([-0.5, 0.25, -3.0, 1.0], F32), np.array([0.5, 0.25, 1.0, 1.0], F32))
    assert list(ends[0]) == [0.0, 0.25, -1.0, 1.0] and list(ends[1]) == [0.5, 0.25, 1.0, 1.0]
    got = fragments([-0.5, 0.25, -3.0, 1.0], [0.5, 0.25, 1.0, 1.0])
    assert got == {(8, 10): 0.125, (9, 10): 0.375, (10, 10): 0.625, (11, 10): 0.875}
    # the far plane on the other side: w - z is 2 at a', -2 at b -> the same half
    got = fragments([0.5, 0.25, -1.0, 1.0], [-0.5, 0.25, 3.0, 1.0])
    assert got == {(8, 10): 0.875, (9, 10): 0.625, (10, 10): 0.375, (11, 10): 0.125}
    # wholly in front of the near plane: dropped
    assert fragments([-0.5, 0.25, -3.0, 1.0], [0.5, 0.25, -2.0, 1.0]) is None


def test_oracle_endpoint_behind_the_eye():
    # x = 3 - 4 t, w = -1 + 4 t: w > 0 from t = 0.25, w - x = -4 + 8 t >= 0 from t = 0.5 (d0 = -4, d1 = 4), w + x = 2 throughout.
    # The clipped end is (1, 0, 0, 1): window x = 16; b is at ndc x = -1 / 3: window x = 5.33. Row 8, centres 5.5 .. 15.5.
    ends = RO.clip_segment(np.array([3.0, 0.0, 0.0, -1.0], F32), np.array([-1.0, 0.0, 0.0, 3.0], F32))
    assert list(ends[0]) == [1.0, 0.0, 0.0, 1.0] and list(ends[1]) == [-1.0, 0.0, 0.0, 3.0]
    got = fragments([3.0, 0.0, 0.0, -1.0], [-1.0, 0.0, 0.0, 3.0])
    assert got == {(i, 8): 0.5 for i in range(5, 16)}
    # straight through the eye: every plane cuts at t = 0.5, where w = 0 — no depth, so the finite-w rule drops it
    assert RO.clip_segment(np.array([0.0, 0.0, 0.0, -1.0], F32), np.array([0.0, 0.0, 0.0, 1.0], F32)) is None
    # both ends behind the eye, and a non-finite coordinate
    assert RO.clip_segment(np.array([0.0, 0.0, 0.0, -1.0], F32), np.array([0.5, 0.0, 0.0, 0.0], F32)) is None
    assert RO.clip_segment(np.array([0.0, 0.0, 0.0, 1.0], F32), np.array([np.inf, 0.0, 0.0, 1.0], F32)) is None
    assert RO.clip_segment(np.array([0.0, np.nan, 0.0, 1.0], F32), np.array([0.0, 0.0, 0.0, 1.0], F32)) is None


def test_oracle_the_major_axis_and_its_tie():
    # window (2, 2) -> (6, 6): |dx| == |dy| goes to x: centres 2.5 .. 5.5, y = the centre itself
    assert set(fragments([-0.75, -0.75, 0.0, 1.0], [-0.25, -0.25, 0.0, 1.0])) == {(2, 2), (3, 3), (4, 4), (5, 5)}
    assert set(fragments([-0.25, -0.25, 0.0, 1.0], [-0.75, -0.75, 0.0, 1.0])) == {(2, 2), (3, 3), (4, 4), (5, 5)}
    # window (2, 2) -> (5, 6): y is the major axis: rows 2 .. 5, x = 2 + 3 (j + 0.5 - 2) / 4 = 2.375, 3.125, 3.875, 4.625
    assert set(fragments([-0.75, -0.75, 0.0, 1.0], [-0.375, -0.25, 0.0, 1.0])) == {(2, 2), (3, 3), (3, 4), (4, 5)}
    # window (2, 2) -> (6, 5): x is: columns 2 .. 5, y = 2 + 3 (i + 0.5 - 2) / 4
    assert set(fragments([-0.75, -0.75, 0.0, 1.0], [-0.25, -0.375, 0.0, 1.0])) == {(2, 2), (3, 3), (4, 3), (5, 4)}
    # the minor coordinate may leave the image: window (14, 14) -> (18, 18) is cut by w - x at (16, 16); y = 16 is no row
    assert set(fragments([0.75, 0.75, 0.0, 1.0], [1.25, 1.25, 0.0, 1.0])) == {(14, 14), (15, 15)}


def test_oracle_a_segment_that_crosses_no_centre():
    # window (3.6, 3.6) -> (4.4, 3.9): no i + 0.5 in [3.6, 4.4). The segment survives the clip, and draws nothing.
    a, b = [-0.55, -0.55, 0.0, 1.0], [-0.45, -0.5125, 0.0, 1.0]
    assert RO.clip_segment(np.array(a, F32), np.array(b, F32)) is not None
    assert fragments(a, b) == {}
    # one step longer and it reaches the centre 4.5
    assert set(fragments(a, [-0.4, -0.5125, 0.0, 1.0])) == {(4, 3)}
    # a point: both ends equal
    assert fragments(a, a) == {}
