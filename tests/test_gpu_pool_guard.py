"""Every product once under the pool's guard (pcv_ctx_set_pool_guard, DESIGN "The pool's contract"): the device pool hands
out blocks that hold 0x00, then 0x01, then 0x4B in every byte and stand between two fences of canary bytes. A product whose
bytes change with the fill reads memory it did not write; a damaged fence is a store past the end of a request. The cases are
in pool_guard_cases.py; each asserts against the truth of the subsystem's own GPU test.

Why these fills, in this order: zero exposes tables that need all ones and stale data that happened to be right; 0x01 is
non-zero but small, in case a value is used as a count or an index; 0x4B4B4B4B is large as a u32, 1.3e7 as an f32 and 3e54 as
an f64, so a sum that starts from it is visibly wrong. A case stops at the first fill that changes its bytes."""
import numpy as np
import pytest

import point_cloud_viewer_amd as pcv
from point_cloud_viewer_amd import _lib as L
from pool_guard_cases import CASES

pytestmark = pytest.mark.gpu
FILLS = (0x00, 0x01, 0x4B)


def back_fence_last(nbytes):
    """The last byte of the back fence of a fresh block: the request rounded up to 256, and 256 more."""
    return (nbytes + 255) // 256 * 256 + 256 - 1


@pytest.mark.parametrize("nbytes", [1, 256, 100_003])
def test_selftest_reports_every_planted_byte_and_nothing_else(nbytes):
    ctx = pcv.Context(0)
    try:
        for fill in FILLS:
            for offset in (nbytes, back_fence_last(nbytes), -1, -256):
                ctx.set_pool_guard(2, fill)  # (resets the report and the serial numbers)
                ctx.pool_guard_selftest(nbytes, offset)
                rep = ctx.pool_guard_report()
                assert rep == {"checked": 2, "damaged": 1, "bytes": nbytes, "serial": 2, "offset": offset}, (fill, offset, rep)
                assert ctx.pool_stats()[0] == 0
            # the caller's own last byte is no fence
            ctx.set_pool_guard(2, fill)
            ctx.pool_guard_selftest(nbytes, nbytes - 1)
            rep = ctx.pool_guard_report()
            assert rep["checked"] == 2 and rep["damaged"] == 0, rep
        with pytest.raises(pcv.PcvError) as e:  # outside the block: refused, nothing is written
            ctx.set_pool_guard(2, 0)
            ctx.pool_guard_selftest(nbytes, back_fence_last(nbytes) + 1)
        assert e.value.code == L.PCV_E_INVALID
        ctx.set_pool_guard(1, 0x4B)
        with pytest.raises(pcv.PcvError):
            ctx.pool_guard_selftest(nbytes, 0)  # no fences in mode 1
        ctx.set_pool_guard(0)
    finally:
        ctx.close()


def test_a_clean_build_reports_zero_and_the_guard_needs_an_empty_pool():
    ctx = pcv.Context(0)
    try:
        ctx.set_pool_guard(2, 0x4B)
        x = np.linspace(0.0, 1.0, 1000)
        rgb = np.zeros((1000, 3), np.uint8)
        tree = ctx.build(0.001, pcv.Aabb([0, 0, 0], [1, 1, 1]), x, x, x, rgb)
        live = ctx.pool_stats()[0]
        assert live > 0
        for mode in (0, 1, 2):
            with pytest.raises(pcv.PcvError, match="live") as e:
                ctx.set_pool_guard(mode, 0)
            assert e.value.code == L.PCV_E_INVALID
        scratch = ctx.pool_guard_report()["checked"]  # the build's scratch blocks, scanned as they were released
        ctx.pool_guard_check()
        live_blocks = ctx.pool_guard_report()["checked"] - scratch
        assert scratch > 0 and live_blocks > 0  # the tree's blobs, scanned while they live
        tree.free()
        rep = ctx.pool_guard_report()
        assert rep["damaged"] == 0 and rep["checked"] == scratch + 2 * live_blocks and ctx.pool_stats()[0] == 0, rep
        # off again: the same build takes what it took before the guard
        ctx.set_pool_guard(0)
        tree = ctx.build(0.001, pcv.Aabb([0, 0, 0], [1, 1, 1]), x, x, x, rgb)
        assert 0 < ctx.pool_stats()[0] < live
        tree.free()
        assert ctx.pool_guard_report()["checked"] == 0
        with pytest.raises(pcv.PcvError):
            ctx.pool_guard_check()
        with pytest.raises(pcv.PcvError):
            ctx.set_pool_guard(3, 0)
    finally:
        ctx.close()


@pytest.mark.parametrize("name", list(CASES))
def test_product_under_the_guard(name, tmp_path):
    for fill in FILLS:
        ctx = pcv.Context(0)  # one context at a time
        try:
            start = ctx.pool_stats()[0]
            ctx.set_pool_guard(2, fill)
            scratch = tmp_path / ("fill_%02x" % fill)
            scratch.mkdir()
            held = CASES[name](ctx, scratch)
            ctx.pool_guard_check()
            for h in held:
                h.free()
            held = None
            for child in sorted(ctx._children, key=lambda c: 0 if isinstance(c, pcv.octree.QueryBatch) else 1):
                child.free()  # what a helper of the case made and kept to itself (batches before the clouds they read)
            rep = ctx.pool_guard_report()
            print(f"{name} fill 0x{fill:02x}: {rep}")
            assert rep["checked"] > 0, "the case allocated nothing from the pool"
            assert rep["damaged"] == 0, f"fill 0x{fill:02x}: {rep}"
            assert ctx.pool_stats()[0] == start, "blocks of the pool are still live after the case freed what it held"
        finally:
            ctx.close()
