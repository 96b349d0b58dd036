"""Host-side checks of the multi-octree xray run (pcv_xray_run_many): the header's bound and the ctypes table agree, the
Python entry refuses an empty list before any library call, and the oracle's union box follows Aabb::grow in list order."""
import os
import re

import pytest

import point_cloud_viewer_amd as pcv
import xray_many_oracle as M
from point_cloud_viewer_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_bound_and_signature():
    header = open(os.path.join(ROOT, "include", "pcv_hip.h")).read()
    bound = int(re.search(r"#define PCV_XRAY_MAX_TREES (\d+)", header).group(1))
    assert bound == _lib.XRAY_MAX_TREES >= 1024
    assert re.search(r"int pcv_xray_run_many\(pcv_ctx\* ctx, pcv_octree\* const\* trees, uint32_t num_trees,", header)
    assert len(_lib._SIGNATURES["pcv_xray_run_many"][1]) == 5


def test_empty_list_raises_before_the_library():
    class NoLib:
        def __getattr__(self, name):
            raise AssertionError(f"library called: {name}")

    ctx = object.__new__(pcv.Context)  # no device: any library call would fail the test
    ctx.lib, ctx.handle = NoLib(), None
    with pytest.raises(ValueError):
        pcv.Context.xray_tiles(ctx, [], 256, 0.1)
    with pytest.raises(ValueError):
        pcv.Context.xray_quadtree(ctx, iter(()), 256, 0.1)


def test_union_box_grows_in_list_order():
    class Box:
        def __init__(self, lo, hi):
            self.bmin, self.bmax = lo, hi

    a = Box((0.0, 0.0, 0.0), (10.0, 10.0, 10.0))
    b = Box((-5.0, 2.0, 3.0), (4.0, 20.0, 5.0))
    c = Box((1.0, -7.0, -1.0), (30.0, 1.0, 2.0))
    assert M.union_box([a]) == ((0.0, 0.0, 0.0), (10.0, 10.0, 10.0))
    assert M.union_box([a, b, c]) == ((-5.0, -7.0, -1.0), (30.0, 20.0, 10.0))
    assert M.union_box([c, b, a]) == M.union_box([a, b, c]) == M.union_box([b, b, a, c])
