"""CPU-side checks of the batched point query (pcv_query_batch_*): argument validation that needs no device, and the Python
wrapper's own checks before it calls the library. The ABI test picks the new symbols up from the header on its own."""
import ctypes as C

import pytest

import point_cloud_viewer_amd as pcv
from point_cloud_viewer_amd import _lib as L
from point_cloud_viewer_amd.octree import OctreeResult


def test_entry_points_reject_a_null_context_or_batch():
    lib = pcv.load_library()
    h = C.c_void_p()
    assert lib.pcv_query_batch_run(None, None, None, None, None, C.byref(h)) == L.PCV_E_INVALID
    assert h.value is None
    ns, npt = C.c_uint64(7), C.c_uint64(7)
    assert lib.pcv_query_batch_sizes(None, C.byref(ns), C.byref(npt)) == L.PCV_E_INVALID
    assert (ns.value, npt.value) == (7, 7)
    assert lib.pcv_query_batch_segments(None, None, None, None) == L.PCV_E_INVALID
    assert lib.pcv_query_batch_points(None, 0, 0, 0, L.MEM_HOST, None, None, None, None, None) == L.PCV_E_INVALID


def test_free_of_null_is_a_no_op():
    pcv.load_library().pcv_query_batch_free(None)


class _NoLibrary:
    def __getattr__(self, name):
        raise AssertionError(f"{name} called although the arguments were invalid")


class _StandInTree:
    lib = _NoLibrary()
    ctx = None
    handle = None


class _StandInShapes:
    count = 3
    handle = None


@pytest.mark.parametrize("intervals", [[], [None], [None, (0.0, 1.0)], [None] * 4])
def test_wrapper_rejects_intervals_of_the_wrong_length(intervals):
    with pytest.raises(ValueError, match="one per shape"):
        OctreeResult.query_batch(_StandInTree(), _StandInShapes(), intervals=intervals)
