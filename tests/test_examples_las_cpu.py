"""examples/build_from_las.c: it compiles as C11 against the header and links the in-tree library, --help lists its options,
bad arguments end with exit status 2 and the usage text, and the LAS structs have the layout the ctypes mirror assumes."""
import ctypes as C
import os
import subprocess

import pytest

import las_truth as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EX = os.path.join(ROOT, "examples")
OPTIONS = ["--octree", "--s2", "--terrain", "--map-tiles", "--resolution", "--level", "--zoom", "--classes", "--drop-withheld", "--color",
           "--attributes", "--global-from-local", "--info"]


@pytest.fixture(scope="module")
def exe():
    subprocess.check_call(["make", "-s", "-C", EX, "bin/build_from_las"])
    return os.path.join(EX, "bin", "build_from_las")


def test_help_lists_every_option(exe):
    p = subprocess.run([exe, "--help"], capture_output=True, text=True)
    assert p.returncode == 0 and p.stderr == ""
    assert p.stdout.startswith("usage: build_from_las <in.las> (--octree DIR --resolution R | --s2 DIR [--level L] | --terrain DIR --resolution R | "
                               "--map-tiles DIR --zoom Z)")
    for option in OPTIONS:
        assert option in p.stdout, option


@pytest.mark.parametrize("args", [
    [],                                                         # nothing
    ["in.las"],                                                 # no product and no --info
    ["in.las", "--octree", "out"],                              # no resolution
    ["in.las", "--octree", "out", "--resolution", "0"],
    ["in.las", "--terrain", "out", "--resolution", "x"],
    ["in.las", "--map-tiles", "out"],                           # no zoom
    ["in.las", "--map-tiles", "out", "--zoom", "24"],
    ["in.las", "--s2", "out", "--level", "31"],
    ["in.las", "--s2", "out", "--octree", "other", "--resolution", "1"],   # two products
    ["in.las", "--info", "--classes", "2,256"],
    ["in.las", "--info", "--classes", "2,,6"],
    ["in.las", "--info", "--color", "rgb32"],
    ["in.las", "--info", "--color", "1,2"],
    ["in.las", "--info", "--color", "1,2,256"],
    ["in.las", "--info", "--global-from-local", "1,2,3,0,0,0"],
    ["in.las", "--info", "--frobnicate"],
    ["in.las", "other.las", "--info"],                          # two inputs
])
def test_bad_arguments_end_with_status_2(exe, args, tmp_path):
    p = subprocess.run([exe] + args, capture_output=True, text=True, cwd=tmp_path)
    assert p.returncode == 2 and "usage" in p.stderr, p.stderr
    assert os.listdir(tmp_path) == []


def test_params_the_file_refuses_are_usage_mistakes_and_a_bad_file_is_an_error(exe, tmp_path):
    T.write_las(tmp_path / "f1.las", 2, 1, T.random_fields(1, 10))
    for args in (["--color", "rgb16"], ["--attributes", "nir"], ["--attributes", "user_data,user_data"], ["--attributes", "bogus"]):
        p = subprocess.run([exe, "f1.las", "--info"] + args, capture_output=True, text=True, cwd=tmp_path)
        assert p.returncode == 2 and "usage" in p.stderr and "LAS:" in p.stderr, p.stderr
    (tmp_path / "not.las").write_bytes(b"ply\n" + b"\0" * 400)
    p = subprocess.run([exe, "not.las", "--info"], capture_output=True, text=True, cwd=tmp_path)
    assert p.returncode == 1 and "signature" in p.stderr
    p = subprocess.run([exe, "missing.las", "--info"], capture_output=True, text=True, cwd=tmp_path)
    assert p.returncode == 1 and "missing.las" in p.stderr


def test_struct_layouts():
    from point_cloud_viewer_amd import _lib as L
    assert C.sizeof(L.LasHeader) == 72 and L.LasHeader.point_format.offset == 2 and L.LasHeader.header_size.offset == 4
    assert L.LasHeader.record_length.offset == 6 and L.LasHeader.offset_to_points.offset == 8 and L.LasHeader.num_points.offset == 16
    assert L.LasHeader.scale.offset == 24 and L.LasHeader.offset.offset == 48
    assert C.sizeof(L.LasParams) == 208 and L.LasParams.constant_color.offset == 4 and L.LasParams.drop_withheld.offset == 7
    assert L.LasParams.keep_intensity.offset == 8 and L.LasParams.piece_points.offset == 12 and L.LasParams.use_transform.offset == 16
    assert L.LasParams.num_extras.offset == 20 and L.LasParams.class_mask.offset == 24 and L.LasParams.global_from_local.offset == 56
    assert L.LasParams.extras.offset == 112
    assert C.sizeof(L.LasInfo) == 2256 and L.LasInfo.max_color.offset == 32 and L.LasInfo.num_pieces.offset == 44
    assert L.LasInfo.class_hist.offset == 48 and L.LasInfo.return_hist.offset == 2096 and L.LasInfo.flag_counts.offset == 2224
    assert C.sizeof(L.LasColumns) == 136 and L.LasColumns.color.offset == 24 and L.LasColumns.extras.offset == 40
    assert L.LAS_MAX_EXTRAS == 12 and L.LAS_RAW_PIECES == 2
