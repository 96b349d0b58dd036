"""examples/build_3d_tiles.c: it compiles as C11 against the header and links the in-tree library, --help lists its options,
bad arguments end with exit status 2 and the usage text, a directory without meta.pb is an error, and the structs have the layout
the ctypes mirror assumes."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EX = os.path.join(ROOT, "examples")
OPTIONS = ["--output-directory", "--error-factor", "--position-mode", "--intensity", "--info"]


@pytest.fixture(scope="module")
def exe():
    subprocess.check_call(["make", "-s", "-C", EX, "bin/build_3d_tiles"])
    return os.path.join(EX, "bin", "build_3d_tiles")


def test_help_lists_every_option(exe):
    p = subprocess.run([exe, "--help"], capture_output=True, text=True)
    assert p.returncode == 0 and p.stderr == ""
    assert p.stdout.startswith("usage: build_3d_tiles <octree dir> --output-directory D [--error-factor F] [--position-mode auto|quantized|float]")
    for option in OPTIONS:
        assert option in p.stdout, option


@pytest.mark.parametrize("args", [
    [],                                                                     # nothing
    ["octree"],                                                             # no output
    ["--output-directory", "out"],                                          # no octree
    ["octree", "--output-directory"],                                       # an option without its value
    ["octree", "--output-directory", "out", "--error-factor", "x"],
    ["octree", "--output-directory", "out", "--error-factor", "0.5x"],
    ["octree", "--output-directory", "out", "--error-factor", "-1"],        # the library's own rule: not negative
    ["octree", "--output-directory", "out", "--error-factor", "inf"],       # ... and finite
    ["octree", "--output-directory", "out", "--position-mode", "half"],
    ["octree", "--output-directory", "out", "--position-mode"],
    ["octree", "--output-directory", "out", "--frobnicate"],
    ["octree", "other", "--output-directory", "out"],                       # two directories
    ["octree", "--output-directory", "out", "--output-directory", "out2"],
])
def test_bad_arguments_end_with_status_2(exe, args, tmp_path):
    p = subprocess.run([exe] + args, capture_output=True, text=True, cwd=tmp_path)
    assert p.returncode == 2 and "usage" in p.stderr, p.stderr
    assert os.listdir(tmp_path) == []


def test_a_directory_without_meta_is_an_error_not_a_usage_mistake(exe, tmp_path):
    p = subprocess.run([exe, str(tmp_path), "--output-directory", str(tmp_path / "out"), "--error-factor", "0.25", "--position-mode", "float",
                        "--intensity", "--info"], capture_output=True, text=True)
    assert p.returncode == 1 and "meta.pb" in p.stderr and os.listdir(tmp_path) == []


def test_struct_layouts():
    from point_cloud_viewer_amd import _lib as L
    assert C.sizeof(L.Tiles3dParams) == 152 and L.Tiles3dParams.transform.offset == 8 and L.Tiles3dParams.flags.offset == 136
    assert L.Tiles3dParams.position_mode.offset == 140 and L.Tiles3dParams.chunk_bytes.offset == 144
    assert C.sizeof(L.Tiles3dInfo) == 40 and L.Tiles3dInfo.total_file_bytes.offset == 24 and L.Tiles3dInfo.chunk_points.offset == 32
    assert C.sizeof(L.Tiles3dTile) == 64 and L.Tiles3dTile.mode.offset == 16 and L.Tiles3dTile.file_bytes.offset == 24
    assert L.Tiles3dTile.feature_json_offset.offset == 32 and L.Tiles3dTile.batch_binary_offset.offset == 56
