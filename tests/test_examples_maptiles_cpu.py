"""examples/build_map_tiles.c: it compiles as C11 against the header and links the in-tree library, --help lists its options,
bad arguments end with exit status 2 and the usage text, and the structs have the layout the ctypes mirror assumes."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EX = os.path.join(ROOT, "examples")
OPTIONS = ["--output-directory", "--zoom", "--min-zoom", "--png", "--background"]


@pytest.fixture(scope="module")
def exe():
    subprocess.check_call(["make", "-s", "-C", EX, "bin/build_map_tiles"])
    return os.path.join(EX, "bin", "build_map_tiles")


def test_help_lists_every_option(exe):
    p = subprocess.run([exe, "--help"], capture_output=True, text=True)
    assert p.returncode == 0 and p.stderr == ""
    assert p.stdout.startswith("usage: build_map_tiles <cloud dir> --output-directory D --zoom Z [--min-zoom A] [--png stored|deflate]")
    for option in OPTIONS:
        assert option in p.stdout, option


@pytest.mark.parametrize("args", [
    [],                                                                        # nothing
    ["cloud"],                                                                 # no output, no zoom
    ["cloud", "--output-directory", "out"],                                    # no zoom
    ["cloud", "--zoom", "20"],                                                 # no output
    ["cloud", "--output-directory", "out", "--zoom", "24"],
    ["cloud", "--output-directory", "out", "--zoom", "x"],
    ["cloud", "--output-directory", "out", "--zoom", "12", "--min-zoom", "13"],  # the library's own rule: min_zoom <= zoom
    ["cloud", "--output-directory", "out", "--zoom", "12", "--png", "gzip"],
    ["cloud", "--output-directory", "out", "--zoom", "12", "--background", "1,2,3"],
    ["cloud", "--output-directory", "out", "--zoom", "12", "--background", "1,2,3,256"],
    ["cloud", "--output-directory", "out", "--zoom", "12", "--frobnicate"],
    ["cloud", "other", "--output-directory", "out", "--zoom", "12"],           # two directories
])
def test_bad_arguments_end_with_status_2(exe, args, tmp_path):
    p = subprocess.run([exe] + args, capture_output=True, text=True, cwd=tmp_path)
    assert p.returncode == 2 and "usage" in p.stderr, p.stderr
    assert os.listdir(tmp_path) == []


def test_a_directory_without_meta_is_an_error_not_a_usage_mistake(exe, tmp_path):
    p = subprocess.run([exe, str(tmp_path), "--output-directory", str(tmp_path / "out"), "--zoom", "20", "--min-zoom", "12", "--png", "deflate",
                        "--background", "255,255,255,255"], capture_output=True, text=True)
    assert p.returncode == 1 and "meta.pb" in p.stderr and os.listdir(tmp_path) == []


def test_struct_layouts():
    from point_cloud_viewer_amd import _lib as L
    assert C.sizeof(L.MapTilesParams) == 32 and L.MapTilesParams.max_tiles.offset == 8 and L.MapTilesParams.staging_points.offset == 24
    assert C.sizeof(L.MapTilesInfo) == 240 and L.MapTilesInfo.zoom.offset == 32 and L.MapTilesInfo.finished.offset == 40
    assert L.MapTilesInfo.tiles.offset == 48
