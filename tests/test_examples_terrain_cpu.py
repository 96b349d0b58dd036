"""examples/build_terrain.c: it compiles as C11 against the header and links the in-tree library, --help lists its options,
bad arguments end with exit status 2 and the usage text, and the structs have the layout the ctypes mirror assumes."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EX = os.path.join(ROOT, "examples")
OPTIONS = ["--output-directory", "--resolution", "--tile-size", "--statistic", "--min-points", "--terrain-from-world", "--origin"]


@pytest.fixture(scope="module")
def exe():
    subprocess.check_call(["make", "-s", "-C", EX, "bin/build_terrain"])
    return os.path.join(EX, "bin", "build_terrain")


def test_help_lists_every_option(exe):
    p = subprocess.run([exe, "--help"], capture_output=True, text=True)
    assert p.returncode == 0 and p.stderr == ""
    assert p.stdout.startswith("usage: build_terrain <cloud dir> --output-directory D --resolution R [--tile-size T] [--statistic max|min|mean]")
    for option in OPTIONS:
        assert option in p.stdout, option


@pytest.mark.parametrize("args", [
    [],                                                                        # nothing
    ["cloud"],                                                                 # no output, no resolution
    ["cloud", "--output-directory", "out"],                                    # no resolution
    ["cloud", "--resolution", "0.5"],                                          # no output
    ["cloud", "--output-directory", "out", "--resolution", "0"],               # the library's own rule: > 0
    ["cloud", "--output-directory", "out", "--resolution", "x"],               # no number
    ["cloud", "--output-directory", "out", "--resolution", "1", "--tile-size", "4097"],
    ["cloud", "--output-directory", "out", "--resolution", "1", "--tile-size", "0"],
    ["cloud", "--output-directory", "out", "--resolution", "1", "--statistic", "median"],
    ["cloud", "--output-directory", "out", "--resolution", "1", "--min-points", "0"],
    ["cloud", "--output-directory", "out", "--resolution", "1", "--terrain-from-world", "0,0,0,0,0,0"],     # six numbers
    ["cloud", "--output-directory", "out", "--resolution", "1", "--terrain-from-world", "0,0,0,0,0,0.6,0.9"],  # no unit quaternion
    ["cloud", "--output-directory", "out", "--resolution", "1", "--origin", "0,0"],
    ["cloud", "--output-directory", "out", "--resolution", "1", "--frobnicate"],
    ["cloud", "other", "--output-directory", "out", "--resolution", "1"],      # two directories
])
def test_bad_arguments_end_with_status_2(exe, args, tmp_path):
    p = subprocess.run([exe] + args, capture_output=True, text=True, cwd=tmp_path)
    assert p.returncode == 2 and "usage" in p.stderr, p.stderr
    assert os.listdir(tmp_path) == []


def test_a_directory_without_meta_is_an_error_not_a_usage_mistake(exe, tmp_path):
    p = subprocess.run([exe, str(tmp_path), "--output-directory", str(tmp_path / "out"), "--resolution", "0.5",
                        "--terrain-from-world", "1,2,3,0,0,0.7071067811865476,0.7071067811865476"], capture_output=True, text=True)
    assert p.returncode == 1 and "meta.pb" in p.stderr and os.listdir(tmp_path) == []


def test_struct_layouts():
    from point_cloud_viewer_amd import _lib as L
    assert C.sizeof(L.TerrainParams) == 120 and L.TerrainParams.world_from_terrain.offset == 40 and L.TerrainParams.min_points.offset == 96
    assert C.sizeof(L.TerrainInfo) == 72 and L.TerrainInfo.pool_bytes.offset == 40 and L.TerrainInfo.finished.offset == 64
