"""examples/query_to_ply.c: it compiles as C11 against the header and links the in-tree library, --help lists its options,
bad arguments end with exit status 2 and the usage text, and the params struct has the layout the ctypes mirror assumes."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EX = os.path.join(ROOT, "examples")
OPTIONS = ["--aabb", "--cells", "--map-tiles", "--all", "--filter", "--attributes", "--output", "--append", "--per-location"]


@pytest.fixture(scope="module")
def exe():
    subprocess.check_call(["make", "-s", "-C", EX, "bin/query_to_ply"])
    return os.path.join(EX, "bin", "query_to_ply")


def test_help_lists_every_option(exe):
    p = subprocess.run([exe, "--help"], capture_output=True, text=True)
    assert p.returncode == 0 and p.stderr == ""
    assert p.stdout.startswith("usage: query_to_ply <cloud dir> (--aabb x0,y0,z0,x1,y1,z1 | --cells tok,.. | --map-tiles z | --all) [--filter NAME:LO:HI]")
    for option in OPTIONS:
        assert option in p.stdout, option
    assert "NAME:LO:HI" in p.stdout and "out_%u.ply" in p.stdout


@pytest.mark.parametrize("args", [
    [],                                                             # nothing
    ["cloud"],                                                      # no location, no output
    ["cloud", "--all"],                                             # no output
    ["cloud", "--output", "o.ply"],                                 # no location
    ["cloud", "--all", "--aabb", "0,0,0,1,1,1", "--output", "o.ply"],  # two locations
    ["cloud", "--aabb", "0,0,0,1,1", "--output", "o.ply"],          # five numbers
    ["cloud", "--aabb", "0,0,0,1,1,x", "--output", "o.ply"],        # no number
    ["cloud", "--cells", "xyz", "--output", "o.ply"],               # no token
    ["cloud", "--map-tiles", "24", "--output", "o.ply"],            # zoom past 23
    ["cloud", "--all", "--filter", "intensity:1", "--output", "o.ply"],  # no interval
    ["cloud", "--all", "--output", "o.ply", "--per-location", "tile.ply"],  # no %u
    ["cloud", "--all", "--output", "o.ply", "--per-location", "tile_%u_%s.ply"],  # another conversion
    ["cloud", "--all", "--output", "o.ply", "--frobnicate"],        # unknown option
    ["cloud", "other", "--all", "--output", "o.ply"],               # two directories
])
def test_bad_arguments_end_with_status_2(exe, args, tmp_path):
    p = subprocess.run([exe] + args, capture_output=True, text=True, cwd=tmp_path)
    assert p.returncode == 2 and ("usage" in p.stderr or "is no cell token" in p.stderr), p.stderr
    assert os.listdir(tmp_path) == []


def test_a_directory_without_meta_is_an_error_not_a_usage_mistake(exe, tmp_path):
    p = subprocess.run([exe, str(tmp_path), "--all", "--output", str(tmp_path / "o.ply")], capture_output=True, text=True)
    assert p.returncode == 1 and "meta.pb" in p.stderr and os.listdir(tmp_path) == []


def test_params_struct_layout():
    from point_cloud_viewer_amd import _lib as L
    assert C.sizeof(L.PlyWriteParams) == 32 and L.PlyWriteParams.attributes.offset == 8 and L.PlyWriteParams.num_attributes.offset == 16
    assert L.PlyWriteParams.chunk_points.offset == 24 and L.PlyWriteParams.open_mode.offset == 4
