"""examples/render_view.c with terrain layers: it compiles as C11 against the header without a warning and links the in-tree
library, its usage lists the new options, and what pcv_render_check_terrain_host refuses ends with exit status 2 before any
device work; the new struct has the layout the ctypes mirror assumes."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EX = os.path.join(ROOT, "examples")
LOOK = ["--look-at", "1", "2", "30", "1", "2", "0", "1.0", "--size", "64x48", "-o", "out.png"]
MATRIX = ["--matrix"] + ["1", "0", "0", "0", "0", "1", "0", "0", "0", "0", "1", "0", "0", "0", "0", "1"] + ["--size", "64x48", "-o", "out.png"]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("render_view") / "render_view"
    lib = os.path.join(ROOT, "point_cloud_viewer_amd")
    p = subprocess.run(["cc", "-std=c11", "-O2", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(ROOT, "include"),
                        os.path.join(EX, "render_view.c"), "-o", str(out), "-L" + lib, "-lpcv_hip", "-lm", "-Wl,-rpath," + lib],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    subprocess.check_call(["make", "-s", "-C", EX, "bin/render_view"])  # and by the examples' own rule
    return str(out)


def test_usage_lists_the_terrain_options(exe):
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 2 and "--terrain <dir>" in p.stderr and "--terrain-window N" in p.stderr


@pytest.mark.parametrize("args,word", [
    (LOOK + ["--terrain"], "usage"),                                               # no value
    (LOOK + ["--terrain", "layer", "--terrain-window"], "usage"),                  # no value
    (LOOK + ["--terrain", "layer", "--terrain-window", "15"], "window must be even"),
    (LOOK + ["--terrain-window", "15"], "window must be even"),                    # checked without a layer too
    (LOOK + ["--terrain", "layer", "--terrain-window", "0"], "2 ..= 1024"),
    (LOOK + ["--terrain", "layer", "--terrain-window", "1026"], "2 ..= 1024"),
    (MATRIX + ["--terrain", "layer"], "--terrain needs --look-at"),                # a bare matrix has no camera position
    (LOOK + ["--terrain", "layer"] * 17, "usage"),                                 # more layers than the example holds
])
def test_bad_terrain_arguments_end_with_status_2(exe, args, word, tmp_path):
    p = subprocess.run([exe, "octree"] + args, capture_output=True, text=True, cwd=tmp_path)
    assert p.returncode == 2 and word in p.stderr and "usage" in p.stderr, p.stderr
    assert os.listdir(tmp_path) == []


def test_struct_layout():
    from point_cloud_viewer_amd import _lib as L
    assert C.sizeof(L.RenderTerrainLayers) == 24 and L.RenderTerrainLayers.window.offset == 4
    assert L.RenderTerrainLayers.layers.offset == 8 and L.RenderTerrainLayers.camera_positions.offset == 16
    assert L.RENDER_TERRAIN_WINDOW == 1024
