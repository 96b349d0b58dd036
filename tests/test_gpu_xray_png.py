"""Compressed xray tiles on the device: node_pngs / write(png="deflate") / merges against the host encoder
(pcv_xray_png_encode_ex on node_images) byte for byte, against the plain Python stream (tests/xray_png_oracle.py) on a
sample, back through Python's zlib, the hand-made tiles of the CPU test through the device encoder, a chunk boundary, and
the C examples. The small clouds are those of tests/test_gpu_xray_merge.py."""
import os
import subprocess

import numpy as np
import pytest

import point_cloud_viewer_amd as pcv
import xray_png_oracle as PO
from test_gpu_query import ctx  # noqa: F401  (module fixture)
from test_gpu_xray_merge import PX, W, build, cloud, shards, write_parts  # noqa: F401  (cloud: module fixture)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def host_pngs(xt, png="deflate"):
    return [pcv.xray_png_encode(img, png=png) for img in xt.node_images()]


@pytest.fixture(scope="module")
def trees(cloud):  # noqa: F811
    return {16: build(cloud, "colored", "transparent"), 7: build(cloud, "xray", "white", tile=7, px=1.0)}


@pytest.mark.parametrize("tile", [16, 7])
def test_node_pngs_equal_the_host_encoder(trees, tile):
    xt = trees[tile]
    got = xt.node_pngs(png="deflate")
    want = host_pngs(xt)
    assert len(got) == len(xt.node_ids) > len(xt.created_ids) > 4  # leaves and parents
    assert got == want, [n for n, g, w in zip(xt.node_ids, got, want) if g != w][:5]
    images = xt.node_images()
    for i in list(range(0, len(got), max(1, len(got) // 6))) + [len(got) - 1]:  # a sample: first leaf ... the root
        assert got[i] == PO.png(images[i]), xt.node_ids[i]
        assert np.array_equal(PO.decode(got[i]), images[i])
    # a range in the middle that starts in the leaves and ends in the parents
    nc = len(xt.created_ids)
    assert xt.node_pngs(nc - 2, 5, png="deflate") == want[nc - 2:nc + 3]
    assert xt.node_pngs(3, 0, png="deflate") == []
    with pytest.raises(pcv.PcvError, match="PCV_E_INVALID"):
        xt.node_pngs(len(got), 1, png="deflate")


def test_stored_node_pngs_are_the_files_of_today(trees, tmp_path):
    xt = trees[16]
    xt.write(tmp_path / "stored")
    got = xt.node_pngs(png="stored")
    assert got == [(tmp_path / "stored" / (n + ".png")).read_bytes() for n in xt.node_ids] == host_pngs(xt, "stored")


def test_hand_made_tiles_through_the_device_encoder(ctx):  # noqa: F811
    tiles = PO.hand_made_tiles()
    by_w = {}
    for name in sorted(tiles):
        by_w.setdefault(tiles[name].shape[1], []).append(name)
    assert {1, 7, 16, 64, 256} <= set(by_w)
    for w, names in sorted(by_w.items()):
        batch = np.stack([tiles[n] for n in names])
        want = [PO.png(tiles[n]) for n in names]
        for chunk_tiles in (0, 1) if w != 256 else (0,):  # one launch for all of them; one tile per chunk
            got = pcv.xray_png_encode_tiles(ctx, batch, chunk_tiles=chunk_tiles)
            assert got == want, (w, chunk_tiles, [n for n, g, x in zip(names, got, want) if g != x])
    assert len(PO.idat(PO.png(tiles["white_256"]))) == 2537
    noise = np.random.default_rng(3).integers(0, 256, (3, 64, 64, 4), dtype=np.uint8)  # larger than raw, inside the bound
    got = pcv.xray_png_encode_tiles(ctx, noise, chunk_tiles=2)
    assert got == [pcv.xray_png_encode(t, png="deflate") for t in noise]
    assert all(64 * 257 < len(PO.idat(g)) <= PO.stream_bound(64, 64) for g in got)


def test_deflate_directory(ctx, trees, tmp_path):  # noqa: F811
    xt = trees[16]
    xt.write(tmp_path / "stored")
    xt.write(tmp_path / "deflate", png="deflate")
    names = sorted(os.listdir(tmp_path / "stored"))
    assert names == sorted(os.listdir(tmp_path / "deflate")) and "meta.pb" in names and "r.png" in names
    assert (tmp_path / "stored" / "meta.pb").read_bytes() == (tmp_path / "deflate" / "meta.pb").read_bytes()
    small = 0
    for n in names:
        if n.endswith(".png"):
            a, b = (tmp_path / "stored" / n).read_bytes(), (tmp_path / "deflate" / n).read_bytes()
            assert np.array_equal(PO.decode(b), PO.decode(a)), n
            small += len(b) < len(a)
    assert small > 0
    assert [(tmp_path / "deflate" / (n + ".png")).read_bytes() for n in xt.node_ids] == host_pngs(xt)
    (back,) = ctx.xray_open(tmp_path / "deflate")
    assert sorted(back.node_ids) == sorted(xt.node_ids)
    by_name = dict(zip(xt.node_ids, xt.node_images()))
    for name, img in zip(back.node_ids, back.node_images()):
        assert np.array_equal(img, by_name[name]), name


def test_chunk_boundary(ctx, trees, tmp_path):  # noqa: F811
    xt = trees[16]
    want = host_pngs(xt)
    assert len(want) > 7
    try:
        ctx.set_xray_chunk_bytes(3 * 4 * W * W)  # three tiles a chunk: several chunks, a ragged last one, one across leaves | parents
        assert xt.node_pngs(png="deflate") == want
        xt.write(tmp_path / "d", png="deflate")
        assert [(tmp_path / "d" / (n + ".png")).read_bytes() for n in xt.node_ids] == want
        assert xt.node_pngs(png="stored") == host_pngs(xt, "stored")
        ctx.set_xray_chunk_bytes(1)  # below a tile: one tile a chunk
        assert xt.node_pngs(0, 5, png="deflate") == want[:5]
    finally:
        ctx.set_xray_chunk_bytes(0)


def test_stored_chunk_boundary(ctx, trees, cloud, tmp_path):  # noqa: F811
    """Stored mode through the chunked download it shares with every kind of quadtree: built, a live merge, a merge of
    opened and live parts, and a range across the leaves | parents seam, three tiles a chunk and then one."""
    xt = trees[16]
    want = host_pngs(xt, "stored")
    nc = len(xt.created_ids)
    assert len(want) > 7 and nc % 3 != 0 and len(want) % 3 != 0  # a chunk across leaves | parents, a ragged last one
    xt.write(tmp_path / "default")
    parts = shards(cloud, 1, "colored", "transparent")
    live = ctx.xray_merge(parts, "transparent")
    live_want = host_pngs(live, "stored")
    dirs = write_parts(parts[:2], tmp_path / "parts")
    mixed = ctx.xray_merge([parts[3], ctx.xray_open(dirs[1])[0], parts[2], ctx.xray_open(dirs[0])[0]], "transparent")
    copied = {f: (d / f).read_bytes() for d in dirs for f in os.listdir(d) if f.endswith(".png")}
    assert len(copied) > 2 and len(live.node_ids) == len(mixed.node_ids) > len(copied) + 2

    def files(d, ids):
        assert set(os.listdir(d)) == {n + ".png" for n in ids} | {"meta.pb"}
        return [(d / (n + ".png")).read_bytes() for n in ids]
    try:
        for k, chunk_bytes in enumerate((3 * 4 * W * W, 1)):  # three tiles a chunk; below a tile: one tile a chunk
            ctx.set_xray_chunk_bytes(chunk_bytes)
            xt.write(tmp_path / f"built{k}")
            assert files(tmp_path / f"built{k}", xt.node_ids) == want
            assert (tmp_path / f"built{k}" / "meta.pb").read_bytes() == (tmp_path / "default" / "meta.pb").read_bytes()
            live.write(tmp_path / f"live{k}")
            assert files(tmp_path / f"live{k}", live.node_ids) == live_want
            for png in ("stored", "deflate"):
                out = tmp_path / f"mixed{k}_{png}"
                mixed.write(out, png=png)
                encoded = dict(zip(mixed.node_ids, host_pngs(mixed, png)))
                for name, got in zip(mixed.node_ids, files(out, mixed.node_ids)):
                    assert got == copied.get(name + ".png", encoded[name]), (png, name)
            assert xt.node_pngs(nc - 2, 5, png="stored") == want[nc - 2:nc + 3]
            assert xt.node_pngs(png="stored") == want and live.node_pngs(png="stored") == live_want
    finally:
        ctx.set_xray_chunk_bytes(0)


def test_merge_of_deflate_shards(ctx, cloud, tmp_path):  # noqa: F811
    whole = build(cloud, "xray", "white")
    parts = shards(cloud, 1, "xray", "white")
    dirs = []
    for k, p in enumerate(parts):
        p.write(tmp_path / f"part{k}", png="deflate")
        dirs.append(tmp_path / f"part{k}")
    merged = pcv.merge_xray_quadtrees(ctx, dirs, tmp_path / "out", "white", png="deflate")
    wi = dict(zip(whole.node_ids, whole.node_images()))
    gi = dict(zip(merged.node_ids, merged.node_images()))
    assert set(gi) == set(wi)
    for name, img in wi.items():
        assert np.array_equal(gi[name], img), name
    for d in dirs:  # the shards' files, byte for byte
        for f in os.listdir(d):
            if f.endswith(".png"):
                assert (tmp_path / "out" / f).read_bytes() == (d / f).read_bytes(), f
    assert (tmp_path / "out" / "r.png").read_bytes() == pcv.xray_png_encode(wi["r"], png="deflate")
    # node_pngs of the merged quadtree: opened nodes as their files are, its own level compressed on the device
    files = merged.node_pngs(png="deflate")
    assert files == [(tmp_path / "out" / (n + ".png")).read_bytes() for n in merged.node_ids]
    # a merge of device-built parts re-encodes everything in the mode asked for
    live = ctx.xray_merge(parts, "white")
    assert live.node_pngs(png="deflate") == host_pngs(live)
    live.write(tmp_path / "live", png="deflate")
    assert [(tmp_path / "live" / (n + ".png")).read_bytes() for n in live.node_ids] == host_pngs(live)
    assert sorted(os.listdir(tmp_path / "live")) == sorted(os.listdir(tmp_path / "out"))


def test_kernel_stats_name_the_new_kernels(ctx, trees):  # noqa: F811
    ctx.set_profiling(True)
    try:
        ctx.reset_kernel_stats()
        trees[7].node_pngs(png="deflate")
        st = ctx.kernel_stats()
    finally:
        ctx.set_profiling(False)
    # XrayTiles.node_pngs asks for the offsets first, then for the bytes: two encodes of one chunk each
    assert st["xray_png_band_kernel"][0] == st["xray_png_layout_kernel"][0] == st["xray_png_gather_kernel"][0] == 2, st
    assert st["xray_png_band_kernel"][1] > 0.0


def test_c_examples_write_the_same_directories(ctx, cloud, tmp_path):  # noqa: F811
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "examples")])
    cloud["tree"].write_dir(str(tmp_path / "octree"))
    opened = ctx.open_dir(tmp_path / "octree")
    xt = opened.xray_quadtree(W, PX, "colored", background="transparent", output_directory=tmp_path / "py", png="deflate")
    exe = os.path.join(ROOT, "examples", "bin", "build_xray_quadtree")
    p = subprocess.run([exe, str(tmp_path / "octree"), "--output-directory", str(tmp_path / "c"), "--resolution", str(PX), "--tile-size",
                        str(W), "--coloring-strategy", "colored", "--tile-background-color", "transparent", "--png", "deflate"],
                       capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr
    names = sorted(os.listdir(tmp_path / "py"))
    assert names == sorted(os.listdir(tmp_path / "c")) and "meta.pb" in names and len(names) > 8
    for n in names:
        assert (tmp_path / "py" / n).read_bytes() == (tmp_path / "c" / n).read_bytes(), n
    assert (tmp_path / "py" / "r.png").read_bytes() == xt.node_pngs(len(xt.node_ids) - 1, 1, png="deflate")[0]
    dirs = write_parts(shards(cloud, 1, "xray", "white"), tmp_path / "parts")
    pcv.merge_xray_quadtrees(ctx, dirs, tmp_path / "mpy", "white", png="deflate")
    exe = os.path.join(ROOT, "examples", "bin", "merge_xray_quadtrees")
    subprocess.check_call([exe, "--output-directory", str(tmp_path / "mc"), "--png", "deflate"] + [str(d) for d in dirs])
    files = sorted(os.listdir(tmp_path / "mpy"))
    assert files == sorted(os.listdir(tmp_path / "mc")) and "r.png" in files
    for f in files:
        assert (tmp_path / "mpy" / f).read_bytes() == (tmp_path / "mc" / f).read_bytes(), f
    assert len((tmp_path / "mc" / "r.png").read_bytes()) < len(pcv.xray_png_encode(np.zeros((W, W, 4), np.uint8)))
