"""The packed hand-over between the chain pass and the record sort (csrc/pcv_encode.hip chain_pass_kernel DIAG 2, rank_hist_kernel on
the plane of 16-bit ranks, csrc/pcv_sort_rec12.hip: packed 8-byte records in, the colour staged through LDS, 12-byte records out).

 - the packed form through pcv_sort_records against the numpy sort of tests/sort_records_truth.py, exactly: tile edges, two tiles
   per workgroup, colour strides 3 and 4 in tensors cut at byte offsets 1, 5 and 15 from their allocation, predicted ranks 0 and
   65 535, the map in LDS and in global memory on both sides of the lowered limits, replay marks, pool-entry records, one pass and
   two passes with the held-back second pass;
 - rank_hist on the 16-bit plane: rows counted on the device from the plane equal the rows counted from u32 keys and the numpy
   count, for n and a last chunk that are no multiples of 8 (every chunk begins at a multiple of 8 192, so a chunk has a tail and
   no head) and bins on both sides of the 32 768-bin launch limit (16 384 / 16 385 as well: the plain count's limit, which the
   rows form crosses inside one launch);
 - single-chain builds byte for byte against the oracle with the packed hand-over (the shipped library) and, in child processes
   on the experiment library, once more with PCV_PACKED_HANDOVER=0 and =1 and with PCV_SORT_ROWS=0 (the plain count on the plane,
   two launches of 16 384 bins for the big tree, and the records unpacked in front of a sort that counts its keys): the digests
   of every byte must be equal, and Octree.packed_handover() says which hand-over each build took."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import order_cases as OC
import point_cloud_viewer_amd as pcv
import sort_records_truth as T
from point_cloud_viewer_amd import synthetic
from sort_records_cases import BIG_N, REC12_CHUNKS, REC12_PIECES, ROWS, ROWS_TRUE
from test_gpu_build import assert_same

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BYTE_FILL = 0xC3


@pytest.fixture(scope="module")
def ctx():
    c = pcv.Context(0)
    yield c
    c.close()


# ---- the packed form through pcv_sort_records -------------------------------------------------------------------------------
def packed_case(seed, n, key_bits, map_entries, stride, replay=0.0, ranks="random", extremes=False):
    """-> (inputs, truth): make_case's colour-less 12-byte records, a tenth of them as pool-entry records (any first word, no
    third code), and the same records packed: second word = third code | predicted rank << 16, the ranks once more as half words
    in the first 2 n bytes of `keys` (the rest of `keys` is filler nobody may read)."""
    inp = T.make_case(seed, n, key_bits, 2, 0, map_entries, replay, stride, ranks)
    keys, vec = inp["keys"].copy(), inp["vec"].copy()
    i = np.arange(n, dtype=np.uint32)
    pool = (i % np.uint32(10)) == 3
    vec[pool, 0] = i[pool] * np.uint32(2654435761)
    vec[pool, 1] = 0
    if extremes and n >= 2:  # predicted ranks 0 and 65 535 (the map has an entry for each)
        keys[0], keys[n - 1] = 0, np.uint32(65535 << 8)
    pred = keys >> np.uint32(8)
    assert map_entries <= 65536 and int(pred.max()) < map_entries
    truth = T.sort_truth(keys, key_bits, vec, (), inp["map"], inp["color"], stride)
    rows = T.rows_truth(keys, vec, map_entries)
    packed_vec = vec.copy()
    packed_vec[:, 1] |= pred << np.uint32(16)
    plane = np.full(n, 0xABCDABCD, dtype=np.uint32)
    plane.view(np.uint16)[:n] = pred.astype(np.uint16)
    return dict(keys=keys, vec=vec, packed_vec=packed_vec, plane=plane, map=inp["map"], color=inp["color"], rows=rows), truth


def run_packed(ctx, inp, truth, key_bits, stride, offset, hold_second, rows="given", packed=True):
    """One sort on device tensors; the colour tensor starts `offset` bytes into its allocation and ends with it. -> (plan, rows)."""
    import torch
    n = len(inp["keys"])
    dev = torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(a.copy().view(np.int32)).to(dev)
    keys = up(inp["plane"] if packed else inp["keys"])
    vec = up(inp["packed_vec"] if packed else inp["vec"])
    dmap = up(inp["map"])
    block = torch.full((offset + n * stride,), BYTE_FILL, dtype=torch.uint8, device=dev)
    assert block.data_ptr() % 16 == 0
    color = block[offset:]
    color.copy_(torch.from_numpy(inp["color"]))
    drows = up(inp["rows"]) if rows == "given" else "device"
    torch.cuda.synchronize()
    out = ctx.sort_records(keys, key_bits, vec=vec, color_in=color, color_stride=stride, map=dmap, rows=drows, hold_second=hold_second,
                           packed=packed)
    torch.cuda.synchronize()
    got_keys, got_vec = keys.cpu().numpy().view(np.uint32), vec.cpu().numpy().view(np.uint32)
    for what, want, got in (("keys", truth["keys"], got_keys), ("vec", truth["vec"], got_vec)):
        msg = T.first_difference(want, got, what, truth, got_vec, None)
        assert msg is None, msg
    host_block = block.cpu().numpy()
    assert np.all(host_block[:offset] == BYTE_FILL) and np.array_equal(host_block[offset:], inp["color"]), "the caller's colour was changed"
    assert np.array_equal(dmap.cpu().numpy().view(np.uint32), inp["map"])
    counted = None if out[3] is None else out[3].cpu().numpy().view(np.uint32)
    return out[4], counted


OFFSETS = (1, 5, 15)
SIZES = (1, 63, 64, 65, 8191, 8192, 8193, 70001)


@pytest.mark.parametrize("stride", (3, 4))
@pytest.mark.parametrize("n", SIZES)
def test_packed_records_at_the_tile_edges(ctx, n, stride):
    """One rows pass of 7 bits, the map (300 entries) in LDS."""
    inp, truth = packed_case(1000 + n + stride, n, 7, 300, stride)
    plan, _ = run_packed(ctx, inp, truth, 7, stride, OFFSETS[(SIZES.index(n) + stride) % 3], hold_second=False)
    p = plan["passes"]
    assert [(q["shift"], q["nbits"], q["hist"], q["down"], q["R"], q["MAP"], q["PL"]) for q in p] == [(8, 7, ROWS, REC12_CHUNKS, 128, 1, 0)], plan
    assert p[0]["dyn_lds"] == 608


FORMS = {  # key_bits, map_entries, stride, offset, hold_second, replay, extremes -> (MAP of the first pass, two_pass, held_back)
    "two_pass_held_lds_s3": ((13, 9000, 3, 5, True, 0.03, False), (1, 1, 1)),
    "two_pass_plain_lds_s4": ((13, 9000, 4, 15, False, 0.0, False), (1, 1, 0)),
    "lds_limit_r128_s3": ((13, 15824, 3, 1, True, 0.03, False), (1, 1, 1)),      # the last map that fits beside the colours
    "past_limit_r128_s3": ((13, 15825, 3, 15, True, 0.03, False), (2, 1, 1)),    # ... one more entry: gathered from global memory
    "lds_limit_r128_s4": ((13, 11728, 4, 5, False, 0.0, False), (1, 1, 0)),
    "past_limit_r128_s4": ((13, 11729, 4, 1, True, 0.0, False), (2, 1, 1)),
    "lds_limit_r256_s3": ((8, 11216, 3, 15, False, 0.03, False), (1, 0, 0)),     # 256 digit values, one pass
    "past_limit_r256_s4": ((8, 7121, 4, 5, False, 0.0, False), (2, 0, 0)),
    "ranks_0_and_65535": ((16, 65536, 3, 1, True, 0.03, True), (2, 0, 0)),       # 16-bit ranks: one rows pass of 8 bits + a generic one
}


@pytest.mark.parametrize("name", list(FORMS))
def test_packed_forms(ctx, name):
    (bits, entries, stride, offset, hold, replay, extremes), (MAP, two, held) = FORMS[name]
    inp, truth = packed_case(2000 + len(name) + entries, 70001, bits, entries, stride, replay, extremes=extremes)
    plan, _ = run_packed(ctx, inp, truth, bits, stride, offset, hold)
    first = plan["passes"][0]
    assert (first["MAP"], plan["two_pass"], plan["held_back"]) == (MAP, two, held), plan
    assert first["hist"] == (ROWS_TRUE if two else ROWS) and first["down"] == REC12_CHUNKS and first["PL"] == 0, plan
    assert first["dyn_lds"] == ((2 * entries + 15) // 16 * 16 if MAP == 1 else 0), plan
    if two:
        assert plan["passes"][1]["down"] == REC12_PIECES and plan["second_ran"] == held, plan
    if extremes:
        assert int(inp["plane"].view(np.uint16)[:70001].max()) == 65535 and int(inp["plane"].view(np.uint16)[:70001].min()) == 0


def test_packed_two_tiles_per_workgroup(ctx):
    """More than 1 024 tiles: every workgroup takes two tiles, so the colours of the second are requested while the first drains
    and parked behind its output phase."""
    inp, truth = packed_case(77, BIG_N, 13, 9000, 3, 0.03)
    plan, _ = run_packed(ctx, inp, truth, 13, 3, 5, hold_second=True)
    assert plan["chunk"] == 2 * 8192 and plan["two_pass"] == 1 and plan["held_back"] == 1 and plan["passes"][0]["MAP"] == 1, plan


@pytest.mark.parametrize("entries", (16384, 16385, 32768, 32769))
def test_rank_hist_on_the_16_bit_plane(ctx, entries):
    """n = 100 003: no multiple of 8, and the last of the 13 chunks (1 699 records) is none either: a tail of three ranks."""
    n, bits = 100003, 15  # (15 bits: the u32 form keeps a map of 16 384 entries in LDS as half words)
    inp, truth = packed_case(3000 + entries, n, bits, entries, 3)
    assert n % 8 != 0 and (n % 8192) % 8 != 0
    _, from_plane = run_packed(ctx, inp, truth, bits, 3, 1, hold_second=False, rows="device")
    _, from_keys = run_packed(ctx, inp, truth, bits, 3, 1, hold_second=False, rows="device", packed=False)
    assert from_plane.shape == inp["rows"].shape == from_keys.shape
    assert np.array_equal(from_plane, from_keys) and np.array_equal(from_plane, inp["rows"])
    assert int(from_plane.sum()) == n


# ---- single-chain builds: packed hand-over == oracle == the old hand-over ------------------------------------------------------
def _clouds():
    """name -> Cloud (tests/order_cases.py), in the order they are built on ONE context."""
    big = synthetic.gaussian_clusters(600_000, seed=31, num_clusters=9, extent=250.0, sigma_range=(0.3, 7.0))
    a = OC.base_cloud("a")
    rgba = np.ascontiguousarray(np.concatenate([a.rgb, np.full((a.n, 1), 9, np.uint8)], axis=1))
    return {
        "starved": OC.CONSTRUCTED["starved"](),  # falls back to the exact pipeline after the sort was queued ...
        "colour": a,                             # ... and the same context then builds a colour-only cloud
        "stride4": OC.Cloud(a.x, a.y, a.z, rgba, None, a.bmin, a.bmax, a.cap, a.res),
        "big_tree": OC.Cloud(big[0], big[1], big[2], big[3], None, big[4], big[5], 150, 0.001),  # more nodes than the LDS map holds
        "intensity": OC.base_cloud("b"),         # the plane: the old hand-over, whatever the switch says
    }


def _build_all(ctx):
    import bench
    out = {}
    for name, cl in _clouds().items():
        t = ctx.build(cl.res, pcv.Aabb(cl.bmin, cl.bmax), cl.x, cl.y, cl.z, cl.rgb, cl.inten, max_points_per_node=cl.cap, single_chain=True,
                      check_resolve=True)
        out[name] = (t, dict(t.build_info(), packed_handover=t.packed_handover()), bench.digest_of_digests(bench.tree_digests(t)))
    return out


_CHILD = r"""
import json, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
import point_cloud_viewer_amd as pcv
import test_gpu_packed_handover as M
built = M._build_all(pcv.Context(0))
print("RESULT " + json.dumps({k: [v[1], v[2]] for k, v in built.items()}))
"""


# the experiment library: the old hand-over, the packed one, and the packed one in front of a sort without rank-count rows
CHILDREN = {"0": {"PCV_PACKED_HANDOVER": "0"}, "1": {"PCV_PACKED_HANDOVER": "1"}, "no_rows": {"PCV_SORT_ROWS": "0"}}
# Octree.packed_handover(): 1 = packed records loaded by the sort's first pass, 2 = unpacked in front of the sort, 0 = old
PACKED = {"starved": 0, "colour": 1, "stride4": 1, "big_tree": 1, "intensity": 0}


@pytest.fixture(scope="module")
def builds(ctx):
    """The shipped library in this process (the trees kept for the oracle), the experiment library in two child processes."""
    sys.path.insert(0, ROOT)
    mine = _build_all(ctx)
    other = {}
    for switch, env in CHILDREN.items():
        p = subprocess.run([sys.executable, "-c", _CHILD, ROOT], env=dict(os.environ, PCV_HIP_LIBRARY="exp", **env),
                           capture_output=True, text=True, timeout=600)
        assert p.returncode == 0 and "RESULT " in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]
        other[switch] = json.loads(p.stdout.split("RESULT ", 1)[1].splitlines()[0])
    yield mine, other
    for t, _, _ in mine.values():
        t.free()


@pytest.mark.parametrize("name", ["starved", "colour", "stride4", "big_tree", "intensity"])
def test_build_equals_oracle_and_the_old_hand_over(builds, name):
    mine, other = builds
    cl = _clouds()[name]
    t, info, digest = mine[name]
    rgb = cl.rgb[:, :3] if cl.rgb.shape[1] == 4 else cl.rgb
    want = OC.Cloud(cl.x, cl.y, cl.z, np.ascontiguousarray(rgb), cl.inten, cl.bmin, cl.bmax, cl.cap, cl.res).oracle()
    assert_same(t.to_dict(), want, check_intensity=cl.inten is not None)
    assert info["packed_handover"] == PACKED[name], info  # (starved: the exact pipeline's records; intensity: the plane)
    for switch in CHILDREN:
        oinfo, odigest = other[switch][name]
        assert odigest == digest, (name, switch, info, oinfo)
        assert oinfo["single_chain"] == info["single_chain"] and oinfo["record_bytes"] == info["record_bytes"], (name, switch, info, oinfo)
        assert oinfo["packed_handover"] == {"0": 0, "1": PACKED[name], "no_rows": 2 * PACKED[name]}[switch], (name, switch, oinfo)
    if name == "starved":
        assert not info["single_chain"] and info["attempts"] in (2, 3), info
    else:
        assert info["single_chain"] and info["record_bytes"] == 12, info
    if name == "big_tree":  # past every lowered LDS-map limit, inside the 16 bits of the packed rank
        assert 15824 < info["predicted_nodes"] <= 65536, info
