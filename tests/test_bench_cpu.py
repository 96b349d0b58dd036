"""bench.py's host-side pieces that the config-3 runs rely on (no GPU): the block-wise cloud generator must hand every
rank exactly its slice of the ONE global cloud, and the digest tables must compare octrees node by node."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_any_slice_of_the_config3_cloud_is_reproducible(monkeypatch):
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: None)  # the generator ends with a device sync
    monkeypatch.setattr(bench, "CLOUD_BLOCK", 1 << 16)  # small blocks: slices that start and end inside blocks
    dev = torch.device("cpu")
    total = 700_001
    x, y, z, rgb = bench.make_cloud_slice(torch, total, 0, total, seed=2, device=dev)
    for world in (1, 3, 8):
        parts = []
        for rank in range(world):
            lo, hi = rank * total // world, (rank + 1) * total // world
            parts.append(bench.make_cloud_slice(torch, total, lo, hi - lo, seed=2, device=dev))
        for k, whole in enumerate((x, y, z, rgb)):
            assert torch.equal(torch.cat([p[k] for p in parts]), whole), (world, k)
    other = bench.make_cloud_slice(torch, total, 0, 1000, seed=3, device=dev)
    assert not torch.equal(other[0], x[:1000])  # the seed matters
    assert float(x.min()) > -200.0 and float(x.max()) < 1200.0  # 64 clusters in a 1000 m cube, sigma <= 20 m
    h = (np.arange(5, dtype=np.int64) * 2654435761) & 0xFFFFFF  # colour = hash of the GLOBAL point index
    assert rgb[:5].numpy().tolist() == np.stack([(h >> 16) & 255, (h >> 8) & 255, h & 255], axis=1).tolist()


def test_digest_tables_compare_node_by_node():
    a = {"r": (10, 3, "x0", "c0", "i0"), "r1": (4, 2, "x1", "c1", "i1"), "r17": (0, 1, "e", "e", "e")}
    same = dict(reversed(list(a.items())))
    assert bench.compare_digests(a, same)["ok"] and bench.digest_of_digests(a) == bench.digest_of_digests(same)
    b = dict(a, r1=(4, 2, "x1", "DIFFERENT", "i1"))
    cmp_ = bench.compare_digests(a, b)
    assert not cmp_["ok"] and cmp_["mismatching_nodes"] == 1 and cmp_["first_mismatches"] == ["r1"]
    assert bench.digest_of_digests(a) != bench.digest_of_digests(b)
    c = {k: v for k, v in a.items() if k != "r17"}
    c["r2"] = (1, 1, "y", "y", "y")
    cmp_ = bench.compare_digests(a, c)
    assert (cmp_["missing_nodes"], cmp_["extra_nodes"], cmp_["mismatching_nodes"]) == (1, 1, 0) and not cmp_["ok"]


def test_build_hash_follows_the_sources(tmp_path, monkeypatch):
    h = bench.build_hash()
    assert len(h) == 16 and h == bench.build_hash()
    # a copy of csrc with one byte changed hashes differently
    import shutil
    src = os.path.join(ROOT, "point_cloud_viewer_amd", "csrc")
    dst = tmp_path / "point_cloud_viewer_amd" / "csrc"
    os.makedirs(dst)
    for name in os.listdir(src):
        if name.endswith((".hip", ".h", ".cpp", ".inc")) or name == "Makefile":
            shutil.copy(os.path.join(src, name), dst / name)
    monkeypatch.setattr(bench, "ROOT", str(tmp_path))
    assert bench.build_hash() == h
    with open(dst / "pcv_sort.hip", "a") as f:
        f.write("// one more byte\n")
    assert bench.build_hash() != h


def test_valu_issue_model_prices_classes_with_the_measured_costs():
    """bench.valu_issue_model: dynamic per-class counts x the issue costs of this round's probe, against 1 024 SIMDs x the
    clock the counter pass saw; the two bounds bracket the mid figure, and a faster launch gives a higher fraction."""
    insts = {"valu_insts_per_point": 600.0, "f64_valu_insts_per_point": 190.0, "f64_arith_insts_per_point": 190.0,
             "cvt_insts_per_point": 36.0, "rest_insts_per_point": 374.0, "rest_static_share_f64_other": 0.4,
             "rest_static_share_cmp32": 0.06, "sustained_clock_GHz": 2.07}
    r = bench.valu_issue_model(insts, 100_000_000, 2.2)
    if r.get("frac") is None:  # no probe recorded for this round yet
        assert "note" in r
        return
    lo, hi = r["frac_bounds"]
    assert 0.0 < lo < r["frac"] < hi < 1.5
    c = r["cycles_per_class"]
    assert 3.5 < c["f64_add_mul_fma"] < 5.5 and 1.8 < c["b32_plain"] < 3.2 and c["b32_compare"] > c["b32_plain"]
    assert bench.valu_issue_model(insts, 100_000_000, 1.1)["frac"] > r["frac"] * 1.9
    # counters of an older profile (no per-class fields): the model says so instead of guessing
    assert bench.valu_issue_model({"valu_insts_per_point": 600.0}, 100_000_000, 2.2)["frac"] is None


def test_query_profile_is_quoted_only_for_the_running_build():
    p = bench.query_profile("0000000000000000")
    assert p.get("profile_matches_build") in (False, None) and "cull_nodes_kernel" not in p
    q = bench.query_profile(bench.build_hash())
    assert q.get("profile_matches_build") in (True, False, None)


def _recorded_full_record():
    """The whole record of a default run of an earlier round (22 KB as one line: what the driver failed to parse in round 5)."""
    import json
    for line in open(os.path.join(ROOT, "profiles", "r05_bench_100M.json")):
        if line.startswith("{"):
            return json.loads(line)
    raise AssertionError("no JSON line in profiles/r05_bench_100M.json")


def test_final_line_is_small(tmp_path, monkeypatch, capsys):
    """the LAST stdout line is the line of record and stays under 4 KB whatever the legs carry; it holds the
    contract fields, roofline, cpu_baseline and one parity verdict per BASELINE config; the whole record goes to a file."""
    import json
    out = _recorded_full_record()
    assert len(json.dumps(out)) > 16_000
    monkeypatch.setattr(bench, "ROOT", str(tmp_path))
    os.makedirs(tmp_path / "gpurun_out")
    bench.emit(out)
    lines = capsys.readouterr().out.strip().splitlines()
    assert len(lines) == 2
    detail, last = lines
    assert len(last) < 4096 and len(detail) < 8192 and len(detail) + len(last) < 12_000
    rec = json.loads(last)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in rec, k
    assert rec["value"] == out["value"] and rec["ms_per_step"] == out["ms_per_step"]
    assert rec["config"]["workload"].startswith("BASELINE config 2") and "model" not in rec["config"]
    r = rec["roofline"]
    assert r["frac"] == out["roofline"]["frac"] and r["traffic"] == out["roofline"]["traffic"] and r["hbm_view"]["frac"]
    assert r["kernel"] == "chain_pass_kernel"  # the symbol rocprofv3 lists, not the library's event slot
    assert set(rec["kernel_ms_per_step"]) >= {"chain_pass_kernel", "downsweep_rec12_kernel", "promote_settle_leaf_kernel",
                                              "downsweep_settle_kernel", "aabb_partial_kernel"}
    assert rec["cpu_baseline"]["kind"] == "port" and rec["cpu_baseline"]["cores"] == out["cpu_baseline"]["cores"]
    assert rec["encode_sort"]["frac_of_8TBps"] == round(out["encode_sort"]["GB/s"] / 8000.0, 4)
    p = rec["parity"]
    assert p["config2"] == {"ok": True, "mismatching_nodes": 0, "nodes": 6073, "tree_digest": out["tree_digest"]}
    assert all(p[k]["ok"] for k in ("config1", "config4", "config5", "intensity", "sharded"))
    whole = json.loads(open(tmp_path / "bench_detail.json").read())
    assert whole == out and json.loads(open(tmp_path / "gpurun_out" / "bench_detail.json").read()) == out
    assert "bench_detail" in json.loads(detail)
    # a leg that failed is a verdict, not a crash of the line; a record without legs (N > 1, --no-legs) still prints
    out2 = dict(out, config5={"error": "RuntimeError: " + "x" * 500}, query=None, sharded=None, intensity=None, config1=None)
    rec2 = bench.final_line(out2)
    assert rec2["parity"]["config5"]["ok"] is False and rec2["parity"]["config4"] is None
    # pathological growth (every string 10 x longer) still fits: the line sheds its optional objects
    fat = json.loads(json.dumps(out))
    fat["config"]["workload"] *= 10
    fat["cpu_baseline"]["sample"] *= 10
    fat["kernel_ms_per_step"] = {f"kernel_with_a_long_name_{i}": 1.0 for i in range(200)}
    assert len(json.dumps(bench.final_line(fat))) <= bench.FINAL_LINE_LIMIT


class _FakeTree:
    """The part of OctreeResult that bench.dump_outputs reads, over host bytes: nodes = [(id_high, id_low, level, encoding,
    point_offset, xyz bytes, rgb bytes)]."""

    def __init__(self, nodes):
        import ctypes as C
        import types
        from point_cloud_viewer_amd import _lib as L
        self.handle, self._C, self._L = 1, C, L
        self.ctx = types.SimpleNamespace(_check=lambda rc: None)
        self.lib = types.SimpleNamespace(pcv_octree_node_data=self._node_data)
        self._nodes = nodes
        self._bufs = [(C.create_string_buffer(xyz, max(1, len(xyz))), C.create_string_buffer(rgb, max(1, len(rgb))))
                      for *_, xyz, rgb in nodes]

    def _node_data(self, handle, i, which, pptr, pln):
        pptr._obj.value = self._C.addressof(self._bufs[i][which])
        pln._obj.value = len(self._nodes[i][5 + which])
        return 0

    @property
    def num_nodes(self):
        return len(self._nodes)

    @property
    def num_points(self):
        return sum(len(nd[6]) // 3 for nd in self._nodes)

    def meta(self):
        return dict(resolution=0.001, bbox_min=np.array([-1.0, -2.0, -3.0]), bbox_max=np.array([4.0, 5.0, 6.0]), version=13)

    def node(self, i):
        hi, lo, level, enc, off, xyz, rgb = self._nodes[i]
        return self._L.NodeInfo(id_high=hi, id_low=lo, num_points=len(rgb) // 3, level=level, encoding=enc,
                                cube_min=(self._C.c_double * 3)(0.5, 1.5, 2.5), cube_edge=8.0, xyz_offset=0, point_offset=off)


def test_dump_outputs_writes_what_the_build_returned(tmp_path, monkeypatch):
    """bench --dump-outputs: node table + the stored .xyz / .rgb values of a seeded sample of points, exact, in float32 /
    float64 .npy files, the same sample on every run. Nodes listed in another order than their points lie in the blobs, an
    empty node, every position encoding."""
    rng = np.random.default_rng(4)
    nodes, want = [], {}
    for level, enc, dt, count, off in ((0, 2, "<u2", 5, 7), (1, 1, "u1", 0, 12), (1, 4, "<f8", 3, 12), (2, 3, "<f4", 7, 0)):
        vals = (rng.integers(0, 256 if enc == 1 else 65536, (count, 3)) if enc <= 2 else rng.random((count, 3))).astype(dt)
        rgb = rng.integers(0, 256, (count, 3)).astype(np.uint8)
        nodes.append(((level << 56) | 0xABCDEF01, (1 << 63) | count, level, enc, off, vals.tobytes(), rgb.tobytes()))
        for k in range(count):
            want[off + k] = (vals[k].astype(np.float64), rgb[k].astype(np.float32))
    tree = _FakeTree(nodes)
    n = tree.num_points
    assert sorted(want) == list(range(n))
    for sample in (n, 6):
        monkeypatch.setattr(bench, "DUMP_MAX_SAMPLE", sample)
        d = tmp_path / f"s{sample}"
        rec = bench.dump_outputs(tree, str(d))
        got = {p.stem: np.load(p) for p in d.glob("*.npy")}
        assert set(got) == {"meta", "nodes", "point_index", "xyz", "rgb"} and rec["sampled_points"] == sample
        assert all(a.dtype in (np.float32, np.float64) for a in got.values()) and rec["bytes"] <= 64 << 20
        assert got["meta"].tolist() == [0.001, -1.0, -2.0, -3.0, 4.0, 5.0, 6.0]
        assert got["nodes"].shape == (4, 13) and got["nodes"][:, 4].tolist() == [5, 0, 3, 7]
        assert got["nodes"][0, :4].tolist() == [0, 0xABCDEF01, 1 << 31, 5] and got["nodes"][3, 12] == 0
        idx = got["point_index"].astype(np.int64)
        assert idx.size == sample and np.all(np.diff(idx) > 0)
        assert np.array_equal(got["xyz"], np.array([want[i][0] for i in idx]))
        assert np.array_equal(got["rgb"], np.array([want[i][1] for i in idx]))
        again = bench.dump_outputs(tree, str(tmp_path / "again"))
        assert again == dict(rec, dir=str(tmp_path / "again"))
        assert np.array_equal(np.load(tmp_path / "again" / "point_index.npy"), got["point_index"])
