"""The record sort on its own (pcv_sort_records) against the numpy truth of tests/sort_records_truth.py, case by case of
tests/sort_records_cases.py: every downsweep form at its tile edges, the two-pass rows form with skewed and empty pieces, the
map on both sides of its LDS limits, color_in, replay marks, first_in0, two tiles per workgroup, the generic record forms.
Every case asserts the plan the library returns and compares every output array exactly; device inputs are views cut out of
larger tensors whose margins must come back untouched. The file ends with the set of kernel forms its plans covered."""
import ctypes as C

import numpy as np
import pytest

import point_cloud_viewer_amd as pcv
import sort_records_truth as T
from point_cloud_viewer_amd import _lib as L
from sort_records_cases import (ALL_GENERIC, ALL_PIECES, ALL_REC12, BIG_N, CASES, IN_HOST_MEMORY, ROWS_ON_DEVICE, check_plan,
                                instantiation_set)

pytestmark = pytest.mark.gpu

PLANS = {}            # case -> the plan the library returned
WORD_FILL = 0x5EEDBEEF  # the margins around device arrays
BYTE_FILL = 0xC3
SMALL = [name for name, c in CASES.items() if not c["big"]]
REUSED = set(ROWS_ON_DEVICE + IN_HOST_MEMORY + ("two_n100003_b13_p0_s1", "edge_n16401_b7", "skew_one_low_digit", "skew_one_low_digit_plane",
                                                 "skew_few", "skew_same"))
_prepared = {}


@pytest.fixture(scope="module")
def ctx():
    c = pcv.Context(0)
    yield c
    c.close()


def prepared(name):
    """-> (inputs, truth, rows) of a case; made once for the cases that several tests run."""
    if name in _prepared:
        return _prepared[name]
    c = CASES[name]
    inp = T.make_case(c["seed"], c["n"], c["key_bits"], c["vec_words"], c["nplanes"], c["map_entries"], c["replay"], c["color_stride"],
                      c["ranks"])
    truth = T.sort_truth(inp["keys"], c["key_bits"], inp["vec"], inp["planes"], inp["map"], inp["color"], c["color_stride"] or 3)
    rows = T.rows_truth(inp["keys"], inp["vec"], c["map_entries"]) if c["rows"] else None
    for a in [inp["keys"], inp["vec"], inp["map"], inp["color"], rows] + inp["planes"]:
        if a is not None:
            a.setflags(write=False)  # shared between tests: left unchanged
    if name in REUSED:
        _prepared[name] = (inp, truth, rows)
    return inp, truth, rows


class DeviceArray:
    """A numpy array on the device as a view cut out of a larger tensor, `before` rows in, with filled margins."""

    def __init__(self, a, before, after):
        import torch
        self.words = a.dtype == np.uint32
        fill = WORD_FILL if self.words else BYTE_FILL
        self.before, self.rows = before, a.shape[0]
        self.big = torch.full((before + a.shape[0] + after,) + a.shape[1:], fill, dtype=torch.int32 if self.words else torch.uint8, device="cuda")
        self.view = self.big[before:before + self.rows]
        self.view.copy_(torch.from_numpy(a.copy().view(np.int32) if self.words else a.copy()))

    def host(self):
        a = self.view.cpu().numpy()
        return a.view(np.uint32) if self.words else a

    def margins_intact(self):
        fill = WORD_FILL if self.words else BYTE_FILL
        m = self.big.cpu().numpy()
        return bool(np.all(m[:self.before] == fill) and np.all(m[self.before + self.rows:] == fill))


def compare(c, truth, keys, vec, planes):
    """Every output with the truth; the first differing slot names its records."""
    plane0 = planes[0] if planes else None
    for what, want, got in [("keys", truth["keys"], keys)] + ([("vec", truth["vec"], vec)] if truth["vec"] is not None else []) + \
            [(f"plane {w}", truth["planes"][w], planes[w]) for w in range(len(truth["planes"]))]:
        msg = T.first_difference(want, got, what, truth, vec, plane0)
        assert msg is None, f"{c['name']}: {msg}"
    if c["color_stride"]:  # the last record of the input, whose colour the first pass reads byte by byte
        slot = int(np.flatnonzero(truth["order"] == c["n"] - 1)[0])
        assert keys[slot] == truth["keys"][slot] and vec[slot, 1] == truth["vec"][slot, 1], f"{c['name']}: the last record's colour"


def run_case(ctx, name, mem=None, rows=None, record=True):
    """One sort: the plan asserted, every output compared. -> (keys, vec, planes, plan) as numpy arrays."""
    import torch
    c = CASES[name]
    inp, truth, given_rows = prepared(name)
    mem = mem or c["mem"]
    rows_mode = rows or c["rows"]
    n, npl = c["n"], c["nplanes"]
    hosted = {"keys": inp["keys"].copy(), "vec": None if inp["vec"] is None else inp["vec"].copy(), "map": inp["map"], "color": inp["color"],
              "rows": given_rows if rows_mode == "given" else None}
    planes_in = [p.copy() for p in inp["planes"]]
    plane0_in = None
    if c["first_in0"]:
        plane0_in = inp["planes"][0]
        planes_in[0] = np.full(n, 0x0BADF00D, dtype=np.uint32)  # only receives the sorted plane
    dev = []
    if mem == "device":
        # words 3 in (4-byte alignment), payloads 3 rows in (8 / 16 bytes), the colour 7 bytes in and at the very end of its tensor
        def put(a, after=5):
            if a is None:
                return None
            d = DeviceArray(a, 7 if a.dtype == np.uint8 else 3, 0 if a.dtype == np.uint8 else after)
            dev.append(d)
            return d
        d = {k: put(v) for k, v in hosted.items()}
        dplanes = [put(p) for p in planes_in]
        dplane0 = put(plane0_in)
        torch.cuda.synchronize()
        arg = lambda x: None if x is None else x.view
        out = ctx.sort_records(arg(d["keys"]), c["key_bits"], vec=arg(d["vec"]), planes=[arg(p) for p in dplanes], plane0_in=arg(dplane0),
                               color_in=arg(d["color"]), color_stride=c["color_stride"] or 3, map=arg(d["map"]),
                               rows="device" if rows_mode == "device" else arg(d["rows"]), hold_second=c["hold_second"])
        torch.cuda.synchronize()
        keys, vec, planes = d["keys"].host(), None if d["vec"] is None else d["vec"].host(), [p.host() for p in dplanes]
        counted = None if out[3] is None else out[3].cpu().numpy().view(np.uint32)
        for x in dev:
            assert x.margins_intact(), f"{name}: a margin of a device array was written"
        for k in ("map", "color", "rows"):  # inputs the kernels read in place
            assert d[k] is None or np.array_equal(d[k].host(), hosted[k]), f"{name}: the caller's {k} was changed"
        if dplane0 is not None:
            assert np.array_equal(dplane0.host(), plane0_in), f"{name}: the caller's plane 0 was changed"
    else:
        out = ctx.sort_records(hosted["keys"], c["key_bits"], vec=hosted["vec"], planes=planes_in, plane0_in=plane0_in,
                               color_in=hosted["color"], color_stride=c["color_stride"] or 3, map=hosted["map"],
                               rows="device" if rows_mode == "device" else hosted["rows"], hold_second=c["hold_second"])
        keys, vec, planes, counted = out[0], out[1], out[2], out[3]
        assert keys is hosted["keys"] and (vec is None or vec is hosted["vec"])  # in place
    plan = out[4]
    check_plan(c, plan)
    if record:
        PLANS[name] = plan
    compare(c, truth, keys, vec, planes)
    if rows_mode == "device":
        assert counted.shape == given_rows.shape and np.array_equal(counted, given_rows), f"{name}: the rows counted on the device differ"
    return keys, vec, planes, plan


@pytest.mark.parametrize("name", SMALL)
def test_case(ctx, name):
    run_case(ctx, name)


def test_skewed_ranks_make_long_and_empty_pieces(ctx):
    """What the skewed cases are for, from the returned plan and the truth's counts: piece k of the second pass holds the records
    whose rank's lower digit is k // blocks, from the first-pass workgroups [blk * gpb, (blk + 1) * gpb)."""
    def piece_sizes(name):
        plan = PLANS.get(name) or run_case(ctx, name)[3]
        c = CASES[name]
        inp, truth, _ = prepared(name)
        low_bits, blocks, gpb, chunk = plan["passes"][0]["nbits"], plan["blocks"], plan["gpb"], plan["chunk"]
        low = (truth["true"] & ((1 << low_bits) - 1)).astype(np.int64)
        blk = (np.arange(c["n"]) // chunk) // gpb
        return np.bincount(low * blocks + blk, minlength=plan["pieces"])
    sizes = piece_sizes("skew_one_low_digit")
    assert sizes.max() > 8192, sizes.max()  # a piece of more than one tile
    assert piece_sizes("skew_one_low_digit_plane").max() > 8192
    sizes = piece_sizes("skew_few")
    assert np.count_nonzero(sizes == 0) > len(sizes) // 2  # most pieces are empty
    sizes = piece_sizes("skew_same")
    assert np.count_nonzero(sizes) == -(-PLANS["skew_same"]["groups"] // PLANS["skew_same"]["gpb"])


@pytest.mark.parametrize("name", ROWS_ON_DEVICE)
def test_rows_counted_on_the_device(ctx, name):
    """pcv_launch_rank_hist_rows' rows equal the truth's word for word, and the sort's output is the same with either."""
    for mem in ("device", "host"):
        given = run_case(ctx, name, mem=mem, record=False)
        counted = run_case(ctx, name, mem=mem, rows="device", record=False)
        assert given[3] == counted[3]
        for a, b in zip([given[0], given[1]] + given[2], [counted[0], counted[1]] + counted[2]):
            assert np.array_equal(a, b)


@pytest.mark.parametrize("name", IN_HOST_MEMORY)
def test_host_and_device_memory_agree(ctx, name):
    dev = run_case(ctx, name, mem="device", record=False)
    host = run_case(ctx, name, mem="host", record=False)
    assert dev[3] == host[3]
    for a, b in zip([dev[0], dev[1]] + dev[2], [host[0], host[1]] + host[2]):
        assert np.array_equal(a, b)


def test_no_records(ctx):
    import torch
    for dev in (False, True):
        def arr(shape):
            return torch.zeros(shape, dtype=torch.int32, device="cuda") if dev else np.zeros(shape, dtype=np.uint32)
        m = arr(10)
        k, v, p, r, plan = ctx.sort_records(arr(0), 7, vec=arr((0, 2)), planes=[arr(0)], map=m, rows="device", hold_second=True)
        assert len(k) == 0 and len(v) == 0 and len(p[0]) == 0 and plan["npasses"] == 0 and plan["passes"] == [] and not plan["second_ran"]
        k, v, p, r, plan = ctx.sort_records(arr(0), 32, planes=[arr(0), arr(0)])
        assert len(k) == 0 and plan["npasses"] == 0


def test_bad_calls_raise_and_leave_the_context_usable(ctx):
    inp, truth, rows = prepared("edge_n16401_b7")
    keys, vec = inp["keys"].copy(), inp["vec"].copy()
    # a null array: the payload of a 12-byte record sort
    a = L.SortRecordsArgs()
    a.n, a.key_bits, a.vec_bytes, a.keys, a.vec, a.mem = len(keys), 7, 8, keys.ctypes.data, None, L.MEM_HOST
    with pytest.raises(L.PcvError) as e:
        ctx._check(ctx.lib.pcv_sort_records(ctx.handle, C.byref(a), None))
    assert e.value.code == L.PCV_E_INVALID and "vec is null" in str(e.value)
    # bad arguments: nine planes; rows without a map; a predicted rank outside the map (checked mode)
    with pytest.raises(ValueError):
        ctx.sort_records(keys, 7, vec=vec, planes=[keys] * 9)
    a.vec, a.nwords = vec.ctypes.data, 9
    with pytest.raises(L.PcvError) as e:
        ctx._check(ctx.lib.pcv_sort_records(ctx.handle, C.byref(a), None))
    assert e.value.code == L.PCV_E_INVALID and "nwords" in str(e.value)
    with pytest.raises(L.PcvError) as e:
        ctx.sort_records(keys, 7, vec=vec, rows=rows)
    assert e.value.code == L.PCV_E_INVALID and "rows need a map" in str(e.value)
    with pytest.raises(L.PcvError) as e:
        ctx.sort_records(keys, 7, vec=vec, map=inp["map"][:5], rows="device")
    assert e.value.code == L.PCV_E_INVALID and "outside the map" in str(e.value)
    with pytest.raises(L.PcvError) as e:
        ctx.sort_records(keys, 16, vec=vec, map=inp["map"], rows=rows)
    assert e.value.code == L.PCV_E_INVALID and "half words" in str(e.value)
    assert np.array_equal(keys, inp["keys"]) and np.array_equal(vec, inp["vec"])  # nothing was touched
    run_case(ctx, "edge_n16401_b7", record=False)  # and the context sorts on
    run_case(ctx, "edge_n16401_b7", mem="host", record=False)


def test_twice_on_one_context(ctx):
    """The sort's scratch block and the side stream are reused: a held-back two-pass sort, a one-pass sort of another size, the
    first again."""
    first = run_case(ctx, "two_n100003_b13_p0_s1", record=False)
    assert first[3]["held_back"] and first[3]["second_ran"]
    run_case(ctx, "edge_n16401_b7", record=False)
    again = run_case(ctx, "two_n100003_b13_p0_s1", record=False)
    assert first[3] == again[3] and np.array_equal(first[0], again[0]) and np.array_equal(first[1], again[1])


# ---- two tiles per workgroup: 8 396 817 records, generated on the device ----------------------------------------------------
def big_inputs(name):
    """Device tensors of one big case from a fixed seed, and their host copies for the truth."""
    import torch
    c = CASES[name]
    n, entries = c["n"], c["map_entries"]
    g = torch.Generator(device="cuda")
    g.manual_seed(c["seed"])
    small = T.make_case(c["seed"], 4 * entries, c["key_bits"], 2, 0, entries, c["replay"], 0, "random")  # (for its map)
    m = small["map"]
    pred = torch.randint(0, entries, (n,), generator=g, device="cuda", dtype=torch.int32)
    i = torch.arange(n, device="cuda", dtype=torch.int32)
    keys = pred << 8
    vec = torch.empty((n, 2), dtype=torch.int32, device="cuda")
    vec[:, 0] = i ^ (T.X_TAG - (1 << 32))
    vec[:, 1] = (i * 7 + 3) & 0xFFFF
    color = None
    if c["color_stride"]:
        color = torch.randint(0, 256, (n * c["color_stride"],), generator=g, device="cuda", dtype=torch.uint8)
    else:
        keys |= torch.randint(0, 256, (n,), generator=g, device="cuda", dtype=torch.int32)
        vec[:, 1] |= torch.randint(0, 1 << 15, (n,), generator=g, device="cuda", dtype=torch.int32) << 16
    plane = i * 40503 + 11 if c["nplanes"] else None  # (wraps: an odd multiplier keeps the words distinct)
    return dict(keys=keys, vec=vec, color=color, plane=plane, map=m)


@pytest.fixture(scope="module", params=[name for name, c in CASES.items() if c["big"]])
def big(ctx, request):
    """One big sort and its truth, shared by the assertions on plan, keys, payloads and planes."""
    import torch
    name = request.param
    c = CASES[name]
    d = big_inputs(name)
    host = {k: None if v is None else (v.cpu().numpy() if k != "map" else v) for k, v in d.items()}
    hk, hv = host["keys"].view(np.uint32), host["vec"].view(np.uint32)
    hp = [] if host["plane"] is None else [host["plane"].view(np.uint32)]
    truth = T.sort_truth(hk, c["key_bits"], hv, hp, host["map"], host["color"], c["color_stride"] or 3)
    rows = torch.from_numpy(T.rows_truth(hk, hv, c["map_entries"]).view(np.int32)).cuda()
    dmap = torch.from_numpy(host["map"].view(np.int32)).cuda()
    planes = [torch.full((c["n"],), 0x0BADF00D, dtype=torch.int32, device="cuda")] if c["nplanes"] else []
    torch.cuda.synchronize()
    out = ctx.sort_records(d["keys"], c["key_bits"], vec=d["vec"], planes=planes, plane0_in=d["plane"] if c["first_in0"] else None,
                           color_in=d["color"], color_stride=c["color_stride"] or 3, map=dmap, rows=rows, hold_second=c["hold_second"])
    torch.cuda.synchronize()
    PLANS[name] = out[4]
    got = dict(keys=out[0].cpu().numpy().view(np.uint32), vec=out[1].cpu().numpy().view(np.uint32),
               planes=[p.cpu().numpy().view(np.uint32) for p in out[2]])
    if c["first_in0"]:
        assert np.array_equal(d["plane"].cpu().numpy(), host["plane"]), "the caller's plane 0 was changed"
    return c, truth, got, out[4]


def test_big_plan(big):
    c, truth, got, plan = big
    assert c["n"] == BIG_N and (plan["groups"], plan["chunk"]) == (513, 16384)  # two tiles per workgroup
    check_plan(c, plan)


def test_big_keys(big):
    c, truth, got, plan = big
    msg = T.first_difference(truth["keys"], got["keys"], "keys", truth, got["vec"], None)
    assert msg is None, f"{c['name']}: {msg}"


def test_big_payloads(big):
    c, truth, got, plan = big
    msg = T.first_difference(truth["vec"], got["vec"], "vec", truth, got["vec"], None)
    assert msg is None, f"{c['name']}: {msg}"
    last = int(np.flatnonzero(truth["order"] == c["n"] - 1)[0])  # the last record of the input: its colour is read bytewise
    assert np.array_equal(got["vec"][last], truth["vec"][last]) and got["keys"][last] == truth["keys"][last]


def test_big_planes(big):
    c, truth, got, plan = big
    assert len(got["planes"]) == len(truth["planes"])
    for w, p in enumerate(truth["planes"]):
        msg = T.first_difference(p, got["planes"][w], f"plane {w}", truth, got["vec"], None)
        assert msg is None, f"{c['name']}: {msg}"


def test_the_cases_above_covered_every_downsweep_form():
    """Over the plans the library returned above: all twelve instantiations of the 12-byte record downsweep (128 / 256 digit values
    x no map / map in LDS / map in global memory x plane or none), the PIECES form with and without the plane, held back and
    not, and the three generic record forms."""
    assert set(PLANS) == set(CASES), sorted(set(CASES) - set(PLANS))
    rec12, pieces, gen = instantiation_set(PLANS.values())
    assert rec12 == ALL_REC12, sorted(ALL_REC12 - rec12)
    assert pieces == ALL_PIECES, sorted(ALL_PIECES - pieces)
    assert gen == ALL_GENERIC, sorted(ALL_GENERIC - gen)
