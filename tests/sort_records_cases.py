"""The cases of the record-sort tests, with the plan each is written to reach. tests/test_sort_records_cpu.py asserts the plans
on the stand-alone drivers (no GPU); tests/test_gpu_sort_records.py runs the cases, asserts the plan the library returns and
compares every output with tests/sort_records_truth.py.

A case: what sort_records_truth.make_case takes (n, key_bits, vec_words, nplanes, map_entries, replay, color_stride, ranks) plus
rows ("given", "device" or None), hold_second, first_in0 and mem; `want` is the plan:
  passes      (shift, nbits, hist, down, R, MAP, PL) per pass, PcvSortHist / PcvSortDown as in csrc/pcv_sort_plan.h
  two_pass, held_back, and for the first pass dyn_lds (MAP 1) and map_lds (a counting pass with the map)."""
from sort_records_truth import geometry

UPSWEEP, UPSWEEP_MAP, ROWS, ROWS_TRUE = range(4)  # PcvSortHist
KEYS, REC_UINT4, REC_UINT2, REC_PLANES, REC12_CHUNKS, REC12_PIECES = range(6)  # PcvSortDown
BIG_N = 8_388_608 + 8_192 + 17  # two tiles per workgroup: more than 1 024 tiles of 8 192

CASES = {}


def case(name, n, key_bits, want, vec_words=2, nplanes=0, map_entries=0, rows=None, hold_second=False, replay=0.0, color_stride=0,
         ranks="random", first_in0=False, mem="device", big=False):
    assert name not in CASES, name
    CASES[name] = dict(name=name, seed=len(CASES) + 1, n=n, key_bits=key_bits, want=want, vec_words=vec_words, nplanes=nplanes,
                       map_entries=map_entries, rows=rows, hold_second=hold_second, replay=replay, color_stride=color_stride,
                       ranks=ranks, first_in0=first_in0, mem=mem, big=big)


def R_of(nbits):
    return 128 if nbits <= 7 else 256


def one_rows_pass(bits, MAP, PL, then=(), dyn_lds=None):
    """One pass with its histogram from the rows, then generic 12-byte passes of the widths `then`."""
    passes = [(8, bits, ROWS, REC12_CHUNKS, R_of(bits), MAP, PL)]
    at = 8 + bits
    for w in then:
        passes.append((at, w, UPSWEEP, REC12_CHUNKS, R_of(w), 0, PL))
        at += w
    return dict(passes=passes, two_pass=0, held_back=0, dyn_lds=dyn_lds)


def two_pass(w1, w2, MAP, PL, held, dyn_lds=None):
    return dict(passes=[(8, w1, ROWS_TRUE, REC12_CHUNKS, R_of(w1), MAP, PL), (8 + w1, w2, ROWS_TRUE, REC12_PIECES, R_of(w2), 0, PL)],
                two_pass=1, held_back=int(held), dyn_lds=dyn_lds)


def counted(widths, PL, map_lds=None, shift=8):
    """12-byte records without rows: every pass counts its keys, the first applies the map where there is one."""
    passes, at = [], shift
    for k, w in enumerate(widths):
        passes.append((at, w, UPSWEEP_MAP if k == 0 and map_lds is not None else UPSWEEP, REC12_CHUNKS, R_of(w), 0, PL))
        at += w
    return dict(passes=passes, two_pass=0, held_back=0, map_lds=map_lds)


def generic(key_bits, down, shift, map_lds=None):
    """The generic record passes: as few as 8-bit digits allow, of equal width."""
    count = -(-key_bits // 8)
    width = -(-key_bits // count)
    passes, at = [], shift
    for k in range(count):
        w = min(width, shift + key_bits - at)
        passes.append((at, w, UPSWEEP_MAP if k == 0 and map_lds is not None else UPSWEEP, down, 256, 0, 0))
        at += w
    return dict(passes=passes, two_pass=0, held_back=0, map_lds=map_lds)


def lds_bytes(entries):  # the map as half words, rounded up to 16 bytes
    return (2 * entries + 15) // 16 * 16


# ---- tile edges, one rows pass -------------------------------------------------------------------------------------------
for n in (1, 63, 8191, 8192, 8193, 16401):
    for bits in (1, 7, 8):
        case(f"edge_n{n}_b{bits}", n, bits, one_rows_pass(bits, 1, 0, dyn_lds=lds_bytes(300)), map_entries=300, rows="given")

# ---- the two-pass rows form ----------------------------------------------------------------------------------------------
for n in (57345, 65536, 100003):
    for bits, (w1, w2) in ((9, (5, 4)), (13, (7, 6)), (14, (7, 7))):
        for plane in (0, 1):
            for second in (0, 1):
                case(f"two_n{n}_b{bits}_p{plane}_s{second}", n, bits, two_pass(w1, w2, 1, plane, second, lds_bytes(9000)), nplanes=plane,
                     map_entries=9000, rows="given", hold_second=bool(second))
case("two_7_groups", 57344, 13, one_rows_pass(7, 1, 0, then=(6,), dyn_lds=lds_bytes(9000)), map_entries=9000, rows="given", hold_second=True)

# ---- skewed ranks in the two-pass form -----------------------------------------------------------------------------------
for mode in ("one_low_digit", "few", "same", "sorted", "falling"):
    case(f"skew_{mode}", 100003, 13, two_pass(7, 6, 1, 0, True, lds_bytes(9000)), map_entries=9000, rows="given", hold_second=True, ranks=mode)
case("skew_one_low_digit_plane", 100003, 13, two_pass(7, 6, 1, 1, False, lds_bytes(9000)), nplanes=1, map_entries=9000, rows="given",
     ranks="one_low_digit")

# ---- wide ranks with the default counters: one rows pass of 8 bits, then a generic 12-byte pass ----------------------------
for plane in (0, 1):
    # 12 000 entries: in LDS without the plane, in global memory with it (256 digit values: 5 000 at most)
    case(f"wide_b15_p{plane}", 100003, 15, one_rows_pass(8, 2 if plane else 1, plane, then=(7,), dyn_lds=None if plane else lds_bytes(12000)),
         nplanes=plane, map_entries=12000, rows="given", hold_second=True)
    # (a map in LDS holds 15 bits of true rank: ranks of 16 bits come with a map in global memory)
    case(f"wide_b16_p{plane}", 100003, 16, one_rows_pass(8, 2, plane, then=(8,)), nplanes=plane, map_entries=20000, rows="given",
         hold_second=True)

# ---- where the map lives -------------------------------------------------------------------------------------------------
case("map_16384", 70001, 12, two_pass(6, 6, 1, 0, False, 32768), map_entries=16384, rows="given")
case("map_16385", 70001, 12, one_rows_pass(6, 2, 0, then=(6,)), map_entries=16385, rows="given")  # (more entries than counters: one pass)
case("map_10000_plane", 70001, 12, two_pass(6, 6, 1, 1, False, 20000), nplanes=1, map_entries=10000, rows="given")
case("map_10001_plane", 70001, 12, two_pass(6, 6, 2, 1, False), nplanes=1, map_entries=10001, rows="given")
case("map_5000_plane_r256", 70001, 8, one_rows_pass(8, 1, 1, dyn_lds=10000), nplanes=1, map_entries=5000, rows="given")
case("map_5001_plane_r256", 70001, 8, one_rows_pass(8, 2, 1), nplanes=1, map_entries=5001, rows="given")
case("map_40000", 70001, 12, one_rows_pass(6, 2, 0, then=(6,)), map_entries=40000, rows="given")

# ---- no rows: the first pass counts the keys and applies the map ----------------------------------------------------------
case("norows_15000", 70001, 13, counted((7, 6), 0, map_lds=1), map_entries=15000, replay=0.03)
case("norows_15001", 70001, 13, counted((7, 6), 0, map_lds=0), map_entries=15001, replay=0.03)
case("norows_15000_plane", 70001, 13, counted((7, 6), 1, map_lds=1), nplanes=1, map_entries=15000)
case("nomap", 70001, 13, counted((7, 6), 0))
case("nomap_plane", 70001, 13, counted((7, 6), 1), nplanes=1)

# ---- color_in --------------------------------------------------------------------------------------------------------------
for stride in (3, 4):
    for plane in (0, 1):
        case(f"color_s{stride}_p{plane}_n8193_one", 8193, 7, one_rows_pass(7, 1, plane, dyn_lds=lds_bytes(300)), nplanes=plane, map_entries=300,
             rows="given", color_stride=stride)
        case(f"color_s{stride}_p{plane}_n70001_one", 70001, 7, one_rows_pass(7, 1, plane, dyn_lds=lds_bytes(300)), nplanes=plane,
             map_entries=300, rows="given", color_stride=stride)
        case(f"color_s{stride}_p{plane}_n8193_b13", 8193, 13, one_rows_pass(7, 1, plane, then=(6,), dyn_lds=lds_bytes(9000)), nplanes=plane,
             map_entries=9000, rows="given", color_stride=stride)
        case(f"color_s{stride}_p{plane}_n70001_two", 70001, 13, two_pass(7, 6, 1, plane, plane == 0, lds_bytes(9000)), nplanes=plane,
             map_entries=9000, rows="given", color_stride=stride, hold_second=plane == 0)

# ---- replay marks: 3 % of the map entries -----------------------------------------------------------------------------------
case("replay_map1_one", 70001, 8, one_rows_pass(8, 1, 0, dyn_lds=lds_bytes(3000)), map_entries=3000, rows="given", replay=0.03)
case("replay_map2_one", 70001, 8, one_rows_pass(8, 2, 0), map_entries=20000, rows="given", replay=0.03)
case("replay_map1_two", 70001, 13, two_pass(7, 6, 1, 0, True, lds_bytes(9000)), map_entries=9000, rows="given", replay=0.03, hold_second=True)
case("replay_map2_two", 70001, 13, two_pass(7, 6, 2, 1, True), nplanes=1, map_entries=12000, rows="given", replay=0.03, hold_second=True)

# ---- first_in0 -------------------------------------------------------------------------------------------------------------
case("first_in0_one", 70001, 7, one_rows_pass(7, 1, 1, dyn_lds=lds_bytes(300)), nplanes=1, map_entries=300, rows="given", first_in0=True)
case("first_in0_two", 70001, 13, two_pass(7, 6, 1, 1, True, lds_bytes(9000)), nplanes=1, map_entries=9000, rows="given", first_in0=True,
     hold_second=True)
case("first_in0_generic", 70001, 11, generic(11, REC_PLANES, 0), vec_words=0, nplanes=2, first_in0=True)

# ---- two tiles per workgroup ---------------------------------------------------------------------------------------------
case("big_two_color", BIG_N, 13, two_pass(7, 6, 1, 0, True, lds_bytes(9000)), map_entries=9000, rows="given", color_stride=3, hold_second=True,
     big=True)
case("big_one_plane", BIG_N, 8, one_rows_pass(8, 1, 1, dyn_lds=lds_bytes(4000)), nplanes=1, map_entries=4000, rows="given", first_in0=True,
     replay=0.03, big=True)

# ---- the generic record forms ------------------------------------------------------------------------------------------------
GENERIC_SHAPES = [(4, 0, 0), (4, 1, 0), (4, 4, 0), (4, 0, 5000), (4, 1, 15001), (4, 4, 5000),  # (vec_words, planes, map_entries)
                  (2, 2, 0), (2, 4, 0), (0, 2, 0), (0, 3, 0), (0, 8, 0)]
for vw, npl, me in GENERIC_SHAPES:
    down = REC_UINT4 if vw == 4 else REC_UINT2 if vw == 2 else REC_PLANES
    for n, all_bits in ((1, (11,)), (4095, (11,)), (4096, (11,)), (4097, (3, 11, 16, 24, 32)), (70001, (3, 11, 16, 24, 32))):
        for bits in all_bits:
            if vw == 2 and bits > 24:
                continue  # (the rank field of a 12-byte record's key has 24 bits)
            case(f"gen_v{vw}_p{npl}_m{me}_n{n}_b{bits}", n, bits,
                 generic(bits, down, 8 if vw == 2 else 0, map_lds=None if not me else int(me <= 15000)), vec_words=vw, nplanes=npl,
                 map_entries=me, replay=0.03 if me else 0.0)

# ---- rows counted on the device: the same sorts as three of the cases above -------------------------------------------------
ROWS_ON_DEVICE = ("edge_n16401_b8", "two_n100003_b13_p1_s1", "color_s3_p0_n70001_two")
# ---- host memory: the same sorts once more from numpy arrays ---------------------------------------------------------------
IN_HOST_MEMORY = ("edge_n1_b7", "two_n65536_b13_p1_s1", "gen_v4_p1_m15001_n4097_b16")


def groups_and_chunk(c):
    """The geometry the plan must state: tiles of 8 192 for 12-byte records with at most one plane, of 4 096 otherwise."""
    if c["vec_words"] == 2 and c["nplanes"] <= 1:
        return geometry(c["n"])
    tiles = -(-c["n"] // 4096)
    chunk = max(1, -(-tiles // 1024)) * 4096
    return max(1, -(-c["n"] // chunk)), chunk


def check_plan(c, plan):
    """Asserts that `plan` (dict: the fields of pcv_sort_plan_info, passes as dicts) is the one the case was written for."""
    want = c["want"]
    got = [(p["shift"], p["nbits"], p["hist"], p["down"], p["R"], p["MAP"], p["PL"]) for p in plan["passes"]]
    assert got == want["passes"], (c["name"], got, want["passes"])
    assert (plan["two_pass"], plan["held_back"]) == (want["two_pass"], want["held_back"]), (c["name"], plan)
    assert (plan["groups"], plan["chunk"]) == groups_and_chunk(c), (c["name"], plan)
    if want.get("dyn_lds") is not None:
        assert plan["passes"][0]["dyn_lds"] == want["dyn_lds"], (c["name"], plan["passes"][0])
    elif plan["passes"]:
        assert plan["passes"][0]["dyn_lds"] == 0, (c["name"], plan["passes"][0])
    if want.get("map_lds") is not None:
        assert plan["passes"][0]["map_lds"] == want["map_lds"], (c["name"], plan["passes"][0])
    if want["two_pass"]:
        assert plan["pieces"] == (1 << plan["passes"][0]["nbits"]) * plan["blocks"], (c["name"], plan)
        assert plan["blocks"] == min(1024 >> plan["passes"][0]["nbits"], plan["groups"]), (c["name"], plan)
        assert plan["gpb"] == -(-plan["groups"] // plan["blocks"]), (c["name"], plan)
    if "second_ran" in plan:
        assert plan["second_ran"] == want["held_back"], (c["name"], plan)


def instantiation_set(plans):
    """{(R, MAP, PL)} of the 12-byte record downsweeps, {(PL, held_back)} of the PIECES form and {down} of the generic passes."""
    rec12, pieces, gen = set(), set(), set()
    for plan in plans:
        for p in plan["passes"]:
            if p["down"] in (REC12_CHUNKS, REC12_PIECES):
                rec12.add((p["R"], p["MAP"], p["PL"]))
            if p["down"] == REC12_PIECES:
                pieces.add((p["PL"], plan["held_back"]))
            if p["down"] in (REC_UINT4, REC_UINT2, REC_PLANES):
                gen.add(p["down"])
    return rec12, pieces, gen


ALL_REC12 = {(R, MAP, PL) for R in (128, 256) for MAP in (0, 1, 2) for PL in (0, 1)}
ALL_PIECES = {(PL, held) for PL in (0, 1) for held in (0, 1)}
ALL_GENERIC = {REC_UINT4, REC_UINT2, REC_PLANES}
