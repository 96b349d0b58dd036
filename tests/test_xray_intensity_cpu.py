"""Host-side checks of colored_with_intensity and binning (pcv_xray_run_ex): pcv_xray_finalize(PCV_XRAY_FN_INTENSITY)
against the numpy restatement on random means and on every discrete case of IntensityColoringStrategy's colour, the
parameter checks of pcv_xray_check_params_ex, the entry points that refuse the strategy, and the Python spellings."""
import ctypes as C
import math

import numpy as np
import pytest

import point_cloud_viewer_amd as pcv
import xray_intensity_oracle as I
from point_cloud_viewer_amd import _lib as L

F32 = np.float32
NAN, INF = float("nan"), float("inf")


def finalize(rows):
    return pcv.xray_finalize("intensity", np.array(rows, dtype=np.float64).reshape(-1, 3))


def oracle(rows):
    r = np.array(rows, dtype=np.float64).reshape(-1, 3).astype(F32)
    return np.concatenate([I.intensity_color(r[i:i + 1, 0], r[i, 1], r[i, 2]) for i in range(r.shape[0])])


def test_ln_matches_libm_within_an_ulp():
    rng = np.random.default_rng(3)
    x = np.concatenate([rng.uniform(0, 5000, 20000), 10.0 ** rng.uniform(-44, 38, 20000), [1.0, 2.0, 0.5, 1e-45, 3.4e38]])
    x = x.astype(F32)
    got, ref = I.ln_f32(x), np.log(x)
    assert got[np.flatnonzero(x == 1.0)[0]] == 0.0
    ulp = np.abs(got.view(np.int32).astype(np.int64) - ref.view(np.int32).astype(np.int64))
    assert ulp.max() <= 1 and (ulp == 0).mean() > 0.9


def test_finalize_intensity_random_means():
    rng = np.random.default_rng(1)
    n = 20000
    lo = rng.uniform(-50, 50, n)
    hi = lo + rng.uniform(0.01, 500, n)
    mean = rng.uniform(lo - 20, hi + 20)
    rows = np.stack([mean, lo, hi], 1)
    got = finalize(rows)
    want = oracle(rows)
    assert np.array_equal(got, want)
    assert np.all(got[:, 3] == 255) and len(np.unique(got[:, 0])) > 200
    # against numpy's own f32 log the brightness differs by at most 1
    ref = np.concatenate([I.intensity_color(rows[i:i + 1, 0].astype(F32), F32(rows[i, 1]), F32(rows[i, 2]), ln=np.log)
                          for i in range(0, n, 7)])
    assert np.abs(ref.astype(int) - got[::7].astype(int)).max() <= 1


DISCRETE = [
    # (mean, min, max) -> brightness
    ((5.0, 5.0, 100.0), 0),          # mean == min: ln(0) = -inf, over a positive denominator
    ((2.0, 5.0, 100.0), 0),          # below min: clamped to min
    ((100.0, 5.0, 100.0), 255),      # at max: ln(d) / ln(d) = 1
    ((500.0, 5.0, 100.0), 255),      # above max: clamped
    ((5.5, 5.0, 6.0), 0),            # max - min == 1: ln(0.5) / 0 = -inf
    ((5.0, 5.0, 6.0), 0),            # max - min == 1 and mean == min: -inf / 0 = -inf
    ((6.0, 5.0, 6.0), 0),            # max - min == 1 and mean == max: 0 / 0 = NaN
    ((5.25, 5.0, 5.5), 255),         # max - min < 1: ln(0.25) / ln(0.5) = 2
    ((5.0, 5.0, 5.5), 255),          # max - min < 1 and mean == min: -inf / negative = +inf
    ((7.0, 10.0, 3.0), 0),           # min > max: clamped to max, ln(negative) = NaN
    ((NAN, 5.0, 100.0), 0),          # NaN mean: NaN.max(min) = min
    ((NAN, 5.0, 5.5), 255),          # NaN mean, max - min < 1: -inf / negative
    ((50.0, NAN, 100.0), 0),         # NaN min: mean - NaN = NaN
    ((50.0, 5.0, NAN), 0),           # NaN max: ln(NaN)
    ((INF, 5.0, 100.0), 255),        # +inf mean: clamped to max
    ((-INF, 5.0, 100.0), 0),
]


@pytest.mark.parametrize("row,b", DISCRETE, ids=[str(i) for i in range(len(DISCRETE))])
def test_finalize_intensity_discrete_cases(row, b):
    got = finalize([row])
    assert tuple(got[0]) == (b, b, b, 255)
    assert np.array_equal(got, oracle([row]))


def test_finalize_intensity_partial_brightness():
    # ln(20) / ln(100) = 0.6505..., * 255 = 165.9 -> 165
    got = finalize([(25.0, 5.0, 105.0)])
    assert tuple(got[0]) == (165, 165, 165, 255)


def params(strategy):
    return L.XrayParams(tile_size_px=256, pixel_size_m=0.1, strategy=strategy, max_stddev=1.0)


def coloring(binning=None, lo=0.0, hi=1.0):
    c = L.XrayColoring(min_intensity=lo, max_intensity=hi)
    if binning is not None:
        c.binning_attribute, c.bin_size = binning[0], binning[1]
    return c


def check(p, col, has_int=True):
    err = C.create_string_buffer(256)
    rc = L.load_library().pcv_xray_check_params_ex(C.byref(p), C.byref(col) if col is not None else None, int(has_int), err, 256)
    return rc, err.value.decode()


def test_check_params_ex_accepts():
    for s in (L.XRAY_COLORED, L.XRAY_COLORED_WITH_INTENSITY, L.XRAY_XRAY, L.XRAY_HEIGHT_STDDEV):
        assert check(params(s), coloring((b"intensity", 16.0)))[0] == L.PCV_OK
        assert check(params(s), coloring())[0] == L.PCV_OK
    # bin size and min / max are not validated
    for size in (0.0, NAN, -3.0, INF):
        assert check(params(L.XRAY_COLORED), coloring((b"intensity", size)))[0] == L.PCV_OK
    assert check(params(L.XRAY_COLORED_WITH_INTENSITY), coloring(lo=NAN, hi=-INF))[0] == L.PCV_OK
    # no coloring: exactly pcv_xray_check_params for the other strategies
    assert check(params(L.XRAY_COLORED), None, has_int=False)[0] == L.PCV_OK
    # binning ignored by xray and height_stddev: no intensity needed
    for s in (L.XRAY_XRAY, L.XRAY_HEIGHT_STDDEV):
        assert check(params(s), coloring((b"intensity", 1.0)), has_int=False)[0] == L.PCV_OK


def test_check_params_ex_refuses():
    bad = [(params(L.XRAY_COLORED), coloring((b"color", 1.0)), True, "only intensity"),
           (params(L.XRAY_COLORED_WITH_INTENSITY), coloring((b"timestamp", 1.0)), True, "only intensity"),
           (params(L.XRAY_XRAY), coloring((b"color", 1.0)), True, "only intensity"),
           (params(L.XRAY_COLORED), coloring((b"intensity", 1.0)), False, "no intensity"),
           (params(L.XRAY_COLORED_WITH_INTENSITY), coloring(), False, "no intensity"),
           (params(L.XRAY_COLORED_WITH_INTENSITY), None, True, "pcv_xray_coloring"),
           (params(7), coloring(), True, "unknown strategy")]
    for p, col, has_int, msg in bad:
        rc, err = check(p, col, has_int)
        assert rc == L.PCV_E_INVALID and msg in err, (msg, err)


def test_entry_points_without_coloring_refuse_the_strategy():
    with pytest.raises(pcv.PcvError, match="pcv_xray_run_ex") as e:
        pcv.xray_check_params(params(L.XRAY_COLORED_WITH_INTENSITY))
    assert e.value.code == L.PCV_E_INVALID
    with pytest.raises(pcv.PcvError, match="unknown strategy"):
        pcv.xray_check_params(params(7))
    pcv.xray_check_params(params(L.XRAY_COLORED_WITH_INTENSITY), coloring=coloring())
    lib = L.load_library()
    for name in ("pcv_xray_run_ex", "pcv_xray_check_params_ex", "pcv_xray_negative"):
        assert hasattr(lib, name)
    assert lib.pcv_xray_negative(None, None) == L.PCV_E_INVALID


def test_python_spellings():
    p = pcv.xray_params(256, 0.1, "colored_with_intensity")
    assert p.strategy == L.XRAY_COLORED_WITH_INTENSITY == 3
    for strategy in ("binned", ("colored_with_intensity", 0.0, 1.0), "intensity"):
        with pytest.raises(ValueError):
            pcv.xray_params(256, 0.1, strategy)
    assert pcv.xray_coloring("colored") is None and pcv.xray_coloring("xray", binning=None) is None
    c = pcv.xray_coloring("colored_with_intensity", 2.0, 300.0)
    assert (c.min_intensity, c.max_intensity, c.binning_attribute) == (2.0, 300.0, None)
    c = pcv.xray_coloring("colored", binning=("intensity", 0.5))
    assert c.binning_attribute == b"intensity" and c.bin_size == 0.5
    for bad in ("intensity=1", ("intensity",), ("intensity", 1.0, 2.0), (3, 1.0)):
        with pytest.raises(ValueError):
            pcv.xray_coloring("colored", binning=bad)
    # the library checks the name
    with pytest.raises(pcv.PcvError, match="only intensity"):
        pcv.xray_check_params(p, coloring=pcv.xray_coloring("colored_with_intensity", binning=("color", 1.0)))


def test_bins_saturate_like_rust():
    v = np.array([1.5, -1.5, NAN, INF, -INF, 0.0, -0.0, 1e30, -1e30], dtype=F32)
    assert I.bins_of(v, 1.0).tolist() == [1, -1, 0, 2**63 - 1, -2**63, 0, 0, 2**63 - 1, -2**63]
    assert I.bins_of(np.array([1.0, -1.0, 0.0], F32), 0.0).tolist() == [2**63 - 1, -2**63, 0]
    assert I.bins_of(np.array([1.0, 7.0], F32), NAN).tolist() == [0, 0]
    assert math.isnan(float(I.ln_f32(F32(-1.0))))


def plan(kept, strategy, col=None, workspace=0, tile=64):
    p = L.XrayParams(tile_size_px=tile, pixel_size_m=0.1, strategy=strategy, max_stddev=1.0, max_workspace_bytes=workspace)
    k = np.ascontiguousarray(kept, dtype=np.uint64)
    n, first, err = C.c_uint64(), np.zeros(len(kept) + 1, np.uint64), C.create_string_buffer(256)
    rc = L.load_library().pcv_xray_plan_groups(k.ctypes.data, k.size, C.byref(p), C.byref(col) if col is not None else None,
                                              first.size, C.byref(n), first.ctypes.data, err, 256)
    return rc, first[:n.value].tolist(), err.value.decode()


def test_sorted_tile_bound():
    """xray_sorted sorts a bucket with u32 indices: the planning refuses a tile of more than 2^30 kept points for the
    sorted strategies, whatever max_workspace_bytes allows, and leaves the other strategies alone"""
    big = 1 << 35  # 32 GiB of workspace: room for 2^30 + 1 records of 16 bytes
    lim = 1 << 30
    assert L.load_library() and lim == 1073741824
    for strategy, col in ((L.XRAY_COLORED_WITH_INTENSITY, coloring()), (L.XRAY_COLORED_WITH_INTENSITY, coloring((b"intensity", 1.0))),
                          (L.XRAY_COLORED, coloring((b"intensity", 1.0)))):
        assert plan([5, lim], strategy, col, big)[0] == L.PCV_OK
        rc, _, err = plan([5, lim + 1], strategy, col, big)
        assert rc == L.PCV_E_INVALID and "1073741825 points" in err and "leaf tile 1" in err, err
    # unbinned colored, xray and height_stddev keep xray_accum: no such bound, only the workspace
    for strategy, col in ((L.XRAY_COLORED, None), (L.XRAY_COLORED, coloring()), (L.XRAY_XRAY, coloring((b"intensity", 1.0))),
                          (L.XRAY_HEIGHT_STDDEV, None)):
        assert plan([5, lim + 1], strategy, col, big)[0] == L.PCV_OK
    rc, _, err = plan([lim + 1], L.XRAY_COLORED, None, 1 << 20)
    assert rc == L.PCV_E_OOM and "max_workspace_bytes" in err


def test_plan_groups_sizes():
    # 64 px: 4 blocks, 16 B each of bucket table, + 16: a tile of k points needs 8 k + 80 bytes (16 k + 80 binned)
    kept = [100, 100, 100, 100]
    assert plan(kept, L.XRAY_COLORED, None, 2 * 880) == (L.PCV_OK, [0, 2], "")
    assert plan(kept, L.XRAY_COLORED, coloring((b"intensity", 1.0)), 2 * 880) == (L.PCV_OK, [0, 1, 2, 3], "")
    assert plan(kept, L.XRAY_COLORED_WITH_INTENSITY, coloring(), 2 * 880) == (L.PCV_OK, [0, 2], "")
    assert plan([], L.XRAY_COLORED, None, 0) == (L.PCV_OK, [], "")
