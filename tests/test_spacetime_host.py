"""Host side of the wavenumber-frequency spectra (no GPU): sdy_spacetime_append_host + sdy_spacetime_segment_power_host -- the
header the kernels compile (csrc/spacetime.h) -- against the numpy restatement, the restatement against np.fft, the identities of
the definition, what the entry points refuse, and what `SpaceTimeSpectra`, `SpaceTimeSpectrumAggregator`,
`space_time_spectrum` and `InferenceAggregator(space_time_spectra=...)` refuse before they touch a device.  Data, restatement and
tolerance: tests/spacetime_utils.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import spacetime_utils as su

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SDY_OK, SDY_ERR_ARG, SDY_ERR_UNSUPPORTED = 0, -1, -2


@pytest.fixture(scope="module")
def sdy():
    import sdy_amd

    return sdy_amd


# ---- the restatement and the host twins -------------------------------------------------------------------------------------
def test_restatement_against_numpy_fft():
    """The direct sums of the restatement and the np.fft formulation agree to 1e-12 of the scale."""
    for H, W in su.GRIDS:
        lats, K, N = su.lats_of(H), su.k_of(W), 12
        gen, target = su.make_data(1, 1, N, H, W)
        north, south = su.band(lats, su.LAT_MAX)
        for detrend in su.DETRENDS:
            for p in su.TAPERS:
                w = su.taper(N, p)
                c = su.lon_coefficients(target[0], north, south, K)                    # (N, R, 2, K1)
                direct = su.segment_power(c, detrend, w)
                fft = su.segment_power_fft(target[0], north, south, K, detrend, w)
                tol = su.tolerance(gen, target, lats, N, su.LAT_MAX, p)
                assert np.abs(direct - fft).max() <= tol, (H, W, detrend, p)


def test_band_and_taper_of_the_package_are_the_restatements(sdy):
    for H in (8, 9, 6, 180, 181):
        for lat_max in (0.4, 15.0, 40.0, 90.0):
            lats = su.lats_of(H)
            if H % 2 == 0 and lat_max < abs(lats).min():
                continue
            assert sdy.spacetime.band_pairs(lats, lat_max) == su.band(lats, lat_max), (H, lat_max)
            assert sdy.spacetime.band_pairs(lats[::-1], lat_max)[0] == su.band(lats[::-1], lat_max)[0]
    for N in (8, 9, 12, 384):
        for p in su.TAPERS:
            # (math.cos against np.cos: both within an ulp of values below 1)
            assert np.abs(np.array(sdy.spacetime.tukey_taper(N, p)) - su.taper(N, p)).max() <= 2.0 ** -52, (N, p)
        assert np.abs(np.array(sdy.spacetime.circle_table(N)).reshape(N, 2) - su.circle(N)).max() <= 2e-16
    assert len(su.band(su.lats_of(180), 15.0)[0]) == 15


@pytest.mark.parametrize("grid", su.GRIDS)
@pytest.mark.parametrize("M", su.MEMBERS)
@pytest.mark.parametrize("N", su.SEGMENTS)
def test_host_twins_against_restatement(sdy, grid, M, N):
    H, W = grid
    lats, K = su.lats_of(H), su.k_of(W)
    n = 2 * N + 5
    gen, target = su.make_data(M, su.SAMPLES, n, H, W)
    R = len(su.band(lats, su.LAT_MAX)[0])
    for hop in su.hops(N):
        for detrend in su.DETRENDS:
            for p in su.TAPERS:
                acc, n_segments = su.host_run(gen, target, lats, N, hop, K, su.LAT_MAX, detrend, p)
                ref, count = su.raw_sums(gen, target, lats, N, hop, K, su.LAT_MAX, detrend, p)
                assert n_segments == count == (n - N) // hop + 1
                for side, members in ((0, M), (1, 1)):
                    tol = su.tolerance(gen, target, lats, N, su.LAT_MAX, p, n_segments * members * R)
                    err = np.abs(acc[side] - ref[side]).max()
                    assert err <= tol, (hop, detrend, p, side, err, tol)


def test_host_run_has_the_same_bits_in_any_cut(sdy):
    H, W, N, hop = 9, 10, 12, 5
    lats, K = su.lats_of(H), su.k_of(W)
    gen, target = su.make_data(3, 2, 40, H, W)
    whole, n_segments = su.host_run(gen, target, lats, N, hop, K, su.LAT_MAX, "linear", 0.2)
    assert n_segments == 6                                       # the ring wraps and a window completes several segments
    for cuts in ((1, 39), (5, 7, 28), (1,) * 40):
        acc, count = su.host_run(gen, target, lats, N, hop, K, su.LAT_MAX, "linear", 0.2, cuts=cuts)
        assert count == n_segments and su.same_bits(acc, whole), cuts


# ---- identities -------------------------------------------------------------------------------------------------------------
H0, W0, N0, K0 = 8, 16, 8, 5
# a wave's samples are rounded to fp32 (2^-24 relative each): its power of 1/4 moves by at most 4 x 2^-24 x 1/4 x 2 < 2^-22, and
# the rounding noise itself has a power below that
FP32_POWER = 2.0 ** -22


def _wave(k0, f0, sign, H=H0, W=W0, n=N0):
    t = np.arange(n).reshape(n, 1, 1)
    j = np.arange(W).reshape(1, 1, W)
    return np.broadcast_to(np.cos(2 * np.pi * (k0 * j / W + sign * f0 * t / n)), (n, H, W)).astype(np.float32)


def _spectrum(x, detrend="none", p=0.0, H=H0, N=N0, K=K0):
    return su.host_spectrum(x, su.lats_of(H), N, N, K, su.LAT_MAX, detrend, p)


@pytest.mark.parametrize("k0,f0", [(2, 1), (5, 3), (1, 4)])
def test_a_wave_lands_in_one_cell(sdy, k0, f0):
    east, west = _spectrum(_wave(k0, f0, -1)), _spectrum(_wave(k0, f0, +1))
    for out, k in ((east, k0), (west, -k0)):
        assert (out[1] == 0.0).all()                                                   # antisymmetric part: exactly 0
        peak = out[0, f0, K0 + k]
        if 2 * f0 == N0:                     # the Nyquist frequency has no direction: both signs of k hold the wave
            assert abs(peak - 0.25) <= FP32_POWER and abs(out[0, f0, K0 - k] - 0.25) <= FP32_POWER
            out[0, f0, K0 - k] = 0.0
        else:
            assert abs(peak - 0.25) <= FP32_POWER, (k, peak)
        out[0, f0, K0 + k] = 0.0
        assert np.abs(out[0]).max() <= FP32_POWER
    # a standing wave cos(k x) cos(f t) is half an eastward and half a westward wave: 1/16 each
    if 2 * f0 != N0:
        t = np.arange(N0).reshape(N0, 1, 1)
        j = np.arange(W0).reshape(1, 1, W0)
        x = np.broadcast_to(np.cos(2 * np.pi * k0 * j / W0) * np.cos(2 * np.pi * f0 * t / N0), (N0, H0, W0)).astype(np.float32)
        out = _spectrum(x)
        assert abs(out[0, f0, K0 + k0] - 1 / 16) <= FP32_POWER and abs(out[0, f0, K0 - k0] - 1 / 16) <= FP32_POWER
        assert out[0, f0, K0 + k0] == out[0, f0, K0 - k0] or abs(out[0, f0, K0 + k0] - out[0, f0, K0 - k0]) <= FP32_POWER


@pytest.mark.parametrize("H", [8, 9])
def test_an_odd_field_has_no_symmetric_power(sdy, H):
    rng = np.random.default_rng(3)
    x = rng.standard_normal((12, H, 10)).astype(np.float32)
    x[:, H - H // 2:] = -x[:, :H // 2][:, ::-1]
    if H % 2:
        x[:, H // 2] = 0.0
    for detrend in su.DETRENDS:
        out = su.host_spectrum(x, su.lats_of(H), 12, 5, 5, su.LAT_MAX, detrend, 0.2)
        assert (out[0] == 0.0).all() and out[1].max() > 0.0
    # and its mirror image: an even field has no antisymmetric power
    x[:, H - H // 2:] = x[:, :H // 2][:, ::-1]
    out = su.host_spectrum(x, su.lats_of(H), 12, 5, 5, su.LAT_MAX, "linear", 0.2)
    assert (out[1] == 0.0).all() and out[0].max() > 0.0


def test_sum_rule(sdy):
    """w = 1 and no detrending: sum_f P_f = (1 / N) sum_n |z_n|^2, here summed over members and pairs as the accumulators are."""
    M, B, H, W, N = 3, 2, 9, 10, 9
    lats, K = su.lats_of(H), 5
    gen, target = su.make_data(M, B, N, H, W)
    acc, n_segments, coef = su.host_run(gen, target, lats, N, N, K, su.LAT_MAX, "none", 0.0, keep_coef=True)
    assert n_segments == 1
    R = coef.shape[2]
    energy = (coef ** 2).sum(axis=(1, -1)) / N                                       # (n_traj, R, 2, K1)
    want_gen = energy[:M * B].reshape(M, B, R, 2, K + 1).sum(axis=(0, 2))
    want_target = energy[M * B:].sum(axis=1)
    for side, want, members in ((0, want_gen, M), (1, want_target, 1)):
        tol = su.tolerance(gen, target, lats, N, su.LAT_MAX, 0.0, members * R * N)
        assert np.abs(acc[side].sum(axis=2) - want).max() <= tol


def test_a_linear_trend_is_removed(sdy):
    rng = np.random.default_rng(5)
    H, W, N = 9, 10, 12
    a = rng.integers(-64, 64, (1, H, W)) / 8.0
    b = rng.integers(-16, 16, (1, H, W)) / 8.0
    x = (a + b * np.arange(N).reshape(N, 1, 1)).astype(np.float32)                    # exact in fp32
    lats = su.lats_of(H)
    for p in su.TAPERS:
        out = su.host_spectrum(x, lats, N, N, 5, su.LAT_MAX, "linear", p)
        assert np.abs(out).max() <= su.tolerance(x, x, lats, N, su.LAT_MAX, p)
    assert np.abs(su.host_spectrum(x, lats, N, N, 5, su.LAT_MAX, "mean", 0.0)).max() > 1e-3


def test_a_large_mean_stays_within_the_tolerance(sdy):
    H, W, N, hop, K = 8, 16, 12, 6, 5
    lats = su.lats_of(H)
    gen, target = su.make_data(3, 2, 30, H, W, amplitude=500.0, mean=1e5)
    R = len(su.band(lats, su.LAT_MAX)[0])
    for detrend in su.DETRENDS:
        acc, n_segments = su.host_run(gen, target, lats, N, hop, K, su.LAT_MAX, detrend, 0.2)
        ref, _ = su.raw_sums(gen, target, lats, N, hop, K, su.LAT_MAX, detrend, 0.2)
        for side, members in ((0, 3), (1, 1)):
            assert np.abs(acc[side] - ref[side]).max() <= su.tolerance(gen, target, lats, N, su.LAT_MAX, 0.2, n_segments * members * R)


def test_a_non_finite_value_makes_its_cells_nan(sdy):
    H, W, N, K = 8, 16, 8, 5
    lats = su.lats_of(H)
    gen, target = su.make_data(2, 2, N, H, W)
    gen[1, 0, 3, 3, 7] = np.nan                                 # member 1 of sample 0, a band row
    target[1, 2, 0, 0] = np.inf                                 # outside the band: nothing happens
    acc, _ = su.host_run(gen, target, lats, N, N, K, su.LAT_MAX, "linear", 0.2)
    assert np.isnan(acc[0, 0]).all() and np.isfinite(acc[0, 1]).all() and np.isfinite(acc[1]).all()


# ---- the entry points -------------------------------------------------------------------------------------------------------
def _append_call():
    gen, target = su.make_data(3, 2, 3, 8, 16)
    north, south = su.band(su.lats_of(8), su.LAT_MAX)
    coef = np.full((8, 8, 2, 2, 6, 2), 7.0)
    a, keep = su.append_args(coef, np.ascontiguousarray(target), np.ascontiguousarray(gen), north, south, 5, 8, 1, 3, 6, su.circle(16))
    return a, keep, coef


def _set(a, field, value):
    if field == "gen0":
        a.gen[0] = None
    elif field == "target0":
        a.target[0] = None
    elif field == "north1":
        a.north[1] = value
    elif field == "south0":
        a.south[0] = value
    elif isinstance(field, tuple):
        for f, v in zip(field, value):
            _set(a, f, v)
    elif isinstance(value, str):
        setattr(a, field, getattr(a, field) + int(value))
    else:
        setattr(a, field, value)


@pytest.mark.parametrize("field,value,code", [
    ("struct_size", 0, SDY_ERR_ARG), ("struct_size", "+8", SDY_ERR_ARG), ("struct_size", "-8", SDY_ERR_ARG),
    ("coef", None, SDY_ERR_ARG), ("coef", "+4", SDY_ERR_ARG), ("lon_table", None, SDY_ERR_ARG), ("lon_table", "+4", SDY_ERR_ARG),
    ("gen0", None, SDY_ERR_ARG), ("target0", None, SDY_ERR_ARG),
    ("gs0", -1, SDY_ERR_ARG), ("gs1", -4, SDY_ERR_ARG), ("ts1", -1, SDY_ERR_ARG),
    ("nvars", 0, SDY_ERR_ARG), ("nvars", 97, SDY_ERR_ARG),
    ("n0", 0, SDY_ERR_ARG), ("n1", -1, SDY_ERR_ARG), ("T", 0, SDY_ERR_ARG), ("H", 0, SDY_ERR_ARG), ("W", 0, SDY_ERR_ARG),
    ("R", 0, SDY_ERR_ARG), ("K", -1, SDY_ERR_ARG), ("K", 9, SDY_ERR_ARG),                       # K > W / 2
    ("north1", 8, SDY_ERR_ARG), ("north1", -1, SDY_ERR_ARG), ("south0", 8, SDY_ERR_ARG), ("south0", -1, SDY_ERR_ARG),
    ("t0", -1, SDY_ERR_ARG), ("t0", 4, SDY_ERR_ARG), ("t1", 4, SDY_ERR_ARG), ("t1", 0, SDY_ERR_ARG),     # outside 0..T, t1 < t0
    (("T", "t0", "t1", "N"), (3, 0, 3, 2), SDY_ERR_ARG),                                        # N < 4
    (("t0", "t1", "N", "T"), (0, 5, 4, 5), SDY_ERR_ARG),                                        # t1 - t0 > N
    ("N", 1025, SDY_ERR_ARG), ("n_first", -1, SDY_ERR_ARG),
    ("R", 129, SDY_ERR_UNSUPPORTED), (("W", "K"), (4097, 5), SDY_ERR_UNSUPPORTED), ("n_first", 1 << 50, SDY_ERR_UNSUPPORTED),
    (("T", "H", "W"), (2, 1 << 15, (1 << 14) + 1), SDY_ERR_UNSUPPORTED),                        # T * H * W > 2^30
    (("n0", "n1"), (1 << 16, 1 << 15), SDY_ERR_UNSUPPORTED),                                    # n0 * n1 >= 2^31
    (("n0", "n1", "N", "R", "W", "K", "H"), (1 << 15, 1 << 15, 1024, 128, 4096, 2047, 128), SDY_ERR_UNSUPPORTED),   # 2^50
])
def test_append_refuses(sdy, field, value, code):
    a, keep, coef = _append_call()
    _set(a, field, value)
    # both entry points check before anything else: the device one is refused without a device
    assert [sdy.lib.sdy_spacetime_append_host(C.byref(a)), sdy.lib.sdy_spacetime_append(C.byref(a), None)] == [code] * 2
    assert (coef == 7.0).all()
    assert [sdy.lib.sdy_spacetime_append_host(None), sdy.lib.sdy_spacetime_append(None, None)] == [SDY_ERR_ARG] * 2


def test_append_good_call_and_a_window_without_counted_times(sdy):
    a, keep, coef = _append_call()
    a.t0 = a.t1 = 3                                           # SDY_OK from both: the device one launches nothing
    assert [sdy.lib.sdy_spacetime_append_host(C.byref(a)), sdy.lib.sdy_spacetime_append(C.byref(a), None)] == [SDY_OK] * 2
    assert (coef == 7.0).all()
    a.t0 = 1
    assert sdy.lib.sdy_spacetime_append_host(C.byref(a)) == SDY_OK
    # window times 1, 2 as counted times 6, 7 in slots 6, 7 of every trajectory; everything else untouched
    assert (coef[:, :6] == 7.0).all() and (coef[:, 6:] != 7.0).all()
    _, target, gen, _ = keep
    north, south = su.band(su.lats_of(8), su.LAT_MAX)
    c = su.lon_coefficients(gen[:, :, 1:], north, south, 5).reshape(6, 2, 2, 2, 6)
    got = coef[:6, 6:, ..., 0] + 1j * coef[:6, 6:, ..., 1]
    assert np.abs(got - c).max() <= 1e-12 * np.abs(gen).max()
    # the ring wraps: counted time 9 goes to slot 1
    a.t0, a.t1, a.n_first = 2, 3, 9
    assert sdy.lib.sdy_spacetime_append_host(C.byref(a)) == SDY_OK
    assert su.same_bits(coef[:, 1], coef[:, 7]) and (coef[:, 0] == 7.0).all() and (coef[:, 2:6] == 7.0).all()


def _power_call():
    rng = np.random.default_rng(1)
    M, B, N, R, K = 3, 2, 8, 2, 5
    coef = rng.standard_normal((M * B + B, N, R, 2, K + 1, 2))
    acc = np.full((2, B, 2, N, K + 1), 7.0)
    a, keep = su.power_args(coef, M, B, N, R, K, 3, "linear", su.taper(N, 0.2), su.circle(N), acc)
    ws = np.zeros(sdy_ws(M, B, N, R, K) // 8)
    a.ws, a.ws_bytes = ws.ctypes.data, ws.nbytes
    return a, keep + (ws,), acc


def sdy_ws(M, B, N, R, K, nvars=1):
    import sdy_amd

    return sdy_amd.lib.sdy_spacetime_workspace_bytes(nvars, M, B, N, R, K)


@pytest.mark.parametrize("field,value,code", [
    ("struct_size", 0, SDY_ERR_ARG), ("struct_size", "+8", SDY_ERR_ARG), ("struct_size", "-8", SDY_ERR_ARG),
    ("coef", None, SDY_ERR_ARG), ("taper", None, SDY_ERR_ARG), ("time_table", None, SDY_ERR_ARG), ("acc", None, SDY_ERR_ARG),
    ("coef", "+4", SDY_ERR_ARG), ("taper", "+4", SDY_ERR_ARG), ("time_table", "+4", SDY_ERR_ARG), ("acc", "+4", SDY_ERR_ARG),
    ("ws", "+4", SDY_ERR_ARG), ("ws_bytes", "-8", SDY_ERR_ARG),
    ("nvars", 0, SDY_ERR_ARG), ("M", 0, SDY_ERR_ARG), ("B", 0, SDY_ERR_ARG), ("R", 0, SDY_ERR_ARG), ("K", -1, SDY_ERR_ARG),
    ("N", 3, SDY_ERR_ARG), ("N", 1025, SDY_ERR_ARG), ("first_slot", -1, SDY_ERR_ARG), ("first_slot", 8, SDY_ERR_ARG),
    ("detrend", -1, SDY_ERR_ARG), ("detrend", 3, SDY_ERR_ARG),
    (("M", "B", "N", "R", "K"), (1 << 15, 1 << 15, 1024, 128, 2047), SDY_ERR_UNSUPPORTED),      # flat indices: 2^50
    (("M", "R"), (1 << 24, 128), SDY_ERR_UNSUPPORTED),                                          # the chunks of a cell: 2^31
])
def test_segment_power_refuses(sdy, field, value, code):
    a, keep, acc = _power_call()
    _set(a, field, value)
    assert [sdy.lib.sdy_spacetime_segment_power_host(C.byref(a)),
            sdy.lib.sdy_spacetime_segment_power(C.byref(a), None)] == [code] * 2
    assert (acc == 7.0).all()
    assert [sdy.lib.sdy_spacetime_segment_power_host(None), sdy.lib.sdy_spacetime_segment_power(None, None)] == [SDY_ERR_ARG] * 2


def test_segment_power_workspace(sdy):
    assert sdy_ws(3, 2, 8, 2, 5) == 8 * (3 * 2 + 2) * 8 * 2 * 2 * 6
    assert sdy_ws(25, 1, 384, 15, 32) == 8 * 26 * 384 * 15 * 2 * 33                   # 79 MB at the headline sizes
    for bad in ((0, 3, 2, 8, 2, 5), (1, 0, 2, 8, 2, 5), (1, 3, 0, 8, 2, 5), (1, 3, 2, 3, 2, 5), (1, 3, 2, 1025, 2, 5),
                (1, 3, 2, 8, 0, 5), (1, 3, 2, 8, 2, -1), (1, 1 << 15, 1 << 15, 1024, 128, 2047)):
        assert sdy.lib.sdy_spacetime_workspace_bytes(*bad) == 0, bad
    # the host twin takes no workspace; the device entry point needs one
    a, keep, acc = _power_call()
    a.ws, a.ws_bytes = None, 0
    assert sdy.lib.sdy_spacetime_segment_power(C.byref(a), None) == SDY_ERR_ARG and (acc == 7.0).all()
    assert sdy.lib.sdy_spacetime_segment_power_host(C.byref(a)) == SDY_OK and (acc[..., 1:, :] > 7.0).all()


def test_structs_carry_their_size_and_are_not_in_the_handshake(sdy):
    from sdy_amd import _lib

    for t in (_lib.SdySpacetimeAppendArgs, _lib.SdySpacetimeSegmentPowerArgs):
        assert t not in _lib.ABI_STRUCTS and t().struct_size == C.sizeof(t) and t._fields_[0][0] == "struct_size"
    assert _lib.SdySpacetimeAppendArgs._fields_[1][0] == "win"
    assert {"sdy_spacetime_append", "sdy_spacetime_append_host", "sdy_spacetime_segment_power",
            "sdy_spacetime_segment_power_host", "sdy_spacetime_workspace_bytes"} <= set(_lib.SIGNATURES)
    hdr = open(os.path.join(ROOT, "include", "sdy_amd.h")).read()
    for name, value in (("PAIRS", _lib.SDY_ST_MAX_PAIRS), ("LON", _lib.SDY_ST_MAX_LON), ("SEGMENT", _lib.SDY_ST_MAX_SEGMENT)):
        assert f"#define SDY_ST_MAX_{name} {value}\n" in hdr
    assert re.search(r"typedef struct sdy_spacetime_append_args sdy_spacetime_append_args;", hdr)
    assert re.search(r"typedef struct sdy_spacetime_segment_power_args sdy_spacetime_segment_power_args;", hdr)
    mk = open(os.path.join(ROOT, "spherical-dyffusion_amd", "csrc", "Makefile")).read()
    assert " spacetime " in mk and " spacetime.h " in mk


# ---- the Python side, as far as it goes without a device ---------------------------------------------------------------------
LATS = su.lats_of(8)


def _window(M=3, B=2, T=3, H=8, W=16, names=("a", "b")):
    g = torch.Generator().manual_seed(0)
    target = {k: torch.randn(B, T, H, W, generator=g) for k in names}
    gen = {k: torch.randn(M, B, T, H, W, generator=g) for k in names}
    return target, gen


def _record(agg, target, gen, **kw):
    agg.record_batch(loss=0.0, target_data=target, gen_data=gen, target_data_norm=target, gen_data_norm=gen, **kw)


def test_specification_refuses(sdy):
    S = sdy.SpaceTimeSpectra
    assert sdy.spacetime.SpaceTimeSpectra is S
    ok = S(LATS, ["a"], 8, lat_max=su.LAT_MAX)
    assert (ok.hop, ok.max_wavenumber, ok.detrend, ok.taper, ok.timestep_hours, ok.n_pairs) == (4, None, "linear", 0.2, 6.0, 2)
    assert list(ok.bands) == ["mjo_east", "mjo_west", "kelvin", "rossby"] and ok.bands["kelvin"] == ("symmetric", 1, 14, 2.5, 20.0)
    assert ok.bands["mjo_west"] == ("symmetric", -3, -1, 30.0, 96.0) and ok.bands["rossby"] == ("symmetric", -10, -1, 10.0, 48.0)
    assert ok.bands["mjo_east"] == ("symmetric", 1, 3, 30.0, 96.0)
    assert ok.wavenumbers(360) == 32 and ok.wavenumbers(16) == 8 and S(LATS, ["a"], 8, lat_max=40, max_wavenumber=3).wavenumbers(16) == 3
    assert S(su.lats_of(180), ["a"], 8).n_pairs == 15                                    # the default band: 15 degrees
    assert ok.frequencies() == [nu / (8 * 6.0 / 24.0) for nu in range(5)]
    assert S(torch.tensor(LATS), ["a"], 8, lat_max=40).north == ok.north                  # a tensor of latitudes
    with pytest.raises(ValueError, match="variables=.. selects nothing"):
        S(LATS, [], 8, lat_max=40)
    bad_lats = LATS.copy()
    bad_lats[0] += 1e-3
    with pytest.raises(ValueError, match="mirror-symmetric"):
        S(bad_lats, ["a"], 8, lat_max=40)
    with pytest.raises(ValueError, match="strictly monotone"):
        S([10.0, -10.0, 10.0, -10.0], ["a"], 8)
    with pytest.raises(ValueError, match="lats is empty"):
        S([], ["a"], 8)
    with pytest.raises(ValueError, match="no latitude row"):                             # R == 0
        S(LATS, ["a"], 8, lat_max=5.0)
    with pytest.raises(ValueError, match="lat_max must not be negative"):
        S(LATS, ["a"], 8, lat_max=-1.0)
    with pytest.raises(ValueError, match="more than 128"):
        S(su.lats_of(1000), ["a"], 8, lat_max=90.0)
    for N in (3, 1025):
        with pytest.raises(ValueError, match="segment_length lies in 4..1024"):
            S(LATS, ["a"], N, lat_max=40)
    for hop in (0, 9):
        with pytest.raises(ValueError, match="hop lies in 1..segment_length"):
            S(LATS, ["a"], 8, hop=hop, lat_max=40)
    with pytest.raises(ValueError, match="max_wavenumber must not be negative"):
        S(LATS, ["a"], 8, max_wavenumber=-1, lat_max=40)
    with pytest.raises(ValueError, match="max_wavenumber 9 on 16 longitudes"):
        S(LATS, ["a"], 8, max_wavenumber=9, lat_max=40).wavenumbers(16)
    with pytest.raises(ValueError, match="detrend is one of"):
        S(LATS, ["a"], 8, detrend="quadratic", lat_max=40)
    for p in (-0.1, 1.1, float("nan")):
        with pytest.raises(ValueError, match="taper lies in"):
            S(LATS, ["a"], 8, taper=p, lat_max=40)
    with pytest.raises(ValueError, match="timestep_hours must be positive"):
        S(LATS, ["a"], 8, timestep_hours=0.0, lat_max=40)
    for band in (("both", 1, 3, 2.0, 4.0), ("symmetric", 1, 3, 2.0), ("symmetric", 3, 1, 2.0, 4.0), ("symmetric", 1, 3, 4.0, 2.0),
                 ("symmetric", 1, 3, 0.0, 2.0)):
        with pytest.raises(ValueError, match="band 'x'"):
            S(LATS, ["a"], 8, lat_max=40, bands={"x": band})


def test_band_masks(sdy):
    spec = sdy.SpaceTimeSpectra(LATS, ["a"], 384, lat_max=40)
    freq = np.array(spec.frequencies())
    for name, (_, k_min, k_max, p_min, p_max) in spec.bands.items():
        mask = spec.band_mask(name, 32).numpy()
        with np.errstate(divide="ignore"):
            period = 1.0 / freq
        rows = (period >= p_min) & (period <= p_max)
        rows[0] = False
        cols = (np.arange(-32, 33) >= k_min) & (np.arange(-32, 33) <= k_max)
        assert np.array_equal(mask, rows[:, None] & cols[None, :]) and mask.any(), name
    # 96 days at 6 h: 384 steps; mjo_east holds nu = 1 .. 3 (periods 96, 48, 32 days) x k = 1 .. 3
    assert spec.band_mask("mjo_east", 32).sum() == 9
    short = sdy.SpaceTimeSpectra(LATS, ["a"], 8, lat_max=40)
    assert not short.band_mask("mjo_east", 8).any()                                   # a band without a cell


def test_class_refuses_before_the_device(sdy):
    A = sdy.SpaceTimeSpectrumAggregator
    assert sdy.spacetime.SpaceTimeSpectrumAggregator is A and issubclass(A, sdy.windows.FieldAccumulator)
    spec = sdy.SpaceTimeSpectra(LATS, ["a", "b"], 8, lat_max=40)
    with pytest.raises(ValueError, match="expected a sdy_amd.SpaceTimeSpectra"):
        A(LATS)
    with pytest.raises(ValueError, match="target must be"):
        A(spec, target="raw")
    agg = A(spec)
    before = dict(vars(agg))
    with pytest.raises(RuntimeError, match="GPU only"):
        _record(agg, *_window())
    for read in (agg.get_data, lambda: agg.get_logs("x")):
        with pytest.raises(ValueError, match="No data recorded"):
            read()
    target, gen = _window()
    flat = {k: v.reshape(-1, *v.shape[2:])[:5] for k, v in gen.items()}
    with pytest.raises(ValueError, match="SpaceTimeSpectrumAggregator needs member-stacked"):
        _record(agg, target, flat)
    with pytest.raises(ValueError, match="member-stacked"):
        _record(agg, target, gen, sample_weights=[0.5, 0.5])
    with pytest.raises(ValueError, match="i_time_start must not be negative"):
        _record(agg, target, gen, i_time_start=-1)
    with pytest.raises(ValueError, match="no generated variable 'c'"):
        _record(A(sdy.SpaceTimeSpectra(LATS, ["a", "c"], 8, lat_max=40)), target, gen)
    with pytest.raises(ValueError, match="share the grid of the specification's 8 latitudes"):
        _record(agg, *_window(H=6))
    with pytest.raises(ValueError, match="max_wavenumber 9 on 16 longitudes"):
        _record(A(sdy.SpaceTimeSpectra(LATS, ["a"], 8, lat_max=40, max_wavenumber=9)), target, gen)
    assert dict(vars(agg)) == before and agg._names is None                           # a refused window changes nothing
    assert (agg.n_times, agg.n_segments) == (0, 0)


def test_class_sizes_its_ring(sdy):
    # 8 bytes x (ring: trajectories x slots x pairs x folds x wavenumbers x (re, im) + accumulators) x variables
    need = 8 * ((3 * 2 + 2) * 8 * 2 * 2 * 9 * 2 + 2 * 2 * 2 * 8 * 9) * 2
    words = "8 trajectories x 2 pairs x 2 parts . 2 sides x 2 samples. x 2 folds x 8 slots x 9 wavenumbers x 2 variables"
    spec = sdy.SpaceTimeSpectra(LATS, ["a", "b"], 8, lat_max=40)
    agg = sdy.SpaceTimeSpectrumAggregator(spec, max_bytes=need - 1)
    with pytest.raises(ValueError, match=f"{words} need {need} bytes of float64 coefficients and accumulators, more than "
                                         f"max_bytes = {need - 1}"):
        _record(agg, *_window())
    assert agg._K is None and agg._names is None
    agg = sdy.SpaceTimeSpectrumAggregator(spec, max_bytes=need)
    with pytest.raises(RuntimeError, match="GPU only"):
        _record(agg, *_window())


def test_inference_aggregator_option(sdy):
    w = torch.ones(8, 16)
    plain = sdy.metrics.InferenceAggregator(w, n_timesteps=3, n_ensemble_members=2)
    assert list(plain._aggregators) == ["mean", "mean_norm", "time_mean"]               # the default set is unchanged
    spec = sdy.SpaceTimeSpectra(LATS, ["a"], 8, lat_max=40)
    agg = sdy.metrics.InferenceAggregator(w, n_timesteps=3, n_ensemble_members=2, space_time_spectra=spec)
    assert list(agg._aggregators) == ["mean", "mean_norm", "time_mean", "space_time_spectra"]
    st = agg._aggregators["space_time_spectra"]
    assert isinstance(st, sdy.SpaceTimeSpectrumAggregator) and st._spec is spec and st._target == "denorm"
    assert hasattr(agg, "get_space_time_spectrum_data")
    with pytest.raises(ValueError, match="expected a sdy_amd.SpaceTimeSpectra"):
        sdy.metrics.InferenceAggregator(w, n_timesteps=3, space_time_spectra=LATS)


def test_one_field_function_refuses_before_the_device(sdy):
    f = sdy.spacetime.space_time_spectrum
    with pytest.raises(ValueError, match="expected .time, lat, lon."):
        f(torch.zeros(8, 16), LATS, 8)
    with pytest.raises(ValueError, match="segment_length lies in"):
        f(torch.zeros(9, 8, 16), LATS, 3, lat_max=40)
    with pytest.raises(ValueError, match="mirror-symmetric"):
        f(torch.zeros(9, 8, 16), LATS + 1.0, 8, lat_max=40)
    with pytest.raises(ValueError, match="No data recorded"):
        f(torch.zeros(7, 8, 16), LATS, 8, lat_max=40)
    with pytest.raises(ValueError, match="share the grid"):
        f(torch.zeros(9, 6, 16), LATS, 8, lat_max=40)
    with pytest.raises(RuntimeError, match="GPU only"):
        f(torch.zeros(9, 8, 16), LATS, 8, lat_max=40)
