"""Regional metric series without a GPU: sdy_region_series_host (the arithmetic the kernel compiles, csrc/region_series.h)
through RegionalMeanAggregator's finalisation against the reference's MeanAggregator run once per region
(tests/golden/fx_region_series.npz), the Regions helpers, the zero-weight rule and the entry point's refusals.  Bounds:
tests/region_series_utils.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import golden_utils as gu
import region_series_utils as ru


@pytest.fixture(scope="module")
def sdy():
    import sdy_amd

    return sdy_amd


def _host(fx):
    return lambda target, gen: ru.host_sums(target, gen, fx["names"], fx["weights"])


@pytest.mark.parametrize("key", ["ens", "det"])
def test_host_twin_against_the_reference(sdy, key):
    """Every region, metric and variable: 1e-12 x term scale against ref64 (the pin), the reference's own fp32 summation
    error against ref32; and the reference alone (ref32 against ref64) stays inside the latter on these fields."""
    fx = ru.fixture()
    case, ens = fx["cases"][key], key == "ens"
    assert sorted(case["metrics"]) == sorted(ru.METRICS + (ru.METRICS_ENSEMBLE if ens else ()))
    assert len(case["ref64"]) == len(case["metrics"]) * len(fx["regions"]) * len(fx["names"])
    got = ru.series_from_windows(case["windows"], fx["names"], fx["regions"], fx["weights"], fx["n_timesteps"], ens, _host(fx))
    args = (case["windows"], fx["names"], fx["regions"], fx["weights"], fx["n_timesteps"], ens)
    ru.check_series(got, case["ref64"], ru.series_bounds(*args, rel=1e-12), f"{key} host vs ref64")
    H, W = fx["area"].shape
    M = 3 if ens else 1
    b32 = ru.series_bounds(*args, rel=(H * W + M + 4) * ru.U)
    ru.check_series(got, case["ref32"], b32, f"{key} host vs ref32")
    ru.check_series(case["ref32"], case["ref64"], b32, f"{key} ref32 vs ref64")
    # rmse stays away from 0 outside the single-cell region (where it is one point's |error|)
    assert min(v.min() for k, v in case["ref64"].items() if k.startswith("weighted_rmse/") and "/cell/" not in k) > 0.1


@pytest.mark.parametrize("key", ["ens", "det"])
def test_host_twin_against_the_restatement(sdy, key):
    fx = ru.fixture()
    for _, target, gen in fx["cases"][key]["windows"]:
        want, _, scales = ru.restate_sums(target, gen, fx["names"], fx["weights"])
        ru.check_sums_restated(_host(fx)(target, gen), want, scales, fx["weights"], f"{key} host vs restatement")


def test_global_region_agrees_with_the_mean_series_fixture(sdy):
    """fx_mean_series.npz (the reference's MeanAggregator on the same grid, global weights) through the host twin with one
    global region, at that fixture's own tolerance."""
    z = gu.load("fx_mean_series")
    import json

    names, n_timesteps = json.loads(str(z["names"])), int(z["n_timesteps"])
    lats = z["lats"]
    W = z["ens::tgt0::a"].shape[-1]
    regions = sdy.Regions(lats, np.arange(W) * 360.0 / W, sdy.metrics.spherical_area_weights(lats, W)).add_global()
    weights = regions.stacked()
    for key in ("ens", "det"):
        windows = [(int(z[f"{key}::i_time_start{i}"]), {n: z[f"{key}::tgt{i}::{n}"] for n in names},
                    {n: z[f"{key}::gen{i}::{n}"] for n in names}) for i in range(3)]
        got = ru.series_from_windows(windows, names, ["global"], weights, n_timesteps, key == "ens",
                                     lambda t, g: ru.host_sums(t, g, names, weights))
        n = 0
        for k in z.files:
            if k.startswith(f"{key}::series::"):
                metric, var = k.split("::")[2].split("/")
                np.testing.assert_allclose(got[f"{metric}/global/{var}"], z[k], rtol=5e-5, atol=5e-6, err_msg=k)
                n += 1
        assert n == (8 if key == "ens" else 6) * len(names)


# ---- Regions -------------------------------------------------------------------------------------------------------------------
def test_regions_rebuild_the_fixture_maps(sdy):
    """The helpers give the maps the fixture's tool built with plain numpy, bit for bit: box inclusion at cell centres, the
    wrap across 0 degrees, area x fraction rounded once to fp32."""
    fx = ru.fixture()
    d = fx["definitions"]
    r = sdy.Regions(fx["lats"], fx["lons"], fx["area"])
    r.add_global().add_lat_band("band", *d["band"]).add_box("wrap_box", lat=d["wrap_box"]["lat"], lon=d["wrap_box"]["lon"])
    cell = np.zeros(fx["area"].shape, bool)
    cell[tuple(d["cell"])] = True
    r.add_fraction("fraction", fx["fraction"]).add_fraction("cell", torch.from_numpy(cell))          # (a bool mask)
    assert r.names == fx["regions"] and len(r) == 5 and r.shape == fx["area"].shape
    assert np.array_equal(r.stacked(), fx["weights"])
    assert torch.equal(r.weight_map("cell"), torch.from_numpy(fx["weights"][4]))


def test_region_boxes_and_longitude_conventions(sdy):
    lats = np.array([-7.5, -5.0, -2.5, 0.0, 2.5, 5.0, 7.5])
    lons = np.arange(0.0, 360.0, 10.0)
    area = np.full((7, 36), 1.0 / (7 * 36))
    r = sdy.Regions(lats, lons, area)
    r.add_box("edges", lat=(-5.0, 5.0), lon=(190.0, 240.0))                # centres ON the four edges belong to the box
    m = r.stacked()[0] > 0
    assert m.sum() == 5 * 6 and m[1:6, 19:25].all()
    r.add_box("wrap", lat=(-90.0, 90.0), lon=(350.0, 10.0))                # lo > hi: across 0 degrees
    assert np.array_equal(np.flatnonzero(r.stacked()[1][0] > 0), [0, 1, 35])
    r.add_box("negative", lat=(-90.0, 90.0), lon=(-10.0, 10.0))            # the box given as -180..180
    assert np.array_equal(r.stacked()[2], r.stacked()[1])
    # the GRID given as -180..180: the same cells in another column order
    shifted = sdy.Regions(lats, np.arange(-180.0, 180.0, 10.0), area).add_box("edges", lat=(-5.0, 5.0), lon=(190.0, 240.0))
    cols = np.flatnonzero(shifted.stacked()[0][3] > 0)
    assert np.array_equal(np.arange(-180.0, 180.0, 10.0)[cols] % 360.0, np.arange(190.0, 250.0, 10.0))
    r.add_lat_band("band", -2.5, 2.5)
    assert np.array_equal(np.flatnonzero(r.stacked()[3][:, 0] > 0), [2, 3, 4])


def test_standard_regions(sdy):
    H, W = 36, 72
    lats = -90.0 + (np.arange(H) + 0.5) * 180.0 / H
    lons = (np.arange(W) + 0.5) * 360.0 / W
    area = sdy.metrics.spherical_area_weights(lats, W)
    r = sdy.Regions.standard(lats, lons, area)
    assert r.names == ["global", "tropics", "nh_extratropics", "sh_extratropics", "nino34"]
    m = r.stacked().astype(np.float64)
    a = area.double().numpy()
    s = m.sum(axis=(1, 2))
    assert abs(s[0] - 1.0) < 1e-6
    assert abs(s[1] + s[2] + s[3] - s[0]) < 1e-7 and abs(s[2] - s[3]) < 1e-7           # a partition, north = south
    assert abs(s[1] - a[np.abs(lats) <= 20.0].sum()) < 1e-7
    nino = m[4] > 0
    assert np.array_equal(np.flatnonzero(nino.any(axis=1)), np.flatnonzero(np.abs(lats) <= 5.0))
    assert np.array_equal(np.flatnonzero(nino.any(axis=0)), np.flatnonzero((lons >= 190.0) & (lons <= 240.0)))
    assert ((m[1] > 0) & ((m[2] > 0) | (m[3] > 0))).sum() == 0


def test_regions_refusals(sdy):
    lats, lons = np.linspace(-60.0, 60.0, 4), np.arange(8) * 45.0
    area = np.full((4, 8), 1.0 / 32)
    new = lambda a=area: sdy.Regions(lats, lons, a)  # noqa: E731
    with pytest.raises(ValueError, match="sum to 0"):
        new().add_box("empty", lat=(70.0, 80.0), lon=(0.0, 90.0))
    with pytest.raises(ValueError, match="sum to 0"):
        new().add_fraction("none", np.zeros((4, 8)))
    bad = area.copy()
    bad[1, 1] = -1.0
    with pytest.raises(ValueError, match="negative or non-finite"):
        new(bad).add_global()
    bad[1, 1] = np.inf
    with pytest.raises(ValueError, match="negative or non-finite"):
        new(bad).add_global()
    for f in (-0.5, 1.5, np.nan):
        with pytest.raises(ValueError, match=r"\[0, 1\]"):
            new().add_fraction("f", np.full((4, 8), f))
    with pytest.raises(ValueError, match="already defined"):
        new().add_global().add_global()
    with pytest.raises(ValueError, match="without '/'"):
        new().add_global("a/b")
    with pytest.raises(ValueError, match="grid"):
        new().add_fraction("shape", np.ones((8, 4)))
    with pytest.raises(ValueError, match="area weights"):
        sdy.Regions(lats, lons, np.ones((8, 4)))
    r = new()
    for i in range(16):
        r.add_global(f"r{i}")
    with pytest.raises(ValueError, match="at most 16"):
        r.add_global("one_more")
    assert len(r) == 16
    with pytest.raises(ValueError, match="no regions"):
        sdy.RegionalMeanAggregator(new())


def test_aggregator_refusals_before_any_launch(sdy):
    """What RegionalMeanAggregator refuses is refused before the device is touched (this machine may have none)."""
    r = sdy.Regions(np.linspace(-60.0, 60.0, 4), np.arange(8) * 45.0, np.full((4, 8), 1.0 / 32)).add_global()
    t, g5 = {"a": torch.zeros(2, 3, 4, 8)}, {"a": torch.zeros(3, 2, 3, 4, 8)}
    ens = sdy.RegionalMeanAggregator(r, n_timesteps=4, is_ensemble=True)
    assert ens.metric_names[-2:] == ["weighted_crps", "weighted_ssr"]
    with pytest.raises(ValueError, match="member-stacked"):
        ens.record_batch(0.0, t, t, t, t, 0)
    with pytest.raises(ValueError, match="outside"):
        ens.record_batch(0.0, t, g5, t, g5, 2)
    with pytest.raises(RuntimeError, match="GPU only"):
        ens.record_batch(0.0, t, g5, t, g5, 0)
    det = sdy.RegionalMeanAggregator(r, n_timesteps=4)
    with pytest.raises(ValueError, match="samples, time, lat, lon"):
        det.record_batch(0.0, t, g5, t, g5, 0)
    with pytest.raises(ValueError, match="grid"):
        det.record_batch(0.0, {"a": torch.zeros(2, 3, 8, 4)}, {"a": torch.zeros(2, 3, 8, 4)}, None, None, 0)
    with pytest.raises(ValueError, match="No batches"):
        det.get_series()
    with pytest.raises(ValueError, match="target must be"):
        sdy.RegionalMeanAggregator(r, target="raw")


# ---- NaN and the zero-weight rule ----------------------------------------------------------------------------------------------
def test_zero_weight_rule_and_nan_propagation(sdy):
    fx = ru.fixture()
    _, target, gen = fx["cases"]["ens"]["windows"][1]
    names, weights = fx["names"], fx["weights"]
    regions = fx["regions"]
    clean = _host(fx)(target, gen)
    band, box, cell = regions.index("band"), regions.index("wrap_box"), regions.index("cell")
    # NaN and inf wherever the band has no weight: the band's sums keep their bits, the global region's become NaN
    outside = weights[band] == 0.0
    t2, g2 = {k: v.copy() for k, v in target.items()}, {k: v.copy() for k, v in gen.items()}
    for k in names:
        t2[k][..., outside] = np.nan
        g2[k][:, ..., outside] = np.inf
    dirty = _host(fx)(t2, g2)
    assert np.array_equal(dirty[:, band], clean[:, band]) and np.isfinite(dirty[:, band]).all()
    assert np.isnan(dirty[:, 0]).all()
    # the restatement follows the same rule
    want, _, _ = ru.restate_sums(t2, g2, names, weights[[band]])
    _, _, scales = ru.restate_sums(target, gen, names, weights[[band]])      # (the term scales of the finite data)
    ru.check_sums_restated(dirty[:, [band]], want, scales, weights[[band]], "band with NaN outside")
    # one NaN in one member at a point of the band, variable "a", sample 1, time 2: the sums of that plane that see the
    # generated data are NaN in the regions holding the point, the target's two sums and everything else keep their bits
    row, col = np.argwhere((weights[band] > 0) & (weights[box] == 0) & (weights[cell] == 0))[0]
    g3 = {k: v.copy() for k, v in gen.items()}
    g3["a"][1, 1, 2, row, col] = np.nan
    hit = _host(fx)(target, g3)
    holds = [r for r in range(len(regions)) if weights[r, row, col] != 0.0]
    assert band in holds and 0 in holds and box not in holds and cell not in holds
    for r in range(len(regions)):
        if r in holds:
            assert np.isnan(hit[0, r, 1, 2, :6]).all() and np.array_equal(hit[0, r, 1, 2, 6:], clean[0, r, 1, 2, 6:])
        else:
            assert np.array_equal(hit[0, r], clean[0, r])
    mask = np.ones(clean.shape, bool)
    mask[0, :, 1, 2] = False
    assert np.array_equal(hit[mask], clean[mask])
    # a NaN target at a weighted point reaches all eight sums
    t4 = {k: v.copy() for k, v in target.items()}
    t4["b"][0, 0, row, col] = np.nan
    assert np.isnan(_host(fx)(t4, gen)[1, band, 0, 0]).all()


# ---- the entry point's refusals --------------------------------------------------------------------------------------------------
def test_entry_point_refusals(sdy):
    from sdy_amd._lib import SDY_REGION_MAX, SDY_REGION_MAX_MEMBERS, SdyRegionSeriesArgs

    assert SdyRegionSeriesArgs in sdy._lib.ABI_STRUCTS and SDY_REGION_MAX == 16 and SDY_REGION_MAX_MEMBERS == 64
    lib, ARG, UNSUP = sdy.lib, -1, -2
    H, W, S, T = 3, 4, 2, 2
    target, gen = ru.seeded_window(2, S, T, H, W, ["a"], 5)
    weights = ru.seeded_regions(2, H, W, 6)
    out = np.zeros((1, 2, S, T, 8))
    ws = np.zeros(1 * 2 * S * T * 1 * 8 + 8)

    def fresh():
        a, keep = ru.region_args(target, gen, ["a"], weights, out)
        a.ws, a.ws_bytes = ru.vp(ws), ws.nbytes
        return a, keep

    need = lib.sdy_region_series_workspace_bytes(1, 2, S, T, H * W)
    assert need == 1 * S * T * 1 * 2 * 8 * 8 and lib.sdy_region_series_workspace_bytes(63, 5, 1, 7, 180 * 360) == 63 * 7 * 64 * 5 * 64
    for bad in ((0, 2, S, T, 12), (97, 2, S, T, 12), (1, 0, S, T, 12), (1, 17, S, T, 12), (1, 2, 0, T, 12), (1, 2, S, 0, 12),
                (1, 2, S, T, 0)):
        assert lib.sdy_region_series_workspace_bytes(*bad) == 0
    a, keep = fresh()
    assert lib.sdy_region_series_host(C.byref(a)) == 0
    both = (lambda a: lib.sdy_region_series_host(C.byref(a)), lambda a: lib.sdy_region_series(C.byref(a), None))
    assert lib.sdy_region_series_host(None) == ARG and lib.sdy_region_series(None, None) == ARG

    def refused(code, **fields):
        for call in both:
            a, keep = fresh()
            for k, v in fields.items():
                setattr(a, k, v)
            assert call(a) == code, fields

    for n in (0, -1, 17):
        refused(ARG, n_regions=n)
    refused(ARG, HW=0)
    refused(ARG, weights=None)
    refused(ARG, out=None)
    refused(ARG, out=ru.vp(out) + 4)
    for field, v in (("nvars", 0), ("nvars", 97), ("n0", 0), ("n1", 0), ("T", 0), ("gs0", -1), ("gs1", -1), ("ts1", -1)):
        refused(ARG, **{field: v})                                                    # sdy_window_check applies
    refused(UNSUP, n0=65)
    refused(UNSUP, T=1 << 29)                                                         # T * HW > 2^30
    refused(UNSUP, n0=1, n1=1 << 30, T=4, HW=1)                                            # more than 2^31 - 1 blocks per variable
    a, keep = fresh()
    a.win.gen[0] = None
    assert lib.sdy_region_series_host(C.byref(a)) == ARG
    # the workspace: the device entry point only (the host twin needs none)
    for fields in (dict(ws=None), dict(ws_bytes=need - 8), dict(ws=ru.vp(ws) + 4)):
        a, keep = fresh()
        for k, v in fields.items():
            setattr(a, k, v)
        assert lib.sdy_region_series(C.byref(a), None) == ARG, fields
    a, keep = fresh()
    a.ws, a.ws_bytes = None, 0
    assert lib.sdy_region_series_host(C.byref(a)) == 0
