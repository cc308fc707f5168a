"""weighted_grad_mag_percent_diff in the inference aggregators (reference src/ace_inference/core/metrics.py:210-241,
aggregator/inference/reduced.py:178, aggregator/one_step/reduced.py:75): the host side that needs no GPU -- the keyword and
the key sets, the C ABI binding and its argument checks, and a float64 restatement of the metric against the reference's
own series (tests/golden/fx_mean_series_grad.npz)."""
import ctypes as C
import json

import pytest
import torch

import golden_utils as gu

GRAD = "weighted_grad_mag_percent_diff"
BASE = ["weighted_rmse", "weighted_bias", "weighted_mean_gen", "weighted_mean_target", "weighted_std_gen",
        "weighted_std_target"]


@pytest.fixture(scope="module")
def sdy():
    import sdy_amd

    return sdy_amd


def _w(H=16, W=32):
    import sdy_amd

    return sdy_amd.metrics.spherical_area_weights(torch.linspace(-80.0, 80.0, H), W)


@pytest.mark.parametrize("ens", [True, False])
def test_mean_aggregator_metric_names(sdy, ens):
    extra = ["weighted_crps", "weighted_ssr"] if ens else []
    off = sdy.metrics.MeanAggregator(_w(), n_timesteps=4, is_ensemble=ens)
    assert sorted(off.metric_names) == sorted(BASE + extra)                  # the default is unchanged
    on = sdy.metrics.MeanAggregator(_w(), n_timesteps=4, is_ensemble=ens, grad_mag_percent_diff=True)
    assert sorted(on.metric_names) == sorted(BASE + extra + [GRAD])


@pytest.mark.parametrize("ens", [True, False])
def test_one_step_aggregator_metric_names(sdy, ens):
    base = ["weighted_rmse", "weighted_bias", "weighted_mean_gen"] + (["weighted_crps", "weighted_ssr"] if ens else [])
    off = sdy.metrics.OneStepMeanAggregator(_w(), target_time=2, is_ensemble=ens)
    assert sorted(off.metric_names) == sorted(base)
    on = sdy.metrics.OneStepMeanAggregator(_w(), target_time=2, is_ensemble=ens, grad_mag_percent_diff=True)
    assert sorted(on.metric_names) == sorted(base + [GRAD])


def test_metric_names_match_the_reference_fixture(sdy):
    """The key sets with the keyword on are the reference's own (both aggregators, ensemble and deterministic)."""
    z = gu.load("fx_mean_series_grad")
    for shp in json.loads(str(z["shapes"])):
        for kind, ens in (("ens", True), ("det", False)):
            key = f"{shp}::{kind}"
            agg = sdy.metrics.MeanAggregator(_w(), n_timesteps=4, is_ensemble=ens, grad_mag_percent_diff=True)
            assert sorted(agg.metric_names) == json.loads(str(z[f"{key}::metrics"]))
            one = sdy.metrics.OneStepMeanAggregator(_w(), target_time=2, is_ensemble=ens, grad_mag_percent_diff=True)
            ref = {k.split("/")[0] for k in json.loads(str(z[f"{key}::one_step_keys"])) if k != "loss"}
            assert set(one.metric_names) == ref


@pytest.mark.parametrize("members", [1, 25])
def test_inference_aggregator_passes_the_keyword_on(sdy, members):
    ens = members > 1
    comp = sdy.metrics.InferenceAggregator(_w(), n_timesteps=8, n_ensemble_members=members, record_step_20=True,
                                           grad_mag_percent_diff=True)
    for name in ("mean", "mean_norm", "mean_step_20"):
        assert GRAD in comp._aggregators[name].metric_names, name
        assert comp._aggregators[name].is_ensemble == ens
    default = sdy.metrics.InferenceAggregator(_w(), n_timesteps=8, n_ensemble_members=members, record_step_20=True)
    for name in ("mean", "mean_norm", "mean_step_20"):
        assert GRAD not in default._aggregators[name].metric_names, name
    with pytest.raises(NotImplementedError):       # zonal-mean images stay out of scope with the metric on
        sdy.metrics.InferenceAggregator(_w(), n_timesteps=8, log_zonal_mean_images=True, grad_mag_percent_diff=True)


def test_binding_signature(sdy):
    from sdy_amd import _lib

    restype, args = _lib.SIGNATURES["sdy_ensemble_series_grad"]
    assert restype is C.c_int
    assert args == [C.c_void_p, C.c_int, C.c_long, C.c_long, C.c_void_p, C.c_long, C.c_void_p, C.c_int, C.c_int, C.c_int,
                    C.c_int, C.c_void_p, C.c_void_p]
    # sdy_ensemble_series keeps its signature
    assert _lib.SIGNATURES["sdy_ensemble_series"][1] == [C.c_void_p, C.c_int, C.c_long, C.c_long, C.c_void_p, C.c_long,
                                                         C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p]


def test_argument_checks_without_gpu(sdy):
    """Validation returns before anything touches the device (the pointers below are never dereferenced)."""
    f = sdy.lib.sdy_ensemble_series_grad
    p = C.c_void_p(16)
    ok = dict(M=5, n_sample=2, T=3, nlat=7, nlon=10)

    def call(**kw):
        a = {**ok, **kw}
        return f(p, a["M"], 1000, 100, p, 100, p, a["n_sample"], a["T"], a["nlat"], a["nlon"], p, None)

    assert call(nlat=1) == -1 and call(nlon=1) == -1 and call(nlat=0) == -1        # SDY_ERR_ARG: torch.gradient refuses too
    assert call(M=0) == -1 and call(T=0) == -1 and call(n_sample=0) == -1
    assert f(None, 5, 1000, 100, p, 100, p, 2, 3, 7, 10, p, None) == -1
    assert call(M=65) == -2                                                        # SDY_ERR_UNSUPPORTED: at most 64 members
    assert call(n_sample=256, T=257) == -2                                         # more than 65535 planes
    with pytest.raises(RuntimeError, match="GPU only"):
        sdy.metrics.ensemble_series(torch.zeros(1, 2, 7, 10), torch.zeros(3, 1, 2, 7, 10), _w(7, 10), grad_mag=True)


def _grad_mag_f64(x):
    gy, gx = torch.gradient(x.double(), dim=(-2, -1))
    return (gy ** 2 + gx ** 2).sqrt()


def test_float64_restatement_matches_the_reference_series():
    """The restatement the GPU tests use (torch.gradient in float64, unit spacing, edge_order 1, longitude not periodic)
    reproduces the reference's own weighted_grad_mag_percent_diff series, on both grids."""
    import sdy_amd

    z = gu.load("fx_mean_series_grad")
    names = json.loads(str(z["names"]))
    n_t = int(z["n_timesteps"])
    for shp in json.loads(str(z["shapes"])):
        lats = torch.from_numpy(z[f"{shp}::lats"])
        W = z[f"{shp}::ens::tgt0::a"].shape[-1]
        w = sdy_amd.metrics.spherical_area_weights(lats, W).double()
        for kind, ens in (("ens", True), ("det", False)):
            key = f"{shp}::{kind}"
            for n in names:
                tot = torch.zeros(n_t, dtype=torch.float64)
                cnt = torch.zeros(n_t, dtype=torch.float64)
                for i in range(3):
                    tgt = torch.from_numpy(z[f"{key}::tgt{i}::{n}"])
                    gen = torch.from_numpy(z[f"{key}::gen{i}::{n}"])
                    gen = gen if ens else gen[None]
                    T_ = (_grad_mag_f64(tgt) * w).sum((-2, -1)) / w.sum()
                    P = ((_grad_mag_f64(gen) * w).sum((-2, -1)) / w.sum()).mean(0)
                    v = (100 * (P - T_) / T_).mean(0)
                    t0 = int(z[f"{key}::i_time_start{i}"])
                    tot[t0:t0 + v.shape[0]] += v
                    cnt[t0:t0 + v.shape[0]] += 1
                want = torch.from_numpy(z[f"{key}::series::{GRAD}/{n}"])
                assert torch.allclose(tot / cnt, want, rtol=1e-4, atol=1e-3), (key, n)
