"""weighted_grad_mag_percent_diff on the device (`sdy_ensemble_series_grad`; reference src/ace_inference/core/metrics.py:210-241,
aggregator/inference/reduced.py:178, aggregator/one_step/reduced.py:75): the aggregators against the reference's own
classes (tests/golden/fx_mean_series_grad.npz), the per-plane sums against a float64 restatement, the other eight sums
against the kernel without the gradient, the composite's logs, and the edges."""
import json

import pytest
import torch

import golden_utils as gu

pytestmark = pytest.mark.gpu
GRAD = "weighted_grad_mag_percent_diff"


def _tol(metric):
    return dict(rtol=1e-4, atol=1e-3) if metric == GRAD else dict(rtol=5e-5, atol=5e-6)


def _windows(z, key, names, ens):
    for i in range(3):
        tgt = {n: torch.from_numpy(z[f"{key}::tgt{i}::{n}"]).cuda() for n in names}
        gen = {n: torch.from_numpy(z[f"{key}::gen{i}::{n}"]).cuda() for n in names}
        if ens:   # as the window driver presents it: a transposed view of the IC-major batch
            gen = {n: v.transpose(0, 1).contiguous().transpose(0, 1) for n, v in gen.items()}
            assert not gen[names[0]].is_contiguous()
        yield float(z[f"{key}::loss{i}"]), tgt, gen, int(z[f"{key}::i_time_start{i}"])


@pytest.mark.parametrize("shp", ["16x32", "7x10"])
@pytest.mark.parametrize("kind", ["ens", "det"])
def test_aggregators_vs_reference(shp, kind):
    """MeanAggregator's series and OneStepMeanAggregator's values with the metric on vs the reference's own aggregators fed
    the same three windows."""
    import sdy_amd

    z = gu.load("fx_mean_series_grad")
    names = json.loads(str(z["names"]))
    key, ens = f"{shp}::{kind}", kind == "ens"
    W = z[f"{key}::tgt0::a"].shape[-1]
    w = sdy_amd.metrics.spherical_area_weights(torch.from_numpy(z[f"{shp}::lats"]), W)
    n_t, target_time = int(z["n_timesteps"]), int(z["target_time"])
    agg = sdy_amd.metrics.MeanAggregator(w, target="denorm", n_timesteps=n_t, is_ensemble=ens, grad_mag_percent_diff=True)
    one = sdy_amd.metrics.OneStepMeanAggregator(w.cuda(), target_time=target_time, is_ensemble=ens,
                                                grad_mag_percent_diff=True)
    for loss, tgt, gen, t0 in _windows(z, key, names, ens):
        agg.record_batch(loss, tgt, gen, tgt, gen, i_time_start=t0)
        one.record_batch(loss, tgt, gen, tgt, gen, i_time_start=t0)
    series = agg.get_series()
    metrics = json.loads(str(z[f"{key}::metrics"]))
    assert GRAD in metrics and sorted(agg.metric_names) == metrics
    assert set(series) == {f"{m}/{n}" for m in metrics for n in names}
    for m in metrics:
        for n in names:
            want = torch.from_numpy(z[f"{key}::series::{m}/{n}"])
            got = series[f"{m}/{n}"].cpu()
            assert got.shape == want.shape == (n_t,)
            assert torch.allclose(got, want, **_tol(m)), (key, m, n, got, want)
    logs = one.get_logs("one")
    ref_keys = json.loads(str(z[f"{key}::one_step_keys"]))
    assert sorted(k[len("one/"):] for k in logs) == ref_keys
    for k in ref_keys:
        want = float(z[f"{key}::one_step::{k}"])
        tol = _tol(k.split("/")[0])
        assert logs[f"one/{k}"] == pytest.approx(want, rel=tol["rtol"], abs=tol["atol"]), (key, k)


def _structured(g, lead, H, W):
    """large-scale waves + small-scale noise: a gradient everywhere, of both kinds."""
    lat = torch.linspace(0, 3.1, H)[:, None]
    lon = torch.linspace(0, 6.2, W)[None, :]
    ph = torch.rand(*lead, 1, 1, generator=g) * 6.28
    return torch.sin(2 * lat + ph) * torch.cos(lon - ph) + 0.3 * torch.randn(*lead, H, W, generator=g) + 1.5


def _grad_mag_f64(x):
    gy, gx = torch.gradient(x.double(), dim=(-2, -1))
    return (gy ** 2 + gx ** 2).sqrt()


CASES = [(H, W, M, 7 if H * W < 1000 else (3 if H < 180 else 2))
         for H, W in ((2, 2), (3, 5), (7, 10), (17, 36), (180, 360)) for M in (1, 3, 25, 64)]


@pytest.mark.parametrize("H,W,M,T", CASES, ids=[f"{h}x{w}-M{m}-T{t}" for h, w, m, t in CASES])
def test_plane_sums_vs_float64_restatement(H, W, M, T):
    """Each plane's truth term T and member-mean term P against torch.gradient in float64 on the CPU, read through strided
    views (members behind samples in memory, truth a time slice of a longer run); the other eight sums equal those of the
    kernel without the gradient."""
    import sdy_amd

    g = torch.Generator().manual_seed(H * 1000 + W * 10 + M)
    S = 2
    lats = torch.linspace(-80.0, 80.0, H)
    w = sdy_amd.metrics.spherical_area_weights(lats, W)
    run = _structured(g, (S, T + 2), H, W)
    truth = run[:, 1:T + 1]                                         # sample stride (T + 2) H W: a strided view
    pred_sm = truth[:, None] + 0.4 * torch.randn(S, M, T, H, W, generator=g)
    pred = pred_sm.cuda().transpose(0, 1)                           # (M, S, T, H, W), member stride T H W, sample stride M T H W
    tc = run.cuda()[:, 1:T + 1]
    assert (M == 1 or not pred.is_contiguous()) and not tc.is_contiguous()
    s = sdy_amd.metrics.ensemble_series(tc, pred, w, grad_mag=True).cpu()
    assert s.shape == (S, T, 10)
    wd = w.double()
    want_t = (_grad_mag_f64(truth) * wd).sum((-2, -1)) / wd.sum()
    want_p = ((_grad_mag_f64(pred_sm) * wd).sum((-2, -1)) / wd.sum()).mean(1)
    assert torch.allclose(s[..., 8], want_t, rtol=1e-6, atol=0), (s[..., 8], want_t)
    assert torch.allclose(s[..., 9], want_p, rtol=1e-6, atol=0), (s[..., 9], want_p)
    # slots 0-7 are the kernel without the gradient (fp64 atomics reorder the sums: not bit for bit)
    s0 = sdy_amd.metrics.ensemble_series(tc, pred, w).cpu()
    assert s0.shape == (S, T, 8)
    assert torch.allclose(s[..., :8], s0, rtol=1e-12, atol=1e-13)


def _synthetic_windows(n_t, E, names, H=16, W=32, seed=5):
    g = torch.Generator().manual_seed(seed)
    t0, out = 0, []
    for nt in (8, 7, n_t - 15):
        tgt = {n: _structured(g, (1, nt), H, W).cuda() for n in names}
        gen = {n: (tgt[n][None] + 0.3 * torch.randn(E, 1, nt, H, W, generator=g).cuda()) for n in names}
        if E == 1:
            gen = {n: v[0] for n, v in gen.items()}
        out.append((0.5, tgt, gen, t0))
        t0 += nt
    return out


@pytest.mark.parametrize("E", [3, 1])
def test_inference_aggregator_logs(E):
    """The composite with the metric on carries it under mean, mean_norm and mean_step_20, each equal to its own
    aggregator's value; the default composite fed the same windows keeps exactly the old key set."""
    import sdy_amd

    names = ["u", "v"]
    n_t = 22
    w = sdy_amd.metrics.spherical_area_weights(torch.linspace(-80.0, 80.0, 16), 32)
    wins = _synthetic_windows(n_t, E, names)
    norm = lambda d: {n: 0.5 * x - 1.0 for n, x in d.items()}        # noqa: E731
    comp = sdy_amd.metrics.InferenceAggregator(w, n_timesteps=n_t, n_ensemble_members=E, record_step_20=True,
                                               grad_mag_percent_diff=True)
    default = sdy_amd.metrics.InferenceAggregator(w, n_timesteps=n_t, n_ensemble_members=E, record_step_20=True)
    ens = E > 1
    mean = sdy_amd.metrics.MeanAggregator(w, target="denorm", n_timesteps=n_t, is_ensemble=ens, grad_mag_percent_diff=True)
    mean_norm = sdy_amd.metrics.MeanAggregator(w, target="norm", n_timesteps=n_t, is_ensemble=ens,
                                               grad_mag_percent_diff=True)
    step = sdy_amd.metrics.OneStepMeanAggregator(w, target_time=20, is_ensemble=ens, grad_mag_percent_diff=True)
    for loss, tgt, gen, t0 in wins:
        for a in (comp, default, mean, mean_norm, step):
            a.record_batch(loss, tgt, gen, norm(tgt), norm(gen), i_time_start=t0)
    steps = comp.get_inference_logs("inference")
    assert len(steps) == n_t
    s_mean, s_norm, s_step = mean.get_series(), mean_norm.get_series(), step.get_logs("mean_step_20")
    for n in names:
        for label, ser in (("mean", s_mean), ("mean_norm", s_norm)):
            got = torch.tensor([st[f"inference/{label}/{GRAD}/{n}"] for st in steps], dtype=torch.float64)
            assert torch.allclose(got, ser[f"{GRAD}/{n}"].cpu(), rtol=1e-12, atol=0), (label, n)
        assert steps[-1][f"inference/mean_step_20/{GRAD}/{n}"] == pytest.approx(s_step[f"mean_step_20/{GRAD}/{n}"],
                                                                               rel=1e-12)
        # the series' step 20 and the one-step value are the same number (one window holds step 20)
        assert s_step[f"mean_step_20/{GRAD}/{n}"] == pytest.approx(float(s_mean[f"{GRAD}/{n}"][20]), rel=1e-9)
    old = default.get_inference_logs("inference")
    assert len(old) == n_t
    for st_on, st_off in zip(steps, old):
        assert not any("grad_mag" in k for k in st_off)
        assert set(st_off) == {k for k in st_on if GRAD not in k}
        for k, v in st_off.items():
            assert st_on[k] == pytest.approx(v, rel=1e-12, abs=1e-13), k


def test_edges():
    import sdy_amd

    w = sdy_amd.metrics.spherical_area_weights(torch.linspace(-80.0, 80.0, 7), 10)
    x = torch.randn(65, 1, 2, 7, 10).cuda()
    with pytest.raises(sdy_amd.SdyError):                              # at most 64 members
        sdy_amd.metrics.ensemble_series(x[0], x, w, grad_mag=True)
    for H, W in ((1, 10), (7, 1)):                                     # torch.gradient refuses a single row / column
        y = torch.randn(3, 1, 2, H, W).cuda()
        with pytest.raises(sdy_amd.SdyError):
            sdy_amd.metrics.ensemble_series(y[0], y, torch.ones(H, W), grad_mag=True)
    # a truth plane without gradient: the reference's 100 (P - T) / T gives inf (P > 0) or nan (P = 0), and nothing raises
    tgt = torch.randn(1, 3, 7, 10).cuda()
    tgt[0, 1] = 2.5
    gen = tgt[None] + 0.1 * torch.randn(4, 1, 3, 7, 10).cuda()
    gen[:, 0, 2] = 1.0
    tgt[0, 2] = 1.0
    agg = sdy_amd.metrics.MeanAggregator(w, n_timesteps=3, is_ensemble=True, grad_mag_percent_diff=True)
    agg.record_batch(0.0, {"a": tgt}, {"a": gen}, {}, {})
    s = agg.get_series()[f"{GRAD}/a"].cpu()
    assert torch.isfinite(s[0]) and torch.isinf(s[1]) and s[1] > 0 and torch.isnan(s[2])
    one = sdy_amd.metrics.OneStepMeanAggregator(w, target_time=1, is_ensemble=True, grad_mag_percent_diff=True)
    one.record_batch(0.0, {"a": tgt}, {"a": gen}, {}, {})
    assert one.get_logs("x")[f"x/{GRAD}/a"] == float("inf")
    with pytest.raises(ValueError):      # a ragged share hands flat rows: still refused with the metric on
        agg.record_batch(0.0, {"a": tgt}, {"a": gen[:, 0]}, {}, {})
