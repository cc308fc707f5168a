"""Derived water-budget variables on the device (`sdy_amd.derived`, kernel `sdy_derived_water`) against the reference's own
`compute_derived_quantities` and `run_inference` (tests/golden/fx_derived.npz, tools/gen_golden.py:gen_derived).

Tolerances: total water path and dry-air pressure within 2e-6 of their largest magnitude (the kernel runs the reference's
fp32 chain without FMA contraction; the level sum may be ordered differently from torch's reduction).  The residual cancels
its terms, so its bound is absolute: 1e-6 of the largest of |twp| / 21600, |LHF| / 2.5e6, |PRATE|, |advection|."""
import json
import types

import numpy as np
import pytest
import torch

import golden_utils as gu
from conftest import rel_l2
from oracle.sfno import SFNOConfig

pytestmark = pytest.mark.gpu
DERIVED = ["surface_pressure_due_to_dry_air", "total_water_path", "total_water_path_budget_residual"]
RESID = DERIVED[2]


def _sigma(ak, bk):
    return types.SimpleNamespace(ak=torch.as_tensor(np.asarray(ak)), bk=torch.as_tensor(np.asarray(bk)))


def _scale(d, twp):
    pick = lambda names: next(d[n] for n in names if n in d)  # noqa: E731
    return max(float(np.abs(twp).max()) / 21600.0, float(np.abs(pick(("LHTFLsfc", "LHFLX"))).max()) / 2.5e6,
               float(np.abs(pick(("PRATEsfc", "surface_precipitation_rate"))).max()),
               float(np.abs(d["tendency_of_total_water_path_due_to_advection"]).max()))


def _close(got, want, scale_resid):
    for n in DERIVED:
        g, w = got[n].detach().cpu().double().numpy(), np.asarray(want[n], np.float64)
        assert g.shape == w.shape, (n, g.shape, w.shape)
        tol = 1e-6 * scale_resid if n == RESID else 2e-6 * np.abs(w).max()
        err = np.abs(g - w).max()
        assert err <= tol, f"{n}: max |err| {err:.3e} > {tol:.3e}"


def test_fixture_cases():
    import sdy_amd

    z = gu.load("fx_derived")
    for case in json.loads(str(z["cases"])):
        names = json.loads(str(z[f"{case}::names"]))
        d = {n: z[f"{case}::in::{n}"] for n in names}
        out = sdy_amd.derived.compute_derived_quantities({n: torch.from_numpy(v).cuda() for n, v in d.items()},
                                                        _sigma(z[f"{case}::ak"], z[f"{case}::bk"]))
        assert list(out) == names + DERIVED
        five = d["PRESsfc" if "PRESsfc" in d else "PS"].ndim == 5
        want = {n: z[f"{case}::{'member' if five else 'ref'}::{n}"] for n in DERIVED}
        _close(out, want, _scale(d, want["total_water_path"]))
        if five:
            # against the reference's own ensemble value: equal but for the residual (differenced over samples there)
            ref = {n: z[f"{case}::ref::{n}"] for n in DERIVED}
            for n in DERIVED[:2]:
                assert np.abs(out[n].cpu().double().numpy() - ref[n]).max() <= 2e-6 * np.abs(ref[n]).max(), n
            diff = np.abs(out[RESID].cpu().numpy() - ref[RESID]).max()
            assert diff > 1e-3 * _scale(d, want["total_water_path"])
        if out[RESID].shape[-3] == 1:
            assert not out[RESID].any()


def _production(M=25, S=1, T=7, H=180, W=360, K=8, seed=5):
    g = torch.Generator(device="cuda").manual_seed(seed)
    rows = S * M
    sh = (rows, T, H, W)
    d = {f"specific_total_water_{k}": torch.rand(sh, device="cuda", generator=g) * 10.0 ** (-2 - 0.5 * k)
         for k in range(K)}
    d["PRESsfc"] = 1.0e5 + 2.5e3 * torch.randn(sh, device="cuda", generator=g)
    d["LHTFLsfc"] = 90.0 + 60.0 * torch.randn(sh, device="cuda", generator=g)
    d["PRATEsfc"] = 6.0e-5 * torch.rand(sh, device="cuda", generator=g)
    d["tendency_of_total_water_path_due_to_advection"] = 2.0e-5 * torch.randn(sh, device="cuda", generator=g)
    ak = [3.0, 5238.4, 11815.8, 17263.1, 19929.5, 17023.4, 8970.5, 1537.5, 0.0][:K + 1]
    bk = [0.0, 0.0, 0.0115, 0.0781, 0.2034, 0.4004, 0.6513, 0.9065, 1.0][:K + 1]
    return d, ak, bk


def _float64(d, ak, bk, time_axis):
    K = len(ak) - 1
    ps = d["PRESsfc"].double()
    twp = sum(((ak[k + 1] + ps * bk[k + 1]) - (ak[k] + ps * bk[k])) * d[f"specific_total_water_{k}"].double()
              for k in range(K)) / 9.80665
    res = torch.zeros_like(twp)
    nxt = [slice(None)] * twp.dim()
    prv = list(nxt)
    nxt[time_axis], prv[time_axis] = slice(1, None), slice(None, -1)
    nxt, prv = tuple(nxt), tuple(prv)
    res[nxt] = (twp[nxt] - twp[prv]) / 21600.0 - (d["LHTFLsfc"].double()[nxt] / 2.5e6 - d["PRATEsfc"].double()[nxt]
                                                   + d["tendency_of_total_water_path_due_to_advection"].double()[nxt])
    return {DERIVED[0]: ps - 9.80665 * twp, DERIVED[1]: twp, RESID: res}


def test_production_shape_strided_view_and_flat_rows():
    """25 members x 2 ICs x 7 times x 180 x 360, K = 8: against float64; the member-stacked strided view the window driver
    makes (no copy) is bitwise its contiguous copy and the same rows passed flat; T = 1 gives an all-zero residual."""
    import sdy_amd

    M, S = 25, 2
    flat, ak, bk = _production(M=M, S=S)
    T, H, W = flat["PRESsfc"].shape[1:]
    der = sdy_amd.derived.deriver(_sigma(np.float32(ak), np.float32(bk)))
    view = {k: v.view(S, M, T, H, W).transpose(0, 1) for k, v in flat.items()}       # loop.py's unfold
    assert not view["PRESsfc"].is_contiguous()
    got_view = der(view)
    got_cont = der({k: v.contiguous() for k, v in view.items()})
    got_flat = der(flat)
    for n in DERIVED:
        assert got_view[n].shape == (M, S, T, H, W) and got_view[n].is_contiguous()
        assert torch.equal(got_view[n], got_cont[n]), n
        assert torch.equal(got_view[n], got_flat[n].view(S, M, T, H, W).transpose(0, 1)), n
    f32 = lambda v: np.float64(np.float32(v))  # noqa: E731
    want = _float64(flat, [f32(a) for a in ak], [f32(b) for b in bk], time_axis=1)
    scale = max(float(want[DERIVED[1]].abs().max()) / 21600.0, float(flat["LHTFLsfc"].abs().max()) / 2.5e6,
                float(flat["PRATEsfc"].abs().max()),
                float(flat["tendency_of_total_water_path_due_to_advection"].abs().max()))
    for n in DERIVED:
        err = float((got_flat[n].double() - want[n]).abs().max())
        tol = 1e-6 * scale if n == RESID else 2e-6 * float(want[n].abs().max())
        assert err <= tol, f"{n}: {err:.3e} > {tol:.3e}"
    # T = 1: an all-zero residual
    one = der({k: v[:, :1] for k, v in flat.items()})
    assert not one[RESID].any() and torch.equal(one[DERIVED[1]], got_flat[DERIVED[1]][:, :1])


def _loop_setup(members):
    import sdy_amd

    z, zl, zw = gu.load("fx_derived"), gu.load("fx_loop_tiny"), gu.load("fx_stepper_tiny")
    rename = json.loads(str(z["loop::rename"]))
    rn = lambda n: rename.get(n, n)  # noqa: E731
    fcfg = SFNOConfig(**json.loads(str(zl["fcfg"])))
    icfg = SFNOConfig(**json.loads(str(zl["icfg"])))
    names = {k: [rn(n) for n in json.loads(str(zl[k]))] for k in ("in_names", "out_names", "forcing_names")}
    n_forc = len(names["forcing_names"])

    def net(cfg, prefix):
        m = sdy_amd.SphericalFourierNeuralOperatorNet(
            num_input_channels=cfg.in_chans - n_forc, num_output_channels=cfg.out_chans, num_conditional_channels=n_forc,
            spatial_shape_in=(cfg.nlat, cfg.nlon), embed_dim=cfg.embed_dim, num_layers=cfg.num_layers,
            mlp_ratio=cfg.mlp_ratio, dropout_mlp=cfg.dropout_mlp, drop_path_rate=cfg.drop_path_rate,
            with_time_emb=cfg.with_time_emb, data_grid=cfg.data_grid, big_skip=cfg.big_skip, pos_embed=cfg.pos_embed)
        m.load_state_dict(gu.state_dict(zw, prefix), strict=True)
        if cfg.with_time_emb:
            m.set_min_max_time(cfg.min_time, cfg.max_time)
        return m

    exp = sdy_amd.MultiHorizonForecastingDYffusion(
        net(fcfg, "f::"), sdy_amd.InterpolationExperiment(net(icfg, "i::"), horizon=6), horizon=6,
        diffusion_config=dict(hack_for_imprecise_interpolation=True, enable_interpolator_dropout=False))
    pr = json.loads(str(zl["prescriber"]))
    stepper = sdy_amd.MultiStepStepper(
        exp, names["in_names"] + names["forcing_names"], names["out_names"], names["forcing_names"],
        means={rn(k[6:]): float(zl[k]) for k in zl.files if k.startswith("mean::")},
        stds={rn(k[5:]): float(zl[k]) for k in zl.files if k.startswith("std::")},
        prescriber=sdy_amd.Prescriber(rn(pr["prescribed_name"]), pr["mask_name"], pr["mask_value"], pr["interpolate"]))
    series = {rn(k[8:]): torch.from_numpy(zl[k]) for k in zl.files if k.startswith("series::")}
    n_total, n_mem = int(zl["n_total"]), int(zl["n_mem_steps"])
    windows = [types.SimpleNamespace(data={k: v[:, i * n_mem:(i + 1) * n_mem + 1] for k, v in series.items()}, times=None)
               for i in range(n_total // n_mem)]
    sigma = _sigma(z["loop::ak"], z["loop::bk"])
    return z, stepper, windows, sigma, n_total, n_mem, names


def _run(stepper, windows, sigma, n_total, n_mem, members, aggregator=None, **kw):
    import sdy_amd

    calls = []

    class Wr:
        def append_batch(self, target, prediction, start_timestep, start_sample, batch_times=None):
            calls.append((start_timestep, start_sample, {k: v.clone() for k, v in prediction.items()},
                          {k: v.clone() for k, v in target.items()}))

    sdy_amd.run_inference(aggregator, stepper, types.SimpleNamespace(loader=windows), n_total, n_mem, members, writer=Wr(),
                          derive=sdy_amd.derived.deriver(sigma), **kw)
    return calls


@pytest.mark.parametrize("members", [1, 3])
def test_run_inference_matches_reference_loop(members):
    """run_inference(derive=deriver(...)) hands writer and aggregator what the reference's loop handed over: targets and
    predictions with the three derived variables (predictions of an ensemble: the reference's per-member values)."""
    z, stepper, windows, sigma, n_total, n_mem, names = _loop_setup(members)
    key = f"loop::m{members}"
    sub = (Ellipsis, slice(None, None, 4), slice(None, None, 8))
    runs = {"default": _run(stepper, windows, sigma, n_total, n_mem, members),
            "host": _run(stepper, windows, sigma, n_total, n_mem, members, host_outputs=True),
            "chunks": _run(stepper, windows, sigma, n_total, n_mem, members, max_batch=2)}
    calls = runs["default"]
    assert [c[0] for c in calls] == [int(v) for v in z[f"{key}::starts"]]
    for w, (_, _, pred, tgt) in enumerate(calls):
        assert list(pred)[-3:] == DERIVED and list(tgt)[-3:] == DERIVED
        for kind, dct, src in (("tgt", tgt, "tgt"), ("pred", pred, "member" if members > 1 else "pred")):
            for n in DERIVED:
                want = torch.from_numpy(z[f"{key}::{src}{w}::{n}"])
                got = dct[n][sub]
                assert got.shape == want.shape, (kind, n)
                # predictions carry the network's parity error (~1e-6 relative), targets only the kernel's rounding
                assert rel_l2(got, want) < (1e-6 if kind == "tgt" else 1e-4), (w, kind, n, rel_l2(got, want))
                sums = torch.from_numpy(z[f"{key}::{src}{w}::{n}::sum"])
                assert rel_l2(dct[n].double().sum(dim=(-2, -1)).cpu(), sums) < (1e-6 if kind == "tgt" else 1e-4)
    for other in ("host", "chunks"):
        for (s0, ss0, p0, t0), (s1, ss1, p1, t1) in zip(calls, runs[other]):
            assert (s0, ss0) == (s1, ss1)
            for n in DERIVED:
                assert torch.equal(p0[n].cpu(), p1[n].cpu()) and torch.equal(t0[n].cpu(), t1[n].cpu()), (other, n)


def test_inference_aggregator_logs_gain_derived_variables():
    import sdy_amd

    z, stepper, windows, sigma, n_total, n_mem, names = _loop_setup(3)
    w = sdy_amd.metrics.spherical_area_weights(torch.linspace(-87.0, 87.0, 32), 64).cuda()
    logs = {}
    for derive in (False, True):
        agg = sdy_amd.metrics.InferenceAggregator(w, sigma_coordinates=sigma, n_timesteps=n_total + 1,
                                                  n_ensemble_members=3)
        sdy_amd.run_inference(agg, stepper, types.SimpleNamespace(loader=windows), n_total, n_mem, 3,
                              derive=sdy_amd.derived.deriver(sigma) if derive else None)
        logs[derive] = (agg.get_logs("inference"), agg.get_inference_logs("inference"))
    plain, full = logs[False][0], logs[True][0]
    for n in DERIVED:
        assert f"inference/time_mean/rmse/{n}" in full and f"inference/time_mean/rmse/{n}" not in plain
        assert f"inference/mean/weighted_rmse/{n}" in logs[True][1][1]
        assert f"inference/mean/weighted_rmse/{n}" not in logs[False][1][1]
        assert f"inference/mean_norm/weighted_rmse/{n}" not in logs[True][1][1]       # normalised data only
    rmse = {k: v for k, v in full.items() if k.startswith("inference/time_mean/rmse/") and not k.endswith("channel_mean")}
    assert len(rmse) == len(names["out_names"]) + 3
    assert abs(full["inference/time_mean/rmse/channel_mean"] - sum(rmse.values()) / len(rmse)) < 1e-9 * max(
        1.0, abs(full["inference/time_mean/rmse/channel_mean"]))
    for k in plain:          # the generated variables' numbers do not change
        if "channel_mean" not in k and isinstance(plain[k], float):
            assert abs(full[k] - plain[k]) <= 1e-6 * max(1.0, abs(plain[k])), k


def test_unit_range_share_gives_the_full_runs_values():
    """A ragged share (flat rows: trajectories 1-3 of 2 ICs x 3 members) gets the same derived values per trajectory as
    the full run."""
    z, stepper, windows, sigma, n_total, n_mem, names = _loop_setup(3)
    full = _run(stepper, windows, sigma, n_total, n_mem, 3)
    part = _run(stepper, windows, sigma, n_total, n_mem, 3, unit_range=(1, 3))
    assert len(full) == len(part)
    for (_, _, pf, _), (_, start, pp, _) in zip(full, part):
        assert start == 1
        for n in DERIVED:
            assert pp[n].dim() == 4 and pp[n].shape[0] == 3
            for r in range(3):
                u = 1 + r
                ic, m = divmod(u, 3)
                assert rel_l2(pp[n][r], pf[n][m, ic]) < 1e-5, (n, u)
