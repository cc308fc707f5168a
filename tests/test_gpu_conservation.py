"""Dry-air conservation diagnostics on the device (`sdy_amd.conservation`, kernels csrc/conservation.hip) and in
`MultiStepStepper`.

Host parity: the kernel and `sdy_dry_air_series_host` walk the same summation tree with the same arithmetic, so `gm` is equal bit
for bit, and so are absdiff and the mean (asserted within one float64 rounding of the sample mean).
Reference parity (corrector_utils.parity_bound, see tests/test_conservation_host.py for the measured ratios and C = 3.25):
    max|ours - ref64| <= C * max|ref32 - ref64| + 4 * 2^-24 * max|ref64|
At the fixture's sizes ref32 / ref64 are the reference's own functions; at 180 x 360, which the fixture cannot hold, ref64 is the
float64 restatement (held to the fixture to 1e-12) and ref32 the same restatement evaluated in float32, sums included.
Stepper: with `conserve_dry_air` the window's mean one-step change of the global-mean dry-air pressure is below
4 * 2^-24 * max|ps| (the second term of the parity bound on the surface pressure: the fp32 roundings of the corrector's solve),
without it the 15 Pa drift of the inputs is more than ten times that (12.4 Pa against 0.026 Pa in float64 on the CPU)."""
import contextlib
import ctypes as C

import pytest
import torch

import conservation_utils as co
import corrector_utils as cu

pytestmark = pytest.mark.gpu
C_PARITY = 3.25
ULP64 = 2.0 ** -52


def _cuda(d):
    return {k: v.cuda() for k, v in d.items()}


def _series(area, ak, bk):
    import sdy_amd

    return sdy_amd.conservation.DryAirSeries(area, co.Sigma(ak, bk))


def _host(data, area, ak, bk):
    import sdy_amd

    return co.host_series(sdy_amd, data, area, ak, bk)


def _assert_equals_host(res, data, area, ak, bk, label):
    gm, absdiff, mean = _host(data, area, ak, bk)
    assert torch.equal(res.gm.cpu(), gm), f"{label}: gm differs from the host entry point"
    T = gm.shape[1]
    if T > 1:
        tol = ULP64 * float(absdiff.abs().max())
        assert float((res.absdiff.cpu() - absdiff).abs().max()) <= tol, label
        assert abs(float(res.mean) - float(mean[0])) <= tol, label
    else:
        assert res.absdiff.shape == (0,) and bool(torch.isnan(res.mean)), label


_DATA = {}


def _case(B, T, K, H, W):
    key = (B, T, K, H, W)
    if key not in _DATA:
        ak, bk = co.levels_for(K)
        _DATA[key] = (co.timeline(B, T, K, H, W, seed=H + 7 * K + B), cu.area_for(H, W), ak, bk)
    return _DATA[key]


SMALL = [(B, T, K, H, W) for (H, W) in ((6, 8), (18, 36)) for K in (1, 2, 8) for B in (1, 3) for T in (1, 2, 3)]


@pytest.mark.parametrize("B,T,K,H,W", SMALL + [(2, 3, 8, 180, 360)])
def test_device_equals_host_entry_point(B, T, K, H, W):
    data, area, ak, bk = _case(B, T, K, H, W)
    res = _series(area, ak, bk)(_cuda(data))
    assert res.gm.shape == (B, T) and res.absdiff.shape == (T - 1,) and res.mean.dim() == 0
    assert res.gm.dtype == res.absdiff.dtype == res.mean.dtype == torch.float64 and res.gm.is_cuda
    _assert_equals_host(res, data, area, ak, bk, f"B{B} T{T} K{K} {H}x{W}")


@pytest.mark.parametrize("name,side", [(n, s) for n in co.set_names() for s in ("gen", "target")])
def test_fixture_parity(name, side):
    import sdy_amd

    d = co.set_data(name)
    sigma = co.Sigma(d["ak"], d["bk"])
    data = _cuda(d[side])
    absdiff = sdy_amd.compute_dry_air_absolute_differences(data, d["area"], sigma)
    mean = sdy_amd.get_dry_air_nonconservation(data, d["area"], sigma)
    gm = _series(d["area"], d["ak"], d["bk"])(data).gm
    assert absdiff.is_cuda and mean.is_cuda and absdiff.shape == (d["meta"]["T"] - 1,) and mean.dim() == 0
    co.check_parity(dict(gm=gm.cpu(), absdiff=absdiff.cpu(), mean=mean.cpu()), d["ref32"][side], d["ref64"][side], C_PARITY,
                    f"{name} {side}")
    if side == "gen":
        metrics, loss = sdy_amd.ConservationLossConfig(dry_air_penalty=d["meta"]["penalty"]).build(d["area"], sigma)(data)
        assert list(metrics) == ["dry_air_loss"] and metrics["dry_air_loss"].dtype == torch.float32 and loss.is_cuda
        assert float(loss) == float(metrics["dry_air_loss"])
        for k, v in (("dry_air_loss", metrics["dry_air_loss"]), ("conservation_loss", loss)):
            err = abs(float(v) - float(d["ref64"][k]))
            bound = cu.parity_bound(d["ref32"][k], d["ref64"][k], C_PARITY)
            print(f"{name} {k}: err {err:.3e} bound {bound:.3e}")
            assert err <= bound
        metrics, loss = sdy_amd.ConservationLossConfig().build(d["area"], sigma)(data)
        assert metrics == {} and float(loss) == 0.0 and loss.is_cuda


def test_production_grid_parity():
    """B = 2, T = 3, K = 8 at 180 x 360: 64 workgroups per row, a ragged last one."""
    data, area, ak, bk = _case(2, 3, 8, 180, 360)
    res = _series(area, ak, bk)(_cuda(data))
    ref64 = dict(zip(("gm", "absdiff", "mean"), co.series64(data, area, ak, bk)))
    ref32 = dict(zip(("gm", "absdiff", "mean"), co.series64(data, area, ak, bk, dtype=torch.float32)))
    co.check_parity(dict(gm=res.gm.cpu(), absdiff=res.absdiff.cpu(), mean=res.mean.cpu()), ref32, ref64, C_PARITY, "180x360")


@pytest.mark.parametrize("K,H,W", [(2, 6, 8), (8, 18, 36), (8, 180, 360)])
def test_row_alone_equals_row_in_batch(K, H, W):
    B, T = (2, 3) if H == 180 else (3, 3)
    data, area, ak, bk = _case(B, T, K, H, W)
    series = _series(area, ak, bk)
    full = series(_cuda(data)).gm
    again = series(_cuda(data)).gm
    assert torch.equal(full, again)
    for b in range(B):
        one = series(_cuda({n: v[b:b + 1] for n, v in data.items()})).gm
        assert torch.equal(one[0], full[b]), b


def test_views_are_read_in_place():
    """The `[:, 0:2]` view of a T = 3 tensor and a channel of a packed, normalised (B, C, H, W) tensor: the result of their
    contiguous / denormalised copies, bit for bit, from the view's own address and strides."""
    B, T, K, H, W = 3, 3, 2, 18, 36
    data, area, ak, bk = _case(B, T, K, H, W)
    series = _series(area, ak, bk)
    dev = _cuda(data)
    names = cu.water_names(dev)
    view = {n: v[:, 0:2] for n, v in dev.items()}
    a, keep, rows, T2 = series.args([view[n] for n in names], view["PRESsfc"])
    assert keep == [] and (rows, T2) == (B, 2)
    for slot, n in ((a.q[0], names[0]), (a.q[1], names[1]), (a.ps, "PRESsfc")):
        assert slot.base == dev[n].data_ptr() and (slot.stride_b, slot.stride_t) == (T * H * W, H * W), n
    got = series(dev, times=slice(0, 2))
    want = series({n: v.contiguous() for n, v in view.items()})
    assert torch.equal(got.gm, want.gm) and torch.equal(got.absdiff, want.absdiff) and torch.equal(got.mean, want.mean)
    _assert_equals_host(got, {n: v[:, 0:2] for n, v in data.items()}, area, ak, bk, "view")
    # a view the two strides cannot express is copied, and says so
    swapped = {n: v.transpose(0, 1)[:, :, None].expand(T, B, 2, H, W) for n, v in dev.items()}
    a, keep, rows, _ = series.args([swapped[n] for n in names], swapped["PRESsfc"])
    assert len(keep) == 3 and rows == T * B
    # packed: (B, C, H, W) normalised, the planes read where they lie and denormalised in the kernel
    order = ["TMP2m"] + names + ["PRESsfc"]
    stats = {n: (float(data[n].mean()), float(data[n].std())) if n in data else (280.0, 1.0) for n in order}
    cols = {n: data[n][:, 1] if n in data else torch.zeros(B, H, W) for n in order}
    packed = torch.stack([((cols[n].double() - stats[n][0]) / stats[n][1]).float() for n in order], 1).contiguous().cuda()
    means, stds = {n: stats[n][0] for n in order}, {n: stats[n][1] for n in order}
    got = series.packed(packed, order, means, stds)
    phys = {n: (packed[:, i] * torch.tensor(stats[n][1]).cuda() + torch.tensor(stats[n][0]).cuda())[:, None].contiguous()
            for i, n in enumerate(order) if n != "TMP2m"}
    want = series(phys)
    assert got.gm.shape == (B, 1) and torch.equal(got.gm, want.gm)
    view = packed.as_strided((B, 1, H, W), (len(order) * H * W, 0, W, 1))
    a, keep, rows, _ = series.args([view, view], view, stats=[stats[n] for n in order[1:]], channels=[1, 2, 3])
    assert keep == [] and a.ps.base == packed.data_ptr() and a.ps.channel == 3 and a.ps.stride_b == len(order) * H * W


@pytest.mark.parametrize("name", co.set_names())
def test_derived_metrics_aggregator(name):
    import sdy_amd

    d = co.set_data(name)
    agg = sdy_amd.DerivedMetricsAggregator(d["area"], co.Sigma(d["ak"], d["bk"]))
    with pytest.raises(ValueError, match="No batches"):
        agg.get_logs("one_step")
    target, gen = _cuda(d["target"]), _cuda(d["gen"])
    for lo, hi in co.batches(d):
        agg.record_batch({n: v[lo:hi] for n, v in target.items()}, {n: v[lo:hi] for n, v in gen.items()}, None, None)
    logs = agg.get_logs("one_step")
    assert list(logs) == co.LOG_KEYS
    for k in co.LOG_KEYS:
        assert logs[k].is_cuda and logs[k].dim() == 0
        err = abs(float(logs[k]) - float(d["ref64"]["logs"][k]))
        ratio = cu.error_ratio(logs[k].cpu(), d["ref32"]["logs"][k], d["ref64"]["logs"][k])
        bound = cu.parity_bound(d["ref32"]["logs"][k], d["ref64"]["logs"][k], C_PARITY)
        print(f"{name} {k}: err {err:.3e} ratio {ratio:.3f} bound {bound:.3e}")
        assert err <= bound, k


def test_derived_metrics_aggregator_pools_members():
    """(members, samples, time, lat, lon) gen: the flat (members * samples, ...) result, from the stacked tensor in place."""
    import sdy_amd

    d = co.set_data("b2t3k8")
    sigma = co.Sigma(d["ak"], d["bk"])
    target, gen = _cuda(d["target"]), _cuda(d["gen"])
    stacked = {n: torch.stack([v, v.flip(0) * (1.0 + 1e-3)], 0) for n, v in gen.items()}        # (2, 2, 3, H, W)
    flat = {n: v.reshape(-1, *v.shape[2:]) for n, v in stacked.items()}
    a, b = sdy_amd.DerivedMetricsAggregator(d["area"], sigma), sdy_amd.DerivedMetricsAggregator(d["area"], sigma)
    a.record_batch(target, stacked, None, None)
    b.record_batch(target, flat, None, None)
    for k in co.LOG_KEYS:
        assert float(a.get_logs("one_step")[k]) == float(b.get_logs("one_step")[k]), k


# ---- the stepper ------------------------------------------------------------------------------------------------------------
NAMES = ["specific_total_water_0", "specific_total_water_1", "PRESsfc", "TMP2m"]
STATS = {"specific_total_water_0": (1.5e-6, 3.0e-7), "specific_total_water_1": (1.5e-2, 3.0e-3), "PRESsfc": (1.0e5, 3.0e3),
         "TMP2m": (280.0, 1.0)}
PENALTY = 0.25


class ReplayModule:
    """The smallest module the stepper accepts: one step per window; the prediction of step i is the i-th normalised, packed
    frame it was given, whatever the state."""
    true_horizon, model = 1, None
    ema_scope = inference_dropout_scope = staticmethod(contextlib.nullcontext)

    def __init__(self, frames):
        self.frames, self.i = frames, 0

    def get_preds_at_t_for_batch(self, batch, horizon, **kw):
        self.i += 1
        return {f"t{horizon}_preds_normed": self.frames[self.i]}


@pytest.fixture(scope="module")
def stepper_runs():
    """B = 2, three steps at 18 x 36, K = 2: the module replays a timeline with a 15 Pa mean pressure drift per step."""
    import sdy_amd

    B, T1, H, W = 2, 4, 18, 36
    ak, bk = co.levels_for(2)
    area = cu.area_for(H, W)
    g = torch.Generator().manual_seed(5)
    data = co.timeline(B, T1, 2, H, W, seed=7)
    data["TMP2m"] = 280.0 + torch.randn(B, T1, H, W, generator=g)
    means, stds = {n: STATS[n][0] for n in NAMES}, {n: STATS[n][1] for n in NAMES}
    frames = [torch.stack([((data[n][:, t].double() - means[n]) / stds[n]).float() for n in NAMES], 1).contiguous().cuda()
              for t in range(T1)]
    sigma = co.Sigma(ak, bk)
    cons = sdy_amd.ConservationLossConfig(dry_air_penalty=PENALTY).build(area, sigma)
    corr = sdy_amd.CorrectorConfig(conserve_dry_air=True).build(area, sigma)
    dev = _cuda(data)

    def run(defer=False, **kw):
        st = sdy_amd.MultiStepStepper(ReplayModule(frames), NAMES, NAMES, [], means, stds, **kw)
        return st.run_on_batch(dict(dev), None, n_forward_steps=T1 - 1, defer_metrics=defer)

    deferred = run(defer=True, conservation_loss=cons)
    unread = deferred.metrics._values is None          # before anything below reads it
    return dict(data=data, area=area, sigma=sigma, ak=ak, bk=bk, steps=T1 - 1, plain=run(), none=run(conservation_loss=None),
                off=run(conservation_loss=sdy_amd.ConservationLossConfig().build(area, sigma)),
                cons=run(conservation_loss=cons), both=run(conservation_loss=cons, corrector=corr), deferred=deferred,
                deferred_unread=unread)


def _close32(a, b):
    return abs(float(a) - float(b)) <= 2.0 ** -23 * abs(float(b))


def test_stepper_dry_air_loss_is_the_nonconservation_of_the_returned_timelines(stepper_runs):
    import sdy_amd

    r = stepper_runs
    m = r["cons"].metrics
    assert list(m) == [f"loss_step_{i}" for i in range(r["steps"])] + ["dry_air_loss", "loss"]
    want = sdy_amd.get_dry_air_nonconservation(r["cons"].gen_data, r["area"], r["sigma"])
    assert m["dry_air_loss"].dtype == torch.float32
    assert float(m["dry_air_loss"]) == float((PENALTY * want.cpu()).to(torch.float32))
    total = sum(float(m[f"loss_step_{i}"]) for i in range(r["steps"])) + float(m["dry_air_loss"])
    print(f"stepper loss {float(m['loss']):.9e} steps + dry_air_loss {total:.9e}")
    assert abs(float(m["loss"]) - total) <= 4.0 * 2.0 ** -24 * abs(total)        # fp32 roundings of the terms and of the sum
    for n in NAMES:
        assert torch.equal(r["cons"].gen_data[n], r["plain"].gen_data[n]), n


def test_stepper_without_conservation_loss_is_unchanged(stepper_runs):
    r = stepper_runs
    keys = [f"loss_step_{i}" for i in range(r["steps"])] + ["loss"]
    for which in ("none", "off"):
        assert list(r[which].metrics) == list(r["plain"].metrics) == keys
        for k in keys:
            assert _close32(r[which].metrics[k], r["plain"].metrics[k]), (which, k)
        for n in NAMES:
            assert torch.equal(r[which].gen_data[n], r["plain"].gen_data[n]), n
    for k in keys[:-1]:
        assert _close32(r["cons"].metrics[k], r["plain"].metrics[k]), k


def test_stepper_corrector_conserves_and_the_drift_shows_without_it(stepper_runs):
    r = stepper_runs
    cpu64 = float(co.series64(r["data"], r["area"], r["ak"], r["bk"])[2])
    bound = 4.0 * cu.EPS32 * float(r["data"]["PRESsfc"].abs().max())
    without = float(r["cons"].metrics["dry_air_loss"]) / PENALTY
    with_corr = float(r["both"].metrics["dry_air_loss"]) / PENALTY
    print(f"dry air non-conservation: inputs in float64 {cpu64:.4e}, stepper {without:.4e}, corrected {with_corr:.3e}, "
          f"bound {bound:.3e}")
    assert cpu64 >= 10.0 * bound, "the inputs do not drift: the test shows nothing"
    assert without >= 10.0 * bound
    assert with_corr <= bound
    # the series is taken from the corrected timelines
    import sdy_amd
    want = sdy_amd.get_dry_air_nonconservation(r["both"].gen_data, r["area"], r["sigma"])
    assert float(r["both"].metrics["dry_air_loss"]) == float((PENALTY * want.cpu()).to(torch.float32))


def test_stepper_deferred_metrics(stepper_runs):
    r = stepper_runs
    assert r["deferred_unread"], "run_on_batch read the metrics although defer_metrics=True"
    assert float(r["deferred"].metrics["dry_air_loss"]) == float(r["cons"].metrics["dry_air_loss"])
    assert _close32(r["deferred"].metrics["loss"], r["cons"].metrics["loss"])


def test_stepper_missing_fields_give_nan(stepper_runs):
    """Without the pressure among the outputs `dry_air_loss` is NaN and so is `loss`: the reference adds it (the fixture's
    `facts` record both)."""
    import sdy_amd

    r = stepper_runs
    assert co.fixture()[2]["no_pressure"]["loss_is_nan"]
    names = [n for n in NAMES if n != "PRESsfc"]
    means, stds = {n: STATS[n][0] for n in names}, {n: STATS[n][1] for n in names}
    frames = [torch.zeros(2, len(names), 18, 36).cuda() for _ in range(3)]
    cons = sdy_amd.ConservationLossConfig(dry_air_penalty=PENALTY).build(r["area"], r["sigma"])
    st = sdy_amd.MultiStepStepper(ReplayModule(frames), names, names, [], means, stds, conservation_loss=cons)
    out = st.run_on_batch({n: r["data"][n][:, :3].cuda() for n in names}, None, n_forward_steps=2)
    m = out.metrics
    assert bool(torch.isnan(m["dry_air_loss"])) and bool(torch.isnan(m["loss"]))
    assert all(bool(torch.isfinite(m[f"loss_step_{i}"])) for i in range(2))
