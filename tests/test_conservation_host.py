"""Dry-air conservation diagnostics (reference core/aggregator/climate_data.py:199-233, core/loss.py, core/aggregator/one_step/
derived.py): the side that needs no GPU.  The host entry point `sdy_dry_air_series_host` -- the kernel's own per-column
arithmetic (csrc/corrector_math.h) and its own summation tree -- against the reference's own functions
(tests/golden/fx_conservation.npz); the float64 restatement the GPU tests use at larger sizes against the same fixture; the C
ABI's argument checks; name resolution, the NaN paths and the refusal of CPU tensors of the Python surface.

Parity bound per quantity (`corrector_utils.parity_bound`), for gm, absdiff and their mean:
    max|ours - ref64| <= c * max|ref32 - ref64| + 4 * 2^-24 * max|ref64|
`ref32` / `ref64` are the reference's functions on float32 / float64 inputs.  Measured ratio max|ours - ref64| / max|ref32 - ref64|
of the host entry point over the 3 sets x (gen, target) (printed by test_host_matches_reference): gm 0.008 .. 0.083, absdiff
0.004 .. 0.274, mean 0.002 .. 0.673 (`b3t3k2` gen: two differences of 48-point means, where the reference's fp32 sums happen to
err by 6e-4 Pa only).  The aggregator's logs, formed the same way from the host entry point on the fixture's two batches of the
`[:, 0:2]` views: 0.005 .. 0.25, and 1.08 for `b3t3k2` gen (ours 8.1e-4 Pa off, the reference 7.5e-4 Pa).  That one is not below 1,
and the float64 sums cannot make it so: on a 48-point grid both errors are the fp32 rounding of the column quantity ps - g * twp
(half an ulp of 1e5 Pa is 3.9e-3 Pa per column, 3e-4 .. 6e-4 Pa once averaged over 48 columns and differenced), which the kernel
keeps on purpose because it is the reference's chain; the reference's fp32 sums add to it or cancel part of it by chance.  At
18 x 36 the sums dominate the reference's error and the ratios are 0.002 .. 0.015.  C = 3.25, 3 x the largest ratio, the headroom
of the corrector tests."""
import ctypes as C

import pytest
import torch

import conservation_utils as co
import corrector_utils as cu

C_PARITY = 3.25
SIDES = [(n, s) for n in co.set_names() for s in ("gen", "target")]


@pytest.fixture(scope="module")
def sdy():
    import sdy_amd

    return sdy_amd


@pytest.mark.parametrize("name,side", SIDES)
def test_restatement_matches_reference_float64(name, side):
    d = co.set_data(name)
    got = co.series64(d[side], d["area"], d["ak"], d["bk"])
    for ours, k in zip(got, ("gm", "absdiff", "mean")):
        ref = d["ref64"][side][k]
        assert ours.shape == ref.shape
        assert float((ours - ref).abs().max()) <= 1e-12 * float(d["ref64"][side]["gm"].abs().max()), k


@pytest.mark.parametrize("name,side", SIDES)
def test_host_matches_reference(sdy, name, side):
    d = co.set_data(name)
    gm, absdiff, mean = co.host_series(sdy, d[side], d["area"], d["ak"], d["bk"])
    co.check_parity(dict(gm=gm, absdiff=absdiff, mean=mean[0]), d["ref32"][side], d["ref64"][side], C_PARITY, f"{name} {side}")


def test_reference_itself_meets_the_bound():
    for name, side in SIDES:
        d = co.set_data(name)
        for k, ref64 in d["ref64"][side].items():
            err = float((d["ref32"][side][k].double() - ref64).abs().max())
            assert err <= cu.parity_bound(d["ref32"][side][k], ref64, 1.0)


@pytest.mark.parametrize("name", co.set_names())
def test_host_logs_match_reference_aggregator(sdy, name):
    """The reference's `DerivedMetricsAggregator` over the fixture's two batches, restated with the host entry point on the
    `[:, 0:2]` views: the batches' means accumulated in one total, divided by the batch count."""
    d = co.set_data(name)
    for i, side in enumerate(("target", "gen")):
        water = lambda v: [v[n] for n in cu.water_names(v)]  # noqa: E731
        total = torch.zeros(1, dtype=torch.float64)
        for lo, hi in co.batches(d):
            view = {n: t[lo:hi, 0:2] for n, t in d[side].items()}
            a, out, keep = co.host_args(water(view), view["PRESsfc"], d["area"], d["ak"], d["bk"])
            a.mean_absdiff, a.accumulate = total.data_ptr(), 1
            assert sdy.lib.sdy_dry_air_series_host(C.byref(a)) == 0
        k = co.LOG_KEYS[i]
        ours, ref32, ref64 = total[0] / 2.0, d["ref32"]["logs"][k], d["ref64"]["logs"][k]
        err = abs(float(ours) - float(ref64))
        print(f"{name} {k}: err {err:.3e} ratio {cu.error_ratio(ours, ref32, ref64):.3f}")
        assert err <= cu.parity_bound(ref32, ref64, C_PARITY), k


def test_row_does_not_depend_on_the_batch_or_the_view(sdy):
    """A row's gm is the same bits alone, in the batch, through the `[:, 0:2]` view and through a packed, normalised layout
    holding the same physical values."""
    d = co.set_data("b3t3k2")
    full = co.host_series(sdy, d["gen"], d["area"], d["ak"], d["bk"])[0]
    for b in range(3):
        one = co.host_series(sdy, {n: v[b:b + 1] for n, v in d["gen"].items()}, d["area"], d["ak"], d["bk"])[0]
        assert torch.equal(one[0], full[b])
    view = {n: v[:, 0:2] for n, v in d["gen"].items()}
    assert not view["PRESsfc"].is_contiguous()
    gm, absdiff, mean = co.host_series(sdy, view, d["area"], d["ak"], d["bk"])
    assert torch.equal(gm, full[:, 0:2])
    assert float(mean[0]) == float(absdiff[0]) == float((full[:, 1] - full[:, 0]).abs().sum() / 3.0)
    # packed (B, C, H, W) at time 1, normalised; the physical values the kernel sees are x * std + mean formed in fp32
    names = ["TMP2m"] + cu.water_names(d["gen"]) + ["PRESsfc"]
    stats = {n: (float(d["gen"][n].mean()), float(d["gen"][n].std())) for n in names}
    packed = torch.stack([((d["gen"][n][:, 1].double() - stats[n][0]) / stats[n][1]).float() for n in names], 1).contiguous()
    phys = {n: (packed[:, i] * torch.tensor(stats[n][1]) + torch.tensor(stats[n][0]))[:, None] for i, n in enumerate(names)}
    plain = co.host_series(sdy, {n: phys[n].contiguous() for n in names[1:]}, d["area"], d["ak"], d["bk"])[0]
    B, n_ch, H, W = packed.shape
    slab = packed.as_strided((B, 1, H, W), (n_ch * H * W, 0, W, 1))
    a, out, keep = co.host_args([slab, slab], slab, d["area"], d["ak"], d["bk"], stats=[stats[n] for n in names[1:]],
                                channels=[1, 2, 3])
    assert sdy.lib.sdy_dry_air_series_host(C.byref(a)) == 0
    assert torch.equal(out[0], plain)


def test_accumulate_adds_to_the_running_total(sdy):
    d = co.set_data("b2t3k8")
    water = [d["gen"][n] for n in cu.water_names(d["gen"])]
    a, out, keep = co.host_args(water, d["gen"]["PRESsfc"], d["area"], d["ak"], d["bk"])
    assert sdy.lib.sdy_dry_air_series_host(C.byref(a)) == 0
    once = float(out[2][0])
    out[2][0] = 10.0
    a.accumulate = 1
    assert sdy.lib.sdy_dry_air_series_host(C.byref(a)) == 0
    assert float(out[2][0]) == 10.0 + once


def test_one_time_step_writes_no_differences(sdy):
    d = co.set_data("b3t3k2")
    one = {n: v[:, :1] for n, v in d["gen"].items()}
    water = [one[n] for n in cu.water_names(one)]
    a, out, keep = co.host_args(water, one["PRESsfc"], d["area"], d["ak"], d["bk"])
    out[2][0] = 7.0
    a.absdiff = None
    assert sdy.lib.sdy_dry_air_series_host(C.byref(a)) == 0
    assert float(out[2][0]) == 7.0 and out[0].shape == (3, 1)
    assert torch.equal(out[0], co.host_series(sdy, d["gen"], d["area"], d["ak"], d["bk"])[0][:, :1])


# ---- the C ABI's argument checks -------------------------------------------------------------------------------------------
def _args(sdy):
    """A valid argument block on host memory: B = 2, T = 3, K = 2, HW = 12, with a workspace."""
    g = torch.Generator().manual_seed(1)
    B, T, H, W = 2, 3, 3, 4
    water = [torch.rand(B, T, H, W, generator=g) * 1e-3 for _ in range(2)]
    ps = 1e5 + torch.rand(B, T, H, W, generator=g)
    a, out, keep = co.host_args(water, ps, torch.ones(H, W), [0.0, 0.5, 0.0], [0.0, 0.4, 1.0])
    ws = torch.zeros(sdy.lib.sdy_dry_air_workspace_bytes(B, T, H * W) // 8, dtype=torch.float64)
    a.ws, a.ws_bytes = ws.data_ptr(), ws.numel() * 8
    return a, (out, keep, ws)


def test_abi_argument_checks(sdy):
    lib = sdy.lib
    a, keep = _args(sdy)
    assert lib.sdy_dry_air_series_host(C.byref(a)) == 0
    assert lib.sdy_dry_air_workspace_bytes(2, 3, 12) == 2 * 3 * 1 * 2 * 8
    assert lib.sdy_dry_air_workspace_bytes(3, 2, 1028) == 3 * 2 * 2 * 2 * 8
    assert lib.sdy_dry_air_workspace_bytes(0, 3, 12) == 0 and lib.sdy_dry_air_workspace_bytes(2, 0, 12) == 0
    assert type(a) in sdy._lib.ABI_STRUCTS          # compared with the library: tests/test_capi_cpu.py

    def bad(mutate, code=-1, device=False):
        b, keep_b = _args(sdy)
        mutate(b)
        fn = lib.sdy_dry_air_series if device else lib.sdy_dry_air_series_host
        rc = fn(C.byref(b), None) if device else fn(C.byref(b))
        assert rc == code, (rc, code)

    for dev in (False, True):      # the device entry point refuses before it launches: no GPU is touched
        bad(lambda b: setattr(b, "K", 0), device=dev)                               # K out of range
        bad(lambda b: setattr(b, "K", 17), device=dev)
        bad(lambda b: setattr(b, "HW", 10), device=dev)                             # HW no multiple of 4
        bad(lambda b: setattr(b, "HW", 0), device=dev)
        bad(lambda b: setattr(b, "B", 0), device=dev)
        bad(lambda b: setattr(b, "T", 0), device=dev)
        bad(lambda b: setattr(b.ps, "stride_b", 38), device=dev)                    # a stride no multiple of 4
        bad(lambda b: setattr(b.q[1], "stride_t", 13), device=dev)
        bad(lambda b: setattr(b.q[0], "stride_b", -36), device=dev)
        bad(lambda b: setattr(b.ps, "channel", -1), device=dev)
        bad(lambda b: setattr(b.ps, "base", b.ps.base + 4), device=dev)             # a plane off the 16-byte boundary
        bad(lambda b: setattr(b, "area", None), device=dev)                         # a null required pointer
        bad(lambda b: setattr(b.ps, "base", None), device=dev)
        bad(lambda b: setattr(b.q[1], "base", None), device=dev)
        bad(lambda b: setattr(b, "gm", None), device=dev)
        bad(lambda b: setattr(b, "absdiff", None), device=dev)
        bad(lambda b: setattr(b, "mean_absdiff", None), device=dev)
        bad(lambda b: setattr(b, "gm", b.gm + 4), device=dev)
        bad(lambda b: setattr(b.ps, "std", 0.0), device=dev)
        bad(lambda b: setattr(b.q[0], "mean", float("nan")), device=dev)
        bad(lambda b: setattr(b, "B", 65536), code=-2, device=dev)
    # the workspace: device entry point only (the host twin keeps its partials to itself)
    bad(lambda b: setattr(b, "ws_bytes", b.ws_bytes - 1), device=True)              # one byte short
    bad(lambda b: setattr(b, "ws", None), device=True)
    bad(lambda b: setattr(b, "ws", b.ws + 4), device=True)
    assert lib.sdy_dry_air_series(None, None) == -1 and lib.sdy_dry_air_series_host(None) == -1
    # levels past K are not required
    b, keep_b = _args(sdy)
    b.q[2].base = None
    assert lib.sdy_dry_air_series_host(C.byref(b)) == 0


# ---- the Python surface: names, NaN paths, errors -----------------------------------------------------------------------------
def _sigma(K=2):
    return co.Sigma(torch.linspace(0.0, 1.0, K + 1), torch.linspace(0.0, 1.0, K + 1))


def test_reexports_and_defaults(sdy):
    assert sdy.ConservationLossConfig().dry_air_penalty is None
    loss = sdy.ConservationLossConfig(dry_air_penalty=0.5).build(torch.ones(4, 6), _sigma())
    assert isinstance(loss, sdy.ConservationLoss) and loss.dry_air_penalty == 0.5
    assert sdy.conservation.ConservationLoss is sdy.ConservationLoss
    assert sdy.conservation.compute_dry_air_absolute_differences is sdy.compute_dry_air_absolute_differences
    assert sdy.conservation.get_dry_air_nonconservation is sdy.get_dry_air_nonconservation
    assert sdy.conservation.DerivedMetricsAggregator is sdy.DerivedMetricsAggregator


def test_name_resolution_follows_climate_data(sdy):
    names = [f"specific_total_water_{k}" for k in (10, 2, 0, 1, 3, 4, 5, 6, 7, 8, 9)] + ["PS", "TMP2m"]
    water, ps = sdy.conservation.resolve(names)
    assert water == [f"specific_total_water_{k}" for k in range(11)] and ps == "PS"
    assert sdy.conservation.resolve(names + ["PRESsfc"])[1] == "PRESsfc"         # the first alias wins (ClimateData._get)
    assert sdy.conservation.resolve(["PRESsfc", "TMP2m"]) is None
    assert sdy.conservation.resolve(["specific_total_water_0"]) is None


def test_missing_fields_give_the_reference_nan(sdy):
    """The fixture records what the reference does: a `(1,)` NaN, a NaN `dry_air_loss`, and a NaN `loss` (it is added)."""
    facts = co.fixture()[2]
    area, sigma = torch.ones(4, 6), _sigma()
    full = {"specific_total_water_0": torch.ones(2, 3, 4, 6), "specific_total_water_1": torch.ones(2, 3, 4, 6),
            "PRESsfc": torch.ones(2, 3, 4, 6)}
    for label, data in (("no_pressure", {k: v for k, v in full.items() if k != "PRESsfc"}), ("no_water", {"PRESsfc": full["PRESsfc"]})):
        assert facts[label] == dict(absdiff_shape=[1], absdiff_all_nan=True, dry_air_loss_is_nan=True, loss_is_nan=True)
        got = sdy.compute_dry_air_absolute_differences(data, area, sigma)
        assert got.shape == (1,) and bool(torch.isnan(got).all())
        mean = sdy.get_dry_air_nonconservation(data, area, sigma)
        assert mean.dim() == 0 and bool(torch.isnan(mean))
        metrics, loss = sdy.ConservationLossConfig(dry_air_penalty=0.25).build(area, sigma)(data)
        assert list(metrics) == ["dry_air_loss"] and bool(torch.isnan(metrics["dry_air_loss"])) and bool(torch.isnan(loss))
        with pytest.raises(KeyError):           # ClimateData raises before DryAir's NaN branch
            sdy.DerivedMetricsAggregator(area, sigma).record_batch(data, data, None, None)
    assert facts["one_time"] == dict(absdiff_shape=[0], absdiff_all_nan=True, dry_air_loss_is_nan=True, loss_is_nan=True)
    assert facts["no_penalty"] == dict(metrics=[], loss=0.0)
    metrics, loss = sdy.ConservationLossConfig().build(area, sigma)(full)       # no penalty: no tensor is touched
    assert metrics == {} and float(loss) == 0.0


def test_errors(sdy):
    area = torch.ones(4, 6)
    d = {"specific_total_water_0": torch.ones(2, 3, 4, 6), "specific_total_water_1": torch.ones(2, 3, 4, 6),
         "PRESsfc": torch.ones(2, 3, 4, 6)}
    with pytest.raises(RuntimeError, match="GPU only"):
        sdy.compute_dry_air_absolute_differences(d, area, _sigma())
    with pytest.raises(RuntimeError, match="GPU only"):
        sdy.ConservationLossConfig(dry_air_penalty=1.0).build(area, _sigma())(d)
    with pytest.raises(RuntimeError, match="GPU only"):
        sdy.DerivedMetricsAggregator(area, _sigma()).record_batch(d, d, None, None)
    with pytest.raises(ValueError, match="vertical levels"):
        sdy.get_dry_air_nonconservation(d, area, _sigma(K=3))
    with pytest.raises(ValueError, match="vertical levels"):
        sdy.ConservationLossConfig().build(area, co.Sigma([0.0, 1.0], [0.0, 0.5, 1.0]))
    with pytest.raises(ValueError, match="No batches"):
        sdy.DerivedMetricsAggregator(area, _sigma()).get_logs("x")


def test_state_round_trip(sdy):
    area, sigma = torch.rand(4, 6), _sigma()
    loss = sdy.ConservationLossConfig(dry_air_penalty=0.125).build(area, sigma)
    state = loss.get_state()
    assert state["config"] == {"dry_air_penalty": 0.125} and state["area_weights"] is area and state["sigma_coordinates"] is sigma
    again = sdy.ConservationLoss.from_state(state)
    assert again.dry_air_penalty == 0.125 and again.get_state()["area_weights"] is area


def test_stepper_takes_a_conservation_loss(sdy):
    names = ["specific_total_water_0", "specific_total_water_1", "PRESsfc"]
    stats = {n: 1.0 for n in names}
    loss = sdy.ConservationLossConfig(dry_air_penalty=0.5).build(torch.ones(4, 6), _sigma())
    assert sdy.MultiStepStepper(None, names, names, [], stats, stats, conservation_loss=loss)._conserve is loss
    assert sdy.MultiStepStepper(None, names, names, [], stats, stats)._conserve is None
    off = sdy.ConservationLossConfig().build(torch.ones(4, 6), _sigma())
    assert sdy.MultiStepStepper(None, names, names, [], stats, stats, conservation_loss=off)._conserve is None
