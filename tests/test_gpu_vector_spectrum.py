"""Rotational / divergent kinetic-energy spectra on the device (csrc/vector_spectrum.hip, sdy_vector_legendre_fwd;
sdy_amd.spectrum): the reduction kernel against the library's host twin, the vector Legendre stage against the float64
products, KineticEnergySpectrumAggregator end to end against the restatement, kinetic_energy_spectrum, and through
InferenceAggregator.  Inputs, restatement and bounds: tests/vector_spectrum_utils.py.

Device against host twin: BIT-IDENTICAL (both compile csrc/vector_spectrum.h in the same order, contraction off).  The stage
and end-to-end bounds are derived, not measured.  Every shape is tiny: a case is a handful of launches."""
import ctypes as C

import numpy as np
import pytest
import torch

import vector_spectrum_utils as vu

pytestmark = pytest.mark.gpu

GUARD = 4096
FILL = 0.5            # what the accumulators hold before the call (the kernel adds)


class Guarded:
    """A device tensor of `shape` filled with `fill`, inside NaN guard bands."""

    def __init__(self, shape, dtype=torch.float64, fill=FILL):
        n = int(np.prod(shape))
        self.raw = torch.full((n + 2 * GUARD,), float("nan"), dtype=dtype, device="cuda")
        self.t = self.raw[GUARD:GUARD + n].view(shape)
        self.t.fill_(fill)

    def guards_intact(self):
        return bool(torch.isnan(self.raw[:GUARD]).all()) and bool(torch.isnan(self.raw[-GUARD:]).all())


def _bits_equal(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def _device_accumulate(lay, bufs, t_start, dev, with_error=True):
    import sdy_amd
    from sdy_amd._lib import current_stream

    d = [None if b is None else torch.from_numpy(b).cuda() for b in bufs]
    assert all(x is None or x.data_ptr() % 16 == 0 for x in d)
    accs = tuple(dev[k].t.data_ptr() if with_error or not k.startswith("err") else None for k in vu.ACCS)
    a = vu.fill_args(lay, *[None if x is None else x.data_ptr() for x in d], t_start, dev["gen_rot"].t.shape[1], accs)
    assert sdy_amd.lib.sdy_vector_degree_power(C.byref(a), current_stream()) == 0
    torch.cuda.synchronize()


@pytest.mark.parametrize("case", vu.REDUCTION_CASES, ids=vu.case_id)
def test_kernel_against_the_host_twin(case):
    lmax, mtr, n0, n1, T, pad, scaled = case
    lay = vu.Layout(lmax, mtr, 2, n0, n1, T, pad)
    nt = 6
    host = {k: np.full((2, nt, lmax), FILL) for k in vu.ACCS}
    dev = {k: Guarded((2, nt, lmax)) for k in vu.ACCS}
    for w, t_start in enumerate((0, 3)):
        bufs = vu.random_case(lay, w, scaled)
        assert vu.host_accumulate(lay, bufs, t_start, host) == 0
        _device_accumulate(lay, bufs, t_start, dev)
    untouched = [t for t in range(nt) if not (0 <= t < T or 3 <= t < 3 + T)]
    for k in vu.ACCS:
        got = dev[k].t.cpu().numpy()
        assert dev[k].guards_intact(), k
        assert not np.isnan(got).any(), f"{k}: a padding field or an entry with m > l was read"
        assert (got[:, untouched] == FILL).all(), k
        print(f"{k}: worst relative distance from the host twin {(np.abs(got - host[k]) / host[k]).max():.2e}")
        assert _bits_equal(got, host[k]), k


def test_kernel_without_the_error_accumulators():
    lay = vu.Layout(7, 5, 2, 3, 2, 3, 0)
    bufs = vu.random_case(lay, 0)
    host = {k: np.full((2, 3, 7), FILL) for k in vu.ACCS}
    assert vu.host_accumulate(lay, bufs, 0, host, with_error=False) == 0
    dev = {k: Guarded((2, 3, 7)) for k in vu.ACCS}
    _device_accumulate(lay, bufs, 0, dev, with_error=False)
    for k in vu.ACCS:
        assert dev[k].guards_intact() and _bits_equal(dev[k].t.cpu().numpy(), host[k]), k
    assert (host["err_rot"] == FILL).all() and (host["err_div"] == FILL).all()


# ---- the stage ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nlat,nlon,grid", [(12, 24, "equiangular"), (12, 24, "legendre-gauss"), (180, 360, "equiangular")])
def test_stage_against_float64(nlat, nlon, grid):
    """sdy_rfft_lon + sdy_vector_legendre_fwd of four fields (two white, a red wind's u and v) against the float64 products,
    within the derived bound of tests/vector_spectrum_utils.py; entries with m > l are exact zeros."""
    import sdy_amd
    from sdy_amd._lib import current_stream, lib
    from sdy_amd.spectrum import VectorShtPlan

    F = 4
    ru, rv = vu.red_wind((1,), nlat, nlon, grid, "stage")
    x = np.concatenate([vu.su.white((2,), nlat, nlon, "stage"), ru, rv]).astype(np.float32)
    plan = sdy_amd.sht.ShtPlan.get(nlat, nlon, nlat, nlon // 2 + 1, grid, torch.cuda.current_device())
    vplan = VectorShtPlan.get(plan)
    lmax, mtr = plan.lmax, plan.mtr
    xd = torch.from_numpy(x).cuda()
    Xf = torch.empty(mtr * nlat * 2 * F, dtype=torch.float32, device="cuda")
    out = [Guarded((lmax, mtr, 2, F), torch.float32, float("nan")) for _ in range(2)]
    s = current_stream()
    assert lib.sdy_rfft_lon(plan.handle, xd.data_ptr(), None, None, None, Xf.data_ptr(), 1, F, s) == 0
    assert lib.sdy_vector_legendre_fwd(vplan.handle, Xf.data_ptr(), out[0].t.data_ptr(), out[1].t.data_ptr(), 1, F, s) == 0
    torch.cuda.synchronize()
    want = vu.products64(x, grid)
    bound = vu.stage_bound(x, grid)
    above = vu.su.m_weights(lmax, mtr) == 0                                   # [l][m]
    worst = 0.0
    for name, o, ref, b in zip(("A_D", "A_M"), out, want, bound):
        assert o.guards_intact(), name
        got = o.t.cpu().numpy().astype(np.float64)                             # [l][m][ri][field]
        assert not np.isnan(got).any(), name
        assert (got[above] == 0).all(), f"{name}: an entry with m > l is not an exact zero"
        ref, b = np.moveaxis(ref[..., :mtr], 0, -1), np.moveaxis(b[..., :mtr], 0, -1)      # [l][m][field]
        for ri, part in enumerate((ref.real, ref.imag)):
            err = np.abs(got[:, :, ri] - part)
            assert (err[b == 0] == 0).all(), name
            ratio = (err[b > 0] / b[b > 0]).max()
            worst = max(worst, float(ratio))
            print(f"{nlat} x {nlon} {grid} {name} {'re' if ri == 0 else 'im'}: largest |error| / bound = {ratio:.4f}")
            assert (err <= b).all(), (name, ri)
    print(f"{nlat} x {nlon} {grid}: largest observed ratio of error to bound {worst:.4f}")


def test_stage_arguments():
    from sdy_amd._lib import lib

    p = 1 << 20
    assert lib.sdy_vector_legendre_fwd(None, p, p, p, 1, 4, None) == -1
    h = C.c_void_p()
    assert lib.sdy_vsht_plan_create(None, C.byref(h)) == -1
    lib.sdy_vsht_plan_destroy(None)


# ---- the aggregator end to end ----------------------------------------------------------------------------------------------
M, S, T1 = 3, 2, 4          # the fields hold one time more than a window uses, for the time-sliced views
PAIRS = {name: (f"{name}_u", f"{name}_v") for name in ("white", "red", "near")}


def _window(nlat, nlon, grid, members, times, sliced=False, flat=False, factor=1.0):
    """(target dict, gen dict) on the device of the chosen members and times of vu.window_winds, plus one variable on the CPU
    that no pair names (it must not be read)."""
    winds = vu.window_winds(nlat, nlon, grid, M, S, T1)
    tgt, gen = {"other": torch.zeros(S, 1, nlat, nlon)}, {"other": torch.zeros(S, 1, nlat, nlon)}
    for name, names in PAIRS.items():
        for var, g, t in zip(names, *winds[name]):
            if sliced:
                gd, td = torch.from_numpy(g[members]).cuda()[:, :, times], torch.from_numpy(t).cuda()[:, times]
                assert not gd.is_contiguous() and not td.is_contiguous()
            else:
                gd = torch.from_numpy(np.ascontiguousarray(g[members][:, :, times])).cuda()
                td = torch.from_numpy(np.ascontiguousarray(t[:, times])).cuda()
            gen[var], tgt[var] = (gd[0] if flat else gd) * factor, td * factor
    return tgt, gen


def _check(data, nlat, nlon, grid, members, times, what):
    assert set(data) == set(PAIRS)
    for name in PAIRS:
        want, bound = vu.pooled(vu.reference_rows(nlat, nlon, grid, M, S, T1, name), members, times)
        assert set(data[name]) == set(vu.LABELS)
        for label in vu.LABELS:
            got = data[name][label].cpu().numpy()
            assert got.shape == want[label].shape, (name, label, got.shape)
            err = np.abs(got - want[label])
            print(f"{what} {grid} {name} {label}: worst |err| / bound = {(err / bound[label].clip(1e-300)).max():.4f}")
            assert (err <= bound[label]).all(), (what, grid, name, label)


@pytest.mark.parametrize("grid", vu.GRIDS)
@pytest.mark.parametrize("what", ["stacked", "flat", "sliced", "two_windows"])
def test_aggregator_against_float64(grid, what):
    import sdy_amd

    nlat, nlon, T = 12, 24, 3
    members = slice(0, 1) if what == "flat" else slice(None)
    times = slice(1, 4) if what == "sliced" else slice(0, 3)
    agg = sdy_amd.KineticEnergySpectrumAggregator(PAIRS, T, grid=grid)
    if what == "two_windows":
        for t0, t1 in ((0, 2), (2, 3)):
            tgt, gen = _window(nlat, nlon, grid, members, slice(t0, t1))
            agg.record_batch(0.0, tgt, gen, None, None, i_time_start=t0)
    else:
        tgt, gen = _window(nlat, nlon, grid, members, times, sliced=what == "sliced", flat=what == "flat")
        agg.record_batch(0.0, tgt, gen, None, None, i_time_start=0)
    data = agg.get_data()
    assert agg.get_logs("x") == {}
    assert all(v.dtype == torch.float64 and v.is_cuda for d in data.values() for v in d.values())
    _check(data, nlat, nlon, grid, members, times, what)


def _close(data, ref, nlat, nlon, grid, what):
    """Two runs of the same rows: each is within `bound` of float64, so they are within 2 x bound of each other."""
    for name in PAIRS:
        _, bound = vu.pooled(vu.reference_rows(nlat, nlon, grid, M, S, T1, name), slice(None), slice(0, 3))
        for label in vu.LABELS:
            diff = (data[name][label] - ref[name][label]).abs().cpu().numpy()
            print(f"{what} {name} {label}: worst |difference| / (2 bound) = {(diff / (2.0 * bound[label]).clip(1e-300)).max():.4f}")
            assert (diff <= 2.0 * bound[label]).all(), (what, name, label)


def test_two_windows_equal_one_and_chunks_equal_none():
    import sdy_amd

    nlat, nlon, grid, T = 12, 24, "equiangular", 3
    tgt, gen = _window(nlat, nlon, grid, slice(None), slice(0, 3))
    one = sdy_amd.KineticEnergySpectrumAggregator(PAIRS, T, grid=grid)
    one.record_batch(0.0, tgt, gen, None, None)
    # one pair of this window: 2 x 3 x 8 generated and 2 x 3 x 4 target fields
    fg, ft, per_x, per_cs = 48, 24, nlat * nlon + 2 * nlat * nlat, 2 * nlat * nlat
    one_pair = 4 * (fg * per_x + 2 * (fg + ft) * per_cs + fg)
    small = sdy_amd.KineticEnergySpectrumAggregator(PAIRS, T, grid=grid, max_workspace_bytes=one_pair + 4096)
    small.record_batch(0.0, tgt, gen, None, None)
    assert small.workspace_bytes <= one_pair + 4096 < one.workspace_bytes
    two = sdy_amd.KineticEnergySpectrumAggregator(PAIRS, T, grid=grid)
    for t0, t1 in ((0, 2), (2, 3)):
        wt, wg = _window(nlat, nlon, grid, slice(None), slice(t0, t1))
        two.record_batch(0.0, wt, wg, None, None, i_time_start=t0)
    _check(small.get_data(), nlat, nlon, grid, slice(None), slice(0, 3), "chunked")
    _close(small.get_data(), one.get_data(), nlat, nlon, grid, "chunked against one chunk")
    _close(two.get_data(), one.get_data(), nlat, nlon, grid, "two windows against one")
    with pytest.raises(ValueError, match="max_workspace_bytes"):
        sdy_amd.KineticEnergySpectrumAggregator(PAIRS, T, grid=grid, max_workspace_bytes=10_000).record_batch(0.0, tgt, gen)
    with pytest.raises(ValueError, match="outside"):
        sdy_amd.KineticEnergySpectrumAggregator(PAIRS, T, grid=grid).record_batch(0.0, tgt, gen, i_time_start=1)


def test_a_power_of_two_in_the_units_scales_exactly():
    """2^7 x (u, v) gives 2^14 x every output, bit for bit: the per-field pre-scale and its undoing are exact."""
    import sdy_amd

    nlat, nlon, grid, T = 12, 24, "equiangular", 3
    out = []
    for f in (1.0, 128.0):
        tgt, gen = _window(nlat, nlon, grid, slice(None), slice(0, 3), factor=f)
        agg = sdy_amd.KineticEnergySpectrumAggregator(PAIRS, T, grid=grid)
        agg.record_batch(0.0, tgt, gen, None, None)
        out.append(agg.get_data())
    for name in PAIRS:
        for label in vu.LABELS:
            assert torch.equal(out[0][name][label] * 128.0 ** 2, out[1][name][label]), (name, label)
            assert bool((out[0][name][label][:, 1:] > 0).all()), (name, label)


def test_kinetic_energy_spectrum_is_the_aggregators_gen_of_one_row():
    import sdy_amd

    nlat, nlon = 12, 24
    for grid in vu.GRIDS:
        (gu, gv), _ = vu.window_winds(nlat, nlon, grid, M, S, T1)["red"]
        u, v = torch.from_numpy(gu[0, 0, :1]).cuda(), torch.from_numpy(gv[0, 0, :1]).cuda()          # (1, H, W)
        agg = sdy_amd.KineticEnergySpectrumAggregator({"w": ("u", "v")}, 1, grid=grid)
        agg.record_batch(0.0, {"u": u[None], "v": v[None]}, {"u": u[None], "v": v[None]})
        d = agg.get_data()["w"]
        e = sdy_amd.kinetic_energy_spectrum(u[0], v[0], grid=grid)
        assert set(e) == {"rot", "div"}
        for part in ("rot", "div"):
            assert e[part].shape == (nlat,) and e[part].dtype == torch.float64
            assert torch.equal(e[part], d[f"gen_{part}"][0]) and torch.equal(e[part], d[f"target_{part}"][0])
            assert bool((d[f"error_{part}"] == 0).all())
        many = sdy_amd.kinetic_energy_spectrum(torch.from_numpy(gu).cuda(), torch.from_numpy(gv).cuda(), grid=grid)
        rows = vu.reference_rows(nlat, nlon, grid, M, S, T1, "red")
        for part in ("rot", "div"):
            assert many[part].shape == (M, S, T1, nlat)
            want, dl = rows[part]["gen"], rows[part]["d_gen"]
            assert (np.abs(many[part].cpu().numpy() - want) <= np.sqrt(2.0 * want) * dl + 0.5 * dl ** 2).all(), part
    with pytest.raises(RuntimeError, match="GPU only"):
        sdy_amd.kinetic_energy_spectrum(torch.zeros(12, 24), torch.zeros(12, 24))
    with pytest.raises(ValueError, match="one shape"):
        sdy_amd.kinetic_energy_spectrum(torch.zeros(12, 24).cuda(), torch.zeros(2, 12, 24).cuda())


def test_refusals():
    import sdy_amd

    KE = sdy_amd.KineticEnergySpectrumAggregator
    z = lambda *shape: torch.zeros(*shape, 12, 24).cuda()      # noqa: E731
    with pytest.raises(ValueError, match="twice"):
        KE({"w": ("u", "u")}, 3)
    agg = KE({"w": ("u", "v")}, 3)
    with pytest.raises(ValueError, match="'v'"):
        agg.record_batch(0.0, {"u": z(2, 3), "v": z(2, 3)}, {"u": z(2, 3)})                          # missing generated v
    with pytest.raises(ValueError, match="'v'"):
        agg.record_batch(0.0, {"u": z(2, 3)}, {"u": z(2, 3), "v": z(2, 3)})                          # missing target v
    with pytest.raises(ValueError, match="shape or layout"):
        agg.record_batch(0.0, {"u": z(2, 3), "v": z(2, 3)}, {"u": z(3, 2, 3), "v": z(2, 3)})         # stacked u, flat v
    with pytest.raises(ValueError, match="shape or layout"):
        agg.record_batch(0.0, {"u": z(2, 3), "v": z(2, 3)}, {"u": z(3, 2, 3), "v": z(4, 2, 3)})      # member counts differ
    with pytest.raises(RuntimeError, match="GPU only"):
        agg.record_batch(0.0, {"u": z(2, 3), "v": z(2, 3).cpu()}, {"u": z(2, 3), "v": z(2, 3)})
    with pytest.raises(RuntimeError, match="No data"):
        agg.get_data()                                                                               # nothing was recorded
    assert sdy_amd.spectrum.wind_pairs(["eastward_wind_0", "TMP2m", "northward_wind_0", "UGRD10m", "VGRD10m",
                                        "eastward_wind_7"]) == {"wind_0": ("eastward_wind_0", "northward_wind_0"),
                                                                "wind_10m": ("UGRD10m", "VGRD10m")}


def test_through_run_inference():
    """InferenceAggregator(wind_pairs=...) behind run_inference on the tiny synthetic stepper gives the arrays of a stand-alone
    aggregator fed the same windows; the log keys are what they are without `wind_pairs`."""
    import sdy_amd
    from sdy_amd import synthetic

    dev = torch.device("cuda", 0)
    n_out, n_forc, nlat, nlon, window, n_windows, members = 4, 2, 32, 64, 6, 2, 2
    exp, _, _ = synthetic.build_sampler(dev, state_chans=n_out, forcing_chans=n_forc, nlat=nlat, nlon=nlon, embed=16, layers=2,
                                        horizon=6, carried_input_only_channel=True)
    stepper, names, out_names = synthetic.build_stepper(exp, n_out, n_forc, carried_input_only_channel=True)
    steps = window * n_windows
    w = sdy_amd.metrics.spherical_area_weights(torch.linspace(-87.0, 87.0, nlat), nlon).cuda()
    pairs = {"wind_a": (out_names[0], out_names[1]), "wind_b": (out_names[2], out_names[3])}

    class Tee:
        def __init__(self, *aggs):
            self.aggs = aggs

        def record_batch(self, **kw):
            for a in self.aggs:
                a.record_batch(**kw)

    logs = {}
    for on in (False, True):
        agg = sdy_amd.metrics.InferenceAggregator(w, n_timesteps=steps + 1, n_ensemble_members=members,
                                                  wind_pairs=pairs if on else None)
        alone = sdy_amd.KineticEnergySpectrumAggregator(pairs, steps + 1)
        sdy_amd.run_inference(Tee(agg, alone), stepper, synthetic.windows(names, n_windows, window, nlat, nlon, n_ics=2, seed=5),
                              steps, window, n_ensemble_members=members, eval_device=dev)
        logs[on] = agg.get_logs("inference")
    assert set(logs[True]) == set(logs[False])
    got, want = agg.get_kinetic_energy_data(), alone.get_data()
    assert set(got) == set(want) == set(pairs)
    for name in pairs:
        for label in vu.LABELS:
            x = got[name][label]
            assert tuple(x.shape) == (steps + 1, nlat) and bool(torch.isfinite(x).all()) and bool((x >= 0).all())
            assert torch.equal(x, want[name][label]), (name, label)
