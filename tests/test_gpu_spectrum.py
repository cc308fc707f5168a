"""Spherical power spectra on the device (csrc/spectrum.hip; sdy_amd.spectrum): the reduction kernel against the library's
host twin, PowerSpectrumAggregator end to end against the float64 restatement, through run_inference, and power_spectrum.
Inputs, restatement and bounds: tests/spectrum_utils.py.

Device against host twin: BIT-IDENTICAL.  Both compile csrc/spectrum.h and share its summation order (orders ascending, rows
in 256 slots, a butterfly over the slot number's bits), so the derivable bound 2 (n + 4) 2^-53 is held with nothing to spare.
Every shape is tiny: a case is a handful of launches."""
import ctypes as C

import numpy as np
import pytest
import torch

import spectrum_utils as su

pytestmark = pytest.mark.gpu

GUARD = 4096          # float64 elements of NaN either side of an accumulator: more than any of these cases' accumulators hold
FILL = 0.5            # what the accumulators hold before the call (the kernel adds)


class Guarded:
    """A float64 device tensor of `shape`, filled with FILL, inside NaN guard bands.  (The guarded buffer of
    tests/sht_stages_utils.py, `Buf`, is float32 and starts out as NaN or as a copy of an input; the accumulators here are
    float64 and are added to, so they start from a finite value.)"""

    def __init__(self, shape):
        n = int(np.prod(shape))
        self.raw = torch.full((n + 2 * GUARD,), float("nan"), dtype=torch.float64, device="cuda")
        self.t = self.raw[GUARD:GUARD + n].view(shape)
        self.t.fill_(FILL)

    def guards_intact(self):
        return bool(torch.isnan(self.raw[:GUARD]).all()) and bool(torch.isnan(self.raw[-GUARD:]).all())


def _bits_equal(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


@pytest.mark.parametrize("case", su.REDUCTION_CASES, ids=su.case_id)
def test_kernel_against_the_host_twin(case):
    import sdy_amd
    from sdy_amd._lib import current_stream

    lmax, mtr, n0, n1, T, pad, scaled = case
    lay = su.Layout(lmax, mtr, 2, n0, n1, T, pad)
    nt = 6
    host = {k: np.full((2, nt, lmax), FILL) for k in ("gen", "target", "error")}
    dev = {k: Guarded((2, nt, lmax)) for k in host}
    for w, t_start in enumerate((0, 3)):
        bufs = su.random_case(lay, w, scaled)
        assert su.host_accumulate(lay, *bufs, t_start, host) == 0
        d = [None if b is None else torch.from_numpy(b).cuda() for b in bufs]
        assert all(x is None or x.data_ptr() % 16 == 0 for x in d)
        a = su.fill_args(lay, *[None if x is None else x.data_ptr() for x in d], t_start, nt,
                         tuple(dev[k].t.data_ptr() for k in ("gen", "target", "error")))
        assert sdy_amd.lib.sdy_degree_power(C.byref(a), current_stream()) == 0
        torch.cuda.synchronize()
    untouched = [t for t in range(nt) if not (0 <= t < T or 3 <= t < 3 + T)]
    for k in host:
        got = dev[k].t.cpu().numpy()
        assert dev[k].guards_intact(), k
        assert not np.isnan(got).any(), f"{k}: a padding field or an entry with m > l was read"
        assert (got[:, untouched] == FILL).all(), k
        rel = np.abs(got - host[k]) / host[k]
        print(f"{k}: worst relative distance from the host twin {rel.max():.2e}")
        assert _bits_equal(got, host[k]), k


def test_kernel_without_the_error_accumulator():
    import sdy_amd
    from sdy_amd._lib import current_stream

    lay = su.Layout(7, 5, 2, 3, 2, 3, 0)
    bufs = su.random_case(lay, 0)
    host = {k: np.full((2, 3, 7), FILL) for k in ("gen", "target", "error")}
    assert su.host_accumulate(lay, *bufs, 0, host, with_error=False) == 0
    dev = {k: Guarded((2, 3, 7)) for k in ("gen", "target")}
    d = [None if b is None else torch.from_numpy(b).cuda() for b in bufs]
    a = su.fill_args(lay, d[0].data_ptr(), d[1].data_ptr(), None, None, 0, 3,
                     (dev["gen"].t.data_ptr(), dev["target"].t.data_ptr(), None))
    assert sdy_amd.lib.sdy_degree_power(C.byref(a), current_stream()) == 0
    torch.cuda.synchronize()
    for k in dev:
        assert dev[k].guards_intact() and _bits_equal(dev[k].t.cpu().numpy(), host[k]), k


# ---- the aggregator end to end ----------------------------------------------------------------------------------------------
M, S, T1 = 3, 2, 4          # the small fields hold one time more than a window uses, for the time-sliced views
NAMES = ("white", "red", "near")


def _window(nlat, nlon, grid, members, times, sliced=False, flat=False):
    """(target dict, gen dict) on the device of the chosen members and times of su.window_fields.  `sliced`: the tensors are
    [:, 1:]-style views of buffers that hold all T1 times (non-contiguous)."""
    fields = su.window_fields(nlat, nlon, grid, M, S, T1)
    tgt, gen = {}, {}
    for name in NAMES:
        g, t = fields[name]
        if sliced:
            gd, td = torch.from_numpy(g[members]).cuda()[:, :, times], torch.from_numpy(t).cuda()[:, times]
            assert not gd.is_contiguous() and not td.is_contiguous()
        else:
            gd = torch.from_numpy(np.ascontiguousarray(g[members][:, :, times])).cuda()
            td = torch.from_numpy(np.ascontiguousarray(t[:, times])).cuda()
        gen[name], tgt[name] = (gd[0] if flat else gd), td
    return tgt, gen


def _check(data, nlat, nlon, grid, members, times, what):
    for name in NAMES:
        want, bound = su.pooled(su.reference_rows(nlat, nlon, grid, M, S, T1, name), members, times)
        for label in ("gen", "target", "error"):
            got = data[name][label].cpu().numpy()
            assert got.shape == want[label].shape, (name, label, got.shape)
            err = np.abs(got - want[label])
            print(f"{what} {grid} {name} {label}: worst |err| / bound = {(err / bound[label]).max():.3f}, "
                  f"worst |err| / P = {(err / want[label]).max():.2e}")
            assert (err <= bound[label]).all(), (what, grid, name, label)


@pytest.mark.parametrize("grid", su.GRIDS)
@pytest.mark.parametrize("what", ["stacked", "flat", "sliced", "two_windows"])
def test_aggregator_against_float64(grid, what):
    import sdy_amd

    nlat, nlon, T = 12, 24, 3
    members = slice(0, 1) if what == "flat" else slice(None)
    times = slice(1, 4) if what == "sliced" else slice(0, 3)
    agg = sdy_amd.PowerSpectrumAggregator(T, grid=grid)
    if what == "two_windows":
        for t0, t1 in ((0, 2), (2, 3)):
            tgt, gen = _window(nlat, nlon, grid, members, slice(t0, t1))
            agg.record_batch(0.0, tgt, gen, None, None, i_time_start=t0)
    else:
        tgt, gen = _window(nlat, nlon, grid, members, times, sliced=what == "sliced", flat=what == "flat")
        agg.record_batch(0.0, tgt, gen, None, None, i_time_start=0)
    data = agg.get_data()
    assert set(data) == set(NAMES) and agg.get_logs("x") == {}
    assert all(v.dtype == torch.float64 and v.is_cuda for d in data.values() for v in d.values())
    _check(data, nlat, nlon, grid, members, times, what)


def _close(data, ref, nlat, nlon, grid, what):
    """Two runs of the same rows: each is within `bound` of float64, so they are within 2 x bound of each other."""
    for name in NAMES:
        _, bound = su.pooled(su.reference_rows(nlat, nlon, grid, M, S, T1, name), slice(None), slice(0, 3))
        for label in ("gen", "target", "error"):
            diff = (data[name][label] - ref[name][label]).abs().cpu().numpy()
            print(f"{what} {name} {label}: worst |difference| / (2 bound) = {(diff / (2.0 * bound[label])).max():.3f}")
            assert (diff <= 2.0 * bound[label]).all(), (what, name, label)


def test_two_windows_equal_one_and_chunks_equal_none():
    """The same times in two windows or in one, the variables in one chunk or one by one (a workspace limit that holds a
    single variable): compared with the one-window, one-chunk aggregator and with float64."""
    import sdy_amd

    nlat, nlon, grid, T = 12, 24, "equiangular", 3
    tgt, gen = _window(nlat, nlon, grid, slice(None), slice(0, 3))
    one = sdy_amd.PowerSpectrumAggregator(T, grid=grid)
    one.record_batch(0.0, tgt, gen, None, None)
    small = sdy_amd.PowerSpectrumAggregator(T, grid=grid, max_workspace_bytes=150_000)
    small.record_batch(0.0, tgt, gen, None, None)
    assert small.workspace_bytes <= 150_000 < one.workspace_bytes
    two = sdy_amd.PowerSpectrumAggregator(T, grid=grid)
    for t0, t1 in ((0, 2), (2, 3)):
        wt, wg = _window(nlat, nlon, grid, slice(None), slice(t0, t1))
        two.record_batch(0.0, wt, wg, None, None, i_time_start=t0)
    _check(small.get_data(), nlat, nlon, grid, slice(None), slice(0, 3), "chunked")
    _close(small.get_data(), one.get_data(), nlat, nlon, grid, "chunked against one chunk")
    _close(two.get_data(), one.get_data(), nlat, nlon, grid, "two windows against one")
    with pytest.raises(ValueError, match="max_workspace_bytes"):
        sdy_amd.PowerSpectrumAggregator(T, grid=grid, max_workspace_bytes=10_000).record_batch(0.0, tgt, gen, None, None)
    with pytest.raises(ValueError, match="outside"):
        sdy_amd.PowerSpectrumAggregator(T, grid=grid).record_batch(0.0, tgt, gen, None, None, i_time_start=1)


def test_a_power_of_two_in_the_units_changes_nothing():
    """Fields are handed to the transform divided by a power of two and the reduction multiplies back: 2^10 x the field gives
    2^20 x the spectrum, bit for bit -- and a field far outside the fp16 range of the split-precision Legendre stage (a
    pressure in Pa) comes out finite."""
    import sdy_amd

    nlat, nlon, grid, T = 12, 24, "equiangular", 3
    tgt, gen = _window(nlat, nlon, grid, slice(None), slice(0, 3))
    out = []
    for f in (1.0, 1024.0):
        agg = sdy_amd.PowerSpectrumAggregator(T, grid=grid)
        agg.record_batch(0.0, {k: v * f for k, v in tgt.items()}, {k: v * f for k, v in gen.items()}, None, None)
        out.append(agg.get_data())
    for name in NAMES:
        for label in ("gen", "target", "error"):
            assert torch.equal(out[0][name][label] * 1024.0 ** 2, out[1][name][label]), (name, label)
    agg = sdy_amd.PowerSpectrumAggregator(T, grid=grid)
    agg.record_batch(0.0, {"ps": tgt["white"] * 1.0e3 + 1.0e5}, {"ps": gen["white"] * 1.0e3 + 1.0e5}, None, None)
    ps = agg.get_data()["ps"]
    assert all(bool(torch.isfinite(v).all()) for v in ps.values())
    assert float(ps["gen"][0, 0]) == pytest.approx(4.0 * np.pi * 1.0e10, rel=1e-2)      # the mean's power: (1e5)^2 x 4 pi


@pytest.mark.parametrize("S180,T180", [(4, 4), (3, 1)], ids=["fields16", "fields4"])
def test_aggregator_at_180x360(S180, T180):
    """The three fields, one variable each, at the production grid: 16 padded fields per side (a multiple of 16: the 360-point
    FFT kernels) and 4 (not one: the generic kernel).  A tight workspace makes every variable a chunk of its own."""
    import sdy_amd
    from sdy_amd import _lib

    nlat, nlon, grid = 180, 360, "equiangular"
    fields = su.window_fields(nlat, nlon, grid, 1, 4, 4)
    gen = {n: torch.from_numpy(np.ascontiguousarray(fields[n][0][0, :S180, :T180])).cuda() for n in NAMES}
    tgt = {n: torch.from_numpy(np.ascontiguousarray(fields[n][1][:S180, :T180])).cuda() for n in NAMES}
    n_fields = T180 * ((S180 + 3) // 4 * 4)
    one_variable = 4 * n_fields * (2 * nlat * nlon + 2 * 2 * nlat * nlat + 1)      # rows, Xf, both coefficient tensors, zeros
    agg = sdy_amd.PowerSpectrumAggregator(T180, grid=grid, max_workspace_bytes=one_variable + 4096)
    agg.record_batch(0.0, tgt, gen, None, None)
    assert agg.workspace_bytes <= one_variable + 4096
    kern = (C.c_int * 2)()
    plan = sdy_amd.sht.ShtPlan.get(nlat, nlon, nlat, nlon // 2 + 1, grid, torch.cuda.current_device())
    assert _lib.lib.sdy_sht_plan_kernels(plan.handle, C.byref(kern)) == 0
    assert kern[1] == 1, "the plan has no 360-point FFT kernels: the two cases would run the same code"
    assert (n_fields % 16 == 0) == (S180 == 4)
    data = agg.get_data()
    for name in NAMES:
        rows = su.reference_rows(nlat, nlon, grid, 1, 4, 4, name)
        rows = {k: (v[:, :S180] if k != "target" else v[:S180]) for k, v in rows.items()}
        want, bound = su.pooled(rows, slice(None), slice(0, T180))
        for label in ("gen", "target", "error"):
            err = np.abs(data[name][label].cpu().numpy() - want[label])
            print(f"180x360 {n_fields} fields {name} {label}: worst |err| / bound = {(err / bound[label]).max():.3f}, "
                  f"worst |err| / P = {(err / want[label]).max():.2e}")
            assert (err <= bound[label]).all(), (name, label)


def test_the_yardstick_of_the_transform():
    """Where EPS_SHT_MEASURED comes from: the relative weighted-L2 distance of sdy_amd.RealSHT from the float64 oracle on the
    fields of the end-to-end cases, printed per grid and field.  The end-to-end bound allows twice the measured value."""
    import sdy_amd

    worst = 0.0
    for nlat, nlon, grids, shape in ((12, 24, su.GRIDS, (M, S, T1)), (180, 360, ("equiangular",), (1, 4, 4))):
        for grid in grids:
            sht = sdy_amd.RealSHT(nlat, nlon, grid=grid)
            for name in NAMES:
                g, t = su.window_fields(nlat, nlon, grid, *shape)[name]
                for side, x, ref in zip(("gen", "target"), (g, t), su.reference_coeffs(nlat, nlon, grid, *shape, name)):
                    a = sht(torch.from_numpy(x).cuda()).cpu().numpy()
                    d = su.sht_distance(a, ref)
                    worst = max(worst, float(d.max()))
                    print(f"{nlat} x {nlon} {grid} {name} {side}: largest {d.max():.3e}, mean {d.mean():.3e}")
    print(f"largest {worst:.4e}; EPS_SHT_MEASURED {su.EPS_SHT_MEASURED:.3e}")
    assert worst <= su.EPS_SHT


def test_power_spectrum_is_the_aggregators_gen_of_one_row():
    import sdy_amd

    nlat, nlon = 12, 24
    for grid in su.GRIDS:
        x = torch.from_numpy(su.window_fields(nlat, nlon, grid, M, S, T1)["red"][0][0, 0, :1]).cuda()      # (1, H, W)
        agg = sdy_amd.PowerSpectrumAggregator(1, grid=grid)
        agg.record_batch(0.0, {"x": x[None]}, {"x": x[None]}, None, None)
        d = agg.get_data()["x"]
        p = sdy_amd.power_spectrum(x[0], grid=grid)
        assert p.shape == (nlat,) and p.dtype == torch.float64
        assert torch.equal(p, d["gen"][0]) and torch.equal(p, d["target"][0]) and bool((d["error"] == 0).all())
        many = sdy_amd.power_spectrum(torch.from_numpy(su.window_fields(nlat, nlon, grid, M, S, T1)["red"][0]).cuda(), grid=grid)
        assert many.shape == (M, S, T1, nlat)
        want = su.reference_rows(nlat, nlon, grid, M, S, T1, "red")["gen"]
        d = su.EPS_SHT * np.sqrt(want.sum(axis=-1, keepdims=True))
        assert (np.abs(many.cpu().numpy() - want) <= 2.0 * np.sqrt(want) * d + d ** 2).all()


def test_through_run_inference():
    """InferenceAggregator(power_spectrum_data=True) behind run_inference on the tiny synthetic stepper gives the arrays of a
    stand-alone aggregator fed the same windows; with the flag off the log keys are what they were."""
    import sdy_amd
    from sdy_amd import synthetic

    dev = torch.device("cuda", 0)
    n_out, n_forc, nlat, nlon, window, n_windows, members = 4, 2, 32, 64, 6, 2, 2
    exp, _, _ = synthetic.build_sampler(dev, state_chans=n_out, forcing_chans=n_forc, nlat=nlat, nlon=nlon, embed=16, layers=2,
                                        horizon=6, carried_input_only_channel=True)
    stepper, names, out_names = synthetic.build_stepper(exp, n_out, n_forc, carried_input_only_channel=True)
    steps = window * n_windows
    w = sdy_amd.metrics.spherical_area_weights(torch.linspace(-87.0, 87.0, nlat), nlon).cuda()

    class Tee:
        def __init__(self, *aggs):
            self.aggs = aggs

        def record_batch(self, **kw):
            for a in self.aggs:
                a.record_batch(**kw)

    logs = {}
    for on in (False, True):
        agg = sdy_amd.metrics.InferenceAggregator(w, n_timesteps=steps + 1, n_ensemble_members=members, power_spectrum_data=on)
        alone = sdy_amd.PowerSpectrumAggregator(steps + 1)
        sdy_amd.run_inference(Tee(agg, alone), stepper, synthetic.windows(names, n_windows, window, nlat, nlon, n_ics=2, seed=5),
                              steps, window, n_ensemble_members=members, eval_device=dev)
        logs[on] = agg.get_logs("inference")
    assert set(logs[True]) == set(logs[False])
    got, want = agg.get_power_spectrum_data(), alone.get_data()
    assert set(got) == set(want) == set(out_names)
    for name in out_names:
        for label in ("gen", "target", "error"):
            x = got[name][label]
            assert tuple(x.shape) == (steps + 1, nlat) and bool(torch.isfinite(x).all()) and bool((x >= 0).all())
            assert torch.equal(x, want[name][label]), (name, label)
