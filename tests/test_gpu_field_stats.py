"""Video statistics and zonal means on the device (csrc/field_stats.hip; sdy_amd.metrics.VideoAggregator / ZonalMeanAggregator)
against the reference's own aggregators (tests/golden/fx_video.npz, fx_zonal_mean.npz), against the library's _host twins and
through run_inference.  Bounds: tests/field_stats_utils.py.  Every shape here is tiny: a case is a handful of launches."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import field_stats_utils as fs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cases():
    return fs.cases()


def _dev(d):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in d.items()}


def _video_acc(agg):
    """The aggregator's accumulators as the (nvars, n_timesteps, HW) numpy arrays the _host twin fills (one grid only)."""
    nt = agg._n_timesteps
    return {s: b.view(len(agg._names), nt, -1).cpu().numpy() for s, b in agg._acc.items()}


def _run_video(case, extended=True):
    import sdy_amd

    agg = sdy_amd.VideoAggregator(case["n_timesteps"], extended)
    for t0, target, gen in case["windows"]:
        agg.record_batch(0.0, _dev(target), _dev(gen), i_time_start=t0)
    return agg


def _labels(data):
    out = {}
    for k, v in data.items():
        if isinstance(v, dict):
            out[f"{k}::gen"], out[f"{k}::target"] = v["gen"].cpu().numpy(), v["target"].cpu().numpy()
        else:
            out[k] = v.cpu().numpy()
    return out


@pytest.mark.parametrize("name", ["g16x32_s1", "g16x32_s2", "g16x32_s3", "g7x10_s1", "g7x10_s2", "g7x10_s3", "pooled"])
def test_video_against_reference_and_host(cases, name):
    case = cases[name]
    H, W = case["windows"][0][1][case["names"][0]].shape[-2:]
    agg = _run_video(case)
    data = agg.get_data()
    assert all(v.dtype == torch.float64 and v.is_cuda and tuple(v.shape) == (10, H, W)
               for d in data.values() for v in (d.values() if isinstance(d, dict) else [d]))
    got = _labels(data)
    assert list(data) == case["labels"]                  # the reference's labels, in its order
    acc = _video_acc(agg)
    n_batches = np.array(agg._n_batches, dtype=np.float64)
    got.update(fs.target_variance(acc, n_batches, case["names"], H, W))
    fs.check_video_against_reference(case, got, name)
    host, host_n = fs.host_video(case)
    assert np.array_equal(host_n, n_batches)
    for stat in fs.VIDEO_STATS:
        if stat in ("err_min", "err_max"):
            assert np.array_equal(acc[stat], host[stat]), stat
        else:
            fs.check_close(acc[stat], host[stat], f"{name} {stat} device vs host")
    # the plain aggregator: the same pair, nothing else; the dataset form
    plain = _run_video(case, extended=False)
    pd = plain.get_data()
    assert list(pd) == case["names"]
    for k in case["names"]:
        assert torch.equal(pd[k]["gen"], data[k]["gen"]) and torch.equal(pd[k]["target"], data[k]["target"])
    ds = agg.get_dataset()
    k = case["names"][0]
    assert ds[k].shape == (2, 10, H, W) and np.array_equal(ds[k][0], got[f"{k}::gen"])
    assert np.array_equal(ds[f"min_err_{k}"], got[f"min_err/{k}"])
    assert set(ds) == {lab.replace("/", "_") for lab in data}


@pytest.mark.parametrize("name", ["g16x32_s1", "g16x32_s2", "g16x32_s3", "g7x10_s1", "g7x10_s2", "g7x10_s3"])
def test_zonal_against_reference_and_host(cases, name):
    import sdy_amd

    case = cases[name]
    agg = sdy_amd.ZonalMeanAggregator(case["n_timesteps"])
    for t0, target, gen in case["windows"]:
        agg.record_batch(0.0, _dev(target), _dev(gen), _dev(target), _dev(gen), t0)
    data = agg.get_data()
    got = {k: v.cpu().numpy() for k, v in data.items()}
    assert set(got) == set(case["zonal"]) and all(v.dtype == torch.float64 for v in data.values())
    fs.check_zonal_against_reference(case, got, name)
    gen_acc, target_acc, _ = fs.host_zonal(case)
    fs.check_close(agg._acc["gen_acc"].cpu().numpy().reshape(gen_acc.shape), gen_acc, f"{name} gen_acc device vs host")
    fs.check_close(agg._acc["target_acc"].cpu().numpy().reshape(target_acc.shape), target_acc, f"{name} target_acc device vs host")


def _random_window(E, S, T, H, W, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    target = torch.randn(S, T, H, W, generator=g)
    gen = target[None] + 0.5 * torch.randn(E, S, T, H, W, generator=g)
    return target, gen


def _both(target, gen, nt=4, t0=1):
    """One window through both aggregators -> (video accumulators, zonal accumulators) as numpy."""
    import sdy_amd

    v, z = sdy_amd.VideoAggregator(nt, True), sdy_amd.ZonalMeanAggregator(nt)
    for agg in (v, z):
        agg.record_batch(0.0, {"x": target, "y": target}, {"x": gen, "y": gen}, i_time_start=t0)
    return {s: b.cpu().numpy() for s, b in v._acc.items()}, {s: b.cpu().numpy() for s, b in z._acc.items()}


def _same(a, b, exact):
    for s in a:
        if exact or s in ("err_min", "err_max"):
            assert np.array_equal(a[s], b[s], equal_nan=True), s
        else:
            fs.check_close(a[s], b[s], s)


def test_member_stacked_views(cases):
    """The member-stacked (E, S, ...) view against the flat pooled rows with the target repeated (video; vector path on
    16 x 32), and a genuinely non-contiguous 5-D view -- a slice of a larger buffer, the transposed view the window driver
    hands over -- against its contiguous copy (both aggregators)."""
    E, S, T, H, W = 3, 2, 2, 16, 32
    target, gen = _random_window(E, S, T, H, W, 7)
    target, gen = target.cuda(), gen.cuda()
    stacked_v, stacked_z = _both(target, gen)
    flat_v, _ = _both(target.repeat(E, 1, 1, 1), gen.reshape(E * S, T, H, W))
    _same(stacked_v, flat_v, exact=False)          # (the rows are summed in another order)
    big = torch.zeros(S + 1, E + 2, T, H, W, device="cuda")
    big[:S, 1:E + 1] = gen.transpose(0, 1)
    view = big[:S, 1:E + 1].transpose(0, 1)
    assert not view.is_contiguous() and view.shape == gen.shape and torch.equal(view, gen)
    view_v, view_z = _both(target, view)
    _same(view_v, stacked_v, exact=True)
    _same(view_z, stacked_z, exact=True)
    big_t = torch.zeros(S, T + 3, H, W, device="cuda")
    big_t[:, 2:2 + T] = target
    tv, tz = _both(big_t[:, 2:2 + T], view)
    _same(tv, stacked_v, exact=True)
    _same(tz, stacked_z, exact=True)


def test_misaligned_pointers_take_the_scalar_path():
    """HW % 4 == 0 but the data start 4 bytes off a 16-byte boundary: the scalar kernels.  A grid point's rows are summed in the
    same order on both paths (video: the same bits); a latitude row's longitudes meet in another order (zonal: 1e-12)."""
    E, S, T, H, W = 3, 2, 2, 8, 12
    target, gen = _random_window(E, S, T, H, W, 11)
    target, gen = target.cuda(), gen.cuda()
    aligned_v, aligned_z = _both(target, gen)

    def shifted(x):
        buf = torch.zeros(x.numel() + 1, device="cuda")
        buf[1:] = x.reshape(-1)
        out = buf[1:].view(x.shape)
        assert out.data_ptr() % 16 == 4
        return out

    off_v, off_z = _both(shifted(target), shifted(gen))
    _same(off_v, aligned_v, exact=True)
    _same(off_z, aligned_z, exact=False)


@pytest.mark.parametrize("H,W,S,T,E", [(3, 360, 1, 2, 1), (3, 360, 1, 2, 3), (5, 10, 2, 3, 1), (70, 4, 2, 3, 2), (4, 1, 3, 2, 1)])
def test_zonal_row_lengths(H, W, S, T, E):
    """W = 360 (the production longitude count: 90 quads, no multiple of 64), W = 10 (scalar path, 16 lanes per row), W = 4 (one
    lane per row) and W = 1, flat and member-stacked, against the _host twin and float64 numpy."""
    import sdy_amd

    target, gen = _random_window(E, S, T, H, W, 100 + W)
    if E == 1:
        gen = gen[0]
    nt, t0 = T + 2, 1
    agg = sdy_amd.ZonalMeanAggregator(nt)
    agg.record_batch(0.0, {"x": target.cuda()}, {"x": gen.cuda()}, i_time_start=t0)
    case = dict(names=["x"], n_timesteps=nt, windows=[(t0, {"x": target.numpy()}, {"x": gen.numpy()})])
    gen_acc, target_acc, _ = fs.host_zonal(case)
    want_gen, want_target = fs.restate_zonal(case)
    for got, host, want in ((agg._acc["gen_acc"], gen_acc, want_gen), (agg._acc["target_acc"], target_acc, want_target)):
        got = got.cpu().numpy().reshape(host.shape)
        fs.check_close(got, host, f"W={W} device vs host")
        fs.check_close(got, want, f"W={W} device vs float64")
        assert (got[:, :, :t0] == 0).all() and (got[:, :, t0 + T:] == 0).all()


def test_more_work_than_one_pass_of_the_grid():
    """One variable with more work items than the launch's threads (the grid-stride loops), at n_batches = 1."""
    S, T, H, W = 2, 3, 180, 360
    target, gen = _random_window(1, S, T, H, W, 3)
    gen = gen[0]
    case = dict(names=["x"], n_timesteps=T, windows=[(0, {"x": target.numpy()}, {"x": gen.numpy()})])
    agg = _run_video(case)
    want = fs.restate_video(case)
    acc = _video_acc(agg)
    for stat in fs.VIDEO_STATS:
        if stat in ("err_min", "err_max"):
            assert np.array_equal(acc[stat], want[stat]), stat
        else:
            fs.check_close(acc[stat], want[stat], f"{stat} vs float64")


def test_times_outside_the_window_are_untouched():
    import sdy_amd
    from sdy_amd._lib import SdyVideoArgs, SdyZonalArgs, current_stream

    S, T, H, W, nt, t0, nv = 2, 3, 7, 10, 9, 4, 2
    target, gen = _random_window(1, S, T, H, W, 5)
    target, gen = target.cuda(), gen[0].cuda()
    sentinel = {s: (777.25 if s == "err_min" else -777.25) for s in fs.VIDEO_STATS}
    acc = {s: torch.full((nv, nt, H * W), sentinel[s], dtype=torch.float64, device="cuda") for s in fs.VIDEO_STATS}
    a = SdyVideoArgs()
    a.nvars = nv
    for j in range(nv):
        a.gen[j], a.target[j] = gen.data_ptr(), target.data_ptr()
    a.n0, a.n1, a.T, a.HW, a.gs0, a.gs1, a.ts1 = 1, S, T, H * W, 0, T * H * W, T * H * W
    a.t_start, a.n_timesteps = t0, nt
    for s, b in acc.items():
        setattr(a, s, b.data_ptr())
    assert sdy_amd.lib.sdy_video_accumulate(C.byref(a), current_stream()) == 0
    for s, b in acc.items():
        b = b.cpu().numpy()
        assert (b[:, :t0] == sentinel[s]).all() and (b[:, t0 + T:] == sentinel[s]).all(), s
        assert (b[:, t0:t0 + T] != sentinel[s]).all(), s
    zacc = [torch.full((nv, S, nt, H), -777.25, dtype=torch.float64, device="cuda") for _ in range(2)]
    z = SdyZonalArgs()
    z.nvars = nv
    for j in range(nv):
        z.gen[j], z.target[j] = gen.data_ptr(), target.data_ptr()
    z.n0, z.n1, z.T, z.H, z.W, z.gs0, z.gs1, z.ts1 = 1, S, T, H, W, 0, T * H * W, T * H * W
    z.t_start, z.n_timesteps = t0, nt
    z.gen_acc, z.target_acc = zacc[0].data_ptr(), zacc[1].data_ptr()
    assert sdy_amd.lib.sdy_zonal_accumulate(C.byref(z), current_stream()) == 0
    for b in zacc:
        b = b.cpu().numpy()
        assert (b[:, :, :t0] == -777.25).all() and (b[:, :, t0 + T:] == -777.25).all()
        assert (b[:, :, t0:t0 + T] != -777.25).all()
    # an out-of-range time offset is refused by the entry point: the return code, and nothing was launched
    before = [b.clone() for b in list(acc.values()) + zacc]
    for t_start in (-1, nt - T + 1, nt, 2 ** 31 - 2):
        a.t_start = z.t_start = t_start
        assert sdy_amd.lib.sdy_video_accumulate(C.byref(a), current_stream()) == -1
        assert sdy_amd.lib.sdy_zonal_accumulate(C.byref(z), current_stream()) == -1
    assert all(torch.equal(x, y) for x, y in zip(before, list(acc.values()) + zacc))
    agg = sdy_amd.VideoAggregator(nt, True)
    with pytest.raises(ValueError, match="outside"):
        agg.record_batch(0.0, {"x": target}, {"x": gen}, i_time_start=nt - T + 1)


def test_through_run_inference():
    """run_inference on the tiny loop fixture (2 windows x 6 steps, 2 samples, 3 members) with the three new keywords: every
    label, finite at every time index; the default log keys unchanged."""
    import sdy_amd
    from test_gpu_derived import _loop_setup

    _, stepper, windows, sigma, n_total, n_mem, names = _loop_setup(3)
    w = sdy_amd.metrics.spherical_area_weights(torch.linspace(-87.0, 87.0, 32), 64).cuda()
    logs = {}
    for on in (False, True):
        agg = sdy_amd.metrics.InferenceAggregator(w, n_timesteps=n_total + 1, n_ensemble_members=3, video_data=on,
                                                  extended_video_data=on, zonal_mean_data=on)
        sdy_amd.run_inference(agg, stepper, types.SimpleNamespace(loader=windows), n_total, n_mem, 3)
        logs[on] = agg.get_logs("inference")
    assert set(logs[True]) == set(logs[False])
    video, zonal = agg.get_video_data(), agg.get_zonal_mean_data()
    out = names["out_names"]
    want = set(out) | {f"{lab}/{n}" for lab in ("bias", "rmse", "min_err", "max_err", "gen_var") for n in out}
    assert set(video) == want
    assert set(zonal) == {f"{lab}/{n}" for lab in ("gen", "error") for n in out}
    for k, v in video.items():
        for x in (v.values() if isinstance(v, dict) else [v]):
            assert tuple(x.shape) == (n_total + 1, 32, 64) and bool(torch.isfinite(x).all()), k
    for k, v in zonal.items():
        assert tuple(v.shape) == (n_total + 1, 32) and bool(torch.isfinite(v).all()), k
