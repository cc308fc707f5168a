"""Video statistics and zonal means without a GPU: the library's _host entry points (sdy_video_accumulate_host,
sdy_zonal_accumulate_host compile the header the kernels compile, csrc/field_stats.h) against the reference's own
VideoAggregator / ZonalMeanAggregator (tests/golden/fx_video.npz, fx_zonal_mean.npz) and against a float64 numpy restatement;
the argument checks of all four entry points; the Python layer's bookkeeping.  Bounds: tests/field_stats_utils.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import field_stats_utils as fs


@pytest.fixture(scope="module")
def cases():
    return fs.cases()


@pytest.fixture(scope="module")
def sdy():
    import sdy_amd

    return sdy_amd


def _grid(case):
    return case["windows"][0][1][case["names"][0]].shape[-2:]


def test_fixture_covers_the_cases(cases):
    assert set(cases) == {f"g{g}_s{s}" for g in ("16x32", "7x10") for s in (1, 2, 3)} | {"pooled"}
    for name, case in cases.items():
        assert case["n_timesteps"] == 10 and [w[0] for w in case["windows"]][:3] == [0, 4, 7]
        assert [w[1][case["names"][0]].shape[1] for w in case["windows"]][:3] == [4, 3, 3]
    assert cases["pooled"]["windows"][0][2]["a"].shape[:2] == (3, 2) and cases["pooled"]["zonal"] is None
    assert (7 * 10) % 4 != 0


@pytest.mark.parametrize("name", ["g16x32_s1", "g16x32_s2", "g16x32_s3", "g7x10_s1", "g7x10_s2", "g7x10_s3", "pooled"])
def test_video_host_against_reference_and_float64(cases, name):
    case = cases[name]
    H, W = _grid(case)
    acc, n_batches = fs.host_video(case)
    assert sorted(set(n_batches)) == ([1.0] if name == "pooled" else [1.0, 2.0])
    got = fs.video_outputs(acc, n_batches, case["names"], H, W)
    got.update(fs.target_variance(acc, n_batches, case["names"], H, W))
    assert set(case["out"]) == {k for k in got if not k.startswith("_Vt/")}
    fs.check_video_against_reference(case, got, name)
    want = fs.restate_video(case)
    for stat in fs.VIDEO_STATS:
        if stat in ("err_min", "err_max"):
            assert np.array_equal(acc[stat], want[stat]), stat
        else:
            fs.check_close(acc[stat], want[stat], f"{name} {stat} vs float64")
    # the plain form updates the two means only, to the same bits
    plain, _ = fs.host_video(case, extended=False)
    assert np.array_equal(plain["gen_mean"], acc["gen_mean"]) and np.array_equal(plain["target_mean"], acc["target_mean"])


def test_one_sample_gives_nan_rmse(cases):
    case = cases["g7x10_s1"]
    acc, n_batches = fs.host_video(case)
    assert np.isnan(acc["err_var"]).all()
    assert all(np.isnan(case["out"][f"rmse/{k}"]).all() for k in case["names"])


@pytest.mark.parametrize("name", ["g16x32_s1", "g16x32_s2", "g16x32_s3", "g7x10_s1", "g7x10_s2", "g7x10_s3"])
def test_zonal_host_against_reference_and_float64(cases, name):
    case = cases[name]
    gen_acc, target_acc, n_batches = fs.host_zonal(case)
    got = fs.zonal_outputs(gen_acc, target_acc, n_batches, case["names"])
    assert set(got) == set(case["zonal"])
    fs.check_zonal_against_reference(case, got, name)
    want_gen, want_target = fs.restate_zonal(case)
    fs.check_close(gen_acc, want_gen, f"{name} gen_acc vs float64")
    fs.check_close(target_acc, want_target, f"{name} target_acc vs float64")


def test_zonal_host_member_mean(cases):
    """A member-stacked gen: the member mean per sample (this library's rule; the reference drops ensembles here)."""
    case = dict(cases["pooled"], zonal=None)
    gen_acc, target_acc, _ = fs.host_zonal(case)
    want_gen, want_target = fs.restate_zonal(case)
    fs.check_close(gen_acc, want_gen, "pooled gen_acc vs float64")
    fs.check_close(target_acc, want_target, "pooled target_acc vs float64")


def test_times_outside_the_window_are_untouched(cases):
    case = cases["g7x10_s2"]
    names, nt = case["names"], case["n_timesteps"]
    t0, target, gen = case["windows"][1]
    sentinel = {s: (777.25 if s == "err_min" else -777.25) for s in fs.VIDEO_STATS}    # (one a min / a max replaces)
    acc = {s: np.full((len(names), nt, 70), sentinel[s]) for s in fs.VIDEO_STATS}
    a, keep = fs.video_args(target, gen, names, t0, nt, acc)
    import sdy_amd

    assert sdy_amd.lib.sdy_video_accumulate_host(C.byref(a)) == 0
    for s in fs.VIDEO_STATS:
        assert (acc[s][:, :t0] == sentinel[s]).all() and (acc[s][:, t0 + a.T:] == sentinel[s]).all(), s
        assert (acc[s][:, t0:t0 + a.T] != sentinel[s]).all(), s


def _valid_video(sdy, case):
    names, nt = case["names"], case["n_timesteps"]
    t0, target, gen = case["windows"][1]
    acc = fs.new_video_acc(len(names), nt, 70)
    a, keep = fs.video_args(target, gen, names, t0, nt, acc)
    return a, (keep, acc)


def _valid_zonal(sdy, case):
    names, nt = case["names"], case["n_timesteps"]
    t0, target, gen = case["windows"][1]
    S = target[names[0]].shape[0]
    accs = np.zeros((len(names), S, nt, 7)), np.zeros((len(names), S, nt, 7))
    a, keep = fs.zonal_args(target, gen, names, t0, nt, *accs)
    return a, (keep, accs)


BAD = [("nvars", 0), ("nvars", 97), ("n0", 0), ("n1", 0), ("n1", -1), ("T", 0), ("n_timesteps", 0), ("gs0", -1), ("gs1", -4),
       ("ts1", -1), ("t_start", -1), ("t_start", 8), ("n_timesteps", 6)]      # windows[1]: t_start 4, T 3, n_timesteps 10


@pytest.mark.parametrize("which", ["video", "zonal"])
def test_argument_checks(sdy, cases, which):
    """Every refusal of the entry points, on the _host twins and -- the checks run before anything touches a device -- on the
    device entry points with host pointers (return codes only; a refused call launches nothing)."""
    lib = sdy.lib
    make = _valid_video if which == "video" else _valid_zonal
    host = lib.sdy_video_accumulate_host if which == "video" else lib.sdy_zonal_accumulate_host
    dev = lib.sdy_video_accumulate if which == "video" else lib.sdy_zonal_accumulate
    a, keep = make(sdy, cases["g7x10_s2"])
    assert host(C.byref(a)) == 0
    assert host(None) == -1 and dev(None, None) == -1
    extents = [("HW", 0), ("HW", -3)] if which == "video" else [("H", 0), ("W", 0), ("W", -2)]
    required = ("gen_mean", "target_mean") if which == "video" else ("gen_acc", "target_acc")
    for field, value in BAD + extents + [(r, None) for r in required]:
        a, keep = make(sdy, cases["g7x10_s2"])
        setattr(a, field, value)
        assert host(C.byref(a)) == -1, (field, value)
        assert dev(C.byref(a), None) == -1, (field, value)
    for arr in ("gen", "target"):
        a, keep = make(sdy, cases["g7x10_s2"])
        getattr(a, arr)[1] = None
        assert host(C.byref(a)) == -1 and dev(C.byref(a), None) == -1, arr
    # t_start + T = n_timesteps is the last window that fits; one more is refused
    a, keep = make(sdy, cases["g7x10_s2"])
    a.t_start = a.n_timesteps - a.T
    assert host(C.byref(a)) == 0
    a.t_start = a.n_timesteps - a.T + 1
    assert host(C.byref(a)) == -1 and dev(C.byref(a), None) == -1
    a.t_start, a.T = 2 ** 31 - 2, 3                 # the sum is formed in 64 bits
    assert host(C.byref(a)) == -1 and dev(C.byref(a), None) == -1
    # sizes the kernels do not cover
    big = [dict(T=2 ** 15, n_timesteps=2 ** 16, **({"HW": 2 ** 15 + 1} if which == "video" else {"H": 2 ** 8, "W": 2 ** 7 + 1})),
           dict(n0=2 ** 16, n1=2 ** 15),
           dict(n_timesteps=2 ** 30, **({"HW": 2 ** 10} if which == "video" else {"H": 2 ** 10, "W": 1}))]
    for change in big:
        a, keep = make(sdy, cases["g7x10_s2"])
        for field, value in change.items():
            setattr(a, field, value)
        assert host(C.byref(a)) == -2, change
        assert dev(C.byref(a), None) == -2, change


def test_struct_sizes_match_the_bindings(sdy):
    from sdy_amd import _lib

    assert _lib.SdyVideoArgs in _lib.ABI_STRUCTS and _lib.SdyZonalArgs in _lib.ABI_STRUCTS   # tests/test_capi_cpu.py
    assert C.sizeof(_lib.SdyVideoArgs) < 4096 and C.sizeof(_lib.SdyZonalArgs) < 4096     # passed to the kernels by value


@pytest.mark.parametrize("cls", ["VideoAggregator", "ZonalMeanAggregator"])
def test_python_bookkeeping_without_a_device(sdy, cls):
    assert getattr(sdy, cls) is getattr(sdy.metrics, cls)
    make = (lambda **kw: sdy.VideoAggregator(10, True, **kw)) if cls == "VideoAggregator" else \
        (lambda **kw: sdy.ZonalMeanAggregator(10, **kw))
    t, g = {"a": torch.zeros(2, 3, 7, 10)}, {"a": torch.zeros(2, 3, 7, 10)}
    agg = make()
    with pytest.raises(RuntimeError, match="No data recorded"):
        agg.get_data()
    with pytest.raises(RuntimeError, match="GPU only"):
        agg.record_batch(0.0, t, g, i_time_start=0)
    with pytest.raises(RuntimeError, match="No data recorded"):       # a refused batch leaves nothing behind
        agg.get_data()
    need = (7 * 10 * 70 * 8) if cls == "VideoAggregator" else (2 * 10 * 2 * 7 * 8)
    with pytest.raises(ValueError, match=str(need)):
        make(max_bytes=need - 1).record_batch(0.0, t, g, i_time_start=0)
    with pytest.raises(RuntimeError, match="GPU only"):               # the limit itself passes
        make(max_bytes=need).record_batch(0.0, t, g, i_time_start=0)
    with pytest.raises(ValueError, match="outside"):
        agg.record_batch(0.0, t, g, i_time_start=8)
    with pytest.raises(ValueError, match="no target"):
        agg.record_batch(0.0, {}, g, i_time_start=0)
    assert agg.get_logs("x") == {}
    assert not getattr(agg, "accepts_sample_weights", False)


def test_inference_aggregator_keywords(sdy):
    m = sdy.metrics
    w = m.spherical_area_weights(torch.linspace(-80.0, 80.0, 7), 10)
    plain = m.InferenceAggregator(w, n_timesteps=10)
    assert "video" not in plain._aggregators and "zonal_mean" not in plain._aggregators
    agg = m.InferenceAggregator(w, n_timesteps=10, video_data=True, zonal_mean_data=True)
    assert isinstance(agg._aggregators["video"], m.VideoAggregator) and not agg._aggregators["video"]._extended
    assert isinstance(agg._aggregators["zonal_mean"], m.ZonalMeanAggregator)
    assert list(agg._aggregators)[:3] == list(plain._aggregators)
    ext = m.InferenceAggregator(w, n_timesteps=10, extended_video_data=True)
    assert ext._aggregators["video"]._extended and "zonal_mean" not in ext._aggregators
    with pytest.raises(RuntimeError, match="No data recorded"):
        agg.get_video_data()
    with pytest.raises(RuntimeError, match="No data recorded"):
        agg.get_zonal_mean_data()
    for kw in ("log_video", "enable_extended_videos", "log_zonal_mean_images"):
        with pytest.raises(NotImplementedError):
            m.InferenceAggregator(w, n_timesteps=10, video_data=True, zonal_mean_data=True, **{kw: True})


def test_reduce_min_max_without_a_process_group(sdy):
    d = sdy.metrics.TorchDistributed()
    x = torch.tensor([1.0, -2.0])
    assert d.reduce_min(x) is x and d.reduce_max(x) is x
