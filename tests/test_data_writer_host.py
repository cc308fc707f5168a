"""Host side of the data writers (`sdy_amd.data_writer`, csrc/coarsen_mean.h through `sdy_time_coarsen_host`): the time
coarsening against the reference's own `TimeCoarsen` (tests/golden/fx_time_coarsen.npz, tools/gen_golden.py:gen_time_coarsen)
and against float64, `sdy_time_coarsen`'s argument checks, and the Python layer's bookkeeping.  No GPU: the kernel compiles the
same header, so the semantics pinned here are what it computes.

Error bound, u = 2^-24: any fp32 summation order of f values followed by one division is within (f + 1) u max|x_i| of the
exact mean; that holds for the library and for the reference's torch result alike.  f = 1 is a copy and f = 2 one rounded add
and an exact halving (normal-range inputs): both bit for bit."""
import ctypes as C
import json
import types

import numpy as np
import pytest
import torch

import golden_utils as gu

ERR_ARG, ERR_UNSUPPORTED = -1, -2
U = 2.0 ** -24
WINDOWS = ((0, 7), (7, 6))        # (start_timestep, times) of the fixture's two windows


@pytest.fixture(scope="module")
def sdy():
    import sdy_amd

    return sdy_amd


@pytest.fixture(scope="module")
def fx():
    z = gu.load("fx_time_coarsen")
    return z, json.loads(str(z["cases"]))


def _bit_equal(a, b):
    return a.dtype == b.dtype == np.float32 and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def exact_and_bound(x, t_first, f):
    """float64 coarsening of (S, T, H, W) and the per-element bound (f + 1) u max|x_i| (0 where a time is copied)."""
    x = x.astype(np.float64)
    n = (x.shape[1] - t_first) // f
    g = x[:, t_first:t_first + n * f].reshape(x.shape[0], n, f, *x.shape[2:])
    mean = np.concatenate([x[:, :t_first], g.mean(axis=2)], axis=1)
    bound = np.concatenate([np.zeros_like(x[:, :t_first]), (f + 1) * U * np.abs(g).max(axis=2)], axis=1)
    return mean, (bound if f > 1 else np.zeros_like(mean))


def host_coarsen(sdy, xs, t_first, f):
    """sdy_time_coarsen_host on a list of equally shaped (S, T, H, W) float32 arrays."""
    from sdy_amd._lib import SdyCoarsenArgs

    S, T, H, W = xs[0].shape
    t_out = t_first + (T - t_first) // f
    xs = [np.ascontiguousarray(x) for x in xs]
    outs = [np.full((S, t_out, H, W), np.nan, dtype=np.float32) for _ in xs]
    a = SdyCoarsenArgs()
    a.nvars = len(xs)
    for i, (x, o) in enumerate(zip(xs, outs)):
        a.data[i], a.s0[i], a.s1[i], a.out[i] = x.ctypes.data, 0, T * H * W, o.ctypes.data
    a.n0, a.n1, a.T, a.HW, a.t_first, a.factor = 1, S, T, H * W, t_first, f
    assert sdy.lib.sdy_time_coarsen_host(C.byref(a)) == 0
    return outs


def expected_calls(z, case):
    """The wrapped writer's calls the fixture recorded, joined per window: (t_first, {source::name: (S, T_out, H, W)})."""
    calls = [{k.split("::", 2)[2]: z[k] for k in z.files if k.startswith(f"{case}::call{j}::")} for j in range(int(z[f"{case}::n_calls"]))]
    assert len(calls) == 3
    tensors = lambda c: {k: v for k, v in c.items() if "::" in k}  # noqa: E731
    first = {k: np.concatenate([calls[0][k], calls[1][k]], axis=1) for k in tensors(calls[0])}
    return calls, [(1, first), (0, tensors(calls[2]))]


def test_fixture_inputs_are_normal_range(fx):
    z, cases = fx
    assert len(cases) == 8 and z["factors"].tolist() == [1, 2, 3, 4]
    tiny = np.finfo(np.float32).tiny
    n = 0
    for k in z.files:
        if "::w" in k and not k.endswith("times"):
            assert z[k].dtype == np.float32 and np.isfinite(z[k]).all() and (np.abs(z[k]) >= tiny).all(), k
            n += 1
    assert n == 2 * 2 * 3


def test_host_entry_point_reproduces_every_fixture_case(sdy, fx):
    z, cases = fx
    for case in cases:
        grid, f = case.split("_f")
        f = int(f)
        _, windows = expected_calls(z, case)
        for w, (t_first, want) in enumerate(windows):
            keys = sorted(want)
            xs = [z[f"{grid}::w{w}::{k}"] for k in keys]
            T = xs[0].shape[1]
            got = host_coarsen(sdy, xs, t_first, f)
            for k, x, g in zip(keys, xs, got):
                assert g.shape[1] == want[k].shape[1] == t_first + (T - t_first) // f, (case, w, k)
                exact, bound = exact_and_bound(x, t_first, f)
                if f <= 2:
                    assert _bit_equal(g, want[k]), (case, w, k)
                assert (np.abs(g.astype(np.float64) - exact) <= bound).all(), (case, w, k)
                assert (np.abs(want[k].astype(np.float64) - exact) <= bound).all(), (case, w, k)
                assert (np.abs(g.astype(np.float64) - want[k]) <= 2 * bound).all(), (case, w, k)
                assert _bit_equal(g[:, :t_first], x[:, :t_first])
        # six times by four: one group, times 4 and 5 of the window dropped (changing them changes nothing)
        if f == 4:
            x = z[f"{grid}::w1::target::a"].copy()
            base = host_coarsen(sdy, [x], 0, 4)[0]
            assert base.shape[1] == 1
            x[:, 4:] = 1.0e30
            assert _bit_equal(host_coarsen(sdy, [x], 0, 4)[0], base)


def test_factor_one_keeps_every_bit_pattern(sdy):
    bits = np.array([0x00000000, 0x80000000, 0x00000001, 0x807FFFFF, 0x7F800000, 0xFF800000, 0x7FC00001, 0x7FA00000],
                    dtype=np.uint32)
    x = np.resize(bits, 2 * 3 * 8).view(np.float32).reshape(2, 3, 2, 4)
    got = host_coarsen(sdy, [x], 0, 1)[0]
    assert np.array_equal(got.view(np.uint32), x.view(np.uint32))


def test_time_coarsen_config(sdy):
    cfg = sdy.TimeCoarsenConfig(coarsen_factor=3)
    assert [cfg.n_coarsened_timesteps(n) for n in (1, 2, 3, 4, 5, 7, 19)] == [1, 1, 1, 2, 2, 3, 7]
    assert sdy.TimeCoarsenConfig(1).n_coarsened_timesteps(19) == 19
    for bad in (0, -2):
        with pytest.raises(ValueError):
            sdy.TimeCoarsenConfig(coarsen_factor=bad)
        with pytest.raises(ValueError):
            sdy.TimeCoarsen(object(), bad)
    inner = object()
    tc = cfg.build(inner)
    assert isinstance(tc, sdy.TimeCoarsen) and tc._data_writer is inner and tc._coarsen_factor == 3


class Recorder:
    def __init__(self):
        self.calls, self.flushed = [], 0

    def append_batch(self, target, prediction, start_timestep, start_sample, batch_times=None):
        self.calls.append((target, prediction, start_timestep, start_sample, batch_times))

    def flush(self):
        self.flushed += 1


@pytest.fixture()
def on_host(sdy, monkeypatch):
    """`sdy_amd.data_writer` with the launch replaced by the host entry point (same header, same checks)."""
    from sdy_amd import data_writer as dw

    launches = []

    def launch(a, device):
        launches.append((a.nvars, a.t_first, a.factor))
        sdy._lib.check(sdy.lib.sdy_time_coarsen_host(C.byref(a)), "sdy_time_coarsen_host")

    monkeypatch.setattr(dw, "_require_device", lambda v: None)
    monkeypatch.setattr(dw, "_launch", launch)
    return dw, launches


def test_call_sequence_and_start_timestep_mapping(fx, on_host):
    """The wrapped writer sees the reference's calls: at timestep 0 the initial condition alone, then the coarsened remainder at
    timestep 1 (both views of one buffer per source, from ONE launch per source); later windows at ((t - 1) // f) + 1."""
    dw, launches = on_host
    z, cases = fx
    for case in cases:
        grid, f = case.split("_f")
        f = int(f)
        recorded, _ = expected_calls(z, case)
        rec = Recorder()
        tc = dw.TimeCoarsen(rec, f)
        del launches[:]
        for w, (t0, _) in enumerate(WINDOWS):
            tgt = {"a": torch.from_numpy(z[f"{grid}::w{w}::target::a"])}
            pred = {n: torch.from_numpy(z[f"{grid}::w{w}::prediction::{n}"]) for n in ("a", "b")}
            tc.append_batch(tgt, pred, t0, int(z["start_sample"]), z[f"{grid}::w{w}::times"])
        assert launches == [(1, 1, f), (2, 1, f), (1, 0, f), (2, 0, f)]
        assert len(rec.calls) == 3
        assert [c[2] for c in rec.calls] == [0, 1, (6 // f) + 1] == [int(c["start_timestep"]) for c in recorded]
        for (tgt, pred, _, ss, times), want in zip(rec.calls, recorded):
            assert ss == int(want["start_sample"]) == 3
            assert np.array_equal(times, want["times"])
            assert list(tgt) == ["a"] and list(pred) == ["a", "b"]
            for src, d in (("target", tgt), ("prediction", pred)):
                for n, v in d.items():
                    w_ = want[f"{src}::{n}"]
                    assert tuple(v.shape) == w_.shape
                    if f <= 2:
                        assert _bit_equal(v.numpy(), w_), (case, src, n)
        ic, rest = rec.calls[0][1]["b"], rec.calls[1][1]["b"]
        assert ic.untyped_storage().data_ptr() == rest.untyped_storage().data_ptr()      # two views of the one output buffer
        tc.flush()
        assert rec.flushed == 1


def test_later_start_timesteps(on_host):
    dw, _ = on_host
    x = {"a": torch.randn(1, 6, 2, 4)}
    for f, starts in ((2, {7: 4, 13: 7}), (3, {7: 3, 13: 5, 4: 2}), (6, {7: 2, 13: 3})):
        for t0, want in starts.items():
            rec = Recorder()
            dw.TimeCoarsen(rec, f).append_batch(x, x, t0, 0)
            assert [c[2] for c in rec.calls] == [want]
            assert rec.calls[0][0]["a"].shape == (1, 6 // f, 2, 4) and rec.calls[0][4] is None


def test_the_time_axis_is_third_from_last_for_member_stacked_predictions(on_host):
    dw, _ = on_host
    g = torch.Generator().manual_seed(3)
    flat = torch.randn(2, 3, 5, 2, 4, generator=g)            # IC-major (samples, members, ...) storage
    stacked = flat.transpose(0, 1)                             # the window driver's (members, samples, time, lat, lon) view
    rec = Recorder()
    dw.TimeCoarsen(rec, 2).append_batch({"a": flat[:, 0]}, {"a": stacked}, 0, 0)
    (_, ic, *_), (_, rest, *_) = rec.calls
    assert ic["a"].shape == (3, 2, 1, 2, 4) and rest["a"].shape == (3, 2, 2, 2, 4)
    assert torch.equal(ic["a"], stacked[:, :, :1])
    assert torch.equal(rest["a"], stacked[:, :, 1:].unfold(2, 2, 2).mean(-1))


def test_windows_the_coarsening_cannot_fill(on_host):
    dw, _ = on_host
    rec = Recorder()
    x = {"a": torch.randn(1, 3, 2, 4)}
    with pytest.raises(ValueError):
        dw.TimeCoarsen(rec, 4).append_batch(x, x, 7, 0)       # three times, groups of four
    assert not rec.calls
    ic = {"a": torch.randn(1, 1, 2, 4)}
    dw.TimeCoarsen(rec, 4).append_batch(ic, ic, 0, 0)          # the initial condition alone is passed on as it is
    assert [c[2] for c in rec.calls] == [0] and torch.equal(rec.calls[0][0]["a"], ic["a"])


def test_cpu_tensors_raise(sdy):
    x = {"a": torch.zeros(1, 4, 2, 4)}
    rec = Recorder()
    with pytest.raises(RuntimeError, match="GPU only"):
        sdy.TimeCoarsen(rec, 2).append_batch(x, x, 0, 0)
    assert not rec.calls


def test_batch_times(sdy, on_host):
    dw, _ = on_host
    x = {"a": torch.randn(2, 7, 2, 4)}

    def run(times, f, t0=0):
        rec = Recorder()
        dw.TimeCoarsen(rec, f).append_batch(x, x, t0, 0, times)
        return [c[4] for c in rec.calls]

    assert run(None, 2) == [None, None]
    t = np.arange(14, dtype=np.float64).reshape(2, 7) * 6.0
    ic, rest = run(t, 3)
    assert np.array_equal(ic, t[:, :1]) and np.array_equal(rest, t[:, 1:].reshape(2, 2, 3).mean(-1))
    ic, rest = run(t, 4)                                       # six times by four: one label, the tail dropped
    assert np.array_equal(rest, t[:, 1:5].mean(axis=1, keepdims=True))
    (only,) = run(t, 2, t0=7)
    assert np.array_equal(only, t[:, :6].reshape(2, 3, 2).mean(-1))
    ic, rest = run(torch.from_numpy(t), 2)
    assert torch.equal(ic, torch.from_numpy(t[:, :1])) and torch.equal(rest, torch.from_numpy(t[:, 1:].reshape(2, 3, 2).mean(-1)))
    d = (np.datetime64("2021-01-01T00:00", "ns") + np.arange(7) * np.timedelta64(6, "h"))[None, :].repeat(2, axis=0)
    d[1] += np.timedelta64(365, "D")
    ic, rest = run(d, 2)
    assert ic.dtype == rest.dtype == d.dtype and np.array_equal(ic, d[:, :1])
    assert np.array_equal(rest, d[:, 1::2] + np.timedelta64(3, "h"))
    ic, rest = run(d, 3)
    assert np.array_equal(rest, d[:, 2::3])
    # an object offering the xarray calls is driven through the reference's calls
    seen = []

    class Times:
        def __init__(self, v):
            self.v = v

        def isel(self, indexers):
            seen.append(("isel", indexers))
            return Times(self.v[:, indexers["time"]])

        def coarsen(self, windows):
            seen.append(("coarsen", windows))
            return types.SimpleNamespace(mean=lambda: Times(self.v.reshape(2, -1, windows["time"]).mean(-1)))

    ic, rest = run(Times(t), 3)
    assert seen == [("isel", {"time": slice(None, 1)}), ("isel", {"time": slice(1, None)}), ("coarsen", {"time": 3})]
    assert np.array_equal(ic.v, t[:, :1]) and np.array_equal(rest.v, t[:, 1:].reshape(2, 2, 3).mean(-1))


def test_struct_size_matches_the_library(sdy):
    from sdy_amd._lib import SDY_MAX_VARS, SdyCoarsenArgs

    from sdy_amd._lib import ABI_STRUCTS

    assert SdyCoarsenArgs in ABI_STRUCTS            # compared with the library: tests/test_capi_cpu.py
    assert C.sizeof(SdyCoarsenArgs) >= SDY_MAX_VARS * 8 * 4 + 7 * 4


def test_argument_validation_returns_without_a_device(sdy):
    from sdy_amd._lib import SdyCoarsenArgs

    lib = sdy.lib
    T, HW = 5, 16
    data = np.zeros((2, T, HW), dtype=np.float32)       # host memory: a launch that passed the checks would not be right
    out = np.full((2, T, HW), 7.0, dtype=np.float32)

    def args(**kw):
        a = SdyCoarsenArgs()
        a.nvars = 1
        a.data[0], a.s0[0], a.s1[0], a.out[0] = data.ctypes.data, 0, T * HW, out.ctypes.data
        a.n0, a.n1, a.T, a.HW, a.t_first, a.factor = 1, 2, T, HW, 1, 2
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    bad = [dict(nvars=0), dict(nvars=97), dict(nvars=-1), dict(n0=0), dict(n1=0), dict(n1=-3), dict(T=0), dict(HW=0), dict(HW=-4),
           dict(factor=0), dict(factor=-1), dict(t_first=-1), dict(t_first=T + 1), dict(t_first=0, factor=T + 1)]
    for entry in (lib.sdy_time_coarsen, lib.sdy_time_coarsen_host):
        call = (lambda a: entry(a, None)) if entry is lib.sdy_time_coarsen else entry
        for kw in bad:
            assert call(C.byref(args(**kw))) == ERR_ARG, kw
        assert call(None) == ERR_ARG
        for field in ("data", "out"):
            a = args()
            getattr(a, field)[0] = None
            assert call(C.byref(a)) == ERR_ARG, field
        for field in ("s0", "s1"):
            a = args()
            getattr(a, field)[0] = -T * HW
            assert call(C.byref(a)) == ERR_ARG, field
        # sizes the index arithmetic does not cover: T * HW > 2^30, n0 * n1 >= 2^31
        assert call(C.byref(args(T=1 << 16, HW=1 << 15))) == ERR_UNSUPPORTED
        assert call(C.byref(args(n0=1 << 16, n1=1 << 15))) == ERR_UNSUPPORTED
    assert (out == 7.0).all()
    # t_first == T is a plain copy of the kept times; the last group may end exactly at T
    assert lib.sdy_time_coarsen_host(C.byref(args(t_first=T))) == 0 and np.array_equal(out, data)


def test_data_writer_config_and_composition(sdy, tmp_path):
    cfg = sdy.DataWriterConfig()
    assert (cfg.log_extended_video_netcdfs, cfg.save_prediction_files, cfg.save_raw_prediction_names, cfg.time_coarsen) == \
        (False, True, None, None)
    assert [f.name for f in __import__("dataclasses").fields(cfg)] == ["log_extended_video_netcdfs", "save_prediction_files",
                                                                       "save_raw_prediction_names", "time_coarsen"]
    with pytest.raises(ValueError, match="save_raw_prediction_names"):
        sdy.DataWriterConfig(save_prediction_files=False, save_raw_prediction_names=["a"])
    sdy.DataWriterConfig(save_prediction_files=False)
    with pytest.raises(NotImplementedError):
        sdy.DataWriter(str(tmp_path), 2, 19, None, None, enable_prediction_netcdfs=True, enable_video_netcdfs=True)
    with pytest.raises(NotImplementedError):
        sdy.DataWriterConfig(log_extended_video_netcdfs=True).build(str(tmp_path), 2, 19, None, None)
    dw = sdy.data_writer
    w = sdy.DataWriterConfig(save_raw_prediction_names=["a"], time_coarsen=sdy.TimeCoarsenConfig(3)).build(
        str(tmp_path), n_samples=2, n_timesteps=19, metadata=None, coords=None)
    kinds = [(type(x), type(x._data_writer)) for x in w._writers]
    assert kinds == [(dw.TimeCoarsen, dw.PredictionDataWriter), (dw.TimeCoarsen, sdy.HistogramDataWriter)]
    pred, hist = (x._data_writer for x in w._writers)
    assert pred._n_timesteps == 7 and hist._n_times == 7 and pred.save_names == ["a"] and pred._n_samples == 2
    w = sdy.DataWriter(str(tmp_path), 2, 19, None, None, enable_prediction_netcdfs=True, enable_video_netcdfs=False,
                       n_ensemble_members=3)
    assert [type(x) for x in w._writers] == [dw.PredictionDataWriter] and w._writers[0]._members == 3
    w = sdy.DataWriter(str(tmp_path), 2, 19, None, None, enable_prediction_netcdfs=False, enable_video_netcdfs=False,
                       n_ensemble_members=3, histogram_ensembles=True)
    assert [type(x) for x in w._writers] == [sdy.HistogramDataWriter]
    assert not list(tmp_path.iterdir())            # nothing is created before the first batch
    assert sdy.loop.NullDataWriter is sdy.NullDataWriter


def test_prediction_writer_takes_host_tensors_and_checks_bounds_first(sdy, tmp_path):
    g = torch.Generator().manual_seed(1)
    meta = {"a": types.SimpleNamespace(units="K", long_name="temperature")}
    coords = {"lat": np.linspace(-60.0, 60.0, 3), "lon": np.arange(4) * 90.0}
    wr = sdy.PredictionDataWriter(str(tmp_path), n_samples=3, n_timesteps=5, metadata=meta, coords=coords, save_names=["a", "b"])
    tgt = {"a": torch.randn(2, 2, 3, 4, generator=g), "skipped": torch.randn(2, 2, 3, 4, generator=g)}
    pred = {"a": torch.randn(2, 2, 3, 4, generator=g), "b": torch.randn(2, 2, 3, 4, generator=g)}
    for st, ss in ((4, 0), (-1, 0), (0, 2), (0, -1)):
        with pytest.raises(ValueError):
            wr.append_batch(tgt, pred, st, ss)
    with pytest.raises(ValueError):
        wr.append_batch(tgt, {"a": pred["a"][None]}, 0, 0)      # a member axis the file does not have
    assert not (tmp_path / "autoregressive_predictions").exists()
    wr.append_batch(tgt, pred, 1, 1)
    wr.flush()
    root = tmp_path / "autoregressive_predictions"
    assert sorted(p.name for p in (root / "target").iterdir()) == ["a.npy", "b.npy"] == sorted(p.name for p in (root / "prediction").iterdir())
    for src, d in (("target", tgt), ("prediction", pred)):
        for n in ("a", "b"):
            f = np.load(root / src / f"{n}.npy")
            assert f.dtype == np.float32 and f.shape == (3, 5, 3, 4)
            if n in d:
                assert _bit_equal(f[1:3, 1:3], d[n].numpy())
                f[1:3, 1:3] = np.nan
            assert np.isnan(f).all()
    index = json.loads((root / "index.json").read_text())
    assert index["dims"] == {"sample": 3, "timestep": 5, "lat": 3, "lon": 4}
    assert index["coords"] == {"lat": [-60.0, 0.0, 60.0], "lon": [0.0, 90.0, 180.0, 270.0]}
    assert index["variables"] == {"a": {"units": "K", "long_name": "temperature"}, "b": {}}
