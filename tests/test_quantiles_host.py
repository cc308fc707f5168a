"""Host side of the time quantiles (no GPU): the key transform, sdy_time_quantile_append_host + sdy_time_quantile_select_host --
the header the kernels compile (csrc/quantile.h) -- against the numpy restatement bit for bit and against np.nanquantile, what
the entry points refuse, and what `TimeQuantileAggregator`, `time_quantiles` and `InferenceAggregator(time_quantiles=...)`
refuse before they touch a device.  Data and comparisons: tests/quantile_utils.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import quantile_utils as qu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SDY_OK, SDY_ERR_ARG, SDY_ERR_UNSUPPORTED = 0, -1, -2


@pytest.fixture(scope="module")
def sdy():
    import sdy_amd

    return sdy_amd


# ---- the key ----------------------------------------------------------------------------------------------------------------
def _table():
    f = np.finfo(np.float32)
    tiny = np.array([1, 2, 0x7FFFFF], np.uint32).view(np.float32)                    # denormals
    pos = np.concatenate([[0.0], tiny, [f.tiny, 1.0, 1.0000001, 3.5, f.max, np.inf]]).astype(np.float32)
    return np.concatenate([-pos[::-1], pos]).astype(np.float32)                      # sorted; -0.0 next to +0.0


def _keys_and_back(sdy, x):
    """The keys the host append writes for a (time,) series at one point, and what select(lower, n = 1) reads back."""
    n = x.size
    field = np.ascontiguousarray(x.reshape(1, 1, n, 1, 1))
    series = qu.host_series(field, field[0], store_gen=0)                              # (1, n, 1)
    keys = series[0, :, 0].copy()
    back = np.empty(n, np.float64)
    for t in range(n):                                                                 # each time alone: a series of one slot
        out, valid = qu.host_select(np.ascontiguousarray(series[:, t:t + 1]), 1, 1, (0, 1, 1, 0, 1), (0.0,), "lower")
        back[t] = out[0, 0, 0, 0]
        assert valid[0, 0, 0] == (0 if np.isnan(x[t]) else 1)
    return keys, back


def test_key_round_trips_and_is_monotone(sdy):
    x = _table()
    keys, back = _keys_and_back(sdy, x)
    assert np.array_equal(keys, qu.key_of(x))
    # bit for bit, up to the sign of zero
    canon = np.where(x == 0, np.float32(0.0), x)
    assert np.array_equal(back.astype(np.float32).view(np.uint32), canon.view(np.uint32))
    assert np.array_equal(qu.value_of(keys).view(np.uint32), canon.view(np.uint32))
    # monotone on the sorted table: equal only for the two zeros
    d = np.diff(keys.astype(np.int64))
    assert (d >= 0).all() and (d == 0).sum() == 1 and keys[x == 0].tolist() == [0x80000000] * 2
    assert keys[0] == 0x007FFFFF and keys[-1] == 0xFF800000                           # -inf first, +inf last
    # every NaN -- both signs, several payloads -- has the one key, and a point of NaNs alone gives NaN
    nans = np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001, 0x7FFFFFFF, 0xFFFFFFFF, 0x7FC12345], np.uint32).view(np.float32)
    keys, back = _keys_and_back(sdy, nans)
    assert (keys == qu.NAN_KEY).all() and np.isnan(back).all()
    assert (qu.key_of(x) != qu.NAN_KEY).all()


# ---- the host twins against the restatement ---------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", qu.GRIDS)
@pytest.mark.parametrize("M", qu.MEMBERS)
@pytest.mark.parametrize("n", qu.TIMES)
def test_host_twins_against_restatement(sdy, grid, M, n):
    H, W = grid
    gen, target = qu.make_data(M, qu.SAMPLES, n, H, W)
    assert np.isnan(gen).any() and np.isinf(gen).any() and np.signbit(gen[:, :, 0, 3, 0]).all()
    series = qu.host_series(gen, target)
    both = np.concatenate([gen.reshape(-1, n, H * W), target.reshape(-1, n, H * W)])
    assert np.array_equal(series, qu.key_of(both))
    for which, group in qu.groupings(M, qu.SAMPLES).items():
        for method in qu.METHODS:
            out, valid = qu.host_select(series, H, W, group, qu.QS, method)
            want, count = qu.want(gen, target, which, qu.QS, method)
            assert qu.same_bits(out, want), (which, method)
            assert np.array_equal(valid, count), which
            assert np.isnan(out[:, :, 0, 1]).all() and (valid[:, 0, 1] == 0).all()       # the all-NaN point
            if method != "linear":                                                       # exactly an fp32 value of the input
                ok = ~np.isnan(out)
                assert np.array_equal(out[ok].astype(np.float32).astype(np.float64), out[ok])


def test_fewer_slots_than_capacity_and_a_target_only_series(sdy):
    """n_slots < capacity reads the first slots only; slots that were never written hold the NaN key and count as nothing; a
    series without gen holds the targets at rows 0 .. samples - 1."""
    gen, target = qu.make_data(3, 2, 6, 5, 8)
    series = qu.host_series(gen, target, capacity=9)
    assert (series[:, 6:] == qu.NAN_KEY).all()
    group = qu.groupings(3, 2)["gen"]
    full, _ = qu.host_select(series, 5, 8, group, qu.QS, "linear")
    assert qu.same_bits(full, qu.want(gen, target, "gen", qu.QS, "linear")[0])
    part, count = qu.host_select(series, 5, 8, group, qu.QS, "linear", n_slots=4)
    want, n = qu.want(gen[:, :, :4], target[:, :4], "gen", qu.QS, "linear")
    assert qu.same_bits(part, want) and np.array_equal(count, n)
    alone = qu.host_series(gen, target, store_gen=0)
    assert alone.shape[0] == 2 and np.array_equal(alone, series[6:, :6])
    out, _ = qu.host_select(alone, 5, 8, (0, 1, 1, 0, 2), qu.QS, "higher")
    assert qu.same_bits(out, qu.want(gen, target, "target", qu.QS, "higher")[0])


@pytest.mark.parametrize("n", qu.TIMES)
def test_host_twins_against_numpy_nanquantile(sdy, n):
    """Finite, NaN-free data and dyadic q: equal under == to np.nanquantile on float64 input, all three methods."""
    gen, target = qu.make_data(3, 2, n, 5, 8, plain=True)
    series = qu.host_series(gen, target)
    for which, group in qu.groupings(3, 2).items():
        values = qu.group_values(gen, target, which).astype(np.float64)
        for method in qu.METHODS:
            out, _ = qu.host_select(series, 5, 8, group, qu.DYADIC, method)
            ref = np.nanquantile(values, qu.DYADIC, axis=0, method=method)               # (Q, groups, H, W)
            assert (out == ref.transpose(1, 0, 2, 3)).all(), (which, method)


# ---- the entry points -------------------------------------------------------------------------------------------------------
def _append_call():
    gen, target = qu.make_data(3, 2, 3, 4, 6, plain=True)
    series = np.full((8, 5, 24), 7, np.uint32)
    a, keep = qu.append_args(series, np.ascontiguousarray(target), np.ascontiguousarray(gen), t0=1, slot0=2)
    return a, keep, series


def _set(a, field, value):
    if field == "gen0":
        a.gen[0] = None
    elif field == "target0":
        a.target[0] = None
    elif field == "q0":
        a.q[0] = value
    elif field == "q1":
        a.q[1] = value
    elif isinstance(field, tuple):
        for f, v in zip(field, value):
            setattr(a, f, v)
    elif isinstance(value, str):
        setattr(a, field, getattr(a, field) + int(value))
    else:
        setattr(a, field, value)


@pytest.mark.parametrize("field,value,code", [
    ("struct_size", 0, SDY_ERR_ARG), ("struct_size", "+8", SDY_ERR_ARG), ("struct_size", "-8", SDY_ERR_ARG),
    ("series", None, SDY_ERR_ARG), ("series", "+2", SDY_ERR_ARG), ("gen0", None, SDY_ERR_ARG), ("target0", None, SDY_ERR_ARG),
    ("capacity", 0, SDY_ERR_ARG), ("capacity", 3, SDY_ERR_ARG),                                  # slot0 + (T - t0) = 4 > 3
    ("slot0", 4, SDY_ERR_ARG), ("slot0", -1, SDY_ERR_ARG), ("t0", 4, SDY_ERR_ARG), ("t0", -1, SDY_ERR_ARG),
    ("store_gen", 2, SDY_ERR_ARG), ("store_gen", -1, SDY_ERR_ARG),
    ("gs0", -1, SDY_ERR_ARG), ("gs1", -4, SDY_ERR_ARG), ("ts1", -1, SDY_ERR_ARG),
    ("nvars", 0, SDY_ERR_ARG), ("nvars", 97, SDY_ERR_ARG),
    ("n0", 0, SDY_ERR_ARG), ("n1", -1, SDY_ERR_ARG), ("T", 0, SDY_ERR_ARG), ("H", 0, SDY_ERR_ARG), ("W", 0, SDY_ERR_ARG),
    (("T", "H", "W"), (2, 1 << 15, (1 << 14) + 1), SDY_ERR_UNSUPPORTED),                         # T * H * W > 2^30
    (("n0", "n1"), (1 << 16, 1 << 15), SDY_ERR_UNSUPPORTED),                                     # n0 * n1 >= 2^31
    (("n0", "n1", "H", "W", "capacity", "slot0"), (1 << 10, 1 << 10, 1 << 10, 1 << 10, 1 << 10, 0), SDY_ERR_UNSUPPORTED),  # 2^50
])
def test_append_refuses(sdy, field, value, code):
    a, keep, series = _append_call()
    _set(a, field, value)
    # both entry points check before anything else: the device one is refused without a device
    assert [sdy.lib.sdy_time_quantile_append_host(C.byref(a)), sdy.lib.sdy_time_quantile_append(C.byref(a), None)] == [code] * 2
    assert (series == 7).all()
    assert [sdy.lib.sdy_time_quantile_append_host(None), sdy.lib.sdy_time_quantile_append(None, None)] == [SDY_ERR_ARG] * 2


def test_append_good_call_and_a_window_without_counted_times(sdy):
    a, keep, series = _append_call()
    a.t0 = a.T                                                # SDY_OK from both: the device one launches nothing
    assert [sdy.lib.sdy_time_quantile_append_host(C.byref(a)), sdy.lib.sdy_time_quantile_append(C.byref(a), None)] == [SDY_OK] * 2
    assert (series == 7).all()
    a.t0 = 1
    assert sdy.lib.sdy_time_quantile_append_host(C.byref(a)) == SDY_OK
    # window times 1, 2 at slots 2, 3 of every trajectory; everything else untouched
    assert (series[:, [0, 1, 4]] == 7).all()
    _, _, gen = keep
    assert np.array_equal(series[:6, 2:4], qu.key_of(gen[:, :, 1:].reshape(6, 2, 24)))


def _select_call(nq=2):
    gen, target = qu.make_data(3, 2, 5, 4, 6, plain=True)
    series = qu.host_series(gen, target)
    a, out, valid, keep = qu.select_args(series, 4, 6, qu.groupings(3, 2)["gen"], (0.25, 0.75)[:nq], "linear")
    return a, out, valid, (keep, series)


@pytest.mark.parametrize("field,value,code", [
    ("struct_size", 0, SDY_ERR_ARG), ("struct_size", "+8", SDY_ERR_ARG), ("struct_size", "-8", SDY_ERR_ARG),
    ("series", None, SDY_ERR_ARG), ("out", None, SDY_ERR_ARG), ("valid", None, SDY_ERR_ARG),
    ("series", "+2", SDY_ERR_ARG), ("out", "+4", SDY_ERR_ARG), ("valid", "+2", SDY_ERR_ARG),
    ("plane", 0, SDY_ERR_ARG), ("n_traj", 0, SDY_ERR_ARG), ("capacity", 0, SDY_ERR_ARG), ("n_slots", 0, SDY_ERR_ARG),
    ("n_slots", 6, SDY_ERR_ARG),                                                                  # more slots than the capacity
    ("count", 0, SDY_ERR_ARG), ("n_groups", 0, SDY_ERR_ARG), ("first", -1, SDY_ERR_ARG), ("step", -1, SDY_ERR_ARG),
    ("stride", -1, SDY_ERR_ARG),
    ("first", 3, SDY_ERR_ARG), ("count", 5, SDY_ERR_ARG), ("n_groups", 5, SDY_ERR_ARG), ("n_traj", 5, SDY_ERR_ARG),   # past n_traj
    ("nq", 0, SDY_ERR_ARG), ("nq", 9, SDY_ERR_ARG), ("method", 3, SDY_ERR_ARG), ("method", -1, SDY_ERR_ARG),
    ("q0", -0.001, SDY_ERR_ARG), ("q1", 1.001, SDY_ERR_ARG), ("q0", float("nan"), SDY_ERR_ARG),
    ("plane", (1 << 30) + 1, SDY_ERR_UNSUPPORTED),
    (("count", "stride", "n_groups", "n_traj", "capacity", "n_slots"), (1 << 16, 1, 1, 1 << 16, 1 << 15, 1 << 15),
     SDY_ERR_UNSUPPORTED),                                                                        # count * n_slots = 2^31
    (("n_traj", "capacity", "n_slots", "plane"), (1 << 20, 1 << 20, 5, 1 << 10), SDY_ERR_UNSUPPORTED),   # series indices: 2^50
    (("n_groups", "step", "count", "n_traj", "plane", "nq"), (1 << 18, 0, 1, 8, 1 << 30, 4), SDY_ERR_UNSUPPORTED),  # out: 2^50
])
def test_select_refuses(sdy, field, value, code):
    a, out, valid, keep = _select_call()
    before = keep[1].copy()
    _set(a, field, value)
    assert [sdy.lib.sdy_time_quantile_select_host(C.byref(a)), sdy.lib.sdy_time_quantile_select(C.byref(a), None)] == [code] * 2
    assert (out == -7.0).all() and (valid == -7).all() and np.array_equal(keep[1], before)
    assert [sdy.lib.sdy_time_quantile_select_host(None), sdy.lib.sdy_time_quantile_select(None, None)] == [SDY_ERR_ARG] * 2


def test_select_takes_one_to_eight_quantiles(sdy):
    gen, target = qu.make_data(3, 2, 5, 4, 6)
    series = qu.host_series(gen, target)
    qs = (0.0, 0.1, 0.25, 0.5, 0.75, 0.9, 0.99, 1.0)
    for nq in range(1, 9):
        out, _ = qu.host_select(series, 4, 6, qu.groupings(3, 2)["gen"], qs[:nq], "linear")
        assert qu.same_bits(out, qu.want(gen, target, "gen", qs[:nq], "linear")[0]), nq


def test_structs_carry_their_size_and_are_not_in_the_handshake(sdy):
    from sdy_amd import _lib

    for t in (_lib.SdyTimeQuantileAppendArgs, _lib.SdyTimeQuantileSelectArgs):
        assert t not in _lib.ABI_STRUCTS and t().struct_size == C.sizeof(t) and t._fields_[0][0] == "struct_size"
    assert _lib.SdyTimeQuantileAppendArgs._fields_[1][0] == "win" and _lib.SDY_MAX_QUANTILES == 8
    assert {"sdy_time_quantile_append", "sdy_time_quantile_append_host", "sdy_time_quantile_select",
            "sdy_time_quantile_select_host"} <= set(_lib.SIGNATURES)
    hdr = open(os.path.join(ROOT, "include", "sdy_amd.h")).read()
    assert "#define SDY_MAX_QUANTILES 8\n" in hdr
    assert re.search(r"typedef struct sdy_time_quantile_append_args sdy_time_quantile_append_args;", hdr)
    assert re.search(r"typedef struct sdy_time_quantile_select_args sdy_time_quantile_select_args;", hdr)


# ---- the Python side, as far as it goes without a device ---------------------------------------------------------------------
def _window(M=3, B=2, T=3, H=4, W=6, names=("a", "b")):
    g = torch.Generator().manual_seed(0)
    target = {k: torch.randn(B, T, H, W, generator=g) for k in names}
    gen = {k: torch.randn(M, B, T, H, W, generator=g) for k in names}
    return target, gen


def _record(agg, target, gen, **kw):
    agg.record_batch(loss=0.0, target_data=target, gen_data=gen, target_data_norm=target, gen_data_norm=gen, **kw)


def test_class_refuses_before_the_device(sdy):
    Q = sdy.TimeQuantileAggregator
    assert sdy.quantiles.TimeQuantileAggregator is Q and issubclass(Q, sdy.windows.FieldAccumulator)
    w = torch.ones(4, 6)
    for bad in ((), (1.5,), (-0.1,), (float("nan"),)):
        with pytest.raises(ValueError, match="quantile"):
            Q(bad, w, n_timesteps=4)
    with pytest.raises(ValueError, match="method is one of"):
        Q((0.5,), w, n_timesteps=4, method="nearest")
    with pytest.raises(ValueError, match="n_timesteps must be at least 2"):
        Q((0.5,), w, n_timesteps=1)
    with pytest.raises(ValueError, match="per_member needs store_gen"):
        Q((0.5,), w, n_timesteps=4, store_gen=False, per_member=True)
    with pytest.raises(ValueError, match="target must be"):
        Q((0.5,), w, n_timesteps=4, target="raw")
    agg = Q((0.5, 0.9), w, n_timesteps=4)
    before = {k: (list(v) if isinstance(v, list) else v) for k, v in vars(agg).items()}
    with pytest.raises(RuntimeError, match="GPU only"):
        _record(agg, *_window())
    for read in (agg.get_data, lambda: agg.get_logs("x"), lambda: agg.threshold_map("a", 0.9)):
        with pytest.raises(ValueError, match="No data recorded."):
            read()
    target, gen = _window()
    flat = {k: v.reshape(-1, *v.shape[2:])[:5] for k, v in gen.items()}
    with pytest.raises(ValueError, match="TimeQuantileAggregator needs member-stacked"):
        _record(agg, target, flat)
    with pytest.raises(ValueError, match="member-stacked"):
        _record(agg, target, gen, sample_weights=[0.5, 0.5])
    with pytest.raises(ValueError, match="times 2..4 outside the aggregator's 4"):
        _record(agg, *_window(), i_time_start=2)
    with pytest.raises(ValueError, match="no generated variable 'c'"):
        _record(Q((0.5,), w, n_timesteps=4, variables=["a", "c"]), *_window())
    assert {k: (list(v) if isinstance(v, list) else v) for k, v in vars(agg).items()} == before
    assert agg._names is None and agg.n_times == 0                                       # a refused window changes nothing


def test_class_sizes_its_series(sdy):
    need = 4 * (3 * 2 + 2) * 3 * 4 * 6 * 2                  # 4 bytes x trajectories x counted times x grid x variables
    words = "4 bytes x 8 trajectories .3 members x 2 samples . 2 targets. x 3 counted times x 4 x 6 grid points x 2 variables"
    agg = sdy.TimeQuantileAggregator((0.5,), torch.ones(4, 6), n_timesteps=4, max_bytes=need - 1)
    with pytest.raises(ValueError, match=f"{words} need {need} bytes of sortable 32-bit keys, more than max_bytes = {need - 1}"):
        _record(agg, *_window())
    agg = sdy.TimeQuantileAggregator((0.5,), torch.ones(4, 6), n_timesteps=4, max_bytes=need)
    with pytest.raises(RuntimeError, match="GPU only"):
        _record(agg, *_window())
    # the targets alone, one variable
    need = 4 * 2 * 3 * 4 * 6
    agg = sdy.TimeQuantileAggregator((0.5,), torch.ones(4, 6), n_timesteps=4, variables=["b"], store_gen=False, max_bytes=need - 1)
    with pytest.raises(ValueError, match=f"2 trajectories .2 targets. x 3 counted times x 4 x 6 grid points x 1 variables need {need} bytes"):
        _record(agg, *_window())


def test_inference_aggregator_option(sdy):
    w = torch.ones(4, 6)
    plain = sdy.metrics.InferenceAggregator(w, n_timesteps=3, n_ensemble_members=2)
    assert list(plain._aggregators) == ["mean", "mean_norm", "time_mean"]               # the default set is unchanged
    agg = sdy.metrics.InferenceAggregator(w, n_timesteps=3, n_ensemble_members=2, time_quantiles=(0.5, 0.99),
                                          time_quantile_variables=["a"])
    assert list(agg._aggregators) == ["mean", "mean_norm", "time_mean", "time_quantiles"]
    q = agg._aggregators["time_quantiles"]
    assert isinstance(q, sdy.TimeQuantileAggregator) and q._quantiles == [0.5, 0.99] and q._variables == ["a"]
    assert hasattr(agg, "get_time_quantile_data")
    import inspect

    names = list(inspect.signature(sdy.metrics.InferenceAggregator.__init__).parameters)
    assert names[-2:] == ["time_quantiles", "time_quantile_variables"] and names[-3] == "event_spells"


def test_one_field_function_refuses_before_the_device(sdy):
    with pytest.raises(ValueError, match="expected .time, lat, lon."):
        sdy.quantiles.time_quantiles(torch.zeros(4, 6), 0.5)
    with pytest.raises(ValueError, match="a quantile lies in"):
        sdy.quantiles.time_quantiles(torch.zeros(5, 4, 6), 1.5)
    with pytest.raises(ValueError, match="method is one of"):
        sdy.quantiles.time_quantiles(torch.zeros(5, 4, 6), 0.5, method="median")
    with pytest.raises(RuntimeError, match="GPU only"):
        sdy.quantiles.time_quantiles(torch.zeros(5, 4, 6), 0.5)
