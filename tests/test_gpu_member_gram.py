"""The member Gram on the device (`sdy_member_gram`, csrc/member_gram.hip; `sdy_amd.member_gram`, `FieldScoreAggregator`) against
exact integers (the check of the operand and C/D lane maps of the float64 matrix instruction and of which tile lands where),
exact arithmetic on seeded fp32 data, the library's _host twin and the float64 restatement: the shapes that cross each boundary
of the kernel, layouts, batch independence, determinism, NaN placement, one production plane, the aggregator's bookkeeping next
to `MeanAggregator` and the way through run_inference.  Bounds: tests/member_gram_utils.py.  Every case is a handful of launches."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import member_gram_utils as mg

pytestmark = pytest.mark.gpu


def _cuda(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _transposed(x):
    """(members, samples, ...) as the window driver hands it over: a transposed view of a sample-major buffer."""
    buf = (x if isinstance(x, torch.Tensor) else _cuda(x)).transpose(0, 1).contiguous()
    return buf.transpose(0, 1)


def device_gram(target, gen, w, clim=None):
    """One sdy_member_gram launch over device tensors {name: tensor}, read in place; w (H, W) numpy, clim {name: (H, W) numpy}
    -> (nvars, S, T, N, N) numpy.  Output and workspace start as NaN: what the launch does not write shows."""
    import sdy_amd
    from sdy_amd._lib import SdyMemberGramArgs, check, current_stream, ptr
    from sdy_amd.windows import fill_window, window_layouts

    lay = window_layouts(target, gen)
    assert len({l.extents for l in lay}) == 1
    l = lay[0]
    HW, N = l.H * l.W, l.n0 + 2
    wd = _cuda(np.asarray(w, np.float32).reshape(-1))
    cd = {k: _cuda(np.asarray(v, np.float32).reshape(-1)) for k, v in (clim or {}).items()}
    out = torch.full((len(lay), l.n1, l.T, mg.entries(N)), float("nan"), dtype=torch.float64, device="cuda")
    ws_bytes = sdy_amd.lib.sdy_member_gram_workspace_bytes(len(lay), l.n0, l.n1, l.T, HW)
    assert ws_bytes > 0
    ws = torch.full((ws_bytes // 8,), float("nan"), dtype=torch.float64, device="cuda")
    a = SdyMemberGramArgs()
    fill_window(a.win, lay, 0, len(lay))
    a.HW, a.weights, a.out, a.ws, a.ws_bytes = HW, ptr(wd), ptr(out), ptr(ws), ws_bytes
    for j, k in enumerate(gen):
        a.climatology[j] = ptr(cd.get(k))
    check(sdy_amd.lib.sdy_member_gram(C.byref(a), current_stream()), "sdy_member_gram")
    torch.cuda.synchronize()
    return mg.unpack(out.cpu().numpy(), N)


def one(target, gen, w, clim=None):
    """One field given as numpy arrays -> (S, T, N, N)."""
    return device_gram({"x": _cuda(target)}, {"x": _cuda(gen)}, w, None if clim is None else {"x": clim})[0]


# grid, members (0: a deterministic 4-D gen), samples, times.  (5, 7): the scalar path, below one quarter; (6, 10): N = 16, one
# full block of rows, and N = 17, the first row of a second block; (16, 32): three blocks, and N = 66: five blocks, the LDS bound;
# (40, 72): three chunks, the last one partial
SHAPES = [((5, 7), 0, 2, 2), ((6, 10), 14, 2, 2), ((6, 10), 15, 2, 2), ((16, 32), 31, 1, 2), ((16, 32), 64, 1, 2),
          ((40, 72), 5, 2, 2)]
IDS = [f"{h}x{w}_m{m}" for (h, w), m, _, _ in SHAPES]


@pytest.mark.parametrize("grid,M,S,T", SHAPES, ids=IDS)
def test_exact_integers(grid, M, S, T):
    """Small integers, every member its own non-symmetric pattern: every entry is an integer below 2^53 in any order of the
    sums and must be numpy's int64 result bit for bit -- a wrong lane map or a misplaced tile cannot hide in a rounding."""
    import sdy_amd

    H, W = grid
    target, gen, w, clim = mg.integer_case(M, S, T, H, W, seed=11 + M)
    for c in (clim, None):
        got = one(target, gen, w, c)
        want = mg.gram_int64(target, gen, w, c)
        assert np.abs(want).max() < 2 ** 53 and (w == 0).any()
        assert np.array_equal(got, want.astype(np.float64)), np.argwhere(got != want)[:8]
    if M == 0:
        assert np.array_equal(one(target, gen[None], w, None), got)              # one member, stacked: the same bits
    # the one-field function: the same launch behind the public interface
    pub = sdy_amd.member_gram(_cuda(target), _cuda(gen), _cuda(w), None)
    assert pub.dtype == torch.float64 and pub.is_cuda and tuple(pub.shape) == (S, T, max(M, 1) + 2, max(M, 1) + 2)
    assert np.array_equal(pub.cpu().numpy(), got)


@pytest.mark.parametrize("grid,M,S,T", SHAPES, ids=IDS)
def test_seeded_against_exact_arithmetic_and_the_host_twin(grid, M, S, T):
    import sdy_amd

    H, W = grid
    if M == 64:
        S, T = 1, 1                                                               # (the exact sums are Python integers)
    target, gen, w, clim = mg.seeded_case(M, S, T, H, W, seed=300 + H + M)
    got = one(target, gen, w, clim)
    G, A = mg.gram_exact(target, gen, w, clim)
    worst = mg.check_against_exact(got, G, A, H * W, scale=mg.EXACT_SCALE, what=f"{H}x{W} M={M} device")
    print(f"{H}x{W} M={M}: worst device error {worst:.3f} x 2^-53 sum w |a_i a_j| (bound {H * W + 4})")
    host = mg.host_gram(sdy_amd, target, gen, w, clim)
    mg.check_two_computed(got, host, A, H * W, scale=mg.EXACT_SCALE, what=f"{H}x{W} M={M} device vs host twin")


def test_same_bits_in_any_layout_batch_grouping_and_run():
    H, W, M, S, T = 40, 72, 5, 3, 2
    ta, ga, w, clim = mg.seeded_case(M, S, T, H, W, seed=21)
    tb, gb, _, _ = mg.seeded_case(M, S, T, H, W, seed=22)
    t, g = {"a": _cuda(ta), "b": _cuda(tb)}, {"a": _cuda(ga), "b": _cuda(gb)}
    cl = {"b": clim}
    base = device_gram(t, g, w, cl)
    assert np.isfinite(base).all()
    assert np.array_equal(device_gram(t, g, w, cl), base)                                           # two runs
    gt = {k: _transposed(v) for k, v in g.items()}
    assert not gt["a"].is_contiguous()
    assert np.array_equal(device_gram(t, gt, w, cl), base)                                          # the window driver's view
    for j, k in enumerate(g):                                                                       # one launch per variable
        assert np.array_equal(device_gram({k: t[k]}, {k: g[k]}, w, cl)[0], base[j])
    alone = device_gram({k: v[1:2] for k, v in t.items()}, {k: v[:, 1:2] for k, v in g.items()}, w, cl)
    assert np.array_equal(alone[:, 0], base[:, 1])                                                  # a sample alone
    # the scalar path (a view 4 bytes off a 16-byte boundary) adds the same terms in the same order
    off = {}
    for k, v in g.items():
        buf = torch.zeros(v.numel() + 1, device="cuda")
        buf[1:] = v.reshape(-1)
        off[k] = buf[1:].view(v.shape)
        assert off[k].data_ptr() % 16 == 4
    assert np.array_equal(device_gram(t, off, w, cl), base)
    # a climatology of zeros against none
    assert np.array_equal(device_gram(t, g, w, {"a": np.zeros((H, W), np.float32), "b": clim}), base)


def test_nan_and_the_zero_weight_rule_on_the_device():
    M, S, T, H, W = 17, 2, 2, 40, 72                  # two blocks of rows, three chunks
    target, gen, w, clim = mg.seeded_case(M, S, T, H, W, seed=31)
    zero, live = np.argwhere(w == 0), np.argwhere(w != 0)
    base = one(target, gen, w, clim)
    g2, t2, c2 = gen.copy(), target.copy(), clim.copy()
    g2[:, :, :, zero[:, 0], zero[:, 1]] = np.nan                                  # every point without weight, every member
    g2[3, 1, 0, zero[0][0], zero[0][1]] = np.inf
    t2[:, :, zero[1::2, 0], zero[1::2, 1]] = np.inf
    c2[zero[::2, 0], zero[::2, 1]] = np.nan
    assert np.array_equal(one(t2, g2, w, c2), base)
    for m, s, t, at in ((0, 0, 1, live[0]), (15, 1, 0, live[len(live) // 2]), (16, 1, 1, live[-1])):
        g3 = gen.copy()
        g3[m, s, t, at[0], at[1]] = np.nan
        got = one(target, g3, w, clim)
        poisoned = np.zeros(got.shape, bool)
        poisoned[s, t, 1 + m, :] = poisoned[s, t, :, 1 + m] = True
        assert np.array_equal(np.isnan(got), poisoned), (m, s, t)
        assert np.array_equal(got[~poisoned], base[~poisoned])


def test_production_plane():
    import sdy_amd

    H, W, M = 180, 360, 3
    target, gen, _, clim = mg.seeded_case(M, 1, 2, H, W, seed=41)
    lats = -90.0 + (np.arange(H) + 0.5)
    w = sdy_amd.metrics.spherical_area_weights(torch.from_numpy(lats), W).numpy().astype(np.float32)
    got = one(target, gen, w, clim)
    want, abs_sums = mg.gram_float64(target, gen, w, clim)
    bound = (H * W + 4) * 2.0 ** -53 * abs_sums
    assert (np.abs(got - want) <= bound).all(), (np.abs(got - want) / abs_sums).max()
    print(f"180x360: worst |device - float64 restatement| {(np.abs(got - want) / abs_sums).max() / 2.0 ** -53:.2f} x 2^-53 "
          f"sum w |a_i a_j| (bound {H * W + 4})")


def _restated_series(windows, names, w, clim, n_timesteps, M, ens):
    """What FieldScoreAggregator must hold: `scores` of the float64 restatement of every window's Gram, the mean over the
    samples added at the window's times and divided by the windows that touched a time."""
    from sdy_amd.field_scores import scores

    total, count = {}, np.zeros(n_timesteps)
    for start, target, gen in windows:
        T = target[names[0]].shape[1]
        count[start:start + T] += 1
        for k in names:
            c = clim.get(k)
            sc = scores(torch.from_numpy(mg.gram_float64(target[k], gen[k], w, c)[0]), M, climatology=c is not None)
            for key, v in sc.items():
                if not ens and (key in ("member_distance", "distance_ratio") or key.endswith("_member_avg")):
                    continue
                total.setdefault(f"{key}/{k}", np.zeros(n_timesteps))[start:start + T] += v.numpy().mean(axis=0)
    return {k: v / count for k, v in total.items()}


@pytest.mark.parametrize("ens", [True, False], ids=["ens", "det"])
def test_aggregator_over_three_windows(ens):
    """FieldScoreAggregator with i_time_start; `ensemble_mean_rmse` against MeanAggregator's `weighted_rmse` on the same windows
    (rtol 1e-6: the fp32 and the float64 per-point chains differ, both sum in float64), everything against `scores` of the
    restated Gram (1e-12: the distances of independent members cancel by no more than a factor of 4)."""
    import sdy_amd

    H, W, S, T, M, n_t, names = 6, 10, 2, 2, (4 if ens else 0), 5, ["a", "b"]
    windows = []
    for i, start in enumerate((0, 2, 3)):
        target, gen = {}, {}
        for j, k in enumerate(names):
            target[k], gen[k], w, c = mg.seeded_case(M, S, T, H, W, seed=50 + 10 * i + j)
            if start == 0:                                                       # the initial condition: members == truth
                gen[k][..., 0, :, :] = target[k][:, 0]
        windows.append((start, target, gen))
    w = np.abs(w) + 0.01                                                         # (MeanAggregator has no zero-weight rule)
    clim = {"a": c}
    agg = sdy_amd.FieldScoreAggregator(torch.from_numpy(w), n_timesteps=n_t, is_ensemble=ens,
                                       climatology={"a": torch.from_numpy(c)})
    glob = sdy_amd.metrics.MeanAggregator(_cuda(w), n_timesteps=n_t, is_ensemble=ens)
    with pytest.raises(ValueError, match="outside"):                             # a refused first window changes nothing
        agg.record_batch(0.0, *[{k: _cuda(v) for k, v in d.items()} for d in windows[0][1:]], None, None, i_time_start=4)
    assert agg._total is None and agg._names is None
    for i, (start, target, gen) in enumerate(windows):
        t, g = {k: _cuda(v) for k, v in target.items()}, {k: _cuda(v) for k, v in gen.items()}
        if ens and i == 1:
            g = {k: _transposed(v) for k, v in g.items()}
        agg.record_batch(0.0, t, g, None, None, i_time_start=start)
        glob.record_batch(0.0, t, g, t, g, i_time_start=start)
    series = agg.get_series()
    got = {k: v.cpu().numpy() for k, v in series.items()}
    assert all(v.is_cuda and v.dtype == torch.float64 and tuple(v.shape) == (n_t,) for v in series.values())
    want = _restated_series(windows, names, w, clim, n_t, max(M, 1), ens)
    assert set(got) == set(want), sorted(set(got) ^ set(want))
    assert ("anomaly_correlation/a" in got) and ("pattern_correlation/b" in got) and ("member_distance/a" in got) == ens
    for k in got:
        assert np.array_equal(np.isnan(got[k]), np.isnan(want[k])), (k, got[k], want[k])
        assert np.allclose(got[k], want[k], rtol=1e-12, atol=1e-12, equal_nan=True), (k, got[k] - want[k])
    # time 0 is the initial condition, counted like any time: distances exactly 0, the ratio 0 / 0
    for k in names:
        assert got[f"error_distance/{k}"][0] == 0.0 and got[f"energy_score/{k}"][0] == 0.0
        assert got[f"ensemble_mean_rmse/{k}"][0] == 0.0 and (got[f"error_distance/{k}"][1:] > 0).all()
        if ens:
            assert got[f"member_distance/{k}"][0] == 0.0 and np.isnan(got[f"distance_ratio/{k}"][0])
            assert np.isfinite(got[f"distance_ratio/{k}"][1:]).all()
    for k, v in glob.get_series().items():
        metric, var = k.split("/")
        if metric == "weighted_rmse":
            np.testing.assert_allclose(got[f"ensemble_mean_rmse/{var}"], v.cpu().numpy(), rtol=1e-6, atol=0.0, err_msg=k)
    logs = agg.get_logs("field_scores")
    assert list(logs) == ["field_scores/series"] and list(logs["field_scores/series"]) == list(series)
    assert all(np.array_equal(logs["field_scores/series"][k], got[k], equal_nan=True) for k in got)
    # a second window at the same times (3 and 4): time 4 is the mean of two equal windows, time 3 now of three windows
    start, target, gen = windows[2]
    t, g = {k: _cuda(v) for k, v in target.items()}, {k: _cuda(v) for k, v in gen.items()}
    agg.record_batch(0.0, t, g, None, None, i_time_start=start)
    again = {k: v.cpu().numpy() for k, v in agg.get_series().items()}
    want = _restated_series(windows + [windows[2]], names, w, clim, n_t, max(M, 1), ens)
    for k in got:
        keep = [0, 1, 2, 4]
        assert np.allclose(again[k][keep], got[k][keep], rtol=1e-14, atol=0.0, equal_nan=True), k
        assert np.allclose(again[k], want[k], rtol=1e-12, atol=1e-12, equal_nan=True) and again[k][3] != got[k][3], k
    # refused windows change nothing: other variables, another sample count, flat rows for an ensemble
    with pytest.raises(ValueError, match="variables"):
        agg.record_batch(0.0, {"a": t["a"]}, {"a": g["a"]}, None, None, i_time_start=start)
    with pytest.raises(ValueError, match="sample count"):
        agg.record_batch(0.0, {k: v[:1] for k, v in t.items()}, {k: v[..., :1, :, :, :] for k, v in g.items()}, None, None,
                         i_time_start=start)
    with pytest.raises(ValueError):
        agg.record_batch(0.0, t, {k: (v.flatten(0, 1) if ens else v[None]) for k, v in g.items()}, None, None,
                         i_time_start=start)
    after = {k: v.cpu().numpy() for k, v in agg.get_series().items()}
    assert all(np.array_equal(after[k], again[k], equal_nan=True) for k in got)


def test_through_run_inference():
    """run_inference on the tiny loop fixture (2 windows x 6 steps, 2 samples, 3 members) with
    InferenceAggregator(field_scores=True): exactly <label>/field_scores/series joins the parent's keys, its columns are
    get_field_scores(), and without the keyword the key set is the parent's."""
    import sdy_amd
    from test_gpu_derived import _loop_setup

    _, stepper, windows, sigma, n_total, n_mem, names = _loop_setup(3)
    w = sdy_amd.metrics.spherical_area_weights(torch.linspace(-87.0, 87.0, 32), 64)
    out = names["out_names"]
    clim = {out[0]: torch.zeros(32, 64)}
    logs, agg = {}, None
    for on in (False, True):
        agg = sdy_amd.metrics.InferenceAggregator(w.cuda(), n_timesteps=n_total + 1, n_ensemble_members=3,
                                                  **(dict(field_scores=True, climatology=clim) if on else {}))
        sdy_amd.run_inference(agg, stepper, types.SimpleNamespace(loader=windows), n_total, n_mem, 3)
        logs[on] = agg.get_logs("inference")
    assert set(logs[True]) - set(logs[False]) == {"inference/field_scores/series"} and set(logs[False]) <= set(logs[True])
    parent = {"inference/mean/series", "inference/mean_norm/series"}
    assert parent <= set(logs[False]) and not any("field_scores" in k for k in logs[False])
    series = agg.get_field_scores()
    metrics = ["error_distance", "energy_score", "ensemble_mean_rmse", "member_distance", "distance_ratio"]
    want_keys = sorted([f"{m}/{v}" for m in metrics for v in out]
                       + [f"{'anomaly' if v == out[0] else 'pattern'}_correlation{sfx}/{v}" for v in out
                          for sfx in ("", "_member_avg")])
    assert sorted(series) == want_keys
    table = logs[True]["inference/field_scores/series"]
    assert table.columns == ["forecast_step"] + want_keys and len(table.data) == n_total + 1
    got = {k: v.cpu().numpy() for k, v in series.items()}
    for j, k in enumerate(want_keys):
        assert np.array_equal(np.asarray([row[1 + j] for row in table.data], np.float64), got[k], equal_nan=True)
    # time 0 is the initial condition all members start from: no distance between them; later they have left the truth
    for v in out:
        assert got[f"member_distance/{v}"][0] == 0.0 and (got[f"error_distance/{v}"][1:] > 0).all()
