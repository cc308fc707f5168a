"""Shared by tests/test_spells_host.py and tests/test_gpu_spells.py: the cases (seeded AR(1) series, so that spells exist,
and one hand-made series), the numpy restatement of the spell state and the duration histograms -- a plain time loop over
boolean arrays, written from the definition (include/sdy_amd.h, sdy_event_spell_args), not from csrc/spells.h -- the
library's _host entry point driven from numpy, and the float64 restatement of `EventSpellAggregator.get_data` / `get_logs`.

States and counts are integers: compared with np.array_equal, never a tolerance.  A log is a quotient of two weighted sums of
H non-negative terms w_lat x integer (and, for the rates, the exact integer n).  Each weighted sum, in any order of its
additions and with the roundings of its products, of the division and of the multiplication by n, is within (H + 8) 2^-53 of
the sum of the absolute values of its terms -- which is the sum itself, the terms being non-negative.  So a log is held to
the relative bound TOL(H) = 2 (H + 8) 2^-53, one (H + 8) 2^-53 for each of its two weighted sums; `longest_bias` (a difference
of two such quotients) to the sum of its two parts' absolute bounds, `mean_duration_ratio` (a quotient of two) to the sum of
the two relative bounds; each of the two with one more rounding of its own.
"""
import ctypes as C

import numpy as np

from event_verif_utils import fill_thresholds
from window_utils import fill_window, vp

SMALL = ("m5_b2_6x8", "m5_b2_6x10", "m25_b1_4x360", "m1_b2_6x8", "nan_m5_b2_6x8", "e8_m5_b1_6x8", "known_m5_b2_6x8")
LOG_METRICS = ("mean_duration_gen", "mean_duration_target", "mean_duration_ratio", "longest_gen", "longest_target",
               "longest_bias", "onset_rate_gen", "onset_rate_target", "time_fraction_gen", "time_fraction_target")
POINT_OUTPUTS = ("longest", "spells", "hits")
EDGES = 2 ** np.arange(15, dtype=np.int64)            # 1, 2, 4, .., 16384
CUTS = ((0, 6), (6, 12), (12, 18), (18, 24))          # 23 counted times: 1 + 5, 6, 6, 6 (time 0 is the initial condition)
N_TIMES = 24


def duration_bin(d):
    """The number of edges 1, 2, 4, .., 16384 that are < d (at most 15, there being 15 edges)."""
    return np.searchsorted(EDGES, np.asarray(d, np.int64), side="left")


def ar1(rng, shape_before_time, n_times, H, W):
    """fp32 series x_t = 0.8 x_{t-1} + 0.6 eps along the time axis, stationary from the first time on: (..., time, H, W)."""
    lead = tuple(shape_before_time)
    x = np.empty(lead + (n_times, H, W), np.float32)
    x[..., 0, :, :] = rng.standard_normal(lead + (H, W)).astype(np.float32)
    for t in range(1, n_times):
        eps = rng.standard_normal(lead + (H, W)).astype(np.float32)
        x[..., t, :, :] = np.float32(0.8) * x[..., t - 1, :, :] + np.float32(0.6) * eps
    return x


def _weights(H, W):
    lat = (np.arange(H) + 0.5) / H * np.pi - np.pi / 2
    return np.repeat(np.cos(lat).astype(np.float32)[:, None], W, axis=1)


def _cut(target, gen, cuts):
    return [(a, {k: np.ascontiguousarray(v[:, a:b]) for k, v in target.items()},
             {k: np.ascontiguousarray(v[..., a:b, :, :]) for k, v in gen.items()}) for a, b in cuts]


def make_case(M, B, H, W, seed, names=("a", "b"), four_d=False, n_times=N_TIMES, cuts=CUTS):
    rng = np.random.default_rng(seed)
    target = {k: ar1(rng, (B,), n_times, H, W) for k in names}
    gen = {k: ar1(rng, (B,) if four_d else (M, B), n_times, H, W) for k in names}
    return dict(M=M, B=B, H=H, W=W, names=list(names), weights=_weights(H, W), n_timesteps=n_times, series=(target, gen),
                cuts=tuple(cuts), windows=_cut(target, gen, cuts))


def recut(case, cuts):
    """The windows of the case's run under another cut."""
    return _cut(*case["series"], cuts)


def _map(rng, H, W, centre, nan_at=()):
    m = (centre + 0.2 * rng.standard_normal((H, W))).astype(np.float32)
    for p in nan_at:
        m[p] = np.nan
    return m


def cases():
    """The small cases of the issue's table, by name."""
    out = {}
    rng = np.random.default_rng(100)
    base = make_case(5, 2, 6, 8, seed=7, names=("a", "b", "c"))                # two runs: 3 events, 1 event; c has none
    base["events"] = {"a": [("wet", "above", 0.3), ("dry", "below", -0.3), ("anomaly", "above", _map(rng, 6, 8, 0.2))],
                      "b": [("wet", "above", 0.3)]}
    out["m5_b2_6x8"] = base
    base = make_case(5, 2, 6, 10, seed=8)                                      # W % 4 != 0: the scalar path
    base["events"] = {k: [("wet", "above", 0.3), ("cool", "below", _map(rng, 6, 10, -0.2))] for k in base["names"]}
    out["m5_b2_6x10"] = base
    base = make_case(25, 1, 4, 360, seed=9)                                    # the headline row: 26 x 90 items of 256 lanes
    base["events"] = {k: [("wet", "above", 0.3), ("dry", "below", -0.3), ("very_wet", "above", 1.0),
                          ("anomaly", "above", _map(rng, 4, 360, 0.0))] for k in base["names"]}
    out["m25_b1_4x360"] = base
    base = make_case(1, 2, 6, 8, seed=10, four_d=True)                         # a 4-D gen
    base["events"] = {k: [("wet", "above", 0.3), ("dry", "below", -0.3)] for k in base["names"]}
    out["m1_b2_6x8"] = base
    base = make_case(5, 2, 6, 8, seed=11)
    for k in base["names"]:
        target, gen = base["series"]
        gen[k][1, 0, 3:5, 2, 3] = np.nan                                       # a NaN member: inside a window ...
        gen[k][4, 1, 11:13, 0, 0] = np.nan                                     # ... and across a window boundary
        gen[k][rng.random(gen[k].shape) < 0.02] = np.nan
        target[k][0, 5:7, 1, 1] = np.nan
        target[k][rng.random(target[k].shape) < 0.02] = np.nan
    base["windows"] = recut(base, CUTS)
    base["events"] = {k: [("anomaly", "above", _map(rng, 6, 8, 0.2, nan_at=((0, 2), (3, 5)))), ("dry", "below", -0.3)]
                      for k in base["names"]}
    out["nan_m5_b2_6x8"] = base
    base = make_case(5, 1, 6, 8, seed=12)                                      # 8 events: above and below, scalars and maps
    base["events"] = {k: [("wet", "above", 0.3), ("dry", "below", -0.3), ("map_hi", "above", _map(rng, 6, 8, 0.5)),
                          ("map_lo", "below", _map(rng, 6, 8, -0.5)), ("positive", "above", 0.0), ("negative", "below", 0.0),
                          ("very_wet", "above", 1.0), ("map_mid", "below", _map(rng, 6, 8, 0.1, nan_at=((5, 7),)))]
                      for k in base["names"]}
    out["e8_m5_b1_6x8"] = base
    out["known_m5_b2_6x8"] = known_case()
    assert list(out) == list(SMALL)
    _check_not_vacuous(out["m5_b2_6x8"])
    return out


def known_case():
    """Every generated trajectory: in the event at the initial condition (not counted) and at the counted times 1 .. 20 (ONE
    spell of 20 times, across every window boundary), outside at 21, inside at 22 and 23 (open at the end).  Every target: in
    at 2, at 4 .. 6 and at 23 (open).  The event: above 0.5; the values are 1 (in) and 0 (out)."""
    M, B, H, W = 5, 2, 6, 8
    g_in = np.zeros(N_TIMES, np.float32)
    g_in[0:21] = 1.0
    g_in[22:24] = 1.0
    t_in = np.zeros(N_TIMES, np.float32)
    t_in[[2, 4, 5, 6, 23]] = 1.0
    target = {k: np.broadcast_to(t_in[None, :, None, None], (B, N_TIMES, H, W)).copy() for k in ("a", "b")}
    gen = {k: np.broadcast_to(g_in[None, None, :, None, None], (M, B, N_TIMES, H, W)).copy() for k in ("a", "b")}
    return dict(M=M, B=B, H=H, W=W, names=["a", "b"], weights=_weights(H, W), n_timesteps=N_TIMES, series=(target, gen),
                cuts=CUTS, windows=_cut(target, gen, CUTS), events={k: [("on", "above", 0.5)] for k in ("a", "b")})


def production_case():
    """180 x 360, 25 members, 2 variables, 2 events (a scalar and a map with NaN points), 3 windows (2 + 3 + 3 counted times)."""
    cuts = ((0, 3), (3, 6), (6, 9))
    case = make_case(25, 1, 180, 360, seed=13, n_times=9, cuts=cuts)
    rng = np.random.default_rng(14)
    case["events"] = {k: [("wet", "above", 0.3), ("cool", "below", _map(rng, 180, 360, -0.2, nan_at=((0, 0), (90, 181), (179, 359))))]
                      for k in case["names"]}
    return case


def event_names(case):
    """The variables with events, in window order."""
    return [k for k in case["names"] if k in case["events"]]


def make_events(case):
    import sdy_amd

    ev = sdy_amd.Events()
    for k in event_names(case):
        for name, direction, thr in case["events"][k]:
            ev.add(k, name, **{direction: thr})
    return ev


def _in(x, direction, c):
    with np.errstate(invalid="ignore"):
        return x < c if direction == "below" else x > c


def _rows(gen, target):
    """-> (rows, time, H, W): the generated trajectories (member-major), then the targets."""
    g = gen if gen.ndim == 5 else gen[None]
    return np.concatenate([g.reshape((-1,) + g.shape[2:]), target], axis=0)


def counted_times(windows):
    return sum(t[next(iter(t))].shape[1] - (1 if start == 0 else 0) for start, t, _ in windows)


def restate(case, windows=None):
    """-> ({var: state (E, 4, rows, H, W) uint32}, {var: closed durations (E, 2, H, 16) float64}): the definition as a time
    loop over boolean arrays."""
    windows = case["windows"] if windows is None else windows
    M, B, H = case["M"], case["B"], case["H"]
    states, closed = {}, {}
    for name in event_names(case):
        x = np.concatenate([_rows(g[name], t[name])[:, (1 if start == 0 else 0):] for start, t, g in windows], axis=1)
        E = len(case["events"][name])
        states[name] = np.zeros((E, 4) + x.shape[:1] + x.shape[2:], np.uint32)
        closed[name] = np.zeros((E, 2, H, 16))
        for e, (_, direction, thr) in enumerate(case["events"][name]):
            inside = _in(x, direction, np.float32(thr) if not isinstance(thr, np.ndarray) else thr)
            run = np.zeros(inside.shape[:1] + inside.shape[2:], np.int64)
            longest, spells, hits = run.copy(), run.copy(), run.copy()
            for t in range(inside.shape[1]):
                now = inside[:, t]
                ended = np.where(~now & (run > 0), run, 0)
                for side, rows in enumerate((slice(0, M * B), slice(M * B, None))):
                    d = ended[rows]
                    lat = np.broadcast_to(np.arange(H)[None, :, None], d.shape)[d > 0]
                    np.add.at(closed[name][e, side], (lat, duration_bin(d[d > 0])), 1.0)
                spells += now & (run == 0)
                run = np.where(now, run + 1, 0)
                hits += now
                longest = np.maximum(longest, run)
            states[name][e] = np.stack([run, longest, spells, hits]).astype(np.uint32)
    return states, closed


def _runs(case):
    """Consecutive variables with events and equal event count: what one call takes."""
    names = event_names(case)
    first = 0
    while first < len(names):
        last = first + 1
        while last < len(names) and len(case["events"][names[last]]) == len(case["events"][names[first]]):
            last += 1
        yield names[first:last]
        first = last


def args(case, target, gen, names, t0, state, durations):
    """SdyEventSpellArgs over contiguous numpy arrays for the variables `names` (equal event count); -> (args, keep-alive)."""
    from sdy_amd._lib import SdyEventSpellArgs

    a = SdyEventSpellArgs()
    keep, (H, W) = fill_window(a.win, target, gen, names)
    a.H, a.W, a.t0, a.state, a.durations = H, W, t0, vp(state), vp(durations)
    return a, keep + fill_thresholds(a.thr, case, names) + [state, durations]


def host(case, windows=None):
    """The case through sdy_event_spell_accumulate_host, window by window -> (states, closed), shaped as `restate` gives them."""
    import sdy_amd

    M, B, H, W = case["M"], case["B"], case["H"], case["W"]
    states, closed = {}, {}
    for names in _runs(case):
        E = len(case["events"][names[0]])
        state = np.zeros((len(names), E, 4, (M + 1) * B, H, W), np.uint32)
        durations = np.zeros((len(names), E, 2, H, 16))
        for start, target, gen in (case["windows"] if windows is None else windows):
            a, keep = args(case, target, gen, names, 1 if start == 0 else 0, state, durations)
            assert sdy_amd.lib.sdy_event_spell_accumulate_host(C.byref(a)) == 0
        for j, k in enumerate(names):
            states[k], closed[k] = state[j], durations[j]
    return states, closed


def same(got, want):
    return list(got) == list(want) and all(got[k].shape == want[k].shape and got[k].dtype == want[k].dtype and
                                           np.array_equal(got[k], want[k]) for k in want)


def lat_weights(case):
    return case["weights"].astype(np.float64).mean(axis=1)


def readout(case, states, closed):
    """What `EventSpellAggregator.get_data()` returns, restated in numpy from a state and the closed durations: {key: float64
    array} in its key order."""
    M, B, H, W = case["M"], case["B"], case["H"], case["W"]
    data = {}
    for k in event_names(case):
        for e, (name, _, thr) in enumerate(case["events"][k]):
            tail = f"{name}/{k}"
            counted = ~np.isnan(thr) if isinstance(thr, np.ndarray) else np.ones((H, W), bool)
            st = states[k][e].astype(np.int64)
            rows, durations = np.zeros((2, H, 4)), closed[k][e].copy()
            for side, r in enumerate((slice(0, M * B), slice(M * B, None))):
                run, longest, spells, hits = (st[w, r] * counted for w in range(4))
                rows[side] = np.stack([hits.sum(axis=(0, 2)), spells.sum(axis=(0, 2)), longest.sum(axis=(0, 2)),
                                       counted.sum(axis=1) * run.shape[0]], axis=1)
                lat = np.broadcast_to(np.arange(H)[None, :, None], run.shape)[run > 0]
                np.add.at(durations[side], (lat, duration_bin(run[run > 0])), 1.0)
            for w, word in ((1, "longest"), (2, "spells"), (3, "hits")):
                x = np.where(counted, st[w].astype(np.float64), np.nan)
                data[f"gen_{word}/{tail}"] = x[:M * B].reshape(M, B, H, W)
                data[f"target_{word}/{tail}"] = x[M * B:]
            data[f"durations_gen/{tail}"], data[f"durations_target/{tail}"] = durations[0], durations[1]
            data[f"duration_edges/{tail}"] = EDGES.astype(np.float64)
            data[f"rows/{tail}"] = rows
    return data


def restate_logs_of_rows(rows, w, n):
    """One (variable, event)'s logs from rows (2, lat, 4) = hits, spells, longest, points -> ({metric: value}, {metric:
    absolute bound}), from the definitions; the bounds as the module docstring derives them."""
    H = len(w)
    rel = 2.0 * (H + 8) * 2.0 ** -53
    nan = float("nan")
    out, bound = {}, {}
    for side, which in enumerate(("gen", "target")):
        hits, spells, longest, points = (float((w * rows[side, :, j]).sum()) for j in range(4))
        out[f"mean_duration_{which}"] = hits / spells if spells > 0 else nan
        out[f"longest_{which}"] = longest / points if points > 0 else nan
        out[f"onset_rate_{which}"] = spells / (n * points) if points > 0 else nan
        out[f"time_fraction_{which}"] = hits / (n * points) if points > 0 else nan
    for key, v in out.items():
        bound[key] = rel * abs(v)
    g, t = out["mean_duration_gen"], out["mean_duration_target"]
    out["mean_duration_ratio"] = g / t if t == t else nan
    bound["mean_duration_ratio"] = 2.0 * rel * abs(out["mean_duration_ratio"]) + 2.0 ** -52 * abs(out["mean_duration_ratio"])
    out["longest_bias"] = out["longest_gen"] - out["longest_target"]
    bound["longest_bias"] = bound["longest_gen"] + bound["longest_target"] + 2.0 ** -52 * abs(out["longest_bias"])
    return {m: out[m] for m in LOG_METRICS}, bound


def restate_logs(case, data, n, label=""):
    """EventSpellAggregator.get_logs(label) in float64 numpy from the restated `rows` -> (logs, bounds)."""
    w, logs, bounds = lat_weights(case), {}, {}
    for k in event_names(case):
        for name, _, _ in case["events"][k]:
            one, bound = restate_logs_of_rows(data[f"rows/{name}/{k}"], w, n)
            for metric in LOG_METRICS:
                key = f"{label}/{metric}/{name}/{k}" if label else f"{metric}/{name}/{k}"
                logs[key], bounds[key] = one[metric], bound[metric]
    return logs, bounds


def close_logs(got, want, bounds, what):
    assert list(got) == list(want), what
    for key, v in want.items():
        g = got[key]
        assert isinstance(g, float), (what, key)
        if np.isnan(v):
            assert np.isnan(g), (what, key, g)
        else:
            print(f"{what} {key}: got {g!r} want {v!r} off {abs(g - v):.3e} bound {bounds[key]:.3e}")
            assert abs(g - v) <= bounds[key], (what, key, g, v, bounds[key])


def _check_not_vacuous(case):
    """m5_b2_6x8, event `wet` of `a`: at least five duration bins are non-empty among the closed spells, some spells are open
    at the end, and at every window boundary some trajectory is in the event on both sides."""
    states, closed = restate(case)
    assert (closed["a"][0].sum(axis=(0, 1)) > 0).sum() >= 5, closed["a"][0].sum(axis=(0, 1))
    assert (states["a"][0, 0] > 0).sum() > 0
    target, gen = case["series"]
    x = _rows(gen["a"], target["a"])
    inside = _in(x, "above", np.float32(0.3))
    for a, _ in case["cuts"][1:]:
        assert (inside[:, a - 1] & inside[:, a]).sum() > 0, a
