"""Shared by tests/test_event_verif_host.py and tests/test_gpu_event_verif.py: cases from seeded numpy (the fields of
tests/rank_hist_utils.py with events on top), the numpy restatement of the event table and the frequency maps
(include/sdy_amd.h, sdy_event_args), the library's _host entry points driven from numpy, and the float64 restatement of
`sdy_amd.events.scores` and of `EventVerificationAggregator.get_logs`.

Tables and maps are integers: compared with np.array_equal, never a tolerance.  The scores are sums of at most 2 (M + 1) H
positive float64 terms and a few divisions: |got - want| <= TOL x scale with scale 1 for everything in [0, 1] and 1 /
uncertainty for the skill score; TOL = 1e-11 is about four times the worst-case bound 2 (M + 1) H x 2^-53 at M = 64, H = 180.
"""
import ctypes as C

import numpy as np

import rank_hist_utils as ru
from window_utils import fill_slots, fill_window, vp

TOL = 1e-11

SMALL = ("m5_b2_6x8", "m2_b3_7x10", "m9_b1_4x36", "m25_b1_4x360", "m64_b1_4x8_e8", "m1_b2_6x8", "known_m5_b2_6x8",
         "clipped_m5_b2_6x8", "nan_m5_b2_6x8")
DEGENERATE = ("known_m5_b2_6x8", "clipped_m5_b2_6x8")
LOG_METRICS = ("brier_score", "brier_skill_score", "brier_reliability", "brier_resolution", "base_rate", "forecast_rate",
               "roc_area")
SLOT_METRICS = ("brier_score", "brier_reliability", "brier_resolution", "uncertainty", "base_rate", "forecast_rate", "roc_area")


def _climate(case, name):
    """(H, W) float32: the target's mean over samples and times, the case's climate as a threshold map can know it."""
    y = np.concatenate([t[name] for _, t, _ in case["windows"]], axis=1)
    return np.nanmean(y.astype(np.float64), axis=(0, 1)).astype(np.float32)


def _with_events(case, events):
    """events: {variable: [(name, "above" | "below", float | (H, W) float32)]}; a variable of the case without events stays in
    the windows and is ignored."""
    case = dict(case)
    case["events"] = events
    _check_base_rates(case)
    return case


def _normal_events(case, name, n):
    """n events of a variable of a "normal" field (climate 280 +- 20, weather +- 3), thresholds near the climate: scalars and
    maps, above and below, in a fixed rotation."""
    clim = _climate(case, name)
    menu = [("warm", "above", 285.0), ("cold", "below", 270.0), ("anomaly", "above", clim + np.float32(1.0)),
            ("cool_anomaly", "below", clim - np.float32(2.0)), ("hot", "above", 300.0), ("mild", "below", 290.0),
            ("strong_anomaly", "above", clim + np.float32(3.0)), ("not_cold", "above", 262.5)]
    return menu[:n]


def cases():
    """The small cases of the issue's table, by name."""
    out = {}
    base = ru.make_case(5, 2, 6, 8, seed=1, names=("a", "b", "c"))
    out["m5_b2_6x8"] = _with_events(base, {"a": _normal_events(base, "a", 3), "b": _normal_events(base, "b", 1)})
    base = ru.make_case(2, 3, 7, 10, seed=2)                          # W % 4 != 0: the scalar path; odd H
    out["m2_b3_7x10"] = _with_events(base, {k: _normal_events(base, k, 2)[::-1] for k in base["names"]})
    base = ru.make_case(9, 1, 4, 36, seed=3)                          # one past a batch of 8 members; 9 units: idle lanes
    out["m9_b1_4x36"] = _with_events(base, {"a": _normal_events(base, "a", 1), "b": _normal_events(base, "b", 3)[2:]})
    base = ru.make_case(25, 1, 4, 360, seed=4)                        # the headline row; E = 4
    out["m25_b1_4x360"] = _with_events(base, {k: _normal_events(base, k, 4) for k in base["names"]})
    base = ru.make_case(64, 1, 4, 8, seed=9)                          # the largest row: rows per block capped by LDS
    out["m64_b1_4x8_e8"] = _with_events(base, {k: _normal_events(base, k, 8) for k in base["names"]})
    base = ru.make_case(1, 2, 6, 8, seed=5, four_d=True)              # a 4-D gen: the contingency table
    out["m1_b2_6x8"] = _with_events(base, {k: _normal_events(base, k, 2) for k in base["names"]})
    base = ru.make_case(5, 2, 6, 8, seed=6, kind="known")
    out["known_m5_b2_6x8"] = _with_events(base, {k: [("above_1p5", "above", 1.5)] for k in base["names"]})
    base = ru.make_case(5, 2, 6, 8, seed=7, kind="clipped")
    out["clipped_m5_b2_6x8"] = _with_events(base, {k: [("wet", "above", 0.0), ("negative", "below", 0.0)] for k in base["names"]})
    base = ru.make_case(5, 2, 6, 8, seed=8, kind="nan")
    ev = {}
    for k in base["names"]:
        thr = _climate(base, k) + np.float32(1.0)
        thr[0, 2] = thr[3, 5] = np.nan                                # (counted times of every window: a map has no time axis)
        ev[k] = [("anomaly", "above", thr), ("cold", "below", 270.0)]
    out["nan_m5_b2_6x8"] = _with_events(base, ev)
    assert list(out) == list(SMALL)
    return out


def production_case():
    """One 180 x 360 window of 25 members, 2 variables, 2 times, later in a run (both times counted), E = 4 with one map."""
    base = ru.production_case()
    pick = lambda k: [_normal_events(base, k, 5)[i] for i in (0, 1, 2, 4)]  # noqa: E731  (warm, cold, the anomaly map, hot)
    return _with_events(base, {k: pick(k) for k in base["names"]})


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


def _members(g):
    return g if g.ndim == 5 else g[None]


def _threshold(thr):
    return thr if isinstance(thr, np.ndarray) else np.float32(thr)


def _in(x, direction, c):
    with np.errstate(invalid="ignore"):
        return x < c if direction == "below" else x > c


def restate(case, pool=False, windows=None):
    """-> ({var: table (n_slots, E, H, 2, M + 1)}, {var: maps (E, 3, H, W)}) float64: the definition in a dozen lines."""
    M, H, W = case["M"], case["H"], case["W"]
    n_slots = 1 if pool else case["n_timesteps"]
    tables = {k: np.zeros((n_slots, len(case["events"][k]), H, 2, M + 1)) for k in event_names(case)}
    maps = {k: np.zeros((len(case["events"][k]), 3, H, W)) for k in event_names(case)}
    for start, target, gen in (case["windows"] if windows is None else windows):
        for name in event_names(case):
            y, g = target[name], _members(gen[name])
            for e, (_, direction, thr) in enumerate(case["events"][name]):
                c = _threshold(thr)
                k, o = _in(g, direction, c).sum(axis=0), _in(y, direction, c)
                counted = ~np.isnan(y) & ~np.isnan(np.broadcast_to(c, y.shape))
                for t in range(1 if start == 0 else 0, y.shape[1]):
                    for oo in (0, 1):
                        for kk in range(M + 1):
                            hit = (k[:, t] == kk) & (o[:, t] == bool(oo)) & counted[:, t]
                            tables[name][0 if pool else start + t, e, :, oo, kk] += hit.sum(axis=(0, 2))
                    maps[name][e, 0] += (k[:, t] * counted[:, t]).sum(axis=0)
                    maps[name][e, 1] += (o[:, t] & counted[:, t]).sum(axis=0)
                    maps[name][e, 2] += counted[:, t].sum(axis=0)
    return tables, maps


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


def fill_thresholds(thr, case, names):
    """The `sdy_event_thresholds` of an argument structure for the variables `names` (equal event count); -> keep-alive list."""
    E = len(case["events"][names[0]])
    scalars, maps = np.full((len(names), E), np.nan, np.float32), []
    for j, k in enumerate(names):
        thr.map_first[j] = len(maps)
        for e, (_, direction, c) in enumerate(case["events"][k]):
            thr.below[j] |= (1 << e) if direction == "below" else 0
            if isinstance(c, np.ndarray):
                thr.is_map[j] |= 1 << e
                maps.append(np.asarray(c, np.float32))
            else:
                scalars[j, e] = c
    maps = np.ascontiguousarray(np.stack(maps)) if maps else None
    thr.n_events, thr.n_maps = E, (0 if maps is None else len(maps))
    thr.scalars, thr.maps = vp(scalars), (None if maps is None else vp(maps))
    return [scalars, maps]


def args(case, target, gen, names, t0, t_start, n_slots, pool, acc):
    """SdyEventArgs over contiguous numpy arrays for the variables `names` (equal event count); -> (args, keep-alive list)."""
    from sdy_amd._lib import SdyEventArgs

    a = SdyEventArgs()
    keep, (H, W) = fill_window(a.win, target, gen, names)
    a.H, a.W, a.acc = H, W, vp(acc)
    fill_slots(a.slots, t0, t_start, n_slots, pool)
    return a, keep + fill_thresholds(a.thr, case, names) + [acc]


def host(case, pool=False, windows=None):
    """The case through the two _host entry points -> (tables, maps), shaped as `restate` gives them."""
    import sdy_amd

    M, H, W = case["M"], case["H"], case["W"]
    n_slots = 1 if pool else case["n_timesteps"]
    tables, maps = {}, {}
    for names in _runs(case):
        E = len(case["events"][names[0]])
        table, freq = np.zeros((len(names), n_slots, E, H, 2, M + 1)), np.zeros((len(names), E, 3, H, W))
        for start, target, gen in (case["windows"] if windows is None else windows):
            t0, t_start = (1 if start == 0 else 0), (0 if pool else start)
            a, keep = args(case, target, gen, names, t0, t_start, n_slots, pool, table)
            assert sdy_amd.lib.sdy_event_table_accumulate_host(C.byref(a)) == 0
            a.acc = vp(freq)
            assert sdy_amd.lib.sdy_event_frequency_accumulate_host(C.byref(a)) == 0
        for j, k in enumerate(names):
            tables[k], maps[k] = table[j], freq[j]
    return tables, maps


def same(got, want):
    return list(got) == list(want) and all(got[k].shape == want[k].shape and np.array_equal(got[k], want[k]) for k in want)


def lat_weights(case):
    return case["weights"].astype(np.float64).mean(axis=1)


def restate_scores(table, w):
    """`sdy_amd.events.scores` of ONE table (lat, 2, M + 1) in float64 numpy, straight from the definitions -> dict."""
    nk_o = (w[:, None, None] * table).sum(axis=0)
    n_k, o_k = nk_o.sum(axis=0), nk_o[1]
    M = len(n_k) - 1
    p = np.arange(M + 1) / M
    n, o = n_k.sum(), o_k.sum()
    nan = float("nan")
    if n == 0:
        return {**{m: nan for m in LOG_METRICS + ("uncertainty",)}, "reliability_curve": np.full(M + 1, nan)}
    b = o / n
    some = n_k > 0
    obar = np.full(M + 1, nan)
    obar[some] = o_k[some] / n_k[some]
    out = {"base_rate": b, "forecast_rate": (n_k * p).sum() / n,
           "brier_score": ((n_k - o_k) * p ** 2 + o_k * (1 - p) ** 2).sum() / n,
           "brier_reliability": (n_k[some] * (p[some] - obar[some]) ** 2).sum() / n,
           "brier_resolution": (n_k[some] * (obar[some] - b) ** 2).sum() / n,
           "uncertainty": b * (1 - b), "reliability_curve": obar}
    out["brier_skill_score"] = 1 - out["brier_score"] / out["uncertainty"] if out["uncertainty"] > 0 else nan
    if o == 0 or o == n:
        out["roc_area"] = nan
    else:
        hr = [o_k[j:].sum() / o for j in range(M + 1, -1, -1)]
        far = [(n_k[j:] - o_k[j:]).sum() / (n - o) for j in range(M + 1, -1, -1)]
        out["roc_area"] = sum(0.5 * (hr[i] + hr[i - 1]) * (far[i] - far[i - 1]) for i in range(1, M + 2))
    return out


def restate_logs(case, tables, label=""):
    """EventVerificationAggregator.get_logs(label) in float64 numpy, from the tables pooled over all slots."""
    w, logs = lat_weights(case), {}
    for k in event_names(case):
        for e, (name, _, _) in enumerate(case["events"][k]):
            s = restate_scores(tables[k][:, e].sum(axis=0), w)
            for metric in LOG_METRICS:
                logs[f"{metric}/{name}/{k}"] = float(s[metric])
    return {f"{label}/{k}": v for k, v in logs.items()} if label else logs


def _check_base_rates(case):
    """Except in the two cases built to be degenerate, every (variable, event) has 0.01 <= base rate <= 0.99, which keeps
    roc_area and brier_skill_score finite: a NaN-equals-NaN comparison cannot hide a wrong table."""
    if _is_degenerate(case):
        return
    tables, _ = restate(case)
    for key, value in restate_logs(case, tables).items():
        if key.startswith("base_rate/"):
            assert 0.01 <= value <= 0.99, (key, value)
        assert np.isfinite(value), (key, value)


def _is_degenerate(case):
    return any(name in ("above_1p5", "negative") for evs in case["events"].values() for name, _, _ in evs)


def close(got, want, what, scale=1.0):
    """Both float64 arrays (or floats): NaN where the other has NaN, else |got - want| <= TOL x scale."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, f"{what}: shape {got.shape} against {want.shape}"
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: NaN pattern differs"
    ok = ~np.isnan(want)
    err = np.abs(got[ok] - want[ok])
    assert (err <= TOL * scale).all(), f"{what}: off by up to {float(err.max()):.3e}, bound {TOL * scale:.3e}"


def close_scores(got, want, what):
    """A dict of scores against the restatement's: scale 1 / uncertainty for the skill score, 1 for the rest."""
    for metric, value in want.items():
        scale = 1.0
        if metric == "brier_skill_score" and np.isfinite(want["uncertainty"]) and want["uncertainty"] > 0:
            scale = 1.0 / want["uncertainty"]
        close(got[metric], value, f"{what} {metric}", scale)
