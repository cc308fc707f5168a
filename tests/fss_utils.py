"""Shared by tests/test_fss_host.py and tests/test_gpu_fss.py: cases from seeded numpy (the fields of tests/rank_hist_utils.py
with events and radii on top), the numpy int64 restatement of the neighbourhood sums (include/sdy_amd.h, sdy_fss_args) -- box
sums by np.roll over d and a clipped loop over rows, nothing clever -- the library's _host entry point driven from numpy, and a
brute-force float64 computation of the scores from the fractions of every centre.

The sums are integers: compared with np.array_equal, never a tolerance.  The scores are compared to TOL = 1e-12 (absolute;
everything lies in [0, 1], or is 1 minus a ratio of two such sums): each is a ratio of two float64 sums of at most a few
thousand non-negative terms, whose relative rounding error stays below 1e-13.
"""
import ctypes as C

import numpy as np

import rank_hist_utils as ru
from event_verif_utils import fill_thresholds
from window_utils import fill_slots, fill_window, vp

TOL = 1e-12
TERMS = ("count", "sum_k", "sum_o", "sum_kk", "sum_ko", "sum_oo")
LOG_METRICS = ("fss", "fbs", "base_rate", "fss_useful", "counted_fraction")
SLOT_METRICS = ("fss", "fbs", "base_rate", "forecast_rate", "fss_useful", "counted_fraction")

SMALL = ("m3_b2_5x8", "m2_b2_4x5", "m4_b2_5x6", "m25_b1_37x40", "m64_b1_33x32_full", "m1_b2_6x8", "nan_m5_b2_6x8")


def _climate(case, name):
    y = np.concatenate([t[name] for _, t, _ in case["windows"]], axis=1)
    return np.nanmean(y.astype(np.float64), axis=(0, 1)).astype(np.float32)


def _with(case, radii, events):
    case = dict(case)
    case["radii"], case["events"] = tuple(radii), events
    return case


def _events(case, name, n):
    """n events of a variable of a "normal" field (climate 280 +- 20, weather +- 3): scalars and maps, above and below."""
    clim = _climate(case, name)
    menu = [("warm", "above", 285.0), ("cool_anomaly", "below", clim - np.float32(2.0)), ("anomaly", "above", clim + np.float32(1.0)),
            ("cold", "below", 270.0)]
    return menu[:n]


def cases():
    """The small cases of the issue's list, by name."""
    out = {}
    base = ru.make_case(3, 2, 5, 8, seed=31, names=("a", "b", "c"))      # clipped rows; wrap; all threshold kinds
    out["m3_b2_5x8"] = _with(base, (0, 1, 2), {"a": _events(base, "a", 4), "b": _events(base, "b", 1)})
    base = ru.make_case(2, 2, 4, 5, seed=32)                             # W = 5 with r = 2: the window is the whole circle
    out["m2_b2_4x5"] = _with(base, (2,), {k: _events(base, k, 2) for k in base["names"]})
    base = ru.make_case(4, 2, 5, 6, seed=33)                             # plane = 30: no 16-byte loads
    out["m4_b2_5x6"] = _with(base, (0, 2), {k: _events(base, k, 3) for k in base["names"]})
    base = ru.make_case(25, 1, 37, 40, seed=34, names=("a",))            # three bands of 16 rows: the halos cross band boundaries
    out["m25_b1_37x40"] = _with(base, (1, 4, 15), {"a": _events(base, "a", 2)})
    ones = np.ones((1, 2, 33, 32), np.float32)                           # K = M n = 61504 at the 16-bit bound, K^2 at the 32-bit one
    full = dict(M=64, B=1, H=33, W=32, names=["a"], weights=ru._weights(33, 32), n_timesteps=3,
                windows=[(1, {"a": ones}, {"a": np.ones((64, 1, 2, 33, 32), np.float32)})])
    out["m64_b1_33x32_full"] = _with(full, (15,), {"a": [("positive", "above", 0.0)]})
    base = ru.make_case(1, 2, 6, 8, seed=35, four_d=True)                # a 4-D gen: one member
    out["m1_b2_6x8"] = _with(base, (0, 1), {k: _events(base, k, 2) for k in base["names"]})
    base = ru.make_case(5, 2, 6, 8, seed=36, kind="nan")                 # NaN targets, NaN members, NaN in a threshold map
    ev = {}
    for k in base["names"]:
        thr = _climate(base, k) + np.float32(1.0)
        thr[0, 2] = thr[3, 5] = np.nan
        ev[k] = [("anomaly", "above", thr), ("cold", "below", 275.0)]
    out["nan_m5_b2_6x8"] = _with(base, (0, 1, 2), ev)
    assert list(out) == list(SMALL)
    return out


def production_case():
    """One 180 x 360 window of 25 members, one variable, 2 times, later in a run (both counted), radii (1, 3, 7, 15)."""
    base = ru.make_case(25, 1, 180, 360, seed=20262, windows=((4, 2),), names=("a",))
    return _with(base, (1, 3, 7, 15), {"a": _events(base, "a", 3)[::2]})


def displaced_case(shift=2):
    """The truth is a field of smooth blobs; every member is the truth moved `shift` longitudes east: a forecast that is right
    but for its place.  One variable, one event, radii (0, 1, 2, 4)."""
    rng = np.random.default_rng(77)
    B, T, H, W, M = 2, 3, 12, 24, 4
    y = rng.standard_normal((B, T, H, W))
    for _ in range(2):                                                   # smoothed: events come in patches of a few points
        y = (y + np.roll(y, 1, -1) + np.roll(y, -1, -1) + np.roll(y, 1, -2) + np.roll(y, -1, -2)) / 5.0
    y = y.astype(np.float32)
    g = np.ascontiguousarray(np.broadcast_to(np.roll(y, shift, axis=-1)[None], (M, B, T, H, W)))
    case = dict(M=M, B=B, H=H, W=W, names=["a"], weights=ru._weights(H, W), n_timesteps=T + 1, windows=[(1, {"a": y}, {"a": g})])
    return _with(case, (0, 1, 2, 4), {"a": [("high", "above", float(np.quantile(y, 0.8)))]})


def event_names(case):
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


def _in(x, direction, c):
    with np.errstate(invalid="ignore"):
        return x < c if direction == "below" else x > c


def point_fields(y, g, direction, thr):
    """-> (k, o, c) int64 (B, T, H, W) of one event: members in it, truth in it, counted; k = o = 0 where c = 0."""
    c = thr if isinstance(thr, np.ndarray) else np.float32(thr)
    counted = ~np.isnan(y) & ~np.isnan(np.broadcast_to(c, y.shape))
    k = _in(_members(g), direction, c).sum(axis=0).astype(np.int64) * counted
    o = (_in(y, direction, c) & counted).astype(np.int64)
    return k, o, counted.astype(np.int64)


def box(x, r):
    """Box sums of x (..., H, W): periodic in longitude (np.roll over d), clipped at the poles (a loop over rows)."""
    H = x.shape[-2]
    h = sum(np.roll(x, d, axis=-1) for d in range(-r, r + 1))
    out = np.zeros_like(x)
    for lat in range(H):
        out[..., lat, :] = h[..., max(0, lat - r):min(H - 1, lat + r) + 1, :].sum(axis=-2)
    return out


def sizes(H, r):
    """n(lat, r) int64 (H,)."""
    lat = np.arange(H)
    return (2 * r + 1) * (np.minimum(H - 1, lat + r) - np.maximum(0, lat - r) + 1)


def restate(case, pool=False, windows=None, brute=False):
    """-> {var: sums (n_slots, E, R, H, 6) int64}: the definition.  brute=True: -> ({var: sums}, {var: (n_slots, E, R, 6) float64})
    with, per (slot, event, radius), the latitude-weighted float64 sums over the counted centres of (F - Of)^2, F^2 + Of^2, 1,
    Of and F, and the weighted number of all centres seen: what the scores are by their definition."""
    H, W, M, radii = case["H"], case["W"], case["M"], case["radii"]
    n_slots = 1 if pool else case["n_timesteps"]
    w = lat_weights(case)
    sums = {k: np.zeros((n_slots, len(case["events"][k]), len(radii), H, 6), np.int64) for k in event_names(case)}
    frac = {k: np.zeros((n_slots, len(case["events"][k]), len(radii), 6)) for k in event_names(case)}
    for start, target, gen in (case["windows"] if windows is None else windows):
        for name in event_names(case):
            for e, (_, direction, thr) in enumerate(case["events"][name]):
                k, o, c = point_fields(target[name], gen[name], direction, thr)
                for j, r in enumerate(radii):
                    K, O, Cn = box(k, r), box(o, r), box(c, r)
                    n = sizes(H, r)[:, None]
                    ok = Cn == n
                    terms = [ok, K * ok, O * ok, K * K * ok, K * O * ok, O * O * ok]
                    F, Of = K / (M * n), O / n
                    parts = [(F - Of) ** 2 * ok, (F * F + Of * Of) * ok, ok, Of * ok, F * ok, np.ones_like(F)]
                    for t in range(1 if start == 0 else 0, k.shape[1]):
                        slot = 0 if pool else start + t
                        for q, x in enumerate(terms):
                            sums[name][slot, e, j, :, q] += x[:, t].sum(axis=(0, 2))
                        for q, x in enumerate(parts):
                            frac[name][slot, e, j, q] += (w[:, None] * x[:, t].sum(axis=0)).sum()
    return (sums, frac) if brute else sums


def brute_scores(frac):
    """The scores from the six weighted float64 sums (..., 6) of `restate(brute=True)` -> dict of (...) arrays."""
    num, ref, cnt, base, rate, seen = np.moveaxis(frac, -1, 0)
    with np.errstate(invalid="ignore", divide="ignore"):
        some = cnt > 0
        out = {"fss": np.where(some & (ref > 0), 1 - num / ref, np.nan), "fbs": np.where(some, num / cnt, np.nan),
               "base_rate": np.where(some, base / cnt, np.nan), "forecast_rate": np.where(some, rate / cnt, np.nan),
               "counted_fraction": np.where(some, cnt / seen, np.nan)}
    out["fss_useful"] = 0.5 + out["base_rate"] / 2
    return out


def restate_logs(case, frac, label=""):
    """FractionsSkillAggregator.get_logs(label) from the brute-force sums pooled over all slots."""
    logs = {}
    for k in event_names(case):
        s = brute_scores(frac[k].sum(axis=0))                            # (E, R)
        for e, (name, _, _) in enumerate(case["events"][k]):
            for j, r in enumerate(case["radii"]):
                for metric in LOG_METRICS:
                    logs[f"{metric}_r{r}/{name}/{k}"] = float(s[metric][e, j])
    return {f"{label}/{k}": v for k, v in logs.items()} if label else logs


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


def args(case, target, gen, names, t0, t_start, n_slots, pool, acc, ws=None):
    """SdyFssArgs over contiguous numpy arrays for the variables `names` (equal event count); -> (args, keep-alive list)."""
    from sdy_amd._lib import SdyFssArgs

    a = SdyFssArgs()
    keep, (H, W) = fill_window(a.win, target, gen, names)
    a.H, a.W, a.acc = H, W, vp(acc)
    fill_slots(a.slots, t0, t_start, n_slots, pool)
    keep += fill_thresholds(a.thr, case, names)
    a.n_radii = len(case["radii"])
    for j, r in enumerate(case["radii"]):
        a.radii[j] = r
    if ws is not None:
        a.ws, a.ws_bytes = vp(ws), ws.nbytes
    return a, keep + [acc, ws]


def host(case, pool=False, windows=None):
    """The case through sdy_fss_accumulate_host -> {var: sums}, shaped as `restate` gives them (float64)."""
    import sdy_amd

    H, R = case["H"], len(case["radii"])
    n_slots = 1 if pool else case["n_timesteps"]
    out = {}
    for names in _runs(case):
        E = len(case["events"][names[0]])
        acc = np.zeros((len(names), n_slots, E, R, H, 6))
        for start, target, gen in (case["windows"] if windows is None else windows):
            a, keep = args(case, target, gen, names, 1 if start == 0 else 0, 0 if pool else start, n_slots, pool, acc)
            assert sdy_amd.lib.sdy_fss_accumulate_host(C.byref(a)) == 0
        for j, k in enumerate(names):
            out[k] = acc[j]
    return out


def same(got, want):
    return list(got) == list(want) and all(got[k].shape == want[k].shape and np.array_equal(got[k], want[k]) for k in want)


def lat_weights(case):
    return case["weights"].astype(np.float64).mean(axis=1)


def close(got, want, what):
    """Both float64 arrays (or floats): NaN where the other has NaN, else |got - want| <= TOL."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, f"{what}: shape {got.shape} against {want.shape}"
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: NaN pattern differs"
    ok = ~np.isnan(want)
    err = np.abs(got[ok] - want[ok])
    assert (err <= TOL).all(), f"{what}: off by up to {float(err.max()):.3e}, bound {TOL:.1e}"
