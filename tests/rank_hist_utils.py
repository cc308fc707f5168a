"""Shared by tests/test_rank_hist_host.py and tests/test_gpu_rank_hist.py: cases from seeded numpy, the numpy restatement of the
rank histogram (include/sdy_amd.h, sdy_rank_hist_args), the library's _host entry point driven from numpy, and the float64
restatement of `RankHistogramAggregator.get_data` / `get_logs`.

Counts and ties are integers: compared with np.array_equal, never a tolerance.  `frequency` and the log scalars are sums of H
+ M exactly represented float64 terms and one division: compared to REL = 1e-12 relative (below 250 x 2^-53 at 180 latitudes,
with two decades of margin).
"""
import ctypes as C

import numpy as np

from window_utils import fill_slots, fill_window, vp

REL = 1e-12

# every case but the production grid: two windows, the first of a run (its time 0 is the initial condition) and a later one
WINDOWS = ((0, 3), (3, 2))
SMALL = ("m5_b2_6x8", "m2_b3_7x10", "m9_b1_4x36", "m25_b1_4x360", "m1_b2_6x8", "known_m5_b2_6x8", "clipped_m5_b2_6x8",
         "nan_m5_b2_6x8")
PRODUCTION = "m25_b1_180x360"


def _weights(H, W):
    """(H, W) float32 cos(latitude) weights, normalised, exactly constant along a row."""
    lat = (np.arange(H) + 0.5) / H * np.pi - np.pi / 2
    w = np.cos(lat) / (np.cos(lat).sum() * W)
    return np.ascontiguousarray(np.repeat(w.astype(np.float32)[:, None], W, axis=1))


def make_case(M, B, H, W, seed, windows=WINDOWS, names=("a", "b"), kind="normal", four_d=False):
    """-> dict(M, B, H, W, names, weights, n_timesteps, windows=[(i_time_start, target {name: (B, T, H, W)}, gen {name: (M, B,
    T, H, W)} (four_d: (B, T, H, W)))]).  kind: "normal" (gen = a biased, under-dispersive copy of the target's climate),
    "clipped" (max(x, 0) for both: ties), "nan" (NaN planted in a few target and a few member points), "known" (member m is
    the constant field m, the target k - 0.5 on latitude k: every point of row k has rank min(k, M))."""
    rng = np.random.default_rng(seed)
    n_total = max(s + T for s, T in windows)
    target, gen = {}, {}
    for k in names:
        if kind == "known":
            y = np.broadcast_to((np.arange(H) - 0.5)[:, None], (B, n_total, H, W)).astype(np.float32)
            g = np.broadcast_to(np.arange(M, dtype=np.float32)[:, None, None, None, None], (M, B, n_total, H, W))
        elif kind == "clipped":
            y = np.maximum(rng.standard_normal((B, n_total, H, W)), 0.0).astype(np.float32)
            g = np.maximum(rng.standard_normal((M, B, n_total, H, W)), 0.0).astype(np.float32)
        else:
            clim = 280.0 + 20.0 * rng.standard_normal((H, W))
            y = (clim + 3.0 * rng.standard_normal((B, n_total, H, W))).astype(np.float32)
            g = (clim + 2.0 * rng.standard_normal((M, B, n_total, H, W)) + 0.5).astype(np.float32)
            if kind == "nan":
                for _ in range(7):
                    y[tuple(rng.integers(n) for n in y.shape)] = np.nan
                for _ in range(11):
                    g[tuple(rng.integers(n) for n in g.shape)] = np.nan
                y[0, -1, 0, 0] = g[0, 0, -1, 0, 1] = np.nan       # (two that are counted times whatever the draws)
        target[k], gen[k] = np.ascontiguousarray(y), np.ascontiguousarray(g)
    out = []
    for start, T in windows:
        out.append((start, {k: target[k][:, start:start + T] for k in names},
                    {k: (gen[k][0, :, start:start + T] if four_d else gen[k][:, :, start:start + T]) for k in names}))
    return dict(M=M, B=B, H=H, W=W, names=list(names), weights=_weights(H, W), n_timesteps=n_total, windows=out)


def cases():
    """The small cases of the issue's table, by name."""
    return {
        "m5_b2_6x8": make_case(5, 2, 6, 8, seed=1),
        "m2_b3_7x10": make_case(2, 3, 7, 10, seed=2),                     # W % 4 != 0: the scalar path; odd H
        "m9_b1_4x36": make_case(9, 1, 4, 36, seed=3),                     # one past a batch of 8 members; 9 units: idle lanes
        "m25_b1_4x360": make_case(25, 1, 4, 360, seed=4),                 # the headline row: 90 units, 3 passes of 32 lanes
        "m1_b2_6x8": make_case(1, 2, 6, 8, seed=5, four_d=True),          # a 4-D gen: one member, two bins
        "known_m5_b2_6x8": make_case(5, 2, 6, 8, seed=6, kind="known"),
        "clipped_m5_b2_6x8": make_case(5, 2, 6, 8, seed=7, kind="clipped"),
        "nan_m5_b2_6x8": make_case(5, 2, 6, 8, seed=8, kind="nan"),
    }


def production_case():
    """One 180 x 360 window of 25 members, 2 variables, 2 times, later in a run (both times counted): 26 MB."""
    return make_case(25, 1, 180, 360, seed=20261, windows=((4, 2),))


def _members(g):
    return g if g.ndim == 5 else g[None]


def restate(case, pool=False, windows=None):
    """-> (counts (nvars, n_slots, H, M + 1), ties (nvars, n_slots, H)) float64: the definition in five lines of numpy."""
    names, M, H = case["names"], case["M"], case["H"]
    n_slots = 1 if pool else case["n_timesteps"]
    counts, ties = np.zeros((len(names), n_slots, H, M + 1)), np.zeros((len(names), n_slots, H))
    for start, target, gen in (case["windows"] if windows is None else windows):
        for j, k in enumerate(names):
            y, g = target[k], _members(gen[k])
            with np.errstate(invalid="ignore"):
                r = (g < y[None]).sum(0)
                ok = ~np.isnan(y)
                tie = (g == y[None]).any(0) & ok
            for t in range(1 if start == 0 else 0, y.shape[1]):
                slot = 0 if pool else start + t
                for b in range(M + 1):
                    counts[j, slot, :, b] += ((r[:, t] == b) & ok[:, t]).sum(axis=(0, 2))
                ties[j, slot] += tie[:, t].sum(axis=(0, 2))
    return counts, ties


def args(target, gen, names, t0, t_start, n_slots, pool, counts, ties):
    """SdyRankHistArgs over contiguous numpy arrays (gen 4-D or member-stacked 5-D); -> (args, keep-alive list)."""
    from sdy_amd._lib import SdyRankHistArgs

    a = SdyRankHistArgs()
    keep, (H, W) = fill_window(a.win, target, gen, names)
    a.H, a.W = H, W
    fill_slots(a.slots, t0, t_start, n_slots, pool)
    a.counts, a.ties = vp(counts), vp(ties)
    return a, keep


def host(case, pool=False, windows=None):
    """The case through sdy_rank_hist_accumulate_host -> (counts, ties), shaped as `restate` gives them."""
    import sdy_amd

    names, M, H = case["names"], case["M"], case["H"]
    n_slots = 1 if pool else case["n_timesteps"]
    counts, ties = np.zeros((len(names), n_slots, H, M + 1)), np.zeros((len(names), n_slots, H))
    for start, target, gen in (case["windows"] if windows is None else windows):
        a, keep = args(target, gen, names, 1 if start == 0 else 0, 0 if pool else start, n_slots, pool, counts, ties)
        assert sdy_amd.lib.sdy_rank_hist_accumulate_host(C.byref(a)) == 0
    return counts, ties


def lat_weights(case):
    return case["weights"].astype(np.float64).mean(axis=1)


def restate_frequency(case, counts):
    """frequency (nvars, n_slots, M + 1) = sum_lat w_lat counts / sum_lat,k w_lat counts; NaN for a slot without counts."""
    weighted = (lat_weights(case)[None, None, :, None] * counts).sum(axis=2)
    with np.errstate(invalid="ignore"):
        return weighted / weighted.sum(axis=2, keepdims=True)


def restate_logs(case, counts, ties, label=""):
    """RankHistogramAggregator.get_logs(label) in float64 numpy, from the counts pooled over all slots."""
    w, M = lat_weights(case), case["M"]
    logs = {}
    for j, k in enumerate(case["names"]):
        bins = (w[:, None] * counts[j].sum(axis=0)).sum(axis=0)
        freq = bins / bins.sum()
        logs[f"reliability_index/{k}"] = float(np.abs(freq - 1.0 / (M + 1)).sum())
        logs[f"outlier_fraction/{k}"] = float(freq[0] + freq[M])
        logs[f"tie_fraction/{k}"] = float((w * ties[j].sum(axis=0)).sum() / bins.sum())
    return {f"{label}/{k}": v for k, v in logs.items()} if label else logs


def close(got, want, what):
    """Both float64 arrays (or floats): NaN where the other has NaN, else |got - want| <= REL |want|."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, f"{what}: shape {got.shape} against {want.shape}"
    assert np.array_equal(np.isnan(got), np.isnan(want)), f"{what}: NaN pattern differs"
    ok = ~np.isnan(want)
    err = np.abs(got[ok] - want[ok])
    bound = REL * np.abs(want[ok])
    assert (err <= bound).all(), f"{what}: off by up to {float((err - bound).max()):.3e} over the bound"
