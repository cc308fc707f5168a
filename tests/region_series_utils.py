"""Shared by tests/test_region_series_host.py and tests/test_gpu_region_series.py: the fixture of the reference's inference
MeanAggregator run once per region (tests/golden/fx_region_series.npz; tools/gen_golden_region_series.py), a driver of
sdy_region_series_host from numpy, a float64 restatement of the eight sums (with the zero-weight rule) and of MeanAggregator's
metric definitions, and the comparison bounds.

Bounds (u = 2^-24; M members, HW grid points).  A raw sum is sum_i w_i q_i, a series value the mean over a window's samples of a
function of the raw sums divided by W_r = sum_i w_i; a bound is a multiple `rel` of the quantity's TERM SCALE, the maxima taken
over the members, samples, times and grid points of a case's variable:
    mse, and the member variance behind ssr      max (g_m - y)^2
    bias                                         max |g_m - y|
    crps                                         max |g_m - y| + max |g_i - g_j|
    mean_gen, mean_target                        max |x|
    the variances behind std_gen / std_target    max x^2     (compared as variances: the one-pass form cancels against mean^2)
  * against `ref64`, the reference's class on float64 inputs (the pin): rel = 1e-12, the bound of field_stats_utils.check_close;
  * against `ref32`, what the reference returns (a sanity check only): rel = (HW + M + 4) u, its own worst-case fp32 summation
    error;
  * raw sums of two float64 paths that add in another order (device against host twin): HW 2^-53 sum_i w_i |q_i| per sum;
  * raw sums against the restatement (whose per-point arithmetic differs in rounding): 1e-12 x term scale x W_r.
Square roots.  weighted_rmse, weighted_std_* and weighted_ssr are roots of a quantity Q with a bound dQ as above (rmse is
compared as a square, ssr through its two squares: ssr^2 = V (M + 1) / (M mse), d ssr^2 = (dV (M + 1) / M + ssr^2 dmse) / mse).
A series holds the mean over samples of the roots, so the bound is taken through the root, sample by sample:
|sqrt(Q + d) - sqrt(Q)| <= min(|d| / sqrt(Q), sqrt|d|) for any Q >= 0 (the root clamped at 0), with Q from the restatement."""
import ctypes as C
import json

import numpy as np

import golden_utils as gu
from window_utils import fill_window, vp

U = 2.0 ** -24
SUMS = ("mse", "var", "crps", "bias", "gen", "gen_sq", "tgt", "tgt_sq")          # the order of sdy_ensemble_series
METRICS = ("weighted_rmse", "weighted_bias", "weighted_mean_gen", "weighted_mean_target", "weighted_std_gen",
           "weighted_std_target")
METRICS_ENSEMBLE = ("weighted_crps", "weighted_ssr")

_cache = {}


def fixture():
    """-> dict(lats, lons, area (H, W) f32, regions [names], weights (R, H, W) f32, fraction, definitions, names, n_timesteps,
    cases={"ens" | "det": dict(windows=[(i_time_start, target {name: (S, T, H, W)}, gen {name: (M, S, T, H, W) | (S, T, H,
    W)})], metrics, ref32 / ref64 = {"<metric>/<region>/<variable>": (n_timesteps,)})}).  Loaded once and shared: read-only."""
    if "fx" in _cache:
        return _cache["fx"]
    z = gu.load("fx_region_series")
    names = json.loads(str(z["names"]))
    fx = dict(lats=z["lats"], lons=z["lons"], area=z["area"], regions=json.loads(str(z["regions"])), weights=z["weights"],
              fraction=z["fraction"], definitions=json.loads(str(z["definitions"])), names=names,
              n_timesteps=int(z["n_timesteps"]), cases={})
    for key in ("ens", "det"):
        windows = [(int(z[f"{key}::i_time_start{i}"]), {n: z[f"{key}::tgt{i}::{n}"] for n in names},
                    {n: z[f"{key}::gen{i}::{n}"] for n in names}) for i in range(3)]
        ref = {tag: {k.split("::", 2)[2]: z[k] for k in z.files if k.startswith(f"{key}::{tag}::")} for tag in ("ref32", "ref64")}
        fx["cases"][key] = dict(windows=windows, metrics=json.loads(str(z[f"{key}::metrics"])), **ref)
    _cache["fx"] = fx
    return fx


def seeded_window(M, S, T, H, W, names, seed):
    """(target {name: (S, T, H, W)}, gen {name: (M, S, T, H, W), or (S, T, H, W) for M == 0}) of the fixture's kind."""
    rng = np.random.default_rng(seed)
    target = {k: (1.0 + 2.0 * rng.standard_normal((S, T, H, W))).astype(np.float32) for k in names}
    shape = (M, S, T, H, W) if M else (S, T, H, W)
    gen = {k: (target[k] + 0.2 + 0.5 * rng.standard_normal(shape)).astype(np.float32) for k in names}
    return target, gen


def seeded_regions(R, H, W, seed):
    """(R, H, W) fp32 maps that overlap: region 0 everywhere (cos-latitude weights), region 1 (if any) a single point, region
    2 (if any) the last eighth of the plane only -- zero over whole chunks when the plane has several --, the rest seeded
    fractions with a third of the points exactly 0."""
    rng = np.random.default_rng(seed)
    lat = (np.arange(H) + 0.5) / H * np.pi - np.pi / 2
    area = np.broadcast_to(np.cos(lat)[:, None], (H, W)) / (np.cos(lat).sum() * W)
    maps = np.zeros((R, H * W))
    for r in range(R):
        if r == 0:
            f = np.ones(H * W)
        elif r == 1:
            f = np.zeros(H * W)
            f[(H * W * 2) // 3] = 1.0
        elif r == 2:
            f = np.zeros(H * W)
            f[H * W - max(H * W // 8, 1):] = 1.0
        else:
            f = rng.random(H * W)
            f[rng.random(H * W) < 1.0 / 3.0] = 0.0
        maps[r] = area.reshape(-1) * f
    return maps.reshape(R, H, W).astype(np.float32)


def _members(gen):
    g = np.asarray(gen, np.float64)
    return g if g.ndim == 5 else g[None]


def restate_point(target, gen):
    """The eight per-point quantities (S, T, H, W, 8) of one variable, float64 numpy, and the term scales of the module
    docstring."""
    y, g = np.asarray(target, np.float64), _members(gen)
    M = g.shape[0]
    with np.errstate(invalid="ignore"):
        return _restate_point(y, g, M)


def _restate_point(y, g, M):
    em = g.mean(axis=0)
    e = em - y
    crps, var, pair_max = np.abs(g - y).mean(axis=0), np.zeros_like(y), 0.0
    if M > 1:
        pairs = np.zeros_like(y)
        for i in range(M):
            d = np.abs(g[i] - g[i + 1:])
            if d.size:
                pairs += d.sum(axis=0)
                pair_max = max(pair_max, float(np.nanmax(d)))
        crps = crps - pairs / (M * (M - 1))
        var = g.var(axis=0, ddof=1)
    q = np.stack([e * e, var, crps, e, em, em * em, y, y * y], axis=-1)
    d = g - y
    xmax = max(float(np.nanmax(np.abs(g))), float(np.nanmax(np.abs(y))))
    scales = dict(sq=float(np.nanmax(d * d)), abs=float(np.nanmax(np.abs(d))), pair=pair_max, x=xmax, x2=xmax * xmax)
    return q, scales


def restate_sums(target, gen, names, weights):
    """-> (sums (nvars, R, S, T, 8), abs_sums the same of w |q|, scales [per variable]).  Zero-weight rule: the points where a
    region's weight is exactly 0 are left out of that region's sums, whatever their values."""
    R = weights.shape[0]
    sums, abs_sums, scales = [], [], []
    for k in names:
        q, sc = restate_point(target[k], gen[k])
        scales.append(sc)
        per_r, per_r_abs = [], []
        for r in range(R):
            w = weights[r].astype(np.float64)
            keep = (w != 0.0)[None, None, :, :, None]
            with np.errstate(invalid="ignore"):
                term = np.where(keep, w[None, None, :, :, None] * q, 0.0)
            per_r.append(term.sum(axis=(2, 3)))
            per_r_abs.append(np.abs(term).sum(axis=(2, 3)))
        sums.append(np.stack(per_r))
        abs_sums.append(np.stack(per_r_abs))
    return np.stack(sums), np.stack(abs_sums), scales


def term_scale(sc):
    """Term scale of each of the eight raw sums."""
    return np.array([sc["sq"], sc["sq"], sc["abs"] + sc["pair"], sc["abs"], sc["x"], sc["x2"], sc["x"], sc["x2"]])


def region_args(target, gen, names, weights, out):
    """SdyRegionSeriesArgs over contiguous numpy arrays; -> (args, keep-alive list)."""
    from sdy_amd._lib import SdyRegionSeriesArgs

    a = SdyRegionSeriesArgs()
    keep, (H, W) = fill_window(a.win, target, gen, names)
    w = np.ascontiguousarray(weights, np.float32).reshape(weights.shape[0], -1)
    assert w.shape[1] == H * W
    a.HW, a.n_regions, a.weights, a.out = H * W, w.shape[0], vp(w), vp(out)
    return a, keep + [w]


def host_sums(target, gen, names, weights):
    """sdy_region_series_host -> (nvars, R, S, T, 8)."""
    import sdy_amd

    S, T = target[names[0]].shape[:2]
    out = np.full((len(names), weights.shape[0], S, T, 8), np.nan)
    a, keep = region_args(target, gen, names, weights, out)
    rc = sdy_amd.lib.sdy_region_series_host(C.byref(a))
    assert rc == 0, rc
    return out


def weight_sums(weights):
    """(R,) float64 sums of the fp32 maps."""
    return weights.reshape(weights.shape[0], -1).astype(np.float64).sum(axis=1)


def finalize(sums, wsum, M, ensemble):
    """MeanAggregator's metric definitions on raw sums (nvars, R, S, T, 8) -> {metric: (nvars, R, S, T)} per sample, and the
    quantities under the roots {"mse", "var_gen", "var_tgt", "ssr2"}."""
    s = sums / wsum[None, :, None, None, None]
    mse, var, crps, bias, mg, mg2, mt, mt2 = [s[..., i] for i in range(8)]
    with np.errstate(invalid="ignore", divide="ignore"):
        vg, vt = np.maximum(mg2 - mg * mg, 0.0), np.maximum(mt2 - mt * mt, 0.0)
        # (numpy's maximum propagates NaN, as torch's clamp_min does)
        vals = {"weighted_rmse": np.sqrt(mse), "weighted_bias": bias, "weighted_mean_gen": mg, "weighted_mean_target": mt,
                "weighted_std_gen": np.sqrt(vg), "weighted_std_target": np.sqrt(vt)}
        roots = {"mse": mse, "var_gen": vg, "var_tgt": vt}
        if ensemble:
            vals["weighted_crps"] = crps
            roots["spread2"] = var * (M + 1) / M
            roots["ssr2"] = roots["spread2"] / mse
            vals["weighted_ssr"] = np.sqrt(var) * ((M + 1) / M) ** 0.5 / np.sqrt(mse)
    return vals, roots


def series_from_windows(windows, names, regions, weights, n_timesteps, ensemble, sums_of):
    """RegionalMeanAggregator's bookkeeping in numpy: `sums_of(target, gen)` -> raw sums of one window.
    -> {"<metric>/<region>/<variable>": (n_timesteps,)}."""
    wsum = weight_sums(weights)
    total, n_batches = {}, np.zeros(n_timesteps)
    for start, target, gen in windows:
        M = _members(gen[names[0]]).shape[0]
        vals, _ = finalize(sums_of(target, gen), wsum, M, ensemble)
        T = target[names[0]].shape[1]
        for metric, v in vals.items():
            tot = total.setdefault(metric, np.zeros((len(names), len(regions), n_timesteps)))
            tot[:, :, start:start + T] += v.mean(axis=2)
        n_batches[start:start + T] += 1
    return {f"{metric}/{region}/{name}": tot[v, r] / n_batches
            for metric, tot in total.items() for r, region in enumerate(regions) for v, name in enumerate(names)}


def _root_bound(Q, dQ):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.minimum(np.where(Q > 0.0, dQ / np.sqrt(Q), np.inf), np.sqrt(dQ))


def series_bounds(windows, names, regions, weights, n_timesteps, ensemble, rel):
    """Per series key the bound (n_timesteps,) of the module docstring for the relative size `rel`, from the restatement; every
    time index of the fixture's kind is touched by one window."""
    wsum = weight_sums(weights)
    out = {}
    for start, target, gen in windows:
        M = _members(gen[names[0]]).shape[0]
        sums, _, scales = restate_sums(target, gen, names, weights)
        _, roots = finalize(sums, wsum, M, ensemble)
        T = target[names[0]].shape[1]
        for v, name in enumerate(names):
            sc = scales[v]
            per_sample = {"weighted_rmse": _root_bound(roots["mse"][v], rel * sc["sq"]),
                          "weighted_bias": np.full(roots["mse"][v].shape, rel * sc["abs"]),
                          "weighted_mean_gen": np.full(roots["mse"][v].shape, rel * sc["x"]),
                          "weighted_mean_target": np.full(roots["mse"][v].shape, rel * sc["x"]),
                          "weighted_std_gen": _root_bound(roots["var_gen"][v], rel * sc["x2"]),
                          "weighted_std_target": _root_bound(roots["var_tgt"][v], rel * sc["x2"])}
            if ensemble:
                per_sample["weighted_crps"] = np.full(roots["mse"][v].shape, rel * (sc["abs"] + sc["pair"]))
                d_ssr2 = (rel * sc["sq"] * (M + 1) / M + roots["ssr2"][v] * rel * sc["sq"]) / roots["mse"][v]
                per_sample["weighted_ssr"] = _root_bound(roots["ssr2"][v], d_ssr2)
            for metric, b in per_sample.items():                     # (R, S, T) -> mean over the samples
                for r, region in enumerate(regions):
                    out.setdefault(f"{metric}/{region}/{name}", np.zeros(n_timesteps))[start:start + T] = b[r].mean(axis=0)
    return out


def check_series(got, want, bounds, what):
    """Every key of `want`: |got - want| <= bound at every time; prints the worst fraction per metric."""
    assert set(want) <= set(got), sorted(set(want) - set(got))[:5]
    worst = {}
    for key, w in want.items():
        g = np.asarray(got[key], np.float64)
        assert g.shape == w.shape and np.isfinite(g).all(), key
        frac = float((np.abs(g - w) / bounds[key]).max())
        metric = key.split("/")[0]
        worst[metric] = max(worst.get(metric, 0.0), frac)
        assert frac <= 1.0, f"{what} {key}: {frac:.3f} of the bound (max |diff| {np.abs(g - w).max():.3e})"
    for metric, frac in worst.items():
        print(f"{what} {metric}: worst {frac:.3e} of the bound")


def check_sums_reordered(got, want, abs_sums, HW, what):
    """Raw sums of two float64 paths that add the same terms in another order: HW 2^-53 sum w |q| per sum."""
    bound = HW * 2.0 ** -53 * abs_sums
    err = np.abs(got - want)
    assert np.isfinite(got).all(), what
    with np.errstate(divide="ignore", invalid="ignore"):
        frac = np.where(bound > 0.0, err / bound, np.where(err == 0.0, 0.0, np.inf))
    print(f"{what}: worst {float(frac.max()):.3e} of the bound HW 2^-53 sum w |q|")
    assert (err <= bound).all(), f"{what}: {float(frac.max()):.3f} of the bound"


def check_sums_restated(got, want, scales, weights, what, rel=1e-12):
    """Raw sums against the restatement: rel x term scale x W_r per sum."""
    wsum = weight_sums(weights)
    assert np.isfinite(got).all(), what
    for v, sc in enumerate(scales):
        bound = rel * term_scale(sc)[None, None, None, :] * wsum[:, None, None, None]
        err = np.abs(got[v] - want[v])
        print(f"{what} var {v}: worst {float((err / bound).max()):.3e} of the bound")
        assert (err <= bound).all(), f"{what} var {v}: {float((err / bound).max()):.3f} of the bound"
