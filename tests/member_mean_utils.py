"""Shared by tests/test_member_mean_host.py and tests/test_gpu_member_mean.py: the fixture of the reference's ensemble
TimeMeanAggregator (tests/golden/fx_time_mean_ensemble.npz; tools/gen_golden_time_mean_ensemble.py), the library's _host entry
points driven from numpy, a float64 restatement of the accumulators and of the statistics, and the comparison bounds.

Bounds (u = 2^-24; S counted times, M members, B samples).  Every statistic is a weighted mean of per-point terms, and a bound
is a multiple of the statistic's TERM SCALE: max (g_m - t)^2 for the mean squared errors, max |g_m - t| for the biases, max
|g_m - t| + max |g_i - g_j| for the CRPS, maxima over members, samples and grid points of the float64 time means.  Root mean
squared errors are compared as squares.  `rmse_member_avg` is a mean of roots r_m; its square moves by 2 r mean(d(mse_m) / (2
r_m)), which is mean d(mse_m) for members of like error (they are: one noise level), so it takes the bound of a mean squared
error.
  * against `ref64`, the reference's class on the inputs cast to float64 (the yardstick): 1e-12 x term scale, the bound
    field_stats_utils.check_close uses;
  * against `ref32`, what the reference returns (a sanity check against fp32, not the pin): the reference's own worst-case
    fp32 summation error (S + M + B H W + 4) u x term scale, plus the fp32 error of the time mean itself, 2 (S + 2) u max|x|
    (times 2 max |g_m - t| for the squares);
  * `spread` / `ssr` (this library's own) against the restatement: spread^2 = mean variance (M + 1) / M with terms up to max
    (g_i - g_j)^2 (M + 1) / M.  A deviation from the ensemble mean also carries the float64 rounding of the mean and of the
    subtractions, eps = 4 x 2^-53 max |g_m - t| whatever the spread (all that is left when the members are equal), so a
    squared deviation moves by 2 max |g_i - g_j| eps + eps^2 on top; ssr^2 = spread^2 / mse moves by (d spread^2 + ssr^2 d
    mse) / mse.
"""
import ctypes as C
import json

import numpy as np

import golden_utils as gu
from window_utils import fill_window, vp

U = 2.0 ** -24


def cases():
    """-> {case: dict(M, B, H, W, names, weights (H, W) float32, windows=[(i_time_start, target {name: (B, T, H, W)}, gen
    {name: (M, B, T, H, W)})], S=counted times, keys=the reference's log keys in its order, ref32 / ref64 = {key: float})}."""
    z = gu.load("fx_time_mean_ensemble")
    out = {}
    for c in json.loads(str(z["cases"])):
        name, names = c["name"], c["names"]
        windows, start = [], 0
        for i, n in enumerate(c["counted"]):
            target = {k: z[f"{name}::w{i}::target::{k}"] for k in names}
            gen = {k: z[f"{name}::w{i}::gen::{k}"] for k in names}
            windows.append((start, target, gen))
            start += target[names[0]].shape[1]
        out[name] = dict(M=c["M"], B=c["B"], H=c["H"], W=c["W"], names=names, weights=z[f"{name}::weights"], windows=windows,
                         S=sum(c["counted"]), keys=c["keys"], ref32=dict(zip(c["keys"], z[f"{name}::ref32"].tolist())),
                         ref64=dict(zip(c["keys"], z[f"{name}::ref64"].tolist())))
    return out


def seeded_case(M, B, H, W, counted, names, seed):
    """A case of the fixture's kind from seeded numpy (no reference values)."""
    rng = np.random.default_rng(seed)
    lat = (np.arange(H) + 0.5) / H * np.pi - np.pi / 2
    weights = (np.cos(lat)[:, None] * (1.0 + 0.1 * rng.random((H, W)))).astype(np.float32)
    S = sum(counted)
    target, gen = {}, {}
    for k in names:
        clim = 280.0 + 20.0 * rng.standard_normal((H, W))
        target[k] = (clim + 3.0 * rng.standard_normal((B, S + 1, H, W))).astype(np.float32)
        gen[k] = (clim + 3.0 * rng.standard_normal((M, B, S + 1, H, W)) + 0.5).astype(np.float32)
    windows, done = [], 0
    for i, n in enumerate(counted):
        first = 0 if i == 0 else done + 1
        windows.append((first, {k: target[k][:, first:done + n + 1] for k in names},
                        {k: gen[k][:, :, first:done + n + 1] for k in names}))
        done += n
    return dict(M=M, B=B, H=H, W=W, names=list(names), weights=weights, windows=windows, S=S)


def restate_sums(case, windows=None):
    """-> (gen_sum (nvars, M, B, H, W), target_sum (nvars, B, H, W), n_times): float64, every window's times added in ascending
    order and the window's sum then added to the running one -- the order include/sdy_amd.h fixes, so these are the bits."""
    names = case["names"]
    gen_sum = np.zeros((len(names), case["M"], case["B"], case["H"], case["W"]))
    target_sum = np.zeros((len(names), case["B"], case["H"], case["W"]))
    n_times = 0
    for start, target, gen in (case["windows"] if windows is None else windows):
        t0 = 1 if start == 0 else 0
        T = target[names[0]].shape[1]
        for j, k in enumerate(names):
            g = gen[k] if gen[k].ndim == 5 else gen[k][None]
            sg, st = np.zeros(gen_sum.shape[1:]), np.zeros(target_sum.shape[1:])
            for t in range(t0, T):
                sg += g[:, :, t].astype(np.float64)
                st += target[k][:, t].astype(np.float64)
            gen_sum[j] += sg
            target_sum[j] += st
        n_times += T - t0
    return gen_sum, target_sum, n_times


def restate_stats(gen_sum, target_sum, weights, n_times):
    """-> (raw (nvars, 2 M + 4) weighted sums as sdy_member_map_stats defines them, scales [per variable dict of term scales])."""
    nvars, M = gen_sum.shape[:2]
    w = weights.astype(np.float64)
    raw, scales = np.zeros((nvars, 2 * M + 4)), []
    for j in range(nvars):
        g, t = gen_sum[j] / n_times, target_sum[j] / n_times
        d = g - t
        raw[j, :M] = (w * d * d).sum(axis=(1, 2, 3))
        raw[j, M:2 * M] = (w * d).sum(axis=(1, 2, 3))
        em = g.mean(axis=0) - t
        raw[j, 2 * M] = (w * em * em).sum()
        raw[j, 2 * M + 1] = (w * em).sum()
        pair = np.abs(g[None] - g[:, None])
        crps = np.abs(d).mean(axis=0)
        var = np.zeros_like(t)
        if M > 1:
            crps = crps - pair.sum(axis=(0, 1)) / (2 * M * (M - 1))
            var = g.var(axis=0, ddof=1)
        raw[j, 2 * M + 2] = (w * crps).sum()
        raw[j, 2 * M + 3] = (w * var).sum()
        scales.append(dict(sq=float((d * d).max()), abs=float(np.abs(d).max()), pair=float(pair.max())))
    return raw, scales


def logs_from_raw(raw, names, B, weights, spread=False):
    """EnsembleTimeMeanAggregator.get_logs("") from the raw sums, in float64 numpy."""
    den = B * weights.astype(np.float64).sum()
    M = (raw.shape[1] - 4) // 2
    logs = {}
    for j, k in enumerate(names):
        s = raw[j] / den
        if M > 1:
            logs[f"rmse_member_avg/{k}"] = float(np.sqrt(s[:M]).mean())
            logs[f"bias_member_avg/{k}"] = float(s[M:2 * M].mean())
        logs[f"rmse/{k}"] = float(np.sqrt(s[2 * M]))
        logs[f"bias/{k}"] = float(s[2 * M + 1])
        if M > 1:
            logs[f"crps/{k}"] = float(s[2 * M + 2])
        if spread:
            logs[f"spread/{k}"] = float(np.sqrt(s[2 * M + 3] * (M + 1) / M))
            logs[f"ssr/{k}"] = logs[f"spread/{k}"] / logs[f"rmse/{k}"]
    return logs


def restate(case, spread=False):
    """-> (logs, scales, max|x|) of a case from the float64 restatement."""
    gen_sum, target_sum, n_times = restate_sums(case)
    raw, scales = restate_stats(gen_sum, target_sum, case["weights"], n_times)
    xmax = max(float(np.abs(d[k]).max()) for _, t, g in case["windows"] for d in (t, g) for k in case["names"])
    return logs_from_raw(raw, case["names"], case["B"], case["weights"], spread), scales, xmax


def sum_args(target, gen, names, t0, gen_sum, target_sum):
    """SdyMemberSumArgs over contiguous numpy arrays (gen 4-D or member-stacked 5-D); -> (args, keep-alive list)."""
    from sdy_amd._lib import SdyMemberSumArgs

    a = SdyMemberSumArgs()
    keep, (H, W) = fill_window(a.win, target, gen, names)
    a.HW, a.t0 = H * W, t0
    a.gen_sum, a.target_sum = vp(gen_sum), vp(target_sum)
    return a, keep


def host_sums(case, windows=None):
    """The case through sdy_member_time_sum_host -> (gen_sum, target_sum, n_times), shaped as restate_sums gives them."""
    import sdy_amd

    names = case["names"]
    gen_sum = np.zeros((len(names), case["M"], case["B"], case["H"], case["W"]))
    target_sum = np.zeros((len(names), case["B"], case["H"], case["W"]))
    n_times = 0
    for start, target, gen in (case["windows"] if windows is None else windows):
        t0 = 1 if start == 0 else 0
        a, keep = sum_args(target, gen, names, t0, gen_sum, target_sum)
        assert sdy_amd.lib.sdy_member_time_sum_host(C.byref(a)) == 0
        n_times += a.T - t0
    return gen_sum, target_sum, n_times


def stats_args(gen_sum, target_sum, weights, n_times, out):
    from sdy_amd._lib import SdyMemberStatsArgs

    a = SdyMemberStatsArgs()
    a.nvars, a.M, a.n1 = gen_sum.shape[:3]
    a.HW = gen_sum.shape[3] * gen_sum.shape[4]
    w = np.ascontiguousarray(weights, np.float32)
    a.gen_sum, a.target_sum, a.weights, a.n_times, a.out = vp(gen_sum), vp(target_sum), vp(w), float(n_times), vp(out)
    return a, [w]


def host_stats(gen_sum, target_sum, weights, n_times):
    """sdy_member_map_stats_host -> raw (nvars, 2 M + 4)."""
    import sdy_amd

    out = np.full((gen_sum.shape[0], 2 * gen_sum.shape[1] + 4), np.nan)
    a, keep = stats_args(gen_sum, target_sum, weights, n_times, out)
    assert sdy_amd.lib.sdy_member_map_stats_host(C.byref(a)) == 0
    return out


def _kind(key):
    return key.split("/")[0]


def _within(got, want, bound, what):
    err = abs(got - want)
    frac = err / bound if bound > 0.0 else (0.0 if err == 0.0 else float("inf"))
    print(f"{what}: |diff| {err:.3e}, {frac:.3f} of the bound {bound:.3e}")
    assert err <= bound, f"{what}: {err:.3e} is {frac:.3f} of the bound"


def check_logs(case, logs, ref, rel, tag, xmax=None, scales=None):
    """`logs` against `ref` ({key: float}), every reference key: |diff| <= rel x term scale (+ the time mean's fp32 error when
    `xmax` is given: the ref32 comparison)."""
    if scales is None:
        _, scales, _ = restate(case)
    S = case["S"]
    for key, want in ref.items():
        kind, name = _kind(key), key.split("/", 1)[1]
        sc = scales[case["names"].index(name)]
        mean_err = 0.0 if xmax is None else 2 * (S + 2) * U * xmax
        got = logs[key]
        if kind in ("rmse", "rmse_member_avg"):
            _within(got ** 2, want ** 2, rel * sc["sq"] + mean_err * 2 * sc["abs"], f"{tag} ({key})^2")
        elif kind in ("bias", "bias_member_avg"):
            _within(got, want, rel * sc["abs"] + mean_err, f"{tag} {key}")
        else:
            assert kind == "crps", key
            _within(got, want, rel * (sc["abs"] + sc["pair"]) + mean_err, f"{tag} {key}")


def check_against_reference(case, logs, tag):
    """The two comparisons of the module docstring, and the reference's key order."""
    assert [k for k in logs if _kind(k) not in ("spread", "ssr")] == case["keys"], (list(logs), case["keys"])
    _, scales, xmax = restate(case)
    check_logs(case, logs, case["ref64"], 1e-12, f"{tag} vs ref64", scales=scales)
    n = case["S"] + case["M"] + case["B"] * case["H"] * case["W"] + 4
    check_logs(case, logs, case["ref32"], n * U, f"{tag} vs ref32", xmax=xmax, scales=scales)


def check_spread(case, logs, want, tag):
    """spread / ssr of `logs` against the restatement's `want` (module docstring)."""
    _, scales, _ = restate(case)
    M = case["M"]
    for j, k in enumerate(case["names"]):
        eps = 4 * 2.0 ** -53 * scales[j]["abs"]
        d_spread2 = (1e-12 * scales[j]["pair"] ** 2 + 2 * scales[j]["pair"] * eps + eps ** 2) * (M + 1) / M
        _within(logs[f"spread/{k}"] ** 2, want[f"spread/{k}"] ** 2, d_spread2, f"{tag} (spread/{k})^2")
        mse, ssr2 = want[f"rmse/{k}"] ** 2, want[f"ssr/{k}"] ** 2
        _within(logs[f"ssr/{k}"] ** 2, ssr2, (d_spread2 + ssr2 * 1e-12 * scales[j]["sq"]) / mse, f"{tag} (ssr/{k})^2")


def check_raw(got, want, scales, weight_total, what, rel=1e-12):
    """Raw weighted sums of two paths (nvars, 2 M + 4): |diff| <= rel x term scale x weight_total, weight_total = n1 sum(w) --
    the ref64 bound before the division by the total weight.  The variance slot's terms reach max (g_i - g_j)^2."""
    M = (want.shape[1] - 4) // 2
    kinds = {"sq": list(range(M)) + [2 * M], "bias": list(range(M, 2 * M)) + [2 * M + 1], "crps": [2 * M + 2], "var": [2 * M + 3]}
    for j in range(want.shape[0]):
        sc = scales[j]
        term = {"sq": sc["sq"], "bias": sc["abs"], "crps": sc["abs"] + sc["pair"], "var": sc["pair"] ** 2}
        for kind, slots in kinds.items():
            assert np.isfinite(got[j, slots]).all(), f"{what} var {j} {kind}"
            err = float(np.abs(got[j, slots] - want[j, slots]).max())
            bound = rel * term[kind] * weight_total
            print(f"{what} var {j} {kind}: max |diff| {err:.3e}, {err / bound if bound else 0.0:.3f} of the bound {bound:.3e}")
            assert err <= bound, f"{what} var {j} {kind}: {err:.3e} > {bound:.3e}"
