"""Shared by tests/test_variability_host.py and tests/test_gpu_variability.py: seeded cases, the library's _host entry points
driven from numpy, a float64 numpy restatement of the state, the maps, the weighted sums and the logs, exact rational
arithmetic on the fp32 inputs, and the comparison bounds.  The reference has nothing of the kind: the yardstick is exact
arithmetic on the inputs.

State of one trajectory (a member of a sample, or a sample's target) at one grid point, counted times x_1 .. x_n (fp32):
  c = x_1, d_t = (double)x_t - (double)c, S1 = sum d_t, S2 = sum d_t^2, P = sum_{t >= 2} d_{t-1} d_t, last = x_n,
every term added to the running value in ascending time (csrc/variability.h).  Arrays: `s1`, `s2`, `p` float64
`(nvars, M B + B, H, W)` -- row i0 B + i1 is member i0 of sample i1, rows M B + i1 are the targets -- and `pair` float32
`(nvars, M B + B, H, W, 2)` = (c, last).

Bounds (u = 2^-53; n counted times).
  * Device state against the _host twin's, the _host twin's against the restatement (`restate_state`, which adds in the same
    order), device maps against _host maps: the same bits.
  * Restatement against exact rational arithmetic (`exact_point`).  The deviations d_t are exact in float64 (two fp32 values
    whose exponents differ by less than 29).  A raw sum is a recursive float64 sum of n terms, each the exact d_t or a product
    rounded once: |computed - exact| <= gamma_n sum |terms| <= (n + 1) u sum |terms| (Higham, Accuracy and Stability of
    Numerical Algorithms, section 4.2; gamma_n = n u / (1 - n u)).
    variance = (S2 - S1 m) / n with m = S1 / n; exactly it is S2 / n - m^2.  The S2 / n part carries the sum's n u S2 / n and
    the roundings of the subtraction and of the division: (n + 2) u S2 / n.  For the m^2 part |dS1| <= (n - 1) u sum |d_t| <=
    (n - 1) u sqrt(n S2) (Cauchy-Schwarz), so S1^2 / n^2 moves by 2 |m| (n - 1) u sqrt(S2 / n) <= (n - 1) u (m^2 + S2 / n),
    and the division S1 / n, the product S1 m, the subtraction and the division by n add 4 u m^2.  Together
    (2 n + 1) u S2 / n + (n + 3) u m^2 <= 2 (n + 3) u (S2 / n + m^2); the clamp at 0 only moves towards the exact value.
  * Device `stats` against _host `stats` and against the restatement (another summation order): 1e-12 x term scale x total
    weight, total weight = B sum(w), the rule of member_mean_utils.check_raw / field_stats_utils.check_close.  Term scales: the
    largest variance (slots 0, 1), the largest (mean_m sd_gen - sd_target)^2 (slot 2), 1 for the lag-1 slots (|lag1| <= 1) and
    the weight slot.
  * Logs: a mean variance is a raw sum over the total weight: 1e-12 x its term scale, roots compared as squares;
    `time_std_ratio`^2 = a / b moves by (da + ratio^2 db) / b; a lag-1 mean is slot / weight slot and moves by 2e-12 / (defined
    fraction), `lag1_bias` by twice that; `lag1_defined_fraction` by 1e-12.
"""
import ctypes as C
from fractions import Fraction

import numpy as np

from window_utils import fill_window, vp

U = 2.0 ** -53
SLOTS = 6
LOG_KEYS = ("time_std_gen", "time_std_target", "time_std_ratio", "time_std_rmse", "lag1_gen", "lag1_target", "lag1_bias",
            "lag1_defined_fraction")
#: the independent time loads of a thread of variability_kernel (kTimesInFlight, csrc/variability.hip); the windowing case has a
#: window of IN_FLIGHT + 1 counted times, one more than a batch
IN_FLIGHT = 6


def seeded_series(M, B, H, W, S, names, seed, mean=280.0, std=3.0, phi=0.6, bias=0.5, spread=20.0):
    """-> dict(M, B, H, W, names, weights (H, W) float32, S, target {name: (B, S + 1, H, W)}, gen {name: (M, B, S + 1, H, W)}):
    AR(1) series along time (coefficient phi, stationary standard deviation std) around a climatology `mean` +- `spread`, float32;
    time 0 is the initial condition."""
    rng = np.random.default_rng(seed)
    lat = (np.arange(H) + 0.5) / H * np.pi - np.pi / 2
    weights = (np.cos(lat)[:, None] * (1.0 + 0.1 * rng.random((H, W)))).astype(np.float32)

    def ar1(shape):                      # time on axis -3
        e = rng.standard_normal(shape)
        x = np.empty(shape)
        x[..., 0, :, :] = e[..., 0, :, :]
        for t in range(1, shape[-3]):
            x[..., t, :, :] = phi * x[..., t - 1, :, :] + np.sqrt(1.0 - phi * phi) * e[..., t, :, :]
        return x

    target, gen = {}, {}
    for k in names:
        clim = mean + spread * rng.standard_normal((H, W))
        target[k] = (clim + std * ar1((B, S + 1, H, W))).astype(np.float32)
        gen[k] = (clim + bias + 0.8 * std * ar1((M, B, S + 1, H, W))).astype(np.float32)
    return dict(M=M, B=B, H=H, W=W, names=list(names), weights=weights, S=S, target=target, gen=gen)


def cut(case, lengths, start=0):
    """The series as windows of `lengths` times each (the initial condition included in the count when start == 0) ->
    [(i_time_start, target {name: (B, T, H, W)}, gen {name: (M, B, T, H, W)})]; the run's times start .. start + sum(lengths)."""
    out, at = [], start
    for n in lengths:
        out.append((at, {k: v[:, at:at + n] for k, v in case["target"].items()},
                    {k: v[:, :, at:at + n] for k, v in case["gen"].items()}))
        at += n
    assert at <= case["S"] + 1
    return out


def rows_of(target, gen):
    """One variable's window as state rows: (M B + B, T, H, W), generated rows first."""
    g = gen if gen.ndim == 5 else gen[None]
    return np.concatenate([g.reshape(-1, *g.shape[2:]), target], axis=0)


def empty_state(nvars, M, B, H, W, fill=0.0):
    rows = M * B + B
    return dict(s1=np.full((nvars, rows, H, W), fill), s2=np.full((nvars, rows, H, W), fill), p=np.full((nvars, rows, H, W), fill),
                pair=np.full((nvars, rows, H, W, 2), fill, np.float32))


def same_state(a, b):
    """The same bits (NaNs in the same places)."""
    return all(np.array_equal(a[k], b[k], equal_nan=True) for k in ("s1", "s2", "p", "pair"))


def restate_state(case, windows):
    """-> (state, n): float64 numpy, every counted time's term added to the running value in ascending time -- the order
    csrc/variability.h fixes, so these are the bits."""
    names = case["names"]
    st = empty_state(len(names), case["M"], case["B"], case["H"], case["W"])
    n = 0
    for start, target, gen in windows:
        t0 = 1 if start == 0 else 0
        T = target[names[0]].shape[1]
        for j, k in enumerate(names):
            x = rows_of(target[k], gen[k])
            if n == 0 and T > t0:
                st["pair"][j, ..., 0] = x[:, t0]
            c = st["pair"][j, ..., 0].astype(np.float64)
            d_prev = st["pair"][j, ..., 1].astype(np.float64) - c
            for i, t in enumerate(range(t0, T)):
                d = x[:, t].astype(np.float64) - c
                st["s1"][j] = st["s1"][j] + d
                st["s2"][j] = st["s2"][j] + d * d
                if n + i > 0:
                    st["p"][j] = st["p"][j] + d_prev * d
                d_prev = d
                st["pair"][j, ..., 1] = x[:, t]
        n += T - t0
    return st, n


def accumulate_args(target, gen, names, t0, first, st):
    """SdyVariabilityArgs over contiguous numpy arrays (gen 4-D or member-stacked 5-D); -> (args, keep-alive list)."""
    from sdy_amd._lib import SdyVariabilityArgs

    a = SdyVariabilityArgs()
    keep, (H, W) = fill_window(a.win, target, gen, names)
    a.HW, a.t0, a.first = H * W, t0, int(first)
    a.s1, a.s2, a.p, a.origin_last = vp(st["s1"]), vp(st["s2"]), vp(st["p"]), vp(st["pair"])
    return a, keep


def host_state(case, windows):
    """The windows through sdy_time_variability_accumulate_host -> (state, n), shaped as restate_state gives them."""
    import sdy_amd

    names = case["names"]
    st = empty_state(len(names), case["M"], case["B"], case["H"], case["W"])
    n = 0
    for start, target, gen in windows:
        t0 = 1 if start == 0 else 0
        T = target[names[0]].shape[1]
        if T - t0 < 1:
            continue
        a, keep = accumulate_args(target, gen, names, t0, n == 0, st)
        assert sdy_amd.lib.sdy_time_variability_accumulate_host(C.byref(a)) == 0
        n += T - t0
    return st, n


def restate_maps(st, n):
    """-> (V, variance, lag1) of every state element, the operations of sdy_tv_finish in its order."""
    s1, s2, p = st["s1"], st["s2"], st["p"]
    n = float(n)
    with np.errstate(invalid="ignore", divide="ignore"):
        m = s1 / n
        v = s2 - s1 * m
        V = np.where(v < 0.0, 0.0, v)
        variance = V / n
        dn = st["pair"][..., 1].astype(np.float64) - st["pair"][..., 0].astype(np.float64)
        cov = (p - m * ((s1 - dn) + s1)) + ((n - 1.0) * m) * m
        lag1 = np.where((n >= 2.0) & (V > 0.0), cov / V, np.nan)
    return V, variance, lag1


def maps_args(st, n, variance, lag1):
    from sdy_amd._lib import SdyVariabilityMapsArgs

    a = SdyVariabilityMapsArgs()
    a.n_elems, a.n_times = st["s1"].size, float(n)
    a.s1, a.s2, a.p, a.origin_last = vp(st["s1"]), vp(st["s2"]), vp(st["p"]), vp(st["pair"])
    a.variance, a.lag1 = vp(variance), vp(lag1)
    return a


def host_maps(st, n):
    """sdy_time_variability_maps_host -> (variance, lag1), shaped as the state."""
    import sdy_amd

    variance, lag1 = np.full(st["s1"].shape, 7.0), np.full(st["s1"].shape, 7.0)
    assert sdy_amd.lib.sdy_time_variability_maps_host(C.byref(maps_args(st, n, variance, lag1))) == 0
    return variance, lag1


def restate_stats(st, weights, n, M, B):
    """-> (raw (nvars, 6) weighted sums as sdy_time_variability_stats defines them, scales [per variable the slots' term scales])."""
    V, variance, lag1 = restate_maps(st, n)
    nvars, _, H, W = V.shape
    w = weights.astype(np.float64)
    raw, scales = np.zeros((nvars, SLOTS)), []
    for j in range(nvars):
        gV, tV = V[j, :M * B].reshape(M, B, H, W), V[j, M * B:]
        gvar, tvar = variance[j, :M * B].reshape(M, B, H, W), variance[j, M * B:]
        glag, tlag = lag1[j, :M * B].reshape(M, B, H, W), lag1[j, M * B:]
        mean_var = gvar.sum(axis=0) / M
        sd_diff = np.sqrt(gvar).sum(axis=0) / M - np.sqrt(tvar)
        defined = (n >= 2) & (tV > 0.0) & (gV > 0.0).all(axis=0)
        mean_lag = np.where(defined, glag.sum(axis=0) / M, 0.0)
        raw[j] = [(w * mean_var).sum(), (w * tvar).sum(), (w * (sd_diff * sd_diff)).sum(), (w * mean_lag).sum(),
                  (w * np.where(defined, tlag, 0.0)).sum(), (w * defined).sum()]
        var_scale = float(max(np.nanmax(gvar), np.nanmax(tvar)))
        scales.append([var_scale, var_scale, float(np.nanmax(sd_diff * sd_diff)), 1.0, 1.0, 1.0])
    return raw, scales


def stats_args(st, weights, n, M, B, out):
    from sdy_amd._lib import SdyVariabilityStatsArgs

    a = SdyVariabilityStatsArgs()
    a.nvars, a.M, a.n1, a.HW = st["s1"].shape[0], M, B, st["s1"].shape[2] * st["s1"].shape[3]
    w = np.ascontiguousarray(weights, np.float32)
    a.s1, a.s2, a.p, a.origin_last = vp(st["s1"]), vp(st["s2"]), vp(st["p"]), vp(st["pair"])
    a.weights, a.n_times, a.out = vp(w), float(n), vp(out)
    return a, [w]


def host_stats(st, weights, n, M, B):
    """sdy_time_variability_stats_host -> raw (nvars, 6)."""
    import sdy_amd

    out = np.full((st["s1"].shape[0], SLOTS), np.nan)
    a, keep = stats_args(st, weights, n, M, B, out)
    assert sdy_amd.lib.sdy_time_variability_stats_host(C.byref(a)) == 0
    return out


def weight_total(case):
    return case["B"] * float(case["weights"].astype(np.float64).sum())


def logs_from_raw(raw, names, total):
    """TimeVariabilityAggregator.get_logs("") from the raw sums and the total weight, in float64 numpy."""
    logs = {}
    for j, k in enumerate(names):
        s = raw[j]
        with np.errstate(invalid="ignore", divide="ignore"):
            sg, stg = np.sqrt(s[0] / total), np.sqrt(s[1] / total)
            vals = [sg, stg, sg / stg if stg > 0.0 else np.nan, np.sqrt(s[2] / total)]
            lg, lt = (s[3] / s[5], s[4] / s[5]) if s[5] > 0.0 else (np.nan, np.nan)
            vals += [lg, lt, lg - lt, s[5] / total]
        logs.update({f"{key}/{k}": float(v) for key, v in zip(LOG_KEYS, vals)})
    return logs


def within(got, want, bound, what):
    err = abs(got - want)
    frac = err / bound if bound > 0.0 else (0.0 if err == 0.0 else float("inf"))
    print(f"{what}: |diff| {err:.3e}, {frac:.3f} of the bound {bound:.3e}")
    assert err <= bound, f"{what}: {err:.3e} is {frac:.3f} of the bound"


def check_raw(got, want, scales, total, what, rel=1e-12):
    """Raw weighted sums of two paths (nvars, 6): |diff| <= rel x term scale x total weight."""
    for j in range(want.shape[0]):
        for slot in range(SLOTS):
            assert np.isfinite(got[j, slot]), f"{what} var {j} slot {slot}"
            within(float(got[j, slot]), float(want[j, slot]), rel * scales[j][slot] * total, f"{what} var {j} slot {slot}")


def check_logs(logs, want, names, scales, what, rel=1e-12):
    """`logs` against the restatement's `want`: keys in order, Python floats, and the bounds of the module docstring."""
    assert list(logs) == list(want) == [f"{key}/{k}" for k in names for key in LOG_KEYS], list(logs)
    assert all(type(v) is float for v in logs.values())
    for j, k in enumerate(names):
        g = lambda key: logs[f"{key}/{k}"]      # noqa: E731
        r = lambda key: want[f"{key}/{k}"]      # noqa: E731
        d_var, d_sd = rel * scales[j][0], rel * scales[j][2]
        within(g("time_std_gen") ** 2, r("time_std_gen") ** 2, d_var, f"{what} (time_std_gen/{k})^2")
        within(g("time_std_target") ** 2, r("time_std_target") ** 2, d_var, f"{what} (time_std_target/{k})^2")
        within(g("time_std_rmse") ** 2, r("time_std_rmse") ** 2, d_sd, f"{what} (time_std_rmse/{k})^2")
        ratio2 = r("time_std_ratio") ** 2
        within(g("time_std_ratio") ** 2, ratio2, (d_var + ratio2 * d_var) / r("time_std_target") ** 2,
               f"{what} (time_std_ratio/{k})^2")
        frac = r("lag1_defined_fraction")
        within(g("lag1_defined_fraction"), frac, rel, f"{what} lag1_defined_fraction/{k}")
        for key, mult in (("lag1_gen", 2.0), ("lag1_target", 2.0), ("lag1_bias", 4.0)):
            within(g(key), r(key), mult * rel / frac, f"{what} {key}/{k}")


# ---- exact rational arithmetic ------------------------------------------------------------------------------------------------
def exact_point(x):
    """x: the counted fp32 values of one trajectory at one grid point, in run order -> dict of exact Fractions: s1, s2, p, their
    sums of |terms| (abs1, abs2, absp), m = S1 / n, variance = S2 / n - m^2, and the same from the raw values."""
    xs = [Fraction(float(v)) for v in x]
    n = len(xs)
    d = [v - xs[0] for v in xs]
    s1, s2 = sum(d), sum(v * v for v in d)
    p = sum(a * b for a, b in zip(d[:-1], d[1:]))
    m = s1 / n
    return dict(n=n, s1=s1, s2=s2, p=p, abs1=sum(abs(v) for v in d), abs2=s2, absp=sum(abs(a * b) for a, b in zip(d[:-1], d[1:])),
                m=m, variance=s2 / n - m * m)


def check_point_exact(x, s1, s2, p, variance, what):
    """The float64 sums and the variance of one trajectory and point against exact arithmetic on its fp32 values `x`: the bounds
    of the module docstring; -> (exact variance as float, the variance bound)."""
    e = exact_point(x)
    n = e["n"]
    for name, got, exact, total in (("S1", s1, e["s1"], e["abs1"]), ("S2", s2, e["s2"], e["abs2"]), ("P", p, e["p"], e["absp"])):
        within(float(abs(Fraction(float(got)) - exact)), 0.0, float((n + 1) * Fraction(U) * total), f"{what} {name} vs exact")
    bound = float(2 * (n + 3) * Fraction(U) * (e["s2"] / n + e["m"] ** 2))
    within(float(abs(Fraction(float(variance)) - e["variance"])), 0.0, bound, f"{what} variance vs exact")
    return float(e["variance"]), bound
