"""What the time-bin tests share: seeded cases, the cut of a run into windows, the way through the _host twin
(sdy_binned_time_accumulate_host on numpy arrays) and the numpy float64 restatement of the aggregator's read-outs.

A case is a run: gen[name] (M, B, S + 1, H, W) fp32 and target[name] (B, S + 1, H, W) fp32 over the global times 0 .. S (time 0
is the initial condition), weights (H, W) fp32.  The state of a run of same-shaped variables is laid out as the kernel's:
gen (n_bins, nvars, rows, H, W) with rows = M * B (pooled: B), target (n_bins, nvars, B, H, W)."""
import ctypes as C

import numpy as np

SDY_OK, SDY_ERR_ARG, SDY_ERR_UNSUPPORTED = 0, -1, -2
# the windowing case: the initial condition alone, then windows of 1, 1, 3 and 7 counted times
SPLIT = [1, 1, 1, 3, 7]


def seeded_case(M, B, H, W, S, names, seed, integer=False, mean=0.0, std=1.0):
    """integer=True: multiples of 2^-10 below 2^20 in magnitude, whose float64 sums are exact in any order."""
    rng = np.random.default_rng(seed)

    def field(*shape):
        if integer:
            return (rng.integers(-(1 << 29), 1 << 29, size=shape).astype(np.float64) / 1024.0).astype(np.float32)
        return (mean + std * rng.standard_normal(shape)).astype(np.float32)

    lat = np.linspace(-85.0, 85.0, H)
    weights = np.repeat(np.cos(np.deg2rad(lat))[:, None], W, axis=1).astype(np.float32)
    return dict(M=M, B=B, H=H, W=W, S=S, names=list(names), weights=weights,
                gen={k: field(M, B, S + 1, H, W) for k in names}, target={k: field(B, S + 1, H, W) for k in names})


def cut(case, sizes, start=0):
    """Windows of `sizes` times from global time `start`: [(start, target, gen)] with views of the case."""
    out = []
    for n in sizes:
        out.append((start, {k: v[:, start:start + n] for k, v in case["target"].items()},
                    {k: v[:, :, start:start + n] for k, v in case["gen"].items()}))
        start += n
    return out


def empty_state(case, n_bins, per_member=True):
    n, M, B, H, W = len(case["names"]), case["M"], case["B"], case["H"], case["W"]
    rows = M * B if per_member else B
    return {"gen_sum": np.zeros((n_bins, n, rows, H, W)), "target_sum": np.zeros((n_bins, n, B, H, W)),
            "gen_max": np.full((n_bins, n, rows, H, W), -np.inf, np.float32),
            "gen_min": np.full((n_bins, n, rows, H, W), np.inf, np.float32),
            "target_max": np.full((n_bins, n, B, H, W), -np.inf, np.float32),
            "target_min": np.full((n_bins, n, B, H, W), np.inf, np.float32)}


def host_args(target, gen, state, n_bins, groups, per_member=True, extremes=True):
    """The argument structure of one call on host arrays: target {name: (B, T, H, W)}, gen {name: (M, B, T, H, W)}, both
    C-contiguous fp32.  -> (args, what has to stay alive)."""
    from sdy_amd import _lib, time_bins

    names = list(gen)
    keep = [np.ascontiguousarray(gen[k], np.float32) for k in names] + [np.ascontiguousarray(target[k], np.float32) for k in names]
    M, B, T, H, W = keep[0].shape
    a = _lib.SdyBinnedSumArgs()
    a.nvars = len(names)
    for j in range(len(names)):
        a.gen[j], a.target[j] = keep[j].ctypes.data, keep[len(names) + j].ctypes.data
    a.n0, a.n1, a.T, a.gs0, a.gs1, a.ts1 = M, B, T, B * T * H * W, T * H * W, T * H * W
    a.HW, a.n_bins, a.bin_vars, a.pool_members = H * W, n_bins, len(names), int(not per_member)
    time_bins.fill_groups(a, groups)
    a.gen_sum, a.target_sum = state["gen_sum"].ctypes.data, state["target_sum"].ctypes.data
    if extremes:
        for k in ("gen_max", "gen_min", "target_max", "target_min"):
            setattr(a, k, state[k].ctypes.data)
    return a, keep


def host_state(case, windows, labels, n_bins, per_member=True, extremes=True, reorder=None):
    """The run through sdy_binned_time_accumulate_host -> (state, counts).  reorder(groups) -> the groups of a call in another
    order (the bits must not depend on it)."""
    import sdy_amd
    from sdy_amd import time_bins

    state = empty_state(case, n_bins, per_member)
    counts = [0] * n_bins
    for start, target, gen in windows:
        T = next(iter(target.values())).shape[1]
        for groups in time_bins.group_times(labels[start:start + T], 1 if start == 0 else 0):
            if reorder is not None:
                groups = reorder(groups)
            a, keep = host_args(target, gen, state, n_bins, groups, per_member, extremes)
            assert sdy_amd.lib.sdy_binned_time_accumulate_host(C.byref(a)) == SDY_OK
            for b, times in groups:
                counts[b] += len(times)
    return state, counts


def same_state(a, b, keys=("gen_sum", "target_sum", "gen_max", "gen_min", "target_max", "target_min")):
    """Bit for bit (a NaN equals a NaN of the same bits)."""
    return all(np.array_equal(np.ascontiguousarray(a[k]).view(np.uint8), np.ascontiguousarray(b[k]).view(np.uint8)) for k in keys)


def counted(case, labels, start=0, stop=None):
    """The global times start .. stop - 1 that are counted: not the initial condition, not labelled -1."""
    stop = case["S"] + 1 if stop is None else stop
    return [t for t in range(max(start, 1), stop) if labels[t] >= 0]


def restate_means(case, labels, n_bins, per_member=True, times=None):
    """numpy float64: {"gen": {name: (n_bins, M or 1, B, H, W)}, "target": {name: (n_bins, B, H, W)}}, the extremes likewise
    under gen_max / gen_min / target_max / target_min (fp32), counts per bin.  An empty bin is NaN."""
    times = counted(case, labels) if times is None else times
    out = {k: {} for k in ("gen", "target", "gen_max", "gen_min", "target_max", "target_min")}
    counts = [sum(1 for t in times if labels[t] == b) for b in range(n_bins)]
    M, B, H, W = case["M"], case["B"], case["H"], case["W"]
    for name in case["names"]:
        g, y = case["gen"][name].astype(np.float64), case["target"][name].astype(np.float64)
        gm = np.full((n_bins, M if per_member else 1, B, H, W), np.nan)
        ym = np.full((n_bins, B, H, W), np.nan)
        ext = {k: np.full(gm.shape if k.startswith("gen") else ym.shape, np.nan, np.float32) for k in list(out)[2:]}
        for b in range(n_bins):
            ts = [t for t in times if labels[t] == b]
            if not ts:
                continue
            gb, yb = g[:, :, ts], y[:, ts]
            gm[b] = gb.mean(axis=2) if per_member else gb.mean(axis=(0, 2))[None]
            ym[b] = yb.mean(axis=1)
            ext["gen_max"][b] = gb.max(axis=2) if per_member else gb.max(axis=(0, 2))[None]
            ext["gen_min"][b] = gb.min(axis=2) if per_member else gb.min(axis=(0, 2))[None]
            ext["target_max"][b], ext["target_min"][b] = yb.max(axis=1), yb.min(axis=1)
        out["gen"][name], out["target"][name] = gm, ym
        for k, v in ext.items():
            out[k][name] = v
    return out, counts


def fair_crps(g, y):
    """(M, ...) members against (...) -> mean |g - y| - sum_ij |g_i - g_j| / (2 M (M - 1))."""
    M = g.shape[0]
    pair = np.abs(g[:, None] - g[None]).sum(axis=(0, 1))
    return np.abs(g - y).mean(axis=0) - pair / (2 * M * (M - 1))


def restate_logs(case, means, counts, names_of_bins):
    """The aggregator's logs from the restated per-member means, float64 numpy.  -> (logs, term scale per variable)."""
    w = case["weights"].astype(np.float64)
    B = case["B"]
    norm = B * w.sum()
    wm = lambda x: float((w * x).sum() / norm)  # noqa: E731  (area-weighted mean over samples and points)
    full = [b for b, c in enumerate(counts) if c > 0]
    logs, scales = {}, {}
    for name in case["names"]:
        g, y = means["gen"][name], means["target"][name]
        M = g.shape[1]
        scales[name] = float(max(np.nanmax(np.abs(g)), np.nanmax(np.abs(y))))
        for b in full:
            key = f"{names_of_bins[b]}/{name}"
            e = g[b].mean(axis=0) - y[b]
            if M > 1:
                logs[f"rmse_member_avg/{key}"] = float(np.mean([np.sqrt(wm((g[b, m] - y[b]) ** 2)) for m in range(M)]))
                logs[f"bias_member_avg/{key}"] = float(np.mean([wm(g[b, m] - y[b]) for m in range(M)]))
            logs[f"rmse/{key}"] = float(np.sqrt(wm(e * e)))
            logs[f"bias/{key}"] = wm(e)
            if M > 1:
                logs[f"crps/{key}"] = wm(fair_crps(g[b], y[b]))
        if len(full) >= 2:
            ge, ye = g[full].mean(axis=1), y[full]
            ga, ya = ge - ge.mean(axis=0), ye - ye.mean(axis=0)
            for what, gv, yv in (("bin_range", ge.max(axis=0) - ge.min(axis=0), ye.max(axis=0) - ye.min(axis=0)),
                                 ("bin_std", np.sqrt((ga * ga).mean(axis=0)), np.sqrt((ya * ya).mean(axis=0)))):
                logs[f"{what}_gen/{name}"], logs[f"{what}_target/{name}"] = wm(gv), wm(yv)
                logs[f"{what}_ratio/{name}"] = wm(gv) / wm(yv)
            logs[f"centred_rmse/{name}"] = float(np.sqrt(wm(((ga - ya) ** 2).mean(axis=0))))
    return logs, scales
