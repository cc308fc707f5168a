#!/usr/bin/env python3
"""Price of the time quantiles (`sdy_amd.TimeQuantileAggregator`) on the BASELINE headline job's window (one device).

    timeout -k 10 900 python tools/quantile_bench.py --rounds 5 --reps 3 --warmup 2

Timed with device events, in the same run and alternating:
  * `sdy_time_quantile_append` of one window as `run_inference` hands it over -- predictions (25 members, 1 initial condition,
    7 times, 180 x 360) as the member-stacked VIEW of the IC-major batch, targets (1, 7, 180, 360), `--vars` variables in one
    launch -- into a series of 26 trajectories (the same slots every time: the entry point does not mind);
  * a device-to-device copy of the bytes the append moves (it reads and writes 4 bytes per value): `append_share_of_copy` is
    the append's read + write rate over the copy's;
  * `sdy_time_quantile_select` at 1, 4 and 8 quantiles, method linear, on one variable's series of `--slots` time slots: the
    targets alone (1 trajectory per point: 64800 lanes) and gen pooled over the members (25 x slots keys per point);
  * the torch restatement of the same select: `torch.sort` along time on the float view of the keys' values, then indexing and
    the interpolation in float64.  Its result is compared with the select's before anything is timed.
No time is fixed in advance: the yardsticks are the copy (append) and the torch sort (select).  Prints ONE JSON line; for the
kernels alone run it under `rocprofv3 --kernel-trace --stats` with `--rounds 1`: `append_kernel`, `select_kernel`.
"""
import argparse
import ctypes as C
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bench  # noqa: E402
from hist_bench import timed  # noqa: E402

QUANTILES = {1: (0.99,), 4: (0.5, 0.9, 0.99, 0.999), 8: (0.01, 0.1, 0.25, 0.5, 0.75, 0.9, 0.99, 0.999)}


def torch_quantiles(x, qs):
    """x (n, points) fp32 without NaN -> (Q, points) float64 by the definition's rank rule on a full sort."""
    import torch

    s = torch.sort(x, dim=0).values
    n = x.shape[0]
    out = []
    for q in qs:
        h = q * (n - 1)
        j = min(math.floor(h), n - 1)
        g = h - j
        lo, hi = s[j].double(), s[min(j + 1, n - 1)].double()
        d = hi - lo
        lerp = hi - d * (1.0 - g) if g >= 0.5 else lo + d * g
        out.append(torch.where(lo == hi, lo, lerp) if g != 0 else lo)
    return torch.stack(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, default=bench.MEMBERS)
    ap.add_argument("--steps", type=int, default=bench.HORIZON, help="forecast steps of one window")
    ap.add_argument("--vars", type=int, default=4, help="variables of the appended window")
    ap.add_argument("--slots", type=int, default=360, help="time slots of the series the select reads")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3, help="repetitions per variant and round")
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()

    import torch

    import sdy_amd
    from sdy_amd import _lib
    from sdy_amd.quantiles import _select
    from sdy_amd.windows import fill_window, window_layouts

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    M, T, nv, S = args.members, args.steps + 1, args.vars, args.slots
    H, W = bench.NLAT, bench.NLON
    g = torch.Generator(device=dev).manual_seed(11)
    names = [f"var{v:02d}" for v in range(nv)]
    pred_all = torch.randn(nv, 1, M, T, H, W, device=dev, generator=g)
    tgt_all = torch.randn(nv, 1, T, H, W, device=dev, generator=g)
    pred = {n: pred_all[i].transpose(0, 1) for i, n in enumerate(names)}
    tgt = {n: tgt_all[i] for i, n in enumerate(names)}
    n_traj = M + 1
    window_series = torch.full((nv, n_traj, T, H * W), -1, dtype=torch.int32, device=dev)
    lay = window_layouts(tgt, pred)
    a = _lib.SdyTimeQuantileAppendArgs()
    fill_window(a.win, lay, 0, nv)
    a.H, a.W, a.t0, a.slot0, a.capacity, a.store_gen, a.series = H, W, 0, 0, T, 1, window_series.data_ptr()

    def append():
        _lib.check(sdy_amd.lib.sdy_time_quantile_append(C.byref(a), _lib.current_stream()), "sdy_time_quantile_append")

    append()
    # spot check: the keys order as the values do, trajectory 0 of variable 0 at the first time
    k0 = window_series[0, 0, 0].view(H, W).to(torch.int64) & 0xFFFFFFFF
    x0 = pred_all[0, 0, 0, 0]
    assert torch.equal(torch.argsort(k0.view(-1), stable=True), torch.argsort(x0.view(-1), stable=True))
    moved = 4 * (pred_all.numel() + tgt_all.numel())
    dst_p, dst_t = torch.empty_like(pred_all), torch.empty_like(tgt_all)

    def d2d():
        dst_p.copy_(pred_all)
        dst_t.copy_(tgt_all)

    # the series the select reads: one variable, M + 1 trajectories, S slots, appended in one call
    long_gen = torch.randn(M, 1, S, H, W, device=dev, generator=g)
    long_tgt = torch.randn(1, S, H, W, device=dev, generator=g)
    series = torch.full((n_traj, S, H * W), -1, dtype=torch.int32, device=dev)
    b = _lib.SdyTimeQuantileAppendArgs()
    fill_window(b.win, window_layouts({"x": long_tgt}, {"x": long_gen}), 0, 1)
    b.H, b.W, b.t0, b.slot0, b.capacity, b.store_gen, b.series = H, W, 0, 0, S, 1, series.data_ptr()
    _lib.check(sdy_amd.lib.sdy_time_quantile_append(C.byref(b), _lib.current_stream()), "sdy_time_quantile_append")
    groups = {"target": (M, 1, 1, 0, 1), "gen": (0, 1, M, 1, 1)}
    values = {"target": long_tgt.view(S, H * W), "gen": long_gen.view(M * S, H * W)}

    def select(which, nq):
        return _select(series.data_ptr(), dev, n_traj, S, S, H, W, *groups[which], QUANTILES[nq], 0)[0]

    for which in groups:
        got, want = select(which, 8)[0].view(8, H * W), torch_quantiles(values[which], QUANTILES[8])
        assert torch.equal(got, want), which
    del got, want
    fns = {"append": append, "d2d": d2d}
    for which in groups:
        for nq in QUANTILES:
            fns[f"select_{which}_q{nq}"] = (lambda w, n: lambda: select(w, n))(which, nq)
        fns[f"torch_sort_{which}_q4"] = (lambda w: lambda: torch_quantiles(values[w], QUANTILES[4]))(which)
    t = timed(fns, args.rounds, args.reps, args.warmup, dev)
    res = {"tool": "quantile_bench", "shape": {"members": M, "samples": 1, "times": T, "nlat": H, "nlon": W, "variables": nv,
                                               "slots": S}, "append_bytes_read": moved, "append_bytes_written": moved}
    for k in fns:
        res[f"{k}_ms"], res[f"{k}_ms_min"] = round(t[k][0], 3), round(t[k][1], 3)
    d2d_rate = 2 * moved / (t["d2d"][0] * 1e-3) / 1e9
    res["d2d_GBps_read_plus_write"] = round(d2d_rate, 1)
    res["append_GBps_read_plus_write"] = round(2 * moved / (t["append"][0] * 1e-3) / 1e9, 1)
    res["append_share_of_copy"] = round(res["append_GBps_read_plus_write"] / d2d_rate, 3)
    for which in groups:
        res[f"select_{which}_keys_per_point"] = values[which].shape[0]
        res[f"select_{which}_q4_over_torch_sort"] = round(t[f"select_{which}_q4"][0] / t[f"torch_sort_{which}_q4"][0], 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
