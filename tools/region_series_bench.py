#!/usr/bin/env python3
"""Price of the regional metric series (`sdy_amd.RegionalMeanAggregator`) on the BASELINE headline job's window (one device).

    timeout -k 10 600 python tools/region_series_bench.py --rounds 5 --reps 3 --warmup 2

One `record_batch` of a window as `run_inference` hands it over: 63 variables, predictions (25 members, 1 initial condition, 7
times, 180 x 360) as the member-stacked VIEW of the IC-major batch, targets (1, 7, 180, 360).  Timed with device events, in the
same run and alternating:
  * `RegionalMeanAggregator.record_batch` with ONE region (`global`) and with the five standard regions (`sdy_region_series`:
    one launch for the 63 variables and all regions, then a handful of torch operations on the sums);
  * `MeanAggregator.record_batch` on the same window (`sdy_ensemble_series`: one launch per variable), the global series the
    one-region case reproduces;
  * a device-to-device copy of the bytes the kernels read from the window.
`*_input_GBps` = window bytes / time, to be held against the copy's read rate (half its read + write rate).  Prints ONE JSON
line; for the kernels separately run it under `rocprofv3 --kernel-trace --stats` with `--rounds 1`: `region_series_kernel`,
`region_combine_kernel`, `ens_series_pass`.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bench  # noqa: E402
from hist_bench import fields, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, default=bench.MEMBERS)
    ap.add_argument("--steps", type=int, default=bench.HORIZON, help="forecast steps of one window")
    ap.add_argument("--vars", type=int, default=bench.STATE_CH)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3, help="repetitions per variant and round")
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()

    import numpy as np
    import torch

    import sdy_amd

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    M, T, nv = args.members, args.steps + 1, args.vars
    H, W = bench.NLAT, bench.NLON
    names = [f"var{v:02d}" for v in range(nv)]
    pred_all = fields(dev, "smooth", nv, M, T, seed=11)
    tgt_all = fields(dev, "smooth", nv, 1, T, seed=12)
    pred = {n: pred_all[i].view(1, M, T, H, W).transpose(0, 1) for i, n in enumerate(names)}
    tgt = {n: tgt_all[i] for i, n in enumerate(names)}
    n_bytes = 4 * (pred_all.numel() + tgt_all.numel())
    lats = np.linspace(-90.0 + 90.0 / H, 90.0 - 90.0 / H, H)
    lons = (np.arange(W) + 0.5) * 360.0 / W
    area = sdy_amd.metrics.spherical_area_weights(torch.from_numpy(lats), W).float()
    standard = sdy_amd.Regions.standard(lats, lons, area)
    one = sdy_amd.Regions(lats, lons, area).add_global()
    aggs = {"regional_1": sdy_amd.RegionalMeanAggregator(one, n_timesteps=T, is_ensemble=True),
            f"regional_{len(standard)}": sdy_amd.RegionalMeanAggregator(standard, n_timesteps=T, is_ensemble=True),
            "mean_aggregator": sdy_amd.metrics.MeanAggregator(area.to(dev), n_timesteps=T, is_ensemble=True)}
    fns = {k: (lambda a=a: a.record_batch(0.0, tgt, pred, tgt, pred, i_time_start=0)) for k, a in aggs.items()}
    for fn in fns.values():
        fn()
    # one spot check before anything is timed: the one-region series are MeanAggregator's
    got, want = aggs["regional_1"].get_series(), aggs["mean_aggregator"].get_series()
    for metric in ("weighted_rmse", "weighted_crps", "weighted_ssr", "weighted_std_gen"):
        a, b = got[f"{metric}/global/{names[0]}"], want[f"{metric}/{names[0]}"]
        assert float(((a - b).abs() / b.abs()).max()) < 1e-5, (metric, a, b)
    dst_p, dst_t = torch.empty_like(pred_all), torch.empty_like(tgt_all)

    def d2d():
        dst_p.copy_(pred_all)
        dst_t.copy_(tgt_all)

    t = timed({**fns, "d2d": d2d}, args.rounds, args.reps, args.warmup, dev)
    res = {"tool": "region_series_bench", "shape": {"members": M, "samples": 1, "times": T, "nlat": H, "nlon": W, "variables": nv},
           "bytes": n_bytes, "regions": standard.names}
    for k in fns:
        res[f"{k}_ms"], res[f"{k}_ms_min"] = round(t[k][0], 3), round(t[k][1], 3)
        res[f"{k}_input_GBps"] = round(n_bytes / (t[k][0] * 1e-3) / 1e9, 1)
    d2d_rate = 2 * n_bytes / (t["d2d"][0] * 1e-3) / 1e9
    res.update(d2d_copy_ms=round(t["d2d"][0], 3), d2d_GBps_read_plus_write=round(d2d_rate, 1))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
