#!/usr/bin/env python3
"""Price of the ensemble rank histograms (`sdy_amd.RankHistogramAggregator`) on the BASELINE headline job's window (one device).

    timeout -k 10 600 python tools/rank_hist_bench.py --rounds 5 --reps 3 --warmup 2

One `record_batch` of a window as `run_inference` hands it over: 63 variables, predictions (25 members, 1 initial condition, 7
times, 180 x 360) as the member-stacked VIEW of the IC-major batch, targets (1, 7, 180, 360), at `i_time_start > 0` so that all
7 times are counted and read.  Timed with device events, in the same run and alternating:
  * `record_batch` of the rank histograms with a lead-time axis (`sdy_rank_hist_accumulate`: one launch for the 63 variables);
  * the same with `pool_times=True` (one slot: a lane group walks the 7 times of its latitude);
  * `ZonalMeanAggregator.record_batch` on the same window: the same traversal (a lane group per latitude row, every member's
    row read once) without the compare chain and the LDS counters;
  * a device-to-device copy of the bytes the kernel reads (what one pass over the data costs at this size on this device).
The kernel reads every input value once (`bytes`); its accumulators are (slots, 180, 26) counts per variable, 0.1 % of that.
`*_input_GBps` = bytes / time, to be held against each other; `share_of_copy` holds the read rate against the copy's read +
write rate.  Prints ONE JSON line; for the kernel alone run it under `rocprofv3 --kernel-trace --stats` with `--rounds 1`:
`rank_hist_kernel`.
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
    area = sdy_amd.metrics.spherical_area_weights(torch.linspace(-89.5, 89.5, H), W).to(dev)
    slots = sdy_amd.RankHistogramAggregator(area, n_timesteps=2 * T)
    pooled = sdy_amd.RankHistogramAggregator(area, n_timesteps=2 * T, pool_times=True)
    zonal = sdy_amd.metrics.ZonalMeanAggregator(n_timesteps=2 * T)
    for agg in (slots, pooled):
        agg.record_batch(0.0, tgt, pred, tgt, pred, i_time_start=T)
    # one spot check against torch before anything is timed: variable 0's counts, bin by bin
    rank = (pred_all[0] < tgt_all[0]).sum(dim=0)                                             # (T, H, W)
    want = torch.stack([(rank == k).sum(dim=-1) for k in range(M + 1)], dim=-1).double()     # (T, H, M + 1)
    got = slots.get_data()[f"counts/{names[0]}"]
    assert torch.equal(got[T:], want) and float(got[:T].sum()) == 0.0
    assert torch.equal(pooled.get_data()[f"counts/{names[0]}"][0], want.sum(dim=0))
    dst_p, dst_t = torch.empty_like(pred_all), torch.empty_like(tgt_all)

    def d2d():
        dst_p.copy_(pred_all)
        dst_t.copy_(tgt_all)

    fns = {"record": lambda: slots.record_batch(0.0, tgt, pred, tgt, pred, i_time_start=T),
           "record_pooled": lambda: pooled.record_batch(0.0, tgt, pred, tgt, pred, i_time_start=T),
           "zonal_record": lambda: zonal.record_batch(0.0, tgt, pred, tgt, pred, i_time_start=T),
           "d2d": d2d}
    t = timed(fns, args.rounds, args.reps, args.warmup, dev)
    res = {"tool": "rank_hist_bench", "shape": {"members": M, "samples": 1, "times": T, "nlat": H, "nlon": W, "variables": nv},
           "bytes": n_bytes}
    for k in ("record", "record_pooled", "zonal_record"):
        res[f"{k}_ms"], res[f"{k}_ms_min"] = round(t[k][0], 3), round(t[k][1], 3)
        res[f"{k}_input_GBps"] = round(n_bytes / (t[k][0] * 1e-3) / 1e9, 1)
    d2d_rate = 2 * n_bytes / (t["d2d"][0] * 1e-3) / 1e9
    res.update(d2d_copy_ms=round(t["d2d"][0], 3), d2d_GBps_read_plus_write=round(d2d_rate, 1),
               share_of_copy=round(res["record_input_GBps"] / d2d_rate, 3),
               share_of_zonal=round(res["record_input_GBps"] / res["zonal_record_input_GBps"], 3))
    logs = slots.get_logs("")
    res["reliability_index_var00"] = round(logs[f"reliability_index/{names[0]}"], 4)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
