#!/usr/bin/env python3
"""Price of the device video / zonal-mean aggregators (`sdy_amd.metrics.VideoAggregator`, `ZonalMeanAggregator`) on the
BASELINE headline job's window (one device).

    timeout -k 10 600 python tools/video_bench.py --rounds 5 --reps 3 --warmup 2

One `record_batch` of a first window as `run_inference` hands it over: 63 variables, predictions (25 members, 1 initial
condition, 7 times = the 6 steps + the initial condition, 180 x 360) as the member-stacked VIEW of the IC-major batch, targets
(1, 7, 180, 360).  Timed with device events, in the same run and alternating:
  * `record_batch` of the plain video aggregator (two means), of the extended one (seven statistics) and of the zonal mean;
  * a device-to-device copy of the same bytes (what one pass over the data costs at this size on this device);
  * a device-to-host copy of the same tensors into pinned memory: what the reference's `.cpu()` costs before its arithmetic
    has looked at a value.
Every aggregator reads each value once: `*_GBps` = input bytes / time (the float64 accumulator traffic, 7 x 7 x 63 x 64800 x 8
bytes read and written for the extended video, is not counted).  Prints ONE JSON line; for the kernels separately run it under
`rocprofv3 --kernel-trace --stats` with `--rounds 1`: `video_kernel`, `zonal_kernel`.
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
    aggs = {"video": sdy_amd.VideoAggregator(T, False), "video_extended": sdy_amd.VideoAggregator(T, True),
            "zonal_mean": sdy_amd.ZonalMeanAggregator(T)}
    for agg in aggs.values():
        agg.record_batch(0.0, tgt, pred, i_time_start=0)
    # one spot check against torch before anything is timed
    want = pred_all[0].double().mean(dim=0)
    got = aggs["video_extended"].get_data()[names[0]]["gen"]
    assert float((got - want).abs().max()) < 1e-9 * float(want.abs().max())
    want = pred_all[0].double().mean(dim=(0, -1))
    got = aggs["zonal_mean"].get_data()[f"gen/{names[0]}"]
    assert float((got - want).abs().max()) < 1e-9 * float(want.abs().max())
    pin_p = torch.empty(pred_all.shape[1:], dtype=torch.float32, pin_memory=True)
    pin_t = torch.empty(tgt_all.shape[1:], dtype=torch.float32, pin_memory=True)
    dst_p, dst_t = torch.empty_like(pred_all), torch.empty_like(tgt_all)

    def d2h():
        for i in range(nv):
            pin_p.copy_(pred_all[i], non_blocking=True)
            pin_t.copy_(tgt_all[i], non_blocking=True)

    def d2d():
        dst_p.copy_(pred_all)
        dst_t.copy_(tgt_all)

    fns = {k: (lambda a=a: a.record_batch(0.0, tgt, pred, i_time_start=0)) for k, a in aggs.items()}
    fns.update(d2h=d2h, d2d=d2d)
    t = timed(fns, args.rounds, args.reps, args.warmup, dev)
    res = {"tool": "video_bench", "shape": {"members": M, "samples": 1, "times": T, "nlat": H, "nlon": W, "variables": nv},
           "bytes": n_bytes}
    for k in aggs:
        res[f"{k}_ms"], res[f"{k}_ms_min"] = round(t[k][0], 3), round(t[k][1], 3)
        res[f"{k}_GBps"] = round(n_bytes / (t[k][0] * 1e-3) / 1e9, 1)
    res.update(d2h_pinned_ms=round(t["d2h"][0], 3), d2h_GBps=round(n_bytes / (t["d2h"][0] * 1e-3) / 1e9, 1),
               d2d_copy_ms=round(t["d2d"][0], 3), d2d_GBps_read_plus_write=round(2 * n_bytes / (t["d2d"][0] * 1e-3) / 1e9, 1))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
