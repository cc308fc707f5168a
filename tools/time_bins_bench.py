#!/usr/bin/env python3
"""Price of the binned time-mean aggregator (`sdy_amd.BinnedTimeMeanAggregator`) on the BASELINE headline job's window (one
device).

    timeout -k 10 600 python tools/time_bins_bench.py --rounds 7 --reps 3 --warmup 2

One `record_batch` of a window as `run_inference` hands it over: 63 variables, predictions (25 members, 1 initial condition, 7
times, 180 x 360) as the member-stacked VIEW of the IC-major batch, targets (1, 7, 180, 360), every window later in the run than
the one before so that all 7 times are counted.  Timed with device events, in the same run and alternating:
  * `one_bin`: every time of the window in one bin (a window inside one month): the traffic of `sdy_member_time_sum`;
  * `two_bins`: a window that straddles two bins (3 + 4 times);
  * `hour_of_day`: four bins, so four groups per window; `hour_of_day_extremes`: the same with `extremes=True`;
  * `yardstick`: `record_batch` of `sdy_amd.EnsembleTimeMeanAggregator` on the same window, which moves the bytes of `one_bin`;
  * `d2d`: a device-to-device copy of the bytes the kernel reads.
Bytes moved per case: the input once, plus the read and the write of every accumulator slice a group touches (8 bytes per
element and direction; with the extremes 16).  Per case the median, the minimum, the maximum and the quartiles of rounds x reps
repeats (at least 20 by default), bytes and TB/s.  Prints ONE JSON line; for the kernel alone run it under
`rocprofv3 --kernel-trace --stats` with `--cases one_bin` (the statistics are per kernel name): `binned_sum_kernel` next to
`member_sum_kernel`.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bench  # noqa: E402
from hist_bench import fields  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, default=bench.MEMBERS)
    ap.add_argument("--steps", type=int, default=bench.HORIZON, help="forecast steps of one window")
    ap.add_argument("--vars", type=int, default=bench.STATE_CH)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=3, help="repetitions per variant and round")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cases", default="", help="comma-separated subset of the binned cases (default: all), e.g. under a kernel "
                    "trace, whose statistics are per kernel name")
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
    slice_bytes = 2 * 8 * nv * (M + 1) * H * W            # one bin of all variables, read and written
    area = sdy_amd.metrics.spherical_area_weights(torch.linspace(-89.5, 89.5, H), W).to(dev)
    n_windows = 2 + args.warmup + args.rounds * args.reps
    n_times = T * (n_windows + 1)
    straddle = np.array(([0] * (T // 2) + [1] * (T - T // 2)) * (n_windows + 1))
    cases = {"one_bin": (np.zeros(n_times, dtype=np.int64), False, 1),
             "two_bins": (straddle, False, 2),
             "hour_of_day": (np.arange(n_times) % 4, False, min(4, T)),
             "hour_of_day_extremes": (np.arange(n_times) % 4, True, min(4, T))}
    if args.cases:
        cases = {k: cases[k] for k in args.cases.split(",")}
    aggs, starts = {}, {}
    for k, (labels, ext, _) in cases.items():
        aggs[k] = sdy_amd.BinnedTimeMeanAggregator(sdy_amd.TimeBins.from_labels(labels), area, extremes=ext)
        starts[k] = T

    def record(k):
        def fn():                           # every window later in the run than the one before
            aggs[k].record_batch(0.0, tgt, pred, tgt, pred, i_time_start=starts[k])
            starts[k] += T
        return fn

    yard = sdy_amd.EnsembleTimeMeanAggregator(area)
    # one spot check against torch before anything is timed: the bin means of one window
    for k in cases:
        record(k)()
    for k, (labels, _, n_groups) in cases.items():
        got = aggs[k].get_bin_means()["gen"][names[0]]
        for b in range(n_groups):
            want = pred_all[0][:, np.flatnonzero(labels[T:2 * T] == b).tolist()].double().mean(dim=1)
            assert float((got[b, :, 0] - want).abs().max()) < 1e-12 * float(want.abs().max()), (k, b)
    dst_p, dst_t = torch.empty_like(pred_all), torch.empty_like(tgt_all)

    def d2d():
        dst_p.copy_(pred_all)
        dst_t.copy_(tgt_all)

    fns = {k: record(k) for k in cases}
    fns["yardstick"] = lambda: yard.record_batch(0.0, tgt, pred, tgt, pred, i_time_start=T)
    fns["d2d"] = d2d

    def one(fn):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(dev)
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize(dev)
        return s.elapsed_time(e)

    for _ in range(args.warmup):
        for fn in fns.values():
            one(fn)
    ms = {k: [] for k in fns}
    for _ in range(args.rounds):
        for k, fn in fns.items():
            for _ in range(args.reps):
                ms[k].append(one(fn))
    res = {"tool": "time_bins_bench", "shape": {"members": M, "samples": 1, "times": T, "nlat": H, "nlon": W, "variables": nv},
           "repeats": args.rounds * args.reps, "input_bytes": n_bytes}
    for k, v in ms.items():
        q = statistics.quantiles(v, n=4) if len(v) >= 2 else [v[0]] * 3
        groups, ext = (cases[k][2], cases[k][1]) if k in cases else (1, False)
        moved = 2 * n_bytes if k == "d2d" else n_bytes + groups * slice_bytes * (2 if ext else 1)
        med = statistics.median(v)
        res[k] = {"ms_median": round(med, 3), "ms_min": round(min(v), 3), "ms_max": round(max(v), 3), "ms_q1": round(q[0], 3),
                  "ms_q3": round(q[2], 3), "bytes": moved, "TBps": round(moved / (med * 1e-3) / 1e12, 3)}
    if "one_bin" in res:
        res["one_bin_over_yardstick"] = round(res["one_bin"]["ms_median"] / res["yardstick"]["ms_median"], 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
