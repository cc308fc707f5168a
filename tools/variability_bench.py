#!/usr/bin/env python3
"""Price of the time-variability aggregator (`sdy_amd.TimeVariabilityAggregator`) on the BASELINE headline job's window (one
device).

    timeout -k 10 600 python tools/variability_bench.py --rounds 5 --reps 3 --warmup 2

One `record_batch` of a window as `run_inference` hands it over: 63 variables, predictions (25 members, 1 initial condition, 7
times, 180 x 360) as the member-stacked VIEW of the IC-major batch, targets (1, 7, 180, 360), at `i_time_start > 0` so that all
7 times are counted and read, and not the run's first window, so that the state is read as well as written.  Timed with device
events, in the same run and alternating:
  * `record_batch` (`sdy_time_variability_accumulate`: one launch for the 63 variables);
  * a device-to-device copy of the bytes the kernel reads from the window (what one pass over the data costs at this size on
    this device);
  * `get_logs` (`sdy_time_variability_stats`, once per run of inference, and the read-back of the sums).
The kernel reads every input value once (`bytes`) and reads and writes the state, 32 bytes per trajectory and grid point
(`state_bytes`, both directions): `record_GBps` = (bytes + state_bytes) / time, to be held against the copy's read + write rate
(`share_of_copy`).  Prints ONE JSON line; for the kernels separately run it under `rocprofv3 --kernel-trace --stats` with
`--rounds 1`: `variability_kernel`, `variability_stats_kernel`, `combine_chunks_kernel`.
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
    state_bytes = 2 * 32 * nv * (M + 1) * H * W
    area = sdy_amd.metrics.spherical_area_weights(torch.linspace(-89.5, 89.5, H), W).to(dev)
    agg = sdy_amd.TimeVariabilityAggregator(area, max_bytes=state_bytes)
    start = [T]

    def record():                     # the same window again, as the run's next one
        agg.record_batch(0.0, tgt, pred, tgt, pred, i_time_start=start[0])
        start[0] += T

    record()
    # one spot check against torch before anything is timed
    want = pred_all[0].double().var(dim=1, unbiased=False).sqrt()
    got = agg.get_data()["gen_time_std"][names[0]][:, 0]
    assert float((got - want).abs().max()) < 1e-9 * float(want.max()), float((got - want).abs().max())
    logs = agg.get_logs("")
    w = area.double()
    want = float(((want ** 2).mean(dim=0) * w).sum().div(w.sum()).sqrt())
    assert abs(logs[f"time_std_gen/{names[0]}"] - want) < 1e-9 * want, (logs[f"time_std_gen/{names[0]}"], want)
    del got, want
    dst_p, dst_t = torch.empty_like(pred_all), torch.empty_like(tgt_all)

    def d2d():
        dst_p.copy_(pred_all)
        dst_t.copy_(tgt_all)

    t = timed({"record": record, "d2d": d2d, "get_logs": lambda: agg.get_logs("")}, args.rounds, args.reps, args.warmup, dev)
    res = {"tool": "variability_bench", "shape": {"members": M, "samples": 1, "times": T, "nlat": H, "nlon": W, "variables": nv},
           "bytes": n_bytes, "state_bytes": state_bytes, "counted_times": agg.n_times}
    for k in ("record", "get_logs"):
        res[f"{k}_ms"], res[f"{k}_ms_min"] = round(t[k][0], 3), round(t[k][1], 3)
    res["record_GBps"] = round((n_bytes + state_bytes) / (t["record"][0] * 1e-3) / 1e9, 1)
    res["record_input_GBps"] = round(n_bytes / (t["record"][0] * 1e-3) / 1e9, 1)
    d2d_rate = 2 * n_bytes / (t["d2d"][0] * 1e-3) / 1e9
    res.update(d2d_copy_ms=round(t["d2d"][0], 3), d2d_GBps_read_plus_write=round(d2d_rate, 1),
               share_of_copy=round(res["record_GBps"] / d2d_rate, 3))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
