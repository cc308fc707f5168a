#!/usr/bin/env python3
"""Price of the eddy-covariance aggregator (`sdy_amd.EddyCovarianceAggregator`) on the BASELINE headline job's window (one device).

    timeout -k 10 600 python tools/eddy_bench.py --rounds 5 --reps 3 --warmup 2

One `record_batch` of a window as `run_inference` hands it over: the eight `CovarianceGroups.standard` level groups (u, v, T, q) of
32 variables, predictions (25 members, 1 initial condition, 7 times, 180 x 360) as the member-stacked VIEW of the IC-major batch,
targets (1, 7, 180, 360), at `i_time_start > 0` so that all 7 times are counted and read, and not the run's first window, so that
the state is read as well as written.  Timed with device events, in the same run and alternating:
  * `record_batch` (the checks, the argument structure and one `sdy_time_covariance_accumulate` launch for the eight groups);
  * `accumulate`: that launch alone, from an argument structure built once;
  * a device-to-device copy of the bytes the kernel reads from the window (what one pass over the data costs at this size on this
    device);
  * `TimeVariabilityAggregator.record_batch` on the same 32 variables (the per-variable second moments: 32 bytes of state per
    trajectory and point);
  * a torch float64 restatement: per group the shifted fields and an `einsum` over time per pair, added to float64 maps;
  * `get_logs` (`sdy_time_covariance_stats`, once per run of inference, and the read-back of the sums).
The kernel reads every input value once (`bytes`) and reads and writes the state, 128 bytes per group, trajectory and grid point
(`state_bytes`, both directions): `accumulate_GBps` = (bytes + state_bytes) / time, to be held against the copy's read + write
rate (`share_of_copy`).  Prints ONE JSON line.  Another build of the library (csrc/Makefile, EXTRA="-DSDY_TC_TIMES_K4=3") is
measured by pointing SDY_AMD_LIB at it.
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bench  # noqa: E402
from hist_bench import fields, timed  # noqa: E402

STEMS = ("eastward_wind", "northward_wind", "air_temperature", "specific_total_water")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, default=bench.MEMBERS)
    ap.add_argument("--steps", type=int, default=bench.HORIZON, help="forecast steps of one window")
    ap.add_argument("--levels", type=int, default=8)
    ap.add_argument("--group-size", type=int, default=4, choices=(2, 3, 4), help="variables per level group (u, v[, T[, q]])")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3, help="repetitions per variant and round")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--skip-torch", action="store_true", help="leave the torch float64 restatement out")
    args = ap.parse_args()

    import torch

    import sdy_amd
    from sdy_amd._lib import current_stream, lib
    from sdy_amd.windows import window_layouts

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    M, T, K = args.members, args.steps + 1, args.group_size
    H, W = bench.NLAT, bench.NLON
    names = [f"{stem}_{k}" for k in range(args.levels) for stem in STEMS[:K]]
    nv = len(names)
    pred_all = fields(dev, "smooth", nv, M, T, seed=11)
    tgt_all = fields(dev, "smooth", nv, 1, T, seed=12)
    pred = {n: pred_all[i].view(1, M, T, H, W).transpose(0, 1) for i, n in enumerate(names)}
    tgt = {n: tgt_all[i] for i, n in enumerate(names)}
    n_bytes = 4 * (pred_all.numel() + tgt_all.numel())
    groups = sdy_amd.CovarianceGroups.standard(names)
    assert len(groups) == args.levels and all(len(v) == K for _, v in groups)
    area = sdy_amd.metrics.spherical_area_weights(torch.linspace(-89.5, 89.5, H), W).to(dev)
    agg = sdy_amd.EddyCovarianceAggregator(groups, area)
    state_once = agg.state_bytes(M, 1, H, W)
    state_bytes = 2 * state_once
    start = [T]

    def record():                     # the same window again, as the run's next one
        agg.record_batch(0.0, tgt, pred, tgt, pred, i_time_start=start[0])
        start[0] += T

    record()
    record()
    # one spot check against torch before anything is timed
    x, y = (pred_all[names.index(f"{stem}_0")].double() for stem in STEMS[:2])
    want = ((x - x.mean(dim=1, keepdim=True)) * (y - y.mean(dim=1, keepdim=True))).mean(dim=1)
    got = agg.get_pair_data("level_0", "u", "v")["gen_cov"][:, 0]
    assert float((got - want).abs().max()) < 1e-9 * float(x.var(dim=1, unbiased=False).max()), float((got - want).abs().max())
    del x, y, got, want
    calls = list(agg._calls(dict(zip(names, window_layouts(tgt, pred))), 0))
    assert len(calls) == 1

    def accumulate():
        for a, _ in calls:
            assert lib.sdy_time_covariance_accumulate(C.byref(a), current_stream()) == 0

    tv = sdy_amd.TimeVariabilityAggregator(area)
    tv_start = [T]

    def variability():
        tv.record_batch(0.0, tgt, pred, tgt, pred, i_time_start=tv_start[0])
        tv_start[0] += T

    variability()
    dst_p, dst_t = torch.empty_like(pred_all), torch.empty_like(tgt_all)

    def d2d():
        dst_p.copy_(pred_all)
        dst_t.copy_(tgt_all)

    fns = {"record": record, "accumulate": accumulate, "d2d": d2d, "variability": variability, "get_logs": lambda: agg.get_logs("")}
    if not args.skip_torch:
        P = K * (K + 1) // 2
        origin = pred_all[:, :, 0].double()
        acc_s = torch.zeros(args.levels, K, M, H, W, dtype=torch.float64, device=dev)
        acc_p = torch.zeros(args.levels, P, M, H, W, dtype=torch.float64, device=dev)

        def torch_f64():              # the generated rows only: 25 of the 26 trajectories
            for g in range(args.levels):
                d = pred_all[g * K:(g + 1) * K].double() - origin[g * K:(g + 1) * K, :, None]
                acc_s[g] += d.sum(dim=2)
                q = 0
                for i in range(K):
                    for j in range(i, K):
                        acc_p[g, q] += torch.einsum("mthw,mthw->mhw", d[i], d[j])
                        q += 1

        fns["torch_f64"] = torch_f64
    t = timed(fns, args.rounds, args.reps, args.warmup, dev)
    res = {"tool": "eddy_bench", "lib": os.path.basename(sdy_amd.LIB_PATH),
           "shape": {"members": M, "samples": 1, "times": T, "nlat": H, "nlon": W, "variables": nv, "groups": args.levels, "K": K},
           "bytes": n_bytes, "state_bytes": state_bytes, "counted_times": agg.n_times}
    for k in fns:
        if k != "d2d":
            res[f"{k}_ms"], res[f"{k}_ms_min"] = round(t[k][0], 3), round(t[k][1], 3)
    for k in ("record", "accumulate"):
        res[f"{k}_GBps"] = round((n_bytes + state_bytes) / (t[k][0] * 1e-3) / 1e9, 1)
    d2d_rate = 2 * n_bytes / (t["d2d"][0] * 1e-3) / 1e9
    res.update(d2d_copy_ms=round(t["d2d"][0], 3), d2d_GBps_read_plus_write=round(d2d_rate, 1),
               share_of_copy=round(res["accumulate_GBps"] / d2d_rate, 3),
               variability_GBps=round((n_bytes + 2 * 32 * nv * (M + 1) * H * W) / (t["variability"][0] * 1e-3) / 1e9, 1))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
