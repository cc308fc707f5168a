#!/usr/bin/env python3
"""Price of the device histograms (`sdy_amd.histogram.HistogramDataWriter`) on the BASELINE headline job's window (one device).

    timeout -k 10 900 python tools/hist_bench.py --rounds 5 --reps 3 --warmup 2

One `append_batch` of a first window as `run_inference` hands it over: 63 variables, predictions (25 members, 1 initial
condition, 7 times = the 6 steps + the initial condition, 180 x 360) as the member-stacked VIEW of the IC-major batch, targets
(1, 7, 180, 360).  Timed with device events, in the same run and alternating with
  * a device-to-host copy of the same tensors into pinned memory (the least `host_outputs=True` + the reference's numpy path
    costs before numpy has looked at a value), and
  * a device-to-device copy of the same bytes (what one pass over the data costs at this size on this device).
`append_batch` reads every value twice (min / max pass, counting pass): `hist_GBps` = 2 x bytes / time.  Two kinds of data,
because the counting pass bins through LDS atomics and lanes that hit one bin serialise:
  noise   independent N(0, 1) per grid point (neighbouring lanes spread over the bins);
  smooth  a zonal profile plus small noise (neighbouring grid points share a bin, as on real fields).
Prints ONE JSON line.  For the three kernels separately run it under `rocprofv3 --kernel-trace --stats` with `--rounds 1`:
`hist_minmax_kernel`, `hist_rebin_kernel`, `hist_count_kernel`.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def fields(device, kind, n_vars, rows, times, seed):
    """(n_vars, rows, times, H, W) on the device"""
    import torch

    g = torch.Generator(device=device).manual_seed(seed)
    H, W = bench.NLAT, bench.NLON
    x = torch.randn(n_vars, rows, times, H, W, device=device, generator=g)
    if kind == "smooth":
        lat = torch.linspace(-1.0, 1.0, H, device=device).view(1, 1, 1, H, 1)
        x = 3.0 * torch.cos(1.5 * lat) + 0.02 * x
    return x


def timed(fns, rounds, reps, warmup, dev):
    import torch

    def one(fn):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(dev)
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize(dev)
        return s.elapsed_time(e)

    for _ in range(warmup):
        for fn in fns.values():
            one(fn)
    ms = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            for _ in range(reps):
                ms[k].append(one(fn))
    return {k: (statistics.median(v), min(v)) for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, default=bench.MEMBERS)
    ap.add_argument("--steps", type=int, default=bench.HORIZON, help="forecast steps of one window")
    ap.add_argument("--vars", type=int, default=bench.STATE_CH)
    ap.add_argument("--bins", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3, help="repetitions per variant and round")
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()

    import torch

    import sdy_amd

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    M, T, nv = args.members, args.steps + 1, args.vars
    names = [f"var{v:02d}" for v in range(nv)]
    res = {"tool": "hist_bench", "shape": {"members": M, "samples": 1, "times": T, "nlat": bench.NLAT, "nlon": bench.NLON,
                                           "variables": nv, "bins": args.bins}}
    for kind in ("noise", "smooth"):
        pred_all = fields(dev, kind, nv, M, T, seed=11)
        tgt_all = fields(dev, kind, nv, 1, T, seed=12)
        pred = {n: pred_all[i].view(1, M, T, bench.NLAT, bench.NLON).transpose(0, 1) for i, n in enumerate(names)}
        tgt = {n: tgt_all[i] for i, n in enumerate(names)}
        n_bytes = 4 * (pred_all.numel() + tgt_all.numel())
        wr = sdy_amd.HistogramDataWriter(None, T, n_bins=args.bins)
        wr.append_batch(tgt, pred, 0, 0)
        ds = wr.get_dataset()          # raises if a flag is set or a value fell outside
        assert int(ds["prediction"][names[0]].sum()) == M * T * bench.NLAT * bench.NLON
        occupied = statistics.median(int((ds["prediction"][n].sum(axis=0) > 0).sum()) for n in names)
        pin_p = torch.empty(pred_all.shape[1:], dtype=torch.float32, pin_memory=True)
        pin_t = torch.empty(tgt_all.shape[1:], dtype=torch.float32, pin_memory=True)
        dst_p, dst_t = torch.empty_like(pred_all), torch.empty_like(tgt_all)

        def d2h():
            for i in range(nv):      # (one pinned buffer per dict entry size, reused: the copies of a stream are serial anyway)
                pin_p.copy_(pred_all[i], non_blocking=True)
                pin_t.copy_(tgt_all[i], non_blocking=True)

        def d2d():
            dst_p.copy_(pred_all)
            dst_t.copy_(tgt_all)

        t = timed({"hist": lambda: wr.append_batch(tgt, pred, 0, 0), "d2h": d2h, "d2d": d2d}, args.rounds, args.reps,
                  args.warmup, dev)
        wr.get_dataset()
        res[kind] = {"bytes": n_bytes, "occupied_bins_median": occupied,
                     "append_batch_ms": round(t["hist"][0], 3), "append_batch_ms_min": round(t["hist"][1], 3),
                     "hist_GBps": round(2 * n_bytes / (t["hist"][0] * 1e-3) / 1e9, 1),
                     "d2h_pinned_ms": round(t["d2h"][0], 3), "d2h_GBps": round(n_bytes / (t["d2h"][0] * 1e-3) / 1e9, 1),
                     "d2d_copy_ms": round(t["d2d"][0], 3),
                     "d2d_GBps_read_plus_write": round(2 * n_bytes / (t["d2d"][0] * 1e-3) / 1e9, 1)}
        del pred_all, tgt_all, pred, tgt, dst_p, dst_t, pin_p, pin_t, wr
        torch.cuda.empty_cache()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
