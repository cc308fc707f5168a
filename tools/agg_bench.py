#!/usr/bin/env python3
"""Price of weighted_grad_mag_percent_diff in the inference aggregators, on the BASELINE headline job's window (one device).

    timeout -k 10 900 python tools/agg_bench.py --rounds 5 --reps 3 --warmup 2

`InferenceAggregator.record_batch` fed what `run_inference` hands over for one steady-state window of bench.py's headline
job: 25 members of one initial condition, the window's 6 forecast steps (the initial condition removed: a strided view of
the IC-major batch, members behind the sample axis), 180 x 360, the 63 output variables, denormalised and normalised data
(`mean`, `mean_norm` and `time_mean`).  Two aggregators, one with `grad_mag_percent_diff=True`, alternate window by window
(`--reps` windows per mode per round, `--rounds` rounds after `--warmup` windows each); each window is timed with device
events and with the host clock (the launches of 63 variables x 2 aggregators are part of the cost).  Unless `--no-window`, one
horizon-6 sampling pass of the 25 members (bench.one_pass, same network as bench.py) is timed too, for the aggregator's share
of a window.  Prints ONE JSON line.  For the kernel alone run it under `rocprofv3 --kernel-trace --stats` with
`--no-window --rounds 1`: `ens_series_kernel` (grad off) and `ens_series_grad_kernel` (grad on) read the same
`bytes_per_launch` of algorithmic input.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402  (constants and the headline job's pieces)


def window(device, members, steps, n_vars, seed):
    """target (1, steps, H, W) and generated (members, 1, steps, H, W) views per variable, as run_inference presents a window
    after its first: the IC-major batch (1 IC x members, steps + 1, H, W) with the initial condition dropped, transposed."""
    import torch

    g = torch.Generator(device=device).manual_seed(seed)
    H, W = bench.NLAT, bench.NLON
    tgt, gen = {}, {}
    for v in range(n_vars):
        name = f"var{v:02d}"
        t = torch.randn(1, steps + 1, H, W, device=device, generator=g)
        x = t[None] + 0.3 * torch.randn(1, members, steps + 1, H, W, device=device, generator=g)
        tgt[name] = t[:, 1:]
        gen[name] = x.transpose(0, 1)[:, :, 1:]
    return tgt, gen


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, default=bench.MEMBERS)
    ap.add_argument("--steps", type=int, default=bench.HORIZON, help="forecast steps of one window")
    ap.add_argument("--vars", type=int, default=bench.STATE_CH)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3, help="windows per mode and round")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-window", action="store_true", help="skip timing the sampling pass")
    args = ap.parse_args()

    import torch

    import sdy_amd

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    lats = torch.linspace(-89.5, 89.5, bench.NLAT)
    w = sdy_amd.metrics.spherical_area_weights(lats, bench.NLON).to(dev)
    tgt, gen = window(dev, args.members, args.steps, args.vars, seed=7)
    tgt_n, gen_n = window(dev, args.members, args.steps, args.vars, seed=8)
    n_t = 1 + 4 * args.steps
    aggs = {mode: sdy_amd.metrics.InferenceAggregator(w, n_timesteps=n_t, n_ensemble_members=args.members,
                                                      grad_mag_percent_diff=(mode == "grad_on"))
            for mode in ("grad_off", "grad_on")}

    def one(mode):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(dev)
        h0 = time.perf_counter()
        s.record()
        aggs[mode].record_batch(loss=0.0, target_data=tgt, gen_data=gen, target_data_norm=tgt_n, gen_data_norm=gen_n,
                                i_time_start=1 + args.steps)
        e.record()
        torch.cuda.synchronize(dev)
        return s.elapsed_time(e), 1e3 * (time.perf_counter() - h0)

    for _ in range(args.warmup):
        for mode in aggs:
            one(mode)
    dev_ms = {m: [] for m in aggs}
    host_ms = {m: [] for m in aggs}
    for _ in range(args.rounds):
        for mode in aggs:
            for _ in range(args.reps):
                d, h = one(mode)
                dev_ms[mode].append(d)
                host_ms[mode].append(h)
    series = aggs["grad_on"]._aggregators["mean"].get_series()
    gm = torch.stack([v for k, v in series.items() if k.startswith("weighted_grad_mag_percent_diff/")])
    assert bool(torch.isfinite(gm[:, 1 + args.steps:1 + 2 * args.steps]).all()), "non-finite grad-mag series"

    H, W, M, T = bench.NLAT, bench.NLON, args.members, args.steps
    res = {"tool": "agg_bench", "shape": {"members": M, "samples": 1, "steps": T, "nlat": H, "nlon": W, "vars": args.vars},
           "windows_per_mode": args.rounds * args.reps,
           "series_launches_per_window": 2 * args.vars,
           "bytes_per_launch": 4 * (M * T * H * W + T * H * W + H * W)}
    for mode in aggs:
        res[f"{mode}_ms"] = round(statistics.median(dev_ms[mode]), 3)
        res[f"{mode}_ms_min"] = round(min(dev_ms[mode]), 3)
        res[f"{mode}_host_ms"] = round(statistics.median(host_ms[mode]), 3)
    res["on_over_off"] = round(res["grad_on_ms"] / res["grad_off_ms"], 3)
    if not args.no_window:
        del aggs, tgt, gen, tgt_n, gen_n
        torch.cuda.empty_cache()
        from sdy_amd import InterpolationExperiment, MultiHorizonForecastingDYffusion, synthetic

        cs, nf, hz = bench.STATE_CH, bench.FORCING_CH, bench.HORIZON
        shape = dict(nlat=H, nlon=W, embed=bench.EMBED, layers=bench.LAYERS)
        fnet = synthetic.build_network(cs, cs, nf, time_range=(0.0, hz - 1.0), weight_seed=4321, **shape)
        inet = synthetic.build_network(2 * cs, cs, nf, dropout_mlp=0.1, drop_path_rate=0.1, time_range=(1.0, hz - 1.0),
                                       weight_seed=4322, dropout_seed=1000, **shape)
        exp = MultiHorizonForecastingDYffusion(fnet, InterpolationExperiment(inet, horizon=hz), horizon=hz)
        x, forc = bench.synthetic_state(0, M, dev)
        x = bench.one_pass(exp, x, forc)
        torch.cuda.synchronize(dev)
        times = []
        for _ in range(2):
            t0 = time.perf_counter()
            x = bench.one_pass(exp, x, forc)
            torch.cuda.synchronize(dev)
            times.append(1e3 * (time.perf_counter() - t0))
        assert bool(torch.isfinite(x).all())
        res["window_ms"] = round(min(times), 1)
        res["grad_off_share_pct"] = round(100 * res["grad_off_ms"] / res["window_ms"], 3)
        res["grad_on_share_pct"] = round(100 * res["grad_on_ms"] / res["window_ms"], 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
