#!/usr/bin/env python3
"""Price of the derived water-budget variables (`sdy_amd.derived`) on the BASELINE headline job's window (one device).

    timeout -k 10 900 python tools/derived_bench.py --rounds 5 --reps 3 --warmup 2

1. The derive pass of one prediction dict: 25 members x 1 initial condition x 7 times (the window's 6 steps + its initial
   condition: the loop derives before dropping it) x 180 x 360, K = 8 levels, as the member-stacked VIEW `run_inference`
   hands over.  `sdy_derived_water` (one launch, all three outputs) against a straightforward torch restatement of the
   same formulas written here (levels stacked on a last axis, pressure thickness by `diff`, sum, time difference), alternating,
   device events.  Algorithmic traffic: 12 input fields read once, 3 output fields written once.
2. `InferenceAggregator.record_batch` on one steady-state window (the set-up of tools/agg_bench.py: 63 variables, 6 steps,
   denormalised + normalised) with and without the three derived variables added to the denormalised dicts, alternating.
Prints ONE JSON line.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import bench  # noqa: E402
from agg_bench import window  # noqa: E402

AK = [3.0, 5238.4, 11815.8, 17263.1, 19929.5, 17023.4, 8970.5, 1537.5, 0.0]
BK = [0.0, 0.0, 0.0115, 0.0781, 0.2034, 0.4004, 0.6513, 0.9065, 1.0]


def inputs(device, members, times, seed):
    """member-stacked views (members, 1, times, H, W) of an IC-major batch, FV3GFS-like magnitudes"""
    import torch

    g = torch.Generator(device=device).manual_seed(seed)
    sh = (members, times, bench.NLAT, bench.NLON)
    flat = {f"specific_total_water_{k}": torch.rand(sh, device=device, generator=g) * 10.0 ** (-2 - 0.5 * k)
            for k in range(len(AK) - 1)}
    flat["PRESsfc"] = 1.0e5 + 2.5e3 * torch.randn(sh, device=device, generator=g)
    flat["LHTFLsfc"] = 90.0 + 60.0 * torch.randn(sh, device=device, generator=g)
    flat["PRATEsfc"] = 6.0e-5 * torch.rand(sh, device=device, generator=g)
    flat["tendency_of_total_water_path_due_to_advection"] = 2.0e-5 * torch.randn(sh, device=device, generator=g)
    return {k: v.view(1, *sh).transpose(0, 1) for k, v in flat.items()}


def torch_derived(d, ak, bk):
    """The three formulas in plain torch (fp32), residual along the time axis (2)."""
    import torch

    q = torch.stack([d[f"specific_total_water_{k}"] for k in range(ak.numel() - 1)], dim=-1)
    ps = d["PRESsfc"]
    dp = (ak + ps.unsqueeze(-1) * bk).diff(dim=-1)
    twp = (dp * q).sum(dim=-1) * (1.0 / 9.80665)
    dry = ps - 9.80665 * twp
    res = torch.zeros_like(twp)
    res[:, :, 1:] = (twp[:, :, 1:] - twp[:, :, :-1]) / 21600.0 - (
        d["LHTFLsfc"][:, :, 1:] / 2.5e6 - d["PRATEsfc"][:, :, 1:]
        + d["tendency_of_total_water_path_due_to_advection"][:, :, 1:])
    return {"surface_pressure_due_to_dry_air": dry, "total_water_path": twp, "total_water_path_budget_residual": res}


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
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3, help="repetitions per variant and round")
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()

    import torch

    import sdy_amd

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    M, T, H, W, K = args.members, args.steps + 1, bench.NLAT, bench.NLON, len(AK) - 1
    d = inputs(dev, M, T, seed=11)
    sigma = type("Sigma", (), {"ak": torch.tensor(AK), "bk": torch.tensor(BK)})()
    der = sdy_amd.derived.deriver(sigma)
    ak_d, bk_d = sigma.ak.to(dev), sigma.bk.to(dev)
    got, ref = der(d), torch_derived(d, ak_d, bk_d)
    for n, v in ref.items():          # same formulas: agree to fp32 rounding (torch's level sum is ordered differently)
        err = float((got[n].double() - v.double()).abs().max())
        assert err <= 1e-5 * float(v.double().abs().max()) + 1e-9, (n, err)
    t = timed({"kernel": lambda: der(d), "torch": lambda: torch_derived(d, ak_d, bk_d)}, args.rounds, args.reps,
              args.warmup, dev)
    field = 4 * M * T * H * W
    res = {"tool": "derived_bench",
           "shape": {"members": M, "samples": 1, "times": T, "nlat": H, "nlon": W, "levels": K},
           "bytes_read": (K + 4) * field, "bytes_written": 3 * field,
           "kernel_ms": round(t["kernel"][0], 4), "kernel_ms_min": round(t["kernel"][1], 4),
           "torch_ms": round(t["torch"][0], 3), "torch_ms_min": round(t["torch"][1], 3)}
    res["torch_over_kernel"] = round(res["torch_ms"] / res["kernel_ms"], 1)
    res["kernel_TBps"] = round((K + 7) * field / (res["kernel_ms"] * 1e-3) / 1e12, 2)
    del d, got, ref
    torch.cuda.empty_cache()

    # record_batch with and without the three derived variables (a steady-state window: initial condition dropped)
    lats = torch.linspace(-89.5, 89.5, H)
    w = sdy_amd.metrics.spherical_area_weights(lats, W).to(dev)
    tgt, gen = window(dev, M, args.steps, args.vars, seed=7)
    tgt_n, gen_n = window(dev, M, args.steps, args.vars, seed=8)
    xt, xg = window(dev, M, args.steps, 3, seed=9)
    names = list(sdy_amd.derived.DERIVED_NAMES)
    tgt_d = dict(tgt, **{names[i]: v for i, v in enumerate(xt.values())})
    gen_d = dict(gen, **{names[i]: v for i, v in enumerate(xg.values())})
    n_t = 1 + 4 * args.steps
    aggs = {m: sdy_amd.metrics.InferenceAggregator(w, n_timesteps=n_t, n_ensemble_members=M) for m in ("off", "on")}
    feeds = {"off": (tgt, gen), "on": (tgt_d, gen_d)}

    def rec(m):
        return lambda: aggs[m].record_batch(loss=0.0, target_data=feeds[m][0], gen_data=feeds[m][1],
                                            target_data_norm=tgt_n, gen_data_norm=gen_n, i_time_start=1 + args.steps)

    t = timed({m: rec(m) for m in aggs}, args.rounds, args.reps, args.warmup, dev)
    res["record_batch_ms"] = round(t["off"][0], 3)
    res["record_batch_derived_ms"] = round(t["on"][0], 3)
    res["record_batch_ratio"] = round(t["on"][0] / t["off"][0], 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
