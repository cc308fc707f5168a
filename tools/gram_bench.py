#!/usr/bin/env python3
"""Price of the field scores (`sdy_amd.FieldScoreAggregator`, `sdy_member_gram`) on the BASELINE headline job's window (one
device).

    timeout -k 10 600 python tools/gram_bench.py --rounds 5 --reps 3 --warmup 2

One `record_batch` of a window as `run_inference` hands it over: 63 variables, predictions (25 members, 1 initial condition, 7
times, 180 x 360) as the member-stacked VIEW of the IC-major batch, targets (1, 7, 180, 360).  Timed with device events, in the
same run and alternating:
  * `FieldScoreAggregator.record_batch` (one `sdy_member_gram` launch pair for the 63 variables, then `scores` on the Grams);
  * the Gram launch pair alone;
  * `RegionalMeanAggregator.record_batch` with ONE region on the same window (the sibling that reads the same bytes);
  * a torch float64 restatement of the Gram (`matmul` per variable, so that its float64 copy of the window fits): the
    yardstick, since nothing else in the library computes this;
  * a device-to-device copy of the bytes the kernels read from the window.
`*_input_GBps` = window bytes / time, to be held against the copy's read rate (half its read + write rate).
The float64 matrix instruction: `mfma_probe` times the Gram launch pair at 62 members (N = 64: ten tiles of
v_mfma_f64_16x16x4_f64 per four grid points and wave, where the headline window has three) on `--probe-vars` variables and
reports the launch's time per instruction and SIMD in cycles: an UPPER bound of the instruction's issue interval (staging and
the waves' reduction are inside the time).  Prints ONE JSON line; for the kernels separately run it under `rocprofv3
--kernel-trace --stats` with `--rounds 1`: `member_gram_kernel`, `combine_chunks_kernel`.
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


def gram_launcher(sdy_amd, tgt, pred, weights):
    """-> (a function that launches sdy_member_gram on the window, its packed output)."""
    import torch

    from sdy_amd._lib import SdyMemberGramArgs, check, current_stream, ptr
    from sdy_amd.windows import fill_window, window_layouts

    lay = window_layouts(tgt, pred)
    l = lay[0]
    N = l.n0 + 2
    out = torch.empty(len(lay), l.n1, l.T, N * (N + 1) // 2, dtype=torch.float64, device=weights.device)
    ws_bytes = sdy_amd.lib.sdy_member_gram_workspace_bytes(len(lay), l.n0, l.n1, l.T, l.H * l.W)
    ws = torch.empty(ws_bytes // 8, dtype=torch.float64, device=weights.device)
    a = SdyMemberGramArgs()
    fill_window(a.win, lay, 0, len(lay))
    a.HW, a.weights, a.out, a.ws, a.ws_bytes = l.H * l.W, ptr(weights), ptr(out), ptr(ws), ws_bytes
    keep = (lay, ws)

    def launch():
        check(sdy_amd.lib.sdy_member_gram(C.byref(a), current_stream()), "sdy_member_gram")
        return keep

    return launch, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, default=bench.MEMBERS)
    ap.add_argument("--steps", type=int, default=bench.HORIZON, help="forecast steps of one window")
    ap.add_argument("--vars", type=int, default=bench.STATE_CH)
    ap.add_argument("--probe-vars", type=int, default=8, help="variables of the 62-member instruction-rate probe (0: skip)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3, help="repetitions per variant and round")
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()

    import numpy as np
    import torch

    import sdy_amd
    from sdy_amd.field_scores import unpack

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
    w_dev = area.to(dev).contiguous()
    one = sdy_amd.Regions(lats, lons, area).add_global()
    field = sdy_amd.FieldScoreAggregator(area, n_timesteps=T, is_ensemble=M > 1)
    regional = sdy_amd.RegionalMeanAggregator(one, n_timesteps=T, is_ensemble=M > 1)
    launch, packed = gram_launcher(sdy_amd, tgt, pred, w_dev.view(-1))
    w64 = w_dev.double().view(1, 1, H * W)

    def torch_gram(i):
        y = tgt_all[i].double().view(1, T, H * W)
        a = torch.cat([torch.ones_like(y), pred_all[i].double().view(M, T, H * W) - y, y]).transpose(0, 1)   # (T, N, HW)
        return (a * w64) @ a.transpose(1, 2)

    def torch_all():
        for i in range(nv):
            torch_gram(i)

    fns = {"record_batch": lambda: field.record_batch(0.0, tgt, pred, tgt, pred, i_time_start=0),
           "gram_launch": launch,
           "regional_1": lambda: regional.record_batch(0.0, tgt, pred, tgt, pred, i_time_start=0),
           "torch_float64": torch_all}
    for fn in fns.values():
        fn()
    # one spot check before anything is timed: the launch against the torch restatement, the RMSE against the sibling's
    got, want = unpack(packed[0, 0], M + 2), torch_gram(0)
    assert float((got - want).abs().max() / want.abs().max()) < 1e-9, (got - want).abs().max()
    a, b = field.get_series()[f"ensemble_mean_rmse/{names[0]}"], regional.get_series()[f"weighted_rmse/global/{names[0]}"]
    assert float(((a - b).abs() / b.abs()).max()) < 1e-9, (a, b)
    dst_p, dst_t = torch.empty_like(pred_all), torch.empty_like(tgt_all)

    def d2d():
        dst_p.copy_(pred_all)
        dst_t.copy_(tgt_all)

    t = timed({**fns, "d2d": d2d}, args.rounds, args.reps, args.warmup, dev)
    res = {"tool": "gram_bench", "shape": {"members": M, "samples": 1, "times": T, "nlat": H, "nlon": W, "variables": nv},
           "bytes": n_bytes}
    for k in fns:
        res[f"{k}_ms"], res[f"{k}_ms_min"] = round(t[k][0], 3), round(t[k][1], 3)
        res[f"{k}_input_GBps"] = round(n_bytes / (t[k][0] * 1e-3) / 1e9, 1)
    d2d_rate = 2 * n_bytes / (t["d2d"][0] * 1e-3) / 1e9
    res.update(d2d_copy_ms=round(t["d2d"][0], 3), d2d_GBps_read_plus_write=round(d2d_rate, 1))
    props = torch.cuda.get_device_properties(dev)
    simds, clock_khz = 4 * props.multi_processor_count, float(getattr(props, "clock_rate", 2.4e6))   # (MI355X: 2400 MHz)
    tiles = lambda m: (lambda nb: nb * (nb + 1) // 2)((m + 2 + 15) // 16)             # noqa: E731
    steps = -(-(H * W) // 256) * 64                           # four-point steps of a plane: whole quarters, padding included
    res["gram_instructions"] = nv * T * steps * tiles(M)
    res["gram_launch_cycles_per_instruction_and_simd"] = round(
        t["gram_launch"][1] * 1e-3 * clock_khz * 1e3 * simds / res["gram_instructions"], 1)

    if args.probe_vars > 0:
        pm, pv = 62, args.probe_vars
        p_all = fields(dev, "smooth", pv, pm, T, seed=13)
        p_pred = {names[i]: p_all[i].view(1, pm, T, H, W).transpose(0, 1) for i in range(pv)}
        p_tgt = {names[i]: tgt_all[i] for i in range(pv)}
        p_launch, _ = gram_launcher(sdy_amd, p_tgt, p_pred, w_dev.view(-1))
        p_launch()
        pt = timed({"probe": p_launch}, args.rounds, args.reps, args.warmup, dev)["probe"]
        count = pv * T * steps * tiles(pm)
        res["mfma_probe"] = {"members": pm, "variables": pv, "ms": round(pt[0], 3), "ms_min": round(pt[1], 3),
                             "instructions": count, "clock_MHz": clock_khz / 1e3, "simds": simds,
                             "cycles_per_instruction_and_simd_upper_bound": round(
                                 pt[1] * 1e-3 * clock_khz * 1e3 * simds / count, 1),
                             "input_GBps": round(4 * (p_all.numel() + pv * T * H * W) / (pt[0] * 1e-3) / 1e9, 1)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
