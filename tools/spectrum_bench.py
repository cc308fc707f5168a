#!/usr/bin/env python3
"""Price of the device power-spectrum aggregator (`sdy_amd.PowerSpectrumAggregator`) on the BASELINE headline job's window
(one device).

    timeout -k 10 600 python tools/spectrum_bench.py --rounds 5 --reps 3 --warmup 2

One `record_batch` of a first window as `run_inference` hands it over: 63 variables, predictions (25 members, 1 initial
condition, 7 times, 180 x 360) as the member-stacked VIEW of the IC-major batch, targets (1, 7, 180, 360).  Timed with device
events, in the same run and alternating:
  * `record_batch`: per chunk of variables the packing copies, two longitude FFTs, two Legendre analyses and one
    `sdy_degree_power` launch;
  * a device-to-device copy of the bytes the reduction alone reads (the coefficients of both sides: lmax x mtr x 2 floats per
    padded field; the triangle m <= l that it actually touches is about half of that);
  * a device-to-device copy of the window's input bytes, for scale.
Prints ONE JSON line; for the kernels separately run it under `rocprofv3 --kernel-trace --stats` with `--rounds 1`:
`degree_power_kernel`.
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
    in_bytes = 4 * (pred_all.numel() + tgt_all.numel())
    agg = sdy_amd.PowerSpectrumAggregator(T)
    agg.record_batch(0.0, tgt, pred, i_time_start=0)
    # one spot check before anything is timed: a[0,0] is the quadrature of the field over the sphere / sqrt(4 pi), so degree 0
    # holds the row mean of (sum_k w_k (2 pi / W) sum_j f[k, j])^2 / (4 pi), w the transform's own quadrature weights
    import ctypes as C

    import numpy as np

    w = np.zeros(H)
    assert sdy_amd.lib.sdy_sht_tables_host(H, W, H, W // 2 + 1, sdy_amd._lib.SDY_GRID["equiangular"], None,
                                           w.ctypes.data_as(C.c_void_p), None) == 0
    wq = torch.from_numpy(w).to(dev)
    integral = (pred_all[0].double().sum(dim=-1) * wq).sum(dim=-1) * (2.0 * torch.pi / W)           # (members, times)
    want = (integral ** 2).mean(dim=0) / (4.0 * torch.pi)
    got = agg.get_data()[names[0]]["gen"][:, 0]
    assert float(((got - want).abs() / want).max()) < 1e-5, (got, want)
    lmax, mtr = H, min(W // 2 + 1, H)
    pad4 = lambda n: (n + 3) // 4 * 4  # noqa: E731
    cs_bytes = 4 * lmax * mtr * 2 * nv * T * (pad4(M) + pad4(1))
    cs_reps = -(-cs_bytes // (1 << 30))                      # equal blocks of at most 1 GiB, cs_bytes in all
    src_cs = torch.empty(cs_bytes // cs_reps // 4, dtype=torch.float32, device=dev)
    dst_cs = torch.empty_like(src_cs)
    dst_p, dst_t = torch.empty_like(pred_all), torch.empty_like(tgt_all)

    def d2d_coeffs():
        for _ in range(cs_reps):
            dst_cs.copy_(src_cs)

    def d2d_inputs():
        dst_p.copy_(pred_all)
        dst_t.copy_(tgt_all)

    fns = {"record_batch": lambda: agg.record_batch(0.0, tgt, pred, i_time_start=0), "d2d_coeffs": d2d_coeffs,
           "d2d_inputs": d2d_inputs}
    t = timed(fns, args.rounds, args.reps, args.warmup, dev)
    res = {"tool": "spectrum_bench", "shape": {"members": M, "samples": 1, "times": T, "nlat": H, "nlon": W, "variables": nv},
           "input_bytes": in_bytes, "coefficient_bytes": cs_reps * 4 * src_cs.numel(), "workspace_bytes": agg.workspace_bytes}
    for k in fns:
        res[f"{k}_ms"], res[f"{k}_ms_min"] = round(t[k][0], 3), round(t[k][1], 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
