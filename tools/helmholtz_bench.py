#!/usr/bin/env python3
"""Price of the Helmholtz fields of the winds (`sdy_amd.helmholtz.deriver`) on the BASELINE headline job's window (one device),
next to the kinetic-energy spectra of the same winds and a copy of the same bytes.

    timeout -k 10 600 python tools/helmholtz_bench.py --rounds 5 --reps 3 --warmup 2

The prediction dict of a first window as `run_inference` hands it to `derive`: nine wind pairs (18 variables), 25 members,
1 initial condition, 7 times, 180 x 360, as the member-stacked VIEW of the IC-major batch.  Timed with device events, in the same
run and alternating:
  * `derive_2`, `derive_4`: the deriver with (vorticity, divergence) and with all four outputs: per chunk of winds the packing
    copies, one longitude FFT, the vector Legendre analysis, ONE `sdy_helmholtz_coefficients` launch, the Legendre synthesis,
    the inverse FFT and (with more than one chunk) the copy out of the staged grids;
  * `kernel_2`, `kernel_4`: `sdy_helmholtz_coefficients` alone on the coefficients of `--chunk-winds` winds;
  * `ke_record_batch`: `KineticEnergySpectrumAggregator.record_batch` on the same pairs (targets (1, 7, 180, 360));
  * `copy`: a device-to-device copy of the input bytes (the 18 prediction variables).
Prints ONE JSON line with medians and minima, the bytes the kernel moves and its rate.  No pass mark.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, default=bench.MEMBERS)
    ap.add_argument("--steps", type=int, default=bench.HORIZON, help="forecast steps of one window")
    ap.add_argument("--pairs", type=int, default=9)
    ap.add_argument("--chunk-winds", type=int, default=348, help="winds of the batch the kernel is timed on alone")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3, help="repetitions per variant and round")
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()

    import torch

    import sdy_amd
    from sdy_amd import helmholtz as hh
    from sdy_amd import spectrum
    from sdy_amd._lib import SdyHelmholtzArgs, check, current_stream, lib, ptr
    from sdy_amd.sht import ShtPlan

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    M, T, npairs = args.members, args.steps + 1, args.pairs
    H, W = bench.NLAT, bench.NLON
    names = [f"eastward_wind_{k}" for k in range(npairs - 1)] + ["UGRD10m"]
    names += [f"northward_wind_{k}" for k in range(npairs - 1)] + ["VGRD10m"]
    pairs = spectrum.wind_pairs(names)
    assert len(pairs) == npairs
    pred_all = fields(dev, "smooth", 2 * npairs, M, T, seed=11)
    tgt_all = fields(dev, "smooth", 2 * npairs, 1, T, seed=12)
    pred = {n: pred_all[i].view(1, M, T, H, W).transpose(0, 1) for i, n in enumerate(names)}
    tgt = {n: tgt_all[i] for i, n in enumerate(names)}
    derive = {2: hh.deriver(names, outputs=("vorticity", "divergence")), 4: hh.deriver(names, outputs=hh.OUTPUTS)}
    out = derive[4](pred)
    assert len(out) == len(pred) + 4 * npairs and all(bool(torch.isfinite(v).all()) for v in out.values())
    del out
    ke = sdy_amd.KineticEnergySpectrumAggregator(pairs, T)
    ke.record_batch(0.0, tgt, pred, i_time_start=0)

    # the kernel alone: the coefficients of one batch of winds
    plan = ShtPlan.get(H, W, H, W // 2 + 1, "equiangular", dev.index, "f32")
    vplan = spectrum.VectorShtPlan.get(plan)
    k = args.chunk_winds
    Fh = (k + 3) // 4 * 4
    F = 2 * Fh
    per_cs = plan.lmax * plan.mtr * 2
    x = torch.zeros(2, Fh, H, W, device=dev)
    for c in range(2):
        x[c, :k].copy_(pred_all[c * npairs:(c + 1) * npairs].reshape(-1, H, W)[:k])
    x = x.view(F, H, W)
    inv, scale = hh._pow2_scales(x)
    zeros = torch.zeros(F, device=dev)
    Xf = torch.empty(F * plan.mtr * H * 2, device=dev)
    Cd, Cm = (torch.empty(F * per_cs, device=dev) for _ in range(2))
    Co = torch.empty(4 * Fh * per_cs, device=dev)
    check(lib.sdy_rfft_lon(plan.handle, ptr(x), ptr(inv), ptr(zeros), None, ptr(Xf), 1, F, current_stream()), "sdy_rfft_lon")
    check(lib.sdy_vector_legendre_fwd(vplan.handle, ptr(Xf), ptr(Cd), ptr(Cm), 1, F, current_stream()), "sdy_vector_legendre_fwd")
    kargs = {}
    for n_out, outs in ((2, ("vorticity", "divergence")), (4, hh.OUTPUTS)):
        a = SdyHelmholtzArgs()
        a.Cs_d, a.Cs_m, a.scale, a.out = ptr(Cd), ptr(Cm), ptr(scale), ptr(Co)
        a.factor = ptr(hh._factors(outs, plan.lmax, hh.DEFAULT_RADIUS, None, dev))
        a.lmax, a.mtr, a.fields, a.u_offset, a.v_offset, a.n_winds = plan.lmax, plan.mtr, F, 0, Fh, k
        a.out_fields, a.out_stride, a.n_out = n_out * Fh, Fh, n_out
        for q, name in enumerate(outs):
            a.part[q] = hh._PART[name]
        kargs[n_out] = a

    def kernel(n_out):
        check(lib.sdy_helmholtz_coefficients(C.byref(kargs[n_out]), current_stream()), "sdy_helmholtz_coefficients")

    sink = torch.empty_like(pred_all)
    fns = {"derive_2": lambda: derive[2](pred), "derive_4": lambda: derive[4](pred),
           "kernel_2": lambda: kernel(2), "kernel_4": lambda: kernel(4),
           "ke_record_batch": lambda: ke.record_batch(0.0, tgt, pred, i_time_start=0),
           "copy": lambda: sink.copy_(pred_all)}
    t = timed(fns, args.rounds, args.reps, args.warmup, dev)
    # the kernel's traffic: only entries with 1 <= l, m <= l are loaded (eight quads a lane); every entry is stored
    live = sum(min(l, plan.mtr - 1) + 1 for l in range(1, plan.lmax))
    res = {"tool": "helmholtz_bench",
           "shape": {"members": M, "samples": 1, "times": T, "nlat": H, "nlon": W, "pairs": npairs, "winds": npairs * M * T,
                     "kernel_winds": k},
           "input_bytes": 4 * pred_all.numel(), "workspace_bytes": hh._ws.bytes, "ke_workspace_bytes": ke.workspace_bytes}
    for name in fns:
        res[f"{name}_ms"], res[f"{name}_ms_min"] = round(t[name][0], 3), round(t[name][1], 3)
    for n_out in (2, 4):
        moved = 4 * (live * 2 * F * 2 + plan.lmax * plan.mtr * 2 * n_out * Fh)
        res[f"kernel_{n_out}_bytes"] = moved
        res[f"kernel_{n_out}_TBps"] = round(moved / (t[f"kernel_{n_out}"][0] * 1e-3) / 1e12, 3)
    res["copy_TBps"] = round(2 * 4 * pred_all.numel() / (t["copy"][0] * 1e-3) / 1e12, 3)
    res["derive_4_over_ke"] = round(t["derive_4"][0] / t["ke_record_batch"][0], 3)
    res["derive_2_over_ke"] = round(t["derive_2"][0] / t["ke_record_batch"][0], 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
