#!/usr/bin/env python3
"""Price of the device kinetic-energy spectra (`sdy_amd.KineticEnergySpectrumAggregator`) on the BASELINE headline job's window
(one device), next to the scalar spectra of the same variables.

    timeout -k 10 600 python tools/ke_spectrum_bench.py --rounds 5 --reps 3 --warmup 2

One `record_batch` of a first window as `run_inference` hands it over: nine wind pairs (18 variables), predictions (25 members,
1 initial condition, 7 times, 180 x 360) as the member-stacked VIEW of the IC-major batch, targets (1, 7, 180, 360).  Timed
with device events, in the same run and alternating:
  * `ke_record_batch`: per chunk of pairs the packing copies, two longitude FFTs, two vector Legendre analyses (two fp32 MFMA
    GEMMs each) and one `sdy_vector_degree_power` launch;
  * `scalar_record_batch`: `PowerSpectrumAggregator.record_batch` on the same 18 variables (split-fp16 Legendre analysis);
  * the three parts of the generated side of ONE chunk on their own (`--chunk-pairs` pairs: one batch of u and v rows): `fft`
    (`sdy_rfft_lon`), `stage` (`sdy_vector_legendre_fwd`) and `reduction` (`sdy_vector_degree_power`, error accumulators on,
    member 0 standing in for the target row), and `scalar_stage` (`sdy_legendre_fwd` of the same batch, ONE product).
Prints ONE JSON line with the times and `ke_over_scalar`, the ratio of the two `record_batch` medians.  No pass mark.
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
    ap.add_argument("--chunk-pairs", type=int, default=2, help="pairs of the chunk whose parts are timed on their own")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3, help="repetitions per variant and round")
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()

    import torch

    import sdy_amd
    from sdy_amd import spectrum
    from sdy_amd._lib import SdyVectorSpectrumArgs, check, current_stream, lib, ptr

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
    ke = sdy_amd.KineticEnergySpectrumAggregator(pairs, T)
    ke.record_batch(0.0, tgt, pred, i_time_start=0)
    sc = sdy_amd.PowerSpectrumAggregator(T)
    sc.record_batch(0.0, tgt, pred, i_time_start=0)
    # one spot check before anything is timed: kinetic_energy_spectrum of one wind is the aggregator's target row of that time
    label, (un, vn) = next(iter(pairs.items()))
    one = sdy_amd.kinetic_energy_spectrum(tgt[un][0, 0], tgt[vn][0, 0])
    got = ke.get_data()[label]
    for part in ("rot", "div"):
        rel = float(((one[part] - got[f"target_{part}"][0]).abs().max() / one[part].abs().max()))
        assert rel < 1e-5, (part, rel)

    # the generated side of one chunk, part by part
    plan = spectrum._plan(H, W, None, None, "equiangular", dev)
    vplan = spectrum.VectorShtPlan.get(plan)
    cp, Rp = args.chunk_pairs, (M + 3) // 4 * 4
    half = cp * T * Rp
    F = 2 * half
    per_cs = plan.lmax * plan.mtr * 2
    x = torch.zeros(2, cp, T, Rp, H, W, device=dev)
    for c in range(2):
        for k in range(cp):
            x[c, k, :, :M].copy_(pred_all[c * npairs + k].transpose(0, 1))
    x = x.view(F, H, W)
    inv, scale = spectrum._field_scales(x)
    zeros = torch.zeros(F, device=dev)
    Xf = torch.empty(F * plan.mtr * H * 2, device=dev)
    Cd, Cm, Cscalar = (torch.empty(F * per_cs, device=dev) for _ in range(3))
    acc = torch.zeros(6, cp, T, plan.lmax, dtype=torch.float64, device=dev)
    a = SdyVectorSpectrumArgs()
    a.gen_d = a.target_d = ptr(Cd)
    a.gen_m = a.target_m = ptr(Cm)
    spectrum._fill_rows(a.rows, plan, ptr(scale), ptr(scale), (F, T * Rp, Rp), (F, T * Rp, Rp), cp, M, 1, T, 0, T)
    a.gen_v_offset = a.target_v_offset = half
    a.gen_rot, a.gen_div, a.target_rot, a.target_div, a.err_rot, a.err_div = (acc[i].data_ptr() for i in range(6))

    def fft():
        check(lib.sdy_rfft_lon(plan.handle, ptr(x), ptr(inv), ptr(zeros), None, ptr(Xf), 1, F, current_stream()), "sdy_rfft_lon")

    def stage():
        check(lib.sdy_vector_legendre_fwd(vplan.handle, ptr(Xf), ptr(Cd), ptr(Cm), 1, F, current_stream()),
              "sdy_vector_legendre_fwd")

    def scalar_stage():
        check(lib.sdy_legendre_fwd(plan.handle, ptr(Xf), ptr(Cscalar), 1, F, current_stream()), "sdy_legendre_fwd")

    def reduction():
        check(lib.sdy_vector_degree_power(C.byref(a), current_stream()), "sdy_vector_degree_power")

    fft()
    stage()
    fns = {"ke_record_batch": lambda: ke.record_batch(0.0, tgt, pred, i_time_start=0),
           "scalar_record_batch": lambda: sc.record_batch(0.0, tgt, pred, i_time_start=0),
           "fft": fft, "stage": stage, "scalar_stage": scalar_stage, "reduction": reduction}
    t = timed(fns, args.rounds, args.reps, args.warmup, dev)
    kern = (C.c_int * 2)()
    check(lib.sdy_sht_plan_kernels(plan.handle, C.byref(kern)), "sdy_sht_plan_kernels")
    res = {"tool": "ke_spectrum_bench",
           "shape": {"members": M, "samples": 1, "times": T, "nlat": H, "nlon": W, "pairs": npairs, "chunk_pairs": cp,
                     "chunk_fields": F},
           "scalar_legendre_back_end": int(kern[0]), "ke_workspace_bytes": ke.workspace_bytes,
           "scalar_workspace_bytes": sc.workspace_bytes,
           "coefficient_bytes_read_by_reduction": 2 * 4 * F * per_cs}
    for k in fns:
        res[f"{k}_ms"], res[f"{k}_ms_min"] = round(t[k][0], 3), round(t[k][1], 3)
    res["ke_over_scalar"] = round(t["ke_record_batch"][0] / t["scalar_record_batch"][0], 3)
    res["stage_over_scalar_stage"] = round(t["stage"][0] / t["scalar_stage"][0], 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
