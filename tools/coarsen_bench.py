#!/usr/bin/env python3
"""Price of the device-side time coarsening and of the prediction writer (`sdy_amd.data_writer`) on the BASELINE headline job's
window (one device).

    timeout -k 10 900 python tools/coarsen_bench.py --rounds 5 --reps 3 --warmup 2

One `append_batch` of a first window as `run_inference` hands it over: 63 variables, predictions (25 members, 1 initial
condition, 7 times = the 6 steps + the initial condition, 180 x 360) as the member-stacked VIEW of the IC-major batch, targets
(1, 7, 180, 360).  Timed with device events, in the same run and alternating:
  coarsen_f2 / coarsen_f6   `TimeCoarsen(null writer).append_batch` at factor 2 and 6: one `sdy_time_coarsen` per source;
  torch_f2 / torch_f6       (a) the torch restatement on the same device: the initial condition sliced off and
                            `unfold(time, f, f).mean(-1)` per variable, as the reference's `_coarsen_tensor_dict` does;
  d2d                       (b) a device-to-device copy of the bytes read;
  d2h                       (c) the pinned device-to-host copy of the uncoarsened tensors;
  write_f1 / write_f2 / write_f6   `PredictionDataWriter.append_batch` + `flush` (pack, D2H, memmap copy; files under --dir,
                            a tmpfs path keeps the disk out of the number) alone and behind `TimeCoarsen`, on the first
                            --write-vars variables (the files of all 63 are 2.9 GB per window), next to
  d2h_sub                   the pinned device-to-host copy of those variables, uncoarsened.
The write variants are timed on the host clock (they end in a host copy) and once per round, everything else with device
events.  Prints ONE JSON
line: medians and minima in ms, `*_GBps` = bytes read / time, and the ratios kernel / torch (must be <= 1), kernel / d2d,
write_fN / d2h.
"""
import argparse
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from hist_bench import fields  # noqa: E402


class Null:
    def append_batch(self, target, prediction, start_timestep, start_sample, batch_times=None):
        pass

    def flush(self):
        pass


def timed(fns, rounds, reps, warmup, dev):
    import torch

    def one(fn, host):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        s.record()
        fn()
        e.record()
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) * 1e3 if host else s.elapsed_time(e)

    for i in range(warmup):
        for k, fn in fns.items():
            if i == 0 or not k.startswith("write"):
                one(fn, k.startswith("write"))
    ms = {k: [] for k in fns}
    for _ in range(rounds):
        for k, fn in fns.items():
            for _ in range(1 if k.startswith("write") else reps):
                ms[k].append(one(fn, k.startswith("write")))
    return {k: (statistics.median(v), min(v)) for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, default=bench.MEMBERS)
    ap.add_argument("--steps", type=int, default=bench.HORIZON, help="forecast steps of one window")
    ap.add_argument("--vars", type=int, default=bench.STATE_CH)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3, help="repetitions per variant and round")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--write-vars", type=int, default=8, help="variables the write variants handle")
    ap.add_argument("--dir", default=None, help="where the prediction files go (default: a temporary directory)")
    args = ap.parse_args()

    import torch

    import sdy_amd

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    M, T, nv = args.members, args.steps + 1, args.vars
    H, W = bench.NLAT, bench.NLON
    names = [f"var{v:02d}" for v in range(nv)]
    pred_all = fields(dev, "noise", nv, M, T, seed=11)
    tgt_all = fields(dev, "noise", nv, 1, T, seed=12)
    pred = {n: pred_all[i].view(1, M, T, H, W).transpose(0, 1) for i, n in enumerate(names)}
    tgt = {n: tgt_all[i] for i, n in enumerate(names)}
    n_bytes = 4 * (pred_all.numel() + tgt_all.numel())
    pin_p = torch.empty(pred_all.shape[1:], dtype=torch.float32, pin_memory=True)
    pin_t = torch.empty(tgt_all.shape[1:], dtype=torch.float32, pin_memory=True)
    dst_p, dst_t = torch.empty_like(pred_all), torch.empty_like(tgt_all)
    out_dir = args.dir or tempfile.mkdtemp(prefix="coarsen_bench_")

    def torch_coarsen(f):
        def run():
            for d, t in ((tgt, 1), (pred, 2)):
                ic = {k: v.narrow(t, 0, 1) for k, v in d.items()}
                rest = {k: v.narrow(t, 1, T - 1).unfold(t, f, f).mean(dim=-1) for k, v in d.items()}
                del ic, rest
        return run

    def d2h():
        for i in range(nv):
            pin_p.copy_(pred_all[i], non_blocking=True)
            pin_t.copy_(tgt_all[i], non_blocking=True)

    def d2d():
        dst_p.copy_(pred_all)
        dst_t.copy_(tgt_all)

    sub = names[:max(1, min(nv, args.write_vars))]
    tgt_sub, pred_sub = {n: tgt[n] for n in sub}, {n: pred[n] for n in sub}

    def d2h_sub():
        for i in range(len(sub)):
            pin_p.copy_(pred_all[i], non_blocking=True)
            pin_t.copy_(tgt_all[i], non_blocking=True)

    fns = {"d2d": d2d, "d2h": d2h, "d2h_sub": d2h_sub}
    for f in (2, 6):
        tc = sdy_amd.TimeCoarsen(Null(), f)
        fns[f"coarsen_f{f}"] = lambda tc=tc: tc.append_batch(tgt, pred, 0, 0)
        fns[f"torch_f{f}"] = torch_coarsen(f)
    writers = {}
    for f in (1, 2, 6):
        n_t = (T - 1) // f + 1
        wr = sdy_amd.PredictionDataWriter(os.path.join(out_dir, f"f{f}"), 1, n_t, n_ensemble_members=M)
        writers[f] = wr
        front = wr if f == 1 else sdy_amd.TimeCoarsen(wr, f)
        fns[f"write_f{f}"] = lambda front=front, wr=wr: (front.append_batch(tgt_sub, pred_sub, 0, 0), wr.flush())
    try:
        # the kernel path is the torch restatement's arithmetic: factor 2 bit for bit
        got, _ = sdy_amd.data_writer.coarsen_tensors([pred[names[0]]], 1, 2)
        want = torch.cat([pred[names[0]][:, :, :1], pred[names[0]][:, :, 1:].unfold(2, 2, 2).mean(-1)], dim=2)
        assert torch.equal(got[0], want)
        t = timed(fns, args.rounds, args.reps, args.warmup, dev)
    finally:
        if args.dir is None:
            shutil.rmtree(out_dir, ignore_errors=True)
    res = {"tool": "coarsen_bench", "shape": {"members": M, "samples": 1, "times": T, "nlat": H, "nlon": W, "variables": nv},
           "bytes": n_bytes, "write_variables": len(sub), "write_bytes": n_bytes * len(sub) // nv}
    for k, (med, lo) in t.items():
        res[f"{k}_ms"], res[f"{k}_ms_min"] = round(med, 3), round(lo, 3)
    for f in (2, 6):
        res[f"coarsen_f{f}_GBps_read"] = round(n_bytes / (t[f"coarsen_f{f}"][0] * 1e-3) / 1e9, 1)
        res[f"coarsen_f{f}_over_torch"] = round(t[f"coarsen_f{f}"][0] / t[f"torch_f{f}"][0], 3)
        res[f"coarsen_f{f}_over_d2d"] = round(t[f"coarsen_f{f}"][0] / t["d2d"][0], 3)
    res["d2d_GBps_read_plus_write"] = round(2 * n_bytes / (t["d2d"][0] * 1e-3) / 1e9, 1)
    res["d2h_GBps"] = round(n_bytes / (t["d2h"][0] * 1e-3) / 1e9, 1)
    for f in (1, 2, 6):
        res[f"write_f{f}_over_d2h"] = round(t[f"write_f{f}"][0] / t["d2h_sub"][0], 3)
    res["kernel_not_slower_than_torch"] = all(res[f"coarsen_f{f}_over_torch"] <= 1.0 for f in (2, 6))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
