"""Price of the post-step corrector on the headline window, per step: 25 members, 34 prognostic variables, K = 8 levels of
specific total water, 180 x 360.  Times, with events on the stream, (a) the three launches of `sdy_corrector` on the stepper's
packed normalised tensors, in place, (b) the copy of `g` the stepper makes before it, and (c) a device copy of as many bytes
as the reduce pass reads (2K + 5 planes per member), the bandwidth yardstick.  The stepper window itself (about 150 ms of
sampling per step on the headline job) is not run here: compare with `bench.py`'s per-step figure.  Prints one JSON line.

    python tools/corrector_bench.py [--members 25] [--vars 34] [--reps 50] [--mode advection_and_precipitation]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sdy_amd  # noqa: E402

ADV = "tendency_of_total_water_path_due_to_advection"


def timed(fn, reps):
    for _ in range(5):
        fn()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    best = float("inf")
    for _ in range(3):
        start.record()
        for _ in range(reps):
            fn()
        stop.record()
        stop.synchronize()
        best = min(best, start.elapsed_time(stop) * 1e3 / reps)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, default=25)
    ap.add_argument("--vars", type=int, default=34)
    ap.add_argument("--levels", type=int, default=8)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--mode", default="advection_and_precipitation")
    a = ap.parse_args()
    B, n, K, H, W = a.members, a.vars, a.levels, 180, 360
    HW = H * W
    names = [f"specific_total_water_{k}" for k in range(K)] + ["PRESsfc", "LHTFLsfc", "PRATEsfc", ADV]
    names += [f"v{i}" for i in range(n - len(names))]
    means = {m: 0.0 for m in names}
    stds = {m: 1.0 for m in names}
    for k in range(K):
        means[f"specific_total_water_{k}"], stds[f"specific_total_water_{k}"] = 10.0 ** (-6 + 4 * k / max(K - 1, 1)), 10.0 ** (-7 + 4 * k / max(K - 1, 1))
    means.update(PRESsfc=1.0e5, LHTFLsfc=80.0, PRATEsfc=3.0e-5)
    stds.update({"PRESsfc": 3.0e3, "LHTFLsfc": 20.0, "PRATEsfc": 5.0e-6, ADV: 1.0e-5})
    ak = torch.tensor([3.0, 5238.4, 11815.8, 17263.1, 19929.5, 17023.4, 8970.5, 1537.5, 0.0])
    bk = torch.tensor([0.0, 0.0, 0.0115, 0.0781, 0.2034, 0.4004, 0.6513, 0.9065, 1.0])
    assert K == 8, "the benchmark carries the 8-level coordinate only"

    class Sigma:
        pass

    Sigma.ak, Sigma.bk = ak, bk
    lat = (torch.arange(H, dtype=torch.float64) + 0.5) / H * torch.pi - torch.pi / 2
    area = torch.cos(lat)[:, None].expand(H, W).float()
    corr = sdy_amd.CorrectorConfig(conserve_dry_air=True, zero_global_mean_moisture_advection=True,
                                   moisture_budget_correction=a.mode).build(area, Sigma)
    packed = corr.bind(names, names, means, stds)
    g0 = torch.Generator(device="cuda").manual_seed(1)
    state = torch.randn(B, n, H, W, device="cuda", generator=g0)
    gen = state + 0.05 * torch.randn(B, n, H, W, device="cuda", generator=g0)
    work = gen.clone()
    ws = packed.workspace(B, HW, gen.device)
    planes = 2 * K + 5
    src = torch.empty(B, planes, HW, device="cuda")
    dst = torch.empty_like(src)
    res = dict(members=B, variables=n, levels=K, grid=[H, W], mode=a.mode, launches_per_step=3,
               reduce_read_bytes=B * planes * HW * 4,
               corrector_us=round(timed(lambda: packed(state, work, ws), a.reps), 2),
               clone_of_g_us=round(timed(lambda: work.copy_(gen), a.reps), 2),
               copy_of_read_bytes_us=round(timed(lambda: dst.copy_(src), a.reps), 2))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
