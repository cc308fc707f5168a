#!/usr/bin/env python3
"""Golden vectors of the ensemble time-mean statistics, by RUNNING THE REFERENCE'S OWN class on CPU (build container only; the
reference is imported through tools/ref_shims.py as tools/gen_golden.py does):

    python tools/gen_golden_time_mean_ensemble.py        # writes tests/golden/fx_time_mean_ensemble.npz

`src.evaluation.aggregators.time_mean.TimeMeanAggregator(is_ensemble=True)` takes one `record_batch` per counted time step:
`(B, H, W)` targets and `(M, B, H, W)` generated data (clones: it keeps the first batch's tensors).  The fixture stores the same
timeline cut into windows as sdy_amd receives them -- `(B, T, H, W)` targets, `(M, B, T, H, W)` gen, the first window with the
initial condition in front, which is not counted -- and the reference's logs twice: `ref32` on the float32 inputs (what the
reference returns) and `ref64`, the same class on the inputs cast to float64.

Cases `(M, B, H, W)` and the counted steps of their windows:
    m3_b2_6x8     (3, 2, 6, 8)    2 + 2    two variables; baseline
    m2_b3_7x10    (2, 3, 7, 10)   2 + 1    two variables; HW = 70: scalar loads
    m25_b1_16x32  (25, 1, 16, 32) 3 + 2    the headline member count: remainders of the loads in flight, 300 pairs
    m5_b2_18x36   (5, 2, 18, 36)  3 + 2 + 2
Inputs: target = a fixed climatology 280 + 20 randn(H, W) plus 3 randn per step, gen = the same plus 0.5, weights = cos(lat)
(1 + 0.1 rand)."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import ref_shims  # noqa: E402

ref_shims.install()

OUT = os.path.join(ROOT, "tests", "golden")
CASES = (("m3_b2_6x8", (3, 2, 6, 8), (2, 2), ("a", "b")),
         ("m2_b3_7x10", (2, 3, 7, 10), (2, 1), ("a", "b")),
         ("m25_b1_16x32", (25, 1, 16, 32), (3, 2), ("a",)),
         ("m5_b2_18x36", (5, 2, 18, 36), (3, 2, 2), ("a",)))


def main(tag="fx_time_mean_ensemble"):
    from src.evaluation.aggregators.time_mean import TimeMeanAggregator

    g = torch.Generator(device="cpu").manual_seed(314159)
    out, cases = {}, []
    for cname, (M, B, H, W), counted, names in CASES:
        S = sum(counted)
        lat = (torch.arange(H, dtype=torch.float64) + 0.5) / H * np.pi - np.pi / 2
        weights = (torch.cos(lat)[:, None] * (1.0 + 0.1 * torch.rand(H, W, generator=g, dtype=torch.float64))).float()
        target, gen = {}, {}
        for k in names:      # time 0 is the initial condition (the same for every member), times 1 .. S are counted
            clim = 280.0 + 20.0 * torch.randn(H, W, generator=g)
            target[k] = clim + 3.0 * torch.randn(B, S + 1, H, W, generator=g)
            gen[k] = clim + 3.0 * torch.randn(M, B, S + 1, H, W, generator=g) + 0.5
            gen[k][:, :, 0] = target[k][:, 0]
        out[f"{cname}::weights"] = weights.numpy()
        done = 0
        for i, n in enumerate(counted):                   # window i: counted times done + 1 .. done + n
            first = 0 if i == 0 else done + 1             # the first window carries the initial condition in front
            for k in names:
                out[f"{cname}::w{i}::target::{k}"] = target[k][:, first:done + n + 1].numpy()
                out[f"{cname}::w{i}::gen::{k}"] = gen[k][:, :, first:done + n + 1].numpy()
            done += n
        keys = None
        for tagp, dt in (("ref32", torch.float32), ("ref64", torch.float64)):
            agg = TimeMeanAggregator(is_ensemble=True, area_weights=weights.to(dt), verbose=False)
            for s in range(1, S + 1):
                agg.record_batch(target_data={k: target[k][:, s].to(dt).clone() for k in names},
                                 gen_data={k: gen[k][:, :, s].to(dt).clone() for k in names})
            logs, media = agg._get_logs()
            assert media == {} and (keys is None or keys == list(logs))
            keys = list(logs)
            out[f"{cname}::{tagp}"] = np.asarray([float(logs[k]) for k in keys], np.float64)
        cases.append(dict(name=cname, M=M, B=B, H=H, W=W, counted=list(counted), names=list(names), keys=keys))
    out["cases"] = json.dumps(cases)
    path = os.path.join(OUT, f"{tag}.npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < (1 << 20), os.path.getsize(path)
    print(f"{tag}: {[c['name'] for c in cases]}; {os.path.getsize(path)} bytes, saved")
    for c in cases:
        d = np.abs(out[f"{c['name']}::ref32"] - out[f"{c['name']}::ref64"]).max()
        print(f"  {c['name']}: keys {c['keys'][:5]} ..., max |ref32 - ref64| {d:.2e}")


if __name__ == "__main__":
    torch.set_num_threads(8)
    main()
