#!/usr/bin/env python3
"""Golden vectors of the dry-air conservation diagnostics, by RUNNING THE REFERENCE'S OWN functions and classes on CPU (build
container only; the reference is imported through tools/ref_shims.py as tools/gen_golden.py does):

    python tools/gen_golden_conservation.py        # writes tests/golden/fx_conservation.npz

`compute_dry_air_absolute_differences` (core/aggregator/climate_data.py), `get_dry_air_nonconservation` and `ConservationLoss`
(core/loss.py) and `DerivedMetricsAggregator` (core/aggregator/one_step/derived.py), each on float32 inputs (`ref32`, what the
reference returns) and on the same inputs in float64 (`ref64`, the same formulas evaluated by the reference's own code in
float64).  The global means `gm` are `metrics.weighted_mean(metrics.surface_pressure_due_to_dry_air(...))`, the expression
inside `compute_dry_air_absolute_differences`.

Three sets `(samples, times, levels, lat, lon)`: `b3t3k2` (3, 3, 2, 6, 8), `b2t3k8` (2, 3, 8, 18, 36), `b1t2k1` (1, 2, 1, 6, 8),
each with a `gen` and a `target` timeline of the magnitudes of tests/corrector_utils.py::fields: ps 1e5 +- 3e3 with a 15 Pa mean
drift and 200 Pa of noise per step, q from 1e-6 aloft to 2e-2 at the surface changing by 5 % per step.  The aggregator gets
each set in two batches (the first sample(s), then the last)."""
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
PENALTY = 0.25


def main(tag="fx_conservation"):
    from src.ace_inference.core import metrics
    from src.ace_inference.core.aggregator.climate_data import ClimateData, compute_dry_air_absolute_differences
    from src.ace_inference.core.aggregator.one_step.derived import DerivedMetricsAggregator
    from src.ace_inference.core.data_loading.data_typing import SigmaCoordinates
    from src.ace_inference.core.loss import ConservationLossConfig, get_dry_air_nonconservation

    g = torch.Generator(device="cpu").manual_seed(271828)
    ak8 = [3.0, 5238.4, 11815.8, 17263.1, 19929.5, 17023.4, 8970.5, 1537.5, 0.0]
    bk8 = [0.0, 0.0, 0.0115, 0.0781, 0.2034, 0.4004, 0.6513, 0.9065, 1.0]
    levels = {1: (ak8[::8], bk8[::8]), 2: (ak8[::4], bk8[::4]), 8: (ak8, bk8)}

    def timeline(B, T, K, H, W):
        q_scale = torch.logspace(-6, -2, K) if K > 1 else torch.tensor([1e-2])
        d = {}
        for k in range(K):
            steps = [q_scale[k] * (1.0 + torch.rand(B, H, W, generator=g))]
            for _ in range(T - 1):
                steps.append(steps[-1] * (1.0 + 0.05 * torch.randn(B, H, W, generator=g)))
            d[f"specific_total_water_{k}"] = torch.stack(steps, dim=1)
        steps = [1.0e5 + 3.0e3 * torch.randn(B, H, W, generator=g)]
        for _ in range(T - 1):
            steps.append(steps[-1] + 15.0 + 200.0 * torch.randn(B, H, W, generator=g))
        d["PRESsfc"] = torch.stack(steps, dim=1)
        d["TMP2m"] = 280.0 + torch.randn(B, T, H, W, generator=g)            # an unrelated variable
        return d

    out, sets = {}, []
    for sname, (B, T, K, H, W) in (("b3t3k2", (3, 3, 2, 6, 8)), ("b2t3k8", (2, 3, 8, 18, 36)), ("b1t2k1", (1, 2, 1, 6, 8))):
        lat = (torch.arange(H, dtype=torch.float64) + 0.5) / H * np.pi - np.pi / 2
        area = (torch.cos(lat)[:, None] * (1.0 + 0.1 * torch.rand(H, W, generator=g, dtype=torch.float64))).float()
        ak, bk = (np.asarray(v, np.float32) for v in levels[K])
        sides = {"gen": timeline(B, T, K, H, W), "target": timeline(B, T, K, H, W)}
        split = max(B - 1, 1)
        sets.append(dict(name=sname, B=B, T=T, K=K, H=H, W=W, names=list(sides["gen"]), split=split, penalty=PENALTY))
        out[f"{sname}::ak"], out[f"{sname}::bk"], out[f"{sname}::area"] = ak, bk, area.numpy()
        for side, d in sides.items():
            out.update({f"{sname}::{side}::{k}": v.numpy() for k, v in d.items()})
        for tagp, dt in (("ref32", torch.float32), ("ref64", torch.float64)):
            sigma = SigmaCoordinates(ak=torch.tensor(ak).to(dt), bk=torch.tensor(bk).to(dt))
            w = area.to(dt)
            cast = {side: {k: v.to(dt) for k, v in d.items()} for side, d in sides.items()}
            for side, d in cast.items():
                cd = ClimateData(d)
                gm = metrics.weighted_mean(metrics.surface_pressure_due_to_dry_air(
                    cd.specific_total_water, cd.surface_pressure, sigma.ak, sigma.bk), w, dim=(2, 3))
                absdiff = compute_dry_air_absolute_differences(cd, area=w, sigma_coordinates=sigma)
                mean = get_dry_air_nonconservation(d, area_weights=w, sigma_coordinates=sigma)
                assert gm.dtype == dt and absdiff.shape == (T - 1,) and torch.equal(absdiff, gm.diff(dim=-1).abs().mean(dim=0))
                out[f"{sname}::{side}::{tagp}::gm"] = gm.numpy()
                out[f"{sname}::{side}::{tagp}::absdiff"] = absdiff.numpy()
                out[f"{sname}::{side}::{tagp}::mean"] = mean.numpy()
            m, loss = ConservationLossConfig(dry_air_penalty=PENALTY).build(w, sigma)(cast["gen"])
            assert list(m) == ["dry_air_loss"]
            out[f"{sname}::{tagp}::dry_air_loss"] = m["dry_air_loss"].to(dt).numpy()
            out[f"{sname}::{tagp}::conservation_loss"] = loss.to(dt).numpy()
            agg = DerivedMetricsAggregator(w, sigma)
            for lo, hi in ((0, split), (split, B)) if B > 1 else ((0, 1), (0, 1)):
                agg.record_batch({k: v[lo:hi] for k, v in cast["target"].items()}, {k: v[lo:hi] for k, v in cast["gen"].items()},
                                 None, None)
            logs = agg.get_logs("one_step")
            assert sorted(logs) == ["one_step/surface_pressure_due_to_dry_air/gen", "one_step/surface_pressure_due_to_dry_air/target"]
            for k, v in logs.items():
                out[f"{sname}::{tagp}::logs::{k}"] = v.to(dt).numpy()
    # the paths without the fields and with a single time step, as recorded facts
    sigma = SigmaCoordinates(ak=torch.tensor(levels[2][0]), bk=torch.tensor(levels[2][1]))
    w = torch.ones(6, 8)
    d = timeline(2, 3, 2, 6, 8)
    facts = {}
    for label, data in (("no_pressure", {k: v for k, v in d.items() if k != "PRESsfc"}),
                        ("no_water", {k: v for k, v in d.items() if not k.startswith("specific_total_water_")}),
                        ("one_time", {k: v[:, :1] for k, v in d.items()})):
        absdiff = compute_dry_air_absolute_differences(ClimateData(data), area=w, sigma_coordinates=sigma)
        m, loss = ConservationLossConfig(dry_air_penalty=PENALTY).build(w, sigma)(data)
        step_loss = torch.tensor(1.5)
        step_loss += loss                                   # what core/stepper.py:572 does with it
        facts[label] = dict(absdiff_shape=list(absdiff.shape), absdiff_all_nan=bool(torch.isnan(absdiff).all()),
                            dry_air_loss_is_nan=bool(torch.isnan(m["dry_air_loss"])), loss_is_nan=bool(torch.isnan(step_loss)))
    m, loss = ConservationLossConfig().build(w, sigma)(d)
    facts["no_penalty"] = dict(metrics=list(m), loss=float(loss))
    out["sets"] = json.dumps(sets)
    out["facts"] = json.dumps(facts)
    path = os.path.join(OUT, f"{tag}.npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < (1 << 20), os.path.getsize(path)
    print(f"{tag}: {[s['name'] for s in sets]}; facts {facts}; {os.path.getsize(path)} bytes, saved")


if __name__ == "__main__":
    torch.set_num_threads(8)
    main()
