#!/usr/bin/env python3
"""Price of DYffusion forward conditioning on the BASELINE headline job (one device, one process).

    timeout -k 10 900 python tools/fcond_bench.py --steps 6 --warmup 2

The job of bench.py's headline (25 members, 180 x 360, E = 256, 8 blocks, horizon 6, interpolator dropout on, the t6 forecast
fed back as the next window's state), run once per forward_conditioning mode -- "none", "data", "data+noise-v1" -- with the
forecaster widened by the 63 channels of x_0 for the two conditioned modes (_base_experiment.num_conditional_channels).
Same weights seeds and states for every mode.  Prints ONE JSON line: member-forecast-steps/s per mode (wall clock over
`--steps` windows after `--warmup`), the ratio to "none", and the concat stage's milliseconds per launch from one profiled
window and of one forecaster forward (ops.stage_timer; event records between launches: not a timed region).
"""
import argparse
import gc
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402  (constants, synthetic_state, one_pass: the headline job's own pieces)

MODES = ("none", "data", "data+noise-v1")


def build(mode, device):
    import torch

    from sdy_amd import InterpolationExperiment, MultiHorizonForecastingDYffusion, synthetic

    cs, nf, hz = bench.STATE_CH, bench.FORCING_CH, bench.HORIZON
    n_fwd = 0 if mode == "none" else cs
    shape = dict(nlat=bench.NLAT, nlon=bench.NLON, embed=bench.EMBED, layers=bench.LAYERS)
    with torch.cuda.device(device):
        fnet = synthetic.build_network(cs, cs, nf + n_fwd, time_range=(0.0, hz - 1.0), weight_seed=4321, **shape)
        inet = synthetic.build_network(2 * cs, cs, nf, dropout_mlp=0.1, drop_path_rate=0.1, time_range=(1.0, hz - 1.0),
                                       weight_seed=4322, dropout_seed=1000, **shape)
    return MultiHorizonForecastingDYffusion(fnet, InterpolationExperiment(inet, horizon=hz), horizon=hz,
                                            diffusion_config=dict(forward_conditioning=mode))


def run(mode, device, B, steps, warmup):
    import torch

    from sdy_amd import ops

    exp = build(mode, device)
    x, forc = bench.synthetic_state(0, B, device)
    for _ in range(warmup):
        x = bench.one_pass(exp, x, forc)
    torch.cuda.synchronize(device)
    t0 = time.perf_counter()
    for _ in range(steps):
        x = bench.one_pass(exp, x, forc)
    torch.cuda.synchronize(device)
    dt = time.perf_counter() - t0
    assert bool(torch.isfinite(x).all()), f"{mode}: non-finite state"
    with ops.stage_timer() as st:          # one window: forecaster and interpolator concats together
        bench.one_pass(exp, x, forc)
    n, ms = st.stages.get("concat", (0, 0.0))
    with ops.stage_timer() as sf:          # one forecaster forward: its concat alone (the generated group)
        exp.model.predict_x_last(initial_condition=x, x_t=x, t=2, static_condition=forc)
    nf, msf = sf.stages.get("concat", (0, 0.0))
    del exp
    gc.collect()
    torch.cuda.empty_cache()
    return {"mfs_per_s": round(B * bench.HORIZON * steps / dt, 3), "concat_launches_per_window": n,
            "concat_ms_per_window": round(ms, 3), "forecaster_concat_ms_per_launch": round(msf / max(nf, 1), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=6, help="timed windows per mode")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--members", type=int, default=bench.MEMBERS)
    args = ap.parse_args()
    import torch

    device = torch.device("cuda", 0)
    torch.cuda.set_device(device)
    with torch.inference_mode():
        res = {m: run(m, device, args.members, args.steps, args.warmup) for m in MODES}
    base = res["none"]["mfs_per_s"]
    for m in MODES:
        res[m]["ratio_to_none"] = round(res[m]["mfs_per_s"] / base, 4)
    print(json.dumps({"tool": "fcond_bench", "unit": "member-forecast-steps/s", "members": args.members,
                      "steps": args.steps, "warmup": args.warmup, "modes": res}))


if __name__ == "__main__":
    main()
