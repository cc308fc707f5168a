#!/usr/bin/env python3
"""Price of the spell-duration statistics (`sdy_amd.EventSpellAggregator`) on the BASELINE headline job's window (one device).

    timeout -k 10 900 python tools/spell_bench.py --rounds 5 --reps 3 --warmup 2

One `record_batch` of a window as `run_inference` hands it over: 63 variables, predictions (25 members, 1 initial condition, 7
times, 180 x 360) as the member-stacked VIEW of the IC-major batch, targets (1, 7, 180, 360), at `i_time_start > 0` so that all
7 times are counted and read, and not the run's first window, so that the state is read as well as written.  The fields are
AR(1) series along time (x_t = 0.8 x_{t-1} + 0.6 eps), so that spells exist, last and end at a realistic rate.  Timed with
device events, in the same run and alternating:
  * `record_batch` of the spells for E = 1 and E = 4 events on every variable (`sdy_event_spell_accumulate`: one launch for the
    63 variables; of E events the first is a threshold map, the others scalars, above and below alternating);
  * `TimeVariabilityAggregator.record_batch` on the same window: the same traversal -- one lane owns a trajectory's points over
    the window's times and a state that is read and written once -- with 32 bytes of state per trajectory-point instead of
    16 E, and no LDS;
  * `EventVerificationAggregator.record_batch` (pooled slots) with the same events: the same compares, no state;
  * a device-to-device copy of the bytes the kernels read from the window (what one pass over the data costs at this size on
    this device);
  * `get_logs` of the spells (torch integer arithmetic over the whole state, once per run of inference).
The spell kernel reads every input value once (`bytes`) and reads and writes the state, 16 bytes per event, trajectory and grid
point (`state_bytes_e<E>`, both directions): `spells_e<E>_GBps` = (bytes + state bytes) / time, to be held against the copy's
read + write rate (`share_of_copy`).  There is no target ratio.  Prints ONE JSON line; for the kernels alone run it under
`rocprofv3 --kernel-trace --stats` with `--rounds 1`: `spell_kernel`, `variability_kernel`, `event_table_kernel`.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import bench  # noqa: E402
from hist_bench import timed  # noqa: E402

COUNTS = (1, 4)


def ar1_fields(device, n_vars, rows, times, seed):
    """(n_vars, rows, times, H, W) on the device: x_t = 0.8 x_{t-1} + 0.6 eps along time, stationary from the first time on."""
    import torch

    g = torch.Generator(device=device).manual_seed(seed)
    x = torch.randn(n_vars, rows, times, bench.NLAT, bench.NLON, device=device, generator=g)
    for t in range(1, times):
        x[:, :, t] = 0.8 * x[:, :, t - 1] + 0.6 * x[:, :, t]
    return x


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
    pred_all = ar1_fields(dev, nv, M, T, seed=11)
    tgt_all = ar1_fields(dev, nv, 1, T, seed=12)
    pred = {n: pred_all[i].view(1, M, T, H, W).transpose(0, 1) for i, n in enumerate(names)}
    tgt = {n: tgt_all[i] for i, n in enumerate(names)}
    n_bytes = 4 * (pred_all.numel() + tgt_all.numel())
    state_bytes = {E: 2 * 16 * E * nv * (M + 1) * H * W for E in COUNTS}
    tv_state_bytes = 2 * 32 * nv * (M + 1) * H * W
    area = sdy_amd.metrics.spherical_area_weights(torch.linspace(-89.5, 89.5, H), W).to(dev)
    lat = torch.linspace(-1.0, 1.0, H).view(H, 1).expand(H, W)
    scalars = (-0.3, 0.8, -0.8)

    def events(E):
        ev = sdy_amd.Events()
        for i, n in enumerate(names):
            ev.add(n, "above_map", above=0.3 + 0.1 * torch.cos(1.5 * lat + i))
            for e in range(1, E):
                ev.add(n, f"s{e}", **{"below" if e % 2 else "above": scalars[e - 1]})
        return ev

    n_steps = T * (4 + (args.warmup + args.rounds * args.reps) * 2)
    spells = {E: sdy_amd.EventSpellAggregator(events(E), area, n_timesteps=n_steps, max_bytes=state_bytes[E]) for E in COUNTS}
    tables = {E: sdy_amd.EventVerificationAggregator(events(E), area, n_timesteps=2 * T, pool_times=True) for E in COUNTS}
    tv = sdy_amd.TimeVariabilityAggregator(area, max_bytes=tv_state_bytes)
    starts = {}

    def in_order(key, agg):          # the same window again, as the run's next one
        starts[key] = T

        def record():
            agg.record_batch(0.0, tgt, pred, tgt, pred, i_time_start=starts[key])
            starts[key] += T
        return record

    fns = {f"spells_e{E}": in_order(f"spells_e{E}", spells[E]) for E in COUNTS}
    fns["variability"] = in_order("variability", tv)
    for E in COUNTS:
        fns[f"table_e{E}"] = (lambda a: lambda: a.record_batch(0.0, tgt, pred, tgt, pred, i_time_start=T))(tables[E])
    for E in COUNTS:
        fns[f"spells_e{E}"]()
        fns[f"spells_e{E}"]()
    # one spot check against torch before anything is timed: variable 0's map event after two windows
    c = events(1).of(names[0])[0].map.to(dev)
    inside = pred_all[0] > c                                                                 # (M, T, H, W)
    want_hits = 2 * inside.sum(dim=1).double()
    run = torch.zeros(M, H, W, dtype=torch.int64, device=dev)
    longest = run.clone()
    for _ in range(2):
        for t in range(T):
            run = torch.where(inside[:, t], run + 1, torch.zeros_like(run))
            longest = torch.maximum(longest, run)
    for E in COUNTS:
        got = spells[E].get_data()
        assert torch.equal(got[f"gen_hits/above_map/{names[0]}"][:, 0], want_hits)
        assert torch.equal(got[f"gen_longest/above_map/{names[0]}"][:, 0], longest.double())
    del got, inside, run, longest, want_hits
    dst_p, dst_t = torch.empty_like(pred_all), torch.empty_like(tgt_all)

    def d2d():
        dst_p.copy_(pred_all)
        dst_t.copy_(tgt_all)

    fns["d2d"] = d2d
    t = timed(fns, args.rounds, args.reps, args.warmup, dev)
    t.update(timed({f"get_logs_e{E}": (lambda a: lambda: a.get_logs(""))(spells[E]) for E in COUNTS}, 1, 2, 1, dev))
    res = {"tool": "spell_bench", "shape": {"members": M, "samples": 1, "times": T, "nlat": H, "nlon": W, "variables": nv},
           "bytes": n_bytes, "variability_state_bytes": tv_state_bytes}
    d2d_rate = 2 * n_bytes / (t["d2d"][0] * 1e-3) / 1e9
    res.update(d2d_copy_ms=round(t["d2d"][0], 3), d2d_GBps_read_plus_write=round(d2d_rate, 1))
    for k in [k for k in fns if k != "d2d"] + [f"get_logs_e{E}" for E in COUNTS]:
        res[f"{k}_ms"], res[f"{k}_ms_min"] = round(t[k][0], 3), round(t[k][1], 3)
    res["variability_GBps"] = round((n_bytes + tv_state_bytes) / (t["variability"][0] * 1e-3) / 1e9, 1)
    for E in COUNTS:
        k = f"spells_e{E}"
        res[f"state_bytes_e{E}"] = state_bytes[E]
        res[f"{k}_GBps"] = round((n_bytes + state_bytes[E]) / (t[k][0] * 1e-3) / 1e9, 1)
        res[f"{k}_share_of_copy"] = round(res[f"{k}_GBps"] / d2d_rate, 3)
        res[f"{k}_over_variability"] = round(t[k][0] / t["variability"][0], 3)
        res[f"{k}_over_table"] = round(t[k][0] / t[f"table_e{E}"][0], 3)
        res[f"{k}_counted_times"] = spells[E].n_times
    logs = spells[1].get_logs("")
    res["mean_duration_gen_var00"] = round(logs[f"mean_duration_gen/above_map/{names[0]}"], 4)
    res["onset_rate_gen_var00"] = round(logs[f"onset_rate_gen/above_map/{names[0]}"], 4)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
