#!/usr/bin/env python3
"""Price of the neighbourhood verification (`sdy_amd.FractionsSkillAggregator`) on the BASELINE headline job's window (one
device).

    timeout -k 10 600 python tools/fss_bench.py --rounds 5 --reps 3 --warmup 2

One `record_batch` of a window as `run_inference` hands it over: 63 variables, predictions (25 members, 1 initial condition, 7
times, 180 x 360) as the member-stacked VIEW of the IC-major batch, targets (1, 7, 180, 360), at `i_time_start > 0` so that all
7 times are counted and read; one event per variable (above a threshold map), radii (1, 3, 7).  Timed with device events, in
the same run and alternating:
  * `FractionsSkillAggregator.record_batch` (`sdy_fss_accumulate`: both launches for the 63 variables);
  * its first launch alone (`sdy_fss_encode`: reads the window once, writes the 16-bit codes) and its second alone
    (`sdy_fss_sum`: the box sums of the codes, per radius);
  * `EventVerificationAggregator.record_batch` of the same events and its launch alone (`sdy_event_table_accumulate`): it
    reads the same bytes, and is what the first launch is judged by;
  * a device-to-device copy of the bytes the kernels read (what one pass over the data costs at this size on this device).
These two are the yardsticks; there is no target ratio.  `*_input_GBps` = window bytes / time; `code_bytes` is what the first
launch writes (the second reads it once per radius, its bands' halo rows again).  Prints ONE JSON line; for the kernels alone
run it under `rocprofv3 --kernel-trace --stats` with `--rounds 1`: `fss_encode_kernel`, `fss_sum_kernel`.
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
    ap.add_argument("--vars", type=int, default=bench.STATE_CH)
    ap.add_argument("--radii", type=int, nargs="+", default=[1, 3, 7])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3, help="repetitions per variant and round")
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()

    import torch

    import sdy_amd
    from sdy_amd._lib import check, current_stream, lib

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    M, T, nv, radii = args.members, args.steps + 1, args.vars, tuple(args.radii)
    H, W = bench.NLAT, bench.NLON
    names = [f"var{v:02d}" for v in range(nv)]
    pred_all = fields(dev, "smooth", nv, M, T, seed=11)
    tgt_all = fields(dev, "smooth", nv, 1, T, seed=12)
    pred = {n: pred_all[i].view(1, M, T, H, W).transpose(0, 1) for i, n in enumerate(names)}
    tgt = {n: tgt_all[i] for i, n in enumerate(names)}
    n_bytes = 4 * (pred_all.numel() + tgt_all.numel())
    area = sdy_amd.metrics.spherical_area_weights(torch.linspace(-89.5, 89.5, H), W).to(dev)
    clim = tgt_all.mean(dim=(1, 2)).cpu()                                                    # (nv, H, W): every event happens
    events = sdy_amd.Events()
    for i, n in enumerate(names):
        events.add(n, "above_mean", above=clim[i])
    fss = sdy_amd.FractionsSkillAggregator(events, radii, area, n_timesteps=2 * T)
    table = sdy_amd.EventVerificationAggregator(events, area, n_timesteps=2 * T)
    for agg in (fss, table):
        agg.record_batch(0.0, tgt, pred, tgt, pred, i_time_start=T)
    # one spot check against torch before anything is timed: variable 0, every radius, sum for sum
    c = clim[0].to(dev)
    k = (pred_all[0] > c).sum(dim=0).double()                                                # (T, H, W)
    o = (tgt_all[0, 0] > c).double()
    got = fss.get_data()

    def box(x, r):
        h = sum(torch.roll(x, d, dims=-1) for d in range(-r, r + 1))
        return torch.stack([h[:, max(0, lat - r):min(H - 1, lat + r) + 1].sum(dim=1) for lat in range(H)], dim=1)

    for r in radii:
        K, O = box(k, r), box(o, r)
        want = torch.stack([torch.full_like(K, 1.0), K, O, K * K, K * O, O * O], dim=-1).sum(dim=2)      # (T, H, 6)
        have = got[f"sums_r{r}/above_mean/{names[0]}"]
        assert torch.equal(have[T:], want) and float(have[:T].sum()) == 0.0, r
    dst_p, dst_t = torch.empty_like(pred_all), torch.empty_like(tgt_all)

    def d2d():
        dst_p.copy_(pred_all)
        dst_t.copy_(tgt_all)

    def record(agg):
        return lambda: agg.record_batch(0.0, tgt, pred, tgt, pred, i_time_start=T)

    # the two launches alone, on the arguments record_batch builds (one call: the 63 variables' codes fit the workspace)
    _, lay = fss._layouts(tgt, pred)
    chunks = list(fss._chunks(lay))
    assert chunks == [(0, nv)], chunks
    a = fss._args(lay, 0, nv, 0, T)

    a_table = table._args(table._layouts(tgt, pred)[1], 0, nv, 0, T, "table")

    def stage(fn, name, args):
        return lambda: check(fn(C.byref(args), current_stream()), name)

    fns = {"fss_record": record(fss), "fss_encode": stage(lib.sdy_fss_encode, "sdy_fss_encode", a),
           "fss_sum": stage(lib.sdy_fss_sum, "sdy_fss_sum", a), "event_table_record": record(table),
           "event_table_launch": stage(lib.sdy_event_table_accumulate, "sdy_event_table_accumulate", a_table), "d2d": d2d}
    t = timed(fns, args.rounds, args.reps, args.warmup, dev)
    res = {"tool": "fss_bench", "shape": {"members": M, "samples": 1, "times": T, "nlat": H, "nlon": W, "variables": nv,
                                          "events": 1, "radii": list(radii)},
           "bytes": n_bytes, "code_bytes": 2 * nv * T * H * W}
    for key in ("fss_record", "fss_encode", "fss_sum", "event_table_record", "event_table_launch"):
        res[f"{key}_ms"], res[f"{key}_ms_min"] = round(t[key][0], 3), round(t[key][1], 3)
    for key in ("fss_record", "fss_encode", "event_table_record", "event_table_launch"):
        res[f"{key}_input_GBps"] = round(n_bytes / (t[key][0] * 1e-3) / 1e9, 1)
    d2d_rate = 2 * n_bytes / (t["d2d"][0] * 1e-3) / 1e9
    res.update(d2d_copy_ms=round(t["d2d"][0], 3), d2d_GBps_read_plus_write=round(d2d_rate, 1))
    res["encode_over_event_table"] = round(t["fss_encode"][0] / t["event_table_launch"][0], 3)
    res["sum_over_encode"] = round(t["fss_sum"][0] / t["fss_encode"][0], 3)
    logs = fss.get_logs("")
    for r in radii:
        res[f"fss_r{r}_var00"] = round(logs[f"fss_r{r}/above_mean/{names[0]}"], 4)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
