#!/usr/bin/env python3
"""Price of the threshold-event verification (`sdy_amd.EventVerificationAggregator`) on the BASELINE headline job's window (one
device).

    timeout -k 10 600 python tools/event_bench.py --rounds 5 --reps 3 --warmup 2

One `record_batch` of a window as `run_inference` hands it over: 63 variables, predictions (25 members, 1 initial condition, 7
times, 180 x 360) as the member-stacked VIEW of the IC-major batch, targets (1, 7, 180, 360), at `i_time_start > 0` so that all
7 times are counted and read.  Timed with device events, in the same run and alternating:
  * `record_batch` of the event tables for E = 1, 4 and 8 events on every variable (`sdy_event_table_accumulate`: one launch for
    the 63 variables; of E events the first is a threshold map, the others scalars, above and below alternating);
  * the same with `frequency_maps=True` (`sdy_event_frequency_accumulate`: a second pass over the same bytes);
  * `RankHistogramAggregator.record_batch` on the same window: the same traversal and the same LDS ownership with one compare
    per member value instead of E;
  * a device-to-device copy of the bytes the kernels read (what one pass over the data costs at this size on this device).
These two are the yardsticks; there is no target ratio.  `*_input_GBps` = bytes / time.  `table_words_ms_e<E>` is the time the
copy's rate gives to reading E x 2 x (M + 1) words per accumulator row: what the tables add to the rank histograms' traffic.
Prints ONE JSON line; for the kernels alone run it under `rocprofv3 --kernel-trace --stats` with `--rounds 1`:
`event_table_kernel`, `event_frequency_kernel`.
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

COUNTS = (1, 4, 8)


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
    n_bytes = 4 * (pred_all.numel() + tgt_all.numel())
    area = sdy_amd.metrics.spherical_area_weights(torch.linspace(-89.5, 89.5, H), W).to(dev)
    # thresholds from the targets' own climate, so that every event happens: the time mean as a map, quantiles as scalars
    clim = tgt_all.mean(dim=(1, 2)).cpu()                                                    # (nv, H, W)
    quant = torch.quantile(tgt_all[:, 0, 0].reshape(nv, -1).cpu(), torch.linspace(0.2, 0.8, 7), dim=1)      # (7, nv)

    def events(E):
        ev = sdy_amd.Events()
        for i, n in enumerate(names):
            ev.add(n, "above_mean", above=clim[i])
            for e in range(1, E):
                ev.add(n, f"q{e}", **{"below" if e % 2 else "above": float(quant[e - 1, i])})
        return ev

    aggs = {}
    for E in COUNTS:
        aggs[f"table_e{E}"] = sdy_amd.EventVerificationAggregator(events(E), area, n_timesteps=2 * T)
        aggs[f"table_maps_e{E}"] = sdy_amd.EventVerificationAggregator(events(E), area, n_timesteps=2 * T, frequency_maps=True)
    rank = sdy_amd.RankHistogramAggregator(area, n_timesteps=2 * T)
    for agg in aggs.values():
        agg.record_batch(0.0, tgt, pred, tgt, pred, i_time_start=T)
    # one spot check against torch before anything is timed: variable 0's first event, bin by bin
    c = clim[0].to(dev)
    k = (pred_all[0] > c).sum(dim=0)                                                         # (T, H, W)
    o = tgt_all[0, 0] > c
    want = torch.stack([torch.stack([((k == b) & (o == bool(oo))).sum(dim=-1) for b in range(M + 1)], dim=-1) for oo in (0, 1)],
                       dim=-2).double()                                                      # (T, H, 2, M + 1)
    for E in COUNTS:
        got = aggs[f"table_e{E}"].get_data()[f"table/above_mean/{names[0]}"]
        assert torch.equal(got[T:], want) and float(got[:T].sum()) == 0.0
    got = aggs["table_maps_e4"].get_data()
    assert torch.equal(got[f"counted/above_mean/{names[0]}"], torch.full((H, W), float(T), dtype=torch.float64, device=dev))
    assert torch.equal(got[f"frequency_gen/above_mean/{names[0]}"], k.sum(dim=0).double() / (M * T))
    dst_p, dst_t = torch.empty_like(pred_all), torch.empty_like(tgt_all)

    def d2d():
        dst_p.copy_(pred_all)
        dst_t.copy_(tgt_all)

    def record(agg):
        return lambda: agg.record_batch(0.0, tgt, pred, tgt, pred, i_time_start=T)

    fns = {k: record(a) for k, a in aggs.items()}
    fns.update(rank_hist_record=record(rank), d2d=d2d)
    t = timed(fns, args.rounds, args.reps, args.warmup, dev)
    res = {"tool": "event_bench", "shape": {"members": M, "samples": 1, "times": T, "nlat": H, "nlon": W, "variables": nv},
           "bytes": n_bytes}
    for k in list(aggs) + ["rank_hist_record"]:
        res[f"{k}_ms"], res[f"{k}_ms_min"] = round(t[k][0], 3), round(t[k][1], 3)
        res[f"{k}_input_GBps"] = round(n_bytes / (t[k][0] * 1e-3) / 1e9, 1)
    d2d_rate = 2 * n_bytes / (t["d2d"][0] * 1e-3) / 1e9
    res.update(d2d_copy_ms=round(t["d2d"][0], 3), d2d_GBps_read_plus_write=round(d2d_rate, 1))
    for E in COUNTS:
        words = nv * T * H * E * 2 * (M + 1) * 8                 # float64 accumulator words, read and written once per row
        res[f"table_words_ms_e{E}"] = round(2 * words / (d2d_rate * 1e9) * 1e3, 4)
        res[f"table_e{E}_over_rank_hist"] = round(t[f"table_e{E}"][0] / t["rank_hist_record"][0], 3)
    logs = aggs["table_e4"].get_logs("")
    res["brier_skill_score_var00"] = round(logs[f"brier_skill_score/above_mean/{names[0]}"], 4)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
