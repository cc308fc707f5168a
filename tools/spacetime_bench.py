#!/usr/bin/env python3
"""Price of the wavenumber-frequency spectra (`sdy_amd.SpaceTimeSpectrumAggregator`) on the BASELINE headline job's window (one
device) and on a segment of `--segment` slots.

    timeout -k 10 900 python tools/spacetime_bench.py --rounds 5 --reps 3 --warmup 2

Timed with device events, in the same run and alternating:
  * `record_batch` of one window as `run_inference` hands it over -- predictions (25 members, 1 initial condition, 7 times, 180
    x 360) as the member-stacked VIEW of the IC-major batch, targets (1, 7, 180, 360), one variable, the default band (30 rows)
    and K = 32 -- once where no segment completes and once where the window's last time completes one (the aggregator's
    host-side counters are set back before every call: the ring does not mind what it holds);
  * the two launches alone: `sdy_spacetime_append` of the 7 times and `sdy_spacetime_segment_power` of one segment;
  * a device-to-device copy of the band's bytes (what the append reads);
  * a torch float64 restatement at the same shapes: the stored band folded and `torch.fft.rfft` along longitude (the append),
    and detrend, taper, `torch.fft.fft` along time, |X|^2 and the sums over members and pairs on the ring (the segment).  Its
    results are compared with the kernels' before anything is timed.
No time is fixed in advance.  Prints ONE JSON line; for the kernels alone run it under `rocprofv3 --kernel-trace --stats` with
`--rounds 1`: `spacetime_store_kernel`, `spacetime_power_kernel`, `spacetime_sum_kernel`.
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
from hist_bench import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, default=bench.MEMBERS)
    ap.add_argument("--steps", type=int, default=bench.HORIZON, help="forecast steps of one window")
    ap.add_argument("--segment", type=int, default=384, help="slots of a segment (96 days of 6-hourly times)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3, help="repetitions per variant and round")
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()

    import torch

    import sdy_amd
    from sdy_amd import _lib
    from sdy_amd.spacetime import circle_table, tukey_taper
    from sdy_amd.windows import fill_window, window_layouts

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    M, T, N = args.members, args.steps + 1, args.segment
    H, W = bench.NLAT, bench.NLON
    g = torch.Generator(device=dev).manual_seed(11)
    pred_all = torch.randn(1, M, T, H, W, device=dev, generator=g)
    tgt = {"pr": torch.randn(1, T, H, W, device=dev, generator=g)}
    pred = {"pr": pred_all.transpose(0, 1)}
    lats = [90.0 - (h + 0.5) * 180.0 / H for h in range(H)]
    spec = sdy_amd.SpaceTimeSpectra(lats, ["pr"], N)
    R, K = spec.n_pairs, spec.wavenumbers(W)
    agg = sdy_amd.SpaceTimeSpectrumAggregator(spec)
    start = 7

    def record(n_times):
        def fn():
            agg._n_times, agg._n_segments, agg._next_start = n_times, 0, start
            agg.record_batch(0.0, tgt, pred, i_time_start=start)
        return fn

    record(N - T)()                                   # allocates; the window's last time completes segment 0
    assert agg.n_segments == 1
    n_traj = M + 1
    coef = agg._view("coef", 0, n_traj, N, R, 2, K + 1, 2)

    # the two launches alone
    lay = window_layouts(tgt, pred)
    lon_table = torch.tensor(circle_table(W), dtype=torch.float64, device=dev)
    a = _lib.SdySpacetimeAppendArgs()
    fill_window(a.win, lay, 0, 1)
    a.H, a.W, a.R, a.K = H, W, R, K
    for p in range(R):
        a.north[p], a.south[p] = spec.north[p], spec.south[p]
    a.lon_table, a.t0, a.t1, a.n_first, a.N, a.coef = lon_table.data_ptr(), 0, T, 0, N, coef.data_ptr()

    def append():
        _lib.check(sdy_amd.lib.sdy_spacetime_append(C.byref(a), _lib.current_stream()), "sdy_spacetime_append")

    ring = torch.randn(coef.shape, dtype=torch.float64, device=dev, generator=g)
    taper = torch.tensor(tukey_taper(N, spec.taper), dtype=torch.float64, device=dev)
    time_table = torch.tensor(circle_table(N), dtype=torch.float64, device=dev)
    acc = torch.zeros(2, 1, 2, N, K + 1, dtype=torch.float64, device=dev)
    ws_bytes = sdy_amd.lib.sdy_spacetime_workspace_bytes(1, M, 1, N, R, K)
    ws = torch.empty(ws_bytes // 8, dtype=torch.float64, device=dev)
    b = _lib.SdySpacetimeSegmentPowerArgs()
    b.coef, b.nvars, b.M, b.B, b.N, b.R, b.K = ring.data_ptr(), 1, M, 1, N, R, K
    b.first_slot, b.detrend = 0, 2
    b.taper, b.time_table, b.acc, b.ws, b.ws_bytes = taper.data_ptr(), time_table.data_ptr(), acc.data_ptr(), ws.data_ptr(), ws_bytes

    def segment():
        _lib.check(sdy_amd.lib.sdy_spacetime_segment_power(C.byref(b), _lib.current_stream()), "sdy_spacetime_segment_power")

    # the torch restatement
    rows_n = torch.tensor(spec.north, device=dev)
    rows_s = torch.tensor(spec.south, device=dev)

    def torch_append():
        out = []
        for x in (pred_all[0], tgt["pr"]):                              # (rows, T, H, W)
            xn, xs = x[:, :, rows_n].double(), x[:, :, rows_s].double()
            y = torch.stack([(xn + xs) / 2, (xn - xs) / 2], dim=3)      # (rows, T, R, 2, W)
            out.append(torch.fft.rfft(y, dim=-1)[..., :K + 1] / W)
        return torch.cat(out)                                           # (n_traj, T, R, 2, K + 1) complex

    d = torch.arange(N, dtype=torch.float64, device=dev) - (N - 1) / 2
    shape = (1, N, 1, 1, 1)

    def torch_segment():
        z = torch.view_as_complex(ring)                                 # (n_traj, N, R, 2, K + 1)
        y = z - z.mean(dim=1, keepdim=True)
        y = y - d.view(shape) * ((d.view(shape) * z).sum(dim=1, keepdim=True) / (d * d).sum())
        X = torch.fft.fft(y * taper.view(shape), dim=1)
        P = (X.real ** 2 + X.imag ** 2) / (N * (taper * taper).sum())
        return torch.stack([P[:M].sum(dim=(0, 2)), P[M:].sum(dim=(0, 2))]).permute(0, 2, 1, 3)    # (2, 2, N, K + 1)

    append()
    got = torch.view_as_complex(coef[:, :T])
    assert (got - torch_append()).abs().max() <= 1e-12 * float(pred_all.abs().max())
    segment()
    want = torch_segment()
    assert (acc[:, 0] - want).abs().max() <= 1e-12 * 25 * float(ring.abs().max()) ** 2 * N * M * R
    band = torch.empty(n_traj * T * 2 * R * W, dtype=torch.float32, device=dev)
    band_dst = torch.empty_like(band)

    fns = {"record_batch": record(0), "record_batch_with_segment": record(N - T), "append": append, "segment_power": segment,
           "d2d_band": lambda: band_dst.copy_(band), "torch_append": torch_append, "torch_segment": torch_segment}
    t = timed(fns, args.rounds, args.reps, args.warmup, dev)
    res = {"tool": "spacetime_bench", "shape": {"members": M, "samples": 1, "times": T, "nlat": H, "nlon": W, "band_rows": 2 * R,
                                                "max_wavenumber": K, "segment": N},
           "band_bytes": band.numel() * 4, "ring_bytes": coef.numel() * 8, "workspace_bytes": ws_bytes,
           "segment_flop": 8 * n_traj * R * 2 * (K + 1) * N * N}
    for k in fns:
        res[f"{k}_ms"], res[f"{k}_ms_min"] = round(t[k][0], 3), round(t[k][1], 3)
    res["segment_power_GFLOPs"] = round(res["segment_flop"] / (t["segment_power"][0] * 1e-3) / 1e9, 1)
    res["append_over_torch"] = round(t["append"][0] / t["torch_append"][0], 3)
    res["segment_over_torch"] = round(t["segment_power"][0] / t["torch_segment"][0], 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
