"""Price of the dry-air conservation series on the headline window: 25 members, 7 times (a horizon-6 window with its initial
condition), K = 8 levels of specific total water, 180 x 360.  Times, with events on the stream, (a) the two launches of
`sdy_dry_air_series` on `(B, T, H, W)` timelines as the stepper holds them (result and workspace allocated per call, as the
stepper does), and (b) a device-to-device copy of as many bytes as the reduce pass reads (K + 1 planes per member and time;
the weights stay in L2), the bandwidth yardstick.  The working set (408 MB read, twice that for the copy) is larger than the
256 MB last-level cache, so neither side is served from it.  Prints one JSON line.

    python tools/conservation_bench.py [--members 25] [--times 7] [--reps 50]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sdy_amd  # noqa: E402


def timed(fn, reps):
    for _ in range(5):
        fn()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    best, runs = float("inf"), []
    for _ in range(5):
        start.record()
        for _ in range(reps):
            fn()
        stop.record()
        stop.synchronize()
        runs.append(start.elapsed_time(stop) * 1e3 / reps)
        best = min(best, runs[-1])
    return best, sorted(runs)[len(runs) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, default=25)
    ap.add_argument("--times", type=int, default=7)
    ap.add_argument("--reps", type=int, default=50)
    a = ap.parse_args()
    B, T, K, H, W = a.members, a.times, 8, 180, 360
    HW = H * W

    class Sigma:
        ak = torch.tensor([3.0, 5238.4, 11815.8, 17263.1, 19929.5, 17023.4, 8970.5, 1537.5, 0.0])
        bk = torch.tensor([0.0, 0.0, 0.0115, 0.0781, 0.2034, 0.4004, 0.6513, 0.9065, 1.0])

    lat = (torch.arange(H, dtype=torch.float64) + 0.5) / H * torch.pi - torch.pi / 2
    area = torch.cos(lat)[:, None].expand(H, W).float()
    series = sdy_amd.conservation.DryAirSeries(area, Sigma)
    g0 = torch.Generator(device="cuda").manual_seed(1)
    data = {f"specific_total_water_{k}": 10.0 ** (-6 + 4 * k / 7) * (1.0 + torch.rand(B, T, H, W, device="cuda", generator=g0))
            for k in range(K)}
    data["PRESsfc"] = 1.0e5 + 3.0e3 * torch.randn(B, T, H, W, device="cuda", generator=g0)
    src = torch.empty(B * T, K + 1, HW, device="cuda")
    dst = torch.empty_like(src)
    read = B * T * (K + 1) * HW * 4
    series_us, series_med = timed(lambda: series(data), a.reps)
    copy_us, copy_med = timed(lambda: dst.copy_(src), a.reps)
    res = dict(members=B, times=T, levels=K, grid=[H, W], launches=2, read_bytes=read,
               series_us=round(series_us, 2), series_median_us=round(series_med, 2),
               series_read_gbps=round(read / series_us * 1e-3, 1),
               copy_of_read_bytes_us=round(copy_us, 2), copy_median_us=round(copy_med, 2),
               copy_read_gbps=round(read / copy_us * 1e-3, 1))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
