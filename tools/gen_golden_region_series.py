#!/usr/bin/env python3
"""Golden vectors of the regional metric series, by RUNNING THE REFERENCE'S OWN class on CPU (build container only; the
reference is imported through tools/ref_shims.py as tools/gen_golden.py does):

    python tools/gen_golden_region_series.py        # writes tests/golden/fx_region_series.npz

The reference has no regions: a region is its inference `MeanAggregator`
(src/ace_inference/core/aggregator/inference/reduced.py) with `area_weights = area * fraction`, one aggregator per region, fed
three windows the way run_inference feeds them (the first window keeps its initial condition), an ensemble case (M = 3, two
samples) and a deterministic one.  Every series is stored twice: `ref32` on the float32 inputs (what the reference returns)
and `ref64`, the same class on the inputs and the fp32 weight maps cast to float64 -- the yardstick of a kernel whose per-point
arithmetic is float64.

Grid 16 x 32 (cell centres: latitudes -84.375 .. 84.375, longitudes 0 .. 348.75).  Regions, as (H, W) fp32 maps
`area * fraction` rounded once:
    global     every cell
    band       the rows with -30 <= lat <= 30
    wrap_box   20 <= lat <= 70, 300 <= lon or lon <= 60: a box across 0 degrees
    fraction   a seeded fraction in [0, 1] per cell, a tenth of the cells exactly 0
    cell       the single cell (row 5, column 7)
Inputs as in gen_mean_series: target = 1 + 2 randn, gen = target + 0.2 + 0.5 randn (rmse stays away from 0).

The archive is written with fixed zip time stamps: running the tool again gives the same bytes."""
import io
import json
import os
import sys
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import ref_shims  # noqa: E402

ref_shims.install()

OUT = os.path.join(ROOT, "tests", "golden")
E, S, T, H, W = 3, 2, 3, 16, 32
NAMES = ["a", "b"]
BAND = (-30.0, 30.0)
WRAP_BOX = dict(lat=(20.0, 70.0), lon=(300.0, 60.0))
CELL = (5, 7)


def save_npz(path, arrays):
    """np.savez_compressed with fixed member time stamps (numpy stamps the members with the current time)."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(a), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue())


def main(tag="fx_region_series"):
    from src.ace_inference.core import metrics as M
    from src.ace_inference.core.aggregator.inference.reduced import MeanAggregator

    class NoDist:            # single process: reduce_mean is the identity
        def reduce_mean(self, t):
            return t

    g = torch.Generator(device="cpu").manual_seed(2718)
    lats = torch.linspace(-84.375, 84.375, H)
    lons = torch.arange(W, dtype=torch.float32) * (360.0 / W)
    area = M.spherical_area_weights(lats, W).double().numpy()
    la, lo = lats.double().numpy(), lons.double().numpy()
    frac = torch.rand(H, W, generator=g, dtype=torch.float64).numpy()
    frac[torch.rand(H, W, generator=g).numpy() < 0.1] = 0.0
    cell = np.zeros((H, W))
    cell[CELL] = 1.0
    fractions = {
        "global": np.ones((H, W)),
        "band": np.broadcast_to(((la >= BAND[0]) & (la <= BAND[1]))[:, None], (H, W)).astype(np.float64),
        "wrap_box": (((la >= WRAP_BOX["lat"][0]) & (la <= WRAP_BOX["lat"][1]))[:, None]
                     & ((lo >= WRAP_BOX["lon"][0]) | (lo <= WRAP_BOX["lon"][1]))[None, :]).astype(np.float64),
        "fraction": frac,
        "cell": cell,
    }
    regions = list(fractions)
    maps = np.stack([(area * fractions[r]).astype(np.float32) for r in regions])
    n_timesteps = 1 + 3 * T
    out = dict(lats=lats.numpy(), lons=lons.numpy(), area=area.astype(np.float32), names=json.dumps(NAMES),
               regions=json.dumps(regions), weights=maps, fraction=frac, n_timesteps=np.int64(n_timesteps),
               definitions=json.dumps(dict(band=BAND, wrap_box=WRAP_BOX, cell=CELL)))
    for is_ens in (True, False):
        key = "ens" if is_ens else "det"
        windows, i_time = [], 0
        for win in range(3):
            nt = T + 1 if win == 0 else T
            tgt = {n: torch.randn(S, nt, H, W, generator=g) * 2.0 + 1.0 for n in NAMES}
            shp = (E, S, nt, H, W) if is_ens else (S, nt, H, W)
            gen = {n: (tgt[n][None] if is_ens else tgt[n]) + torch.randn(*shp, generator=g) * 0.5 + 0.2 for n in NAMES}
            windows.append((i_time, tgt, gen))
            for n in NAMES:
                out[f"{key}::tgt{win}::{n}"] = tgt[n].numpy()
                out[f"{key}::gen{win}::{n}"] = gen[n].numpy()
            out[f"{key}::i_time_start{win}"] = np.int64(i_time)
            i_time += nt
        metrics = None
        for tagp, dt in (("ref32", torch.float32), ("ref64", torch.float64)):
            for r, region in enumerate(regions):
                agg = MeanAggregator(torch.from_numpy(maps[r]).to(dt), target="denorm", n_timesteps=n_timesteps,
                                     is_ensemble=is_ens, dist=NoDist(), device=torch.device("cpu"))
                for start, tgt, gen in windows:
                    t64 = {n: v.to(dt) for n, v in tgt.items()}
                    g64 = {n: v.to(dt) for n, v in gen.items()}
                    agg.record_batch(loss=0.0, target_data=t64, gen_data=g64, target_data_norm=t64, gen_data_norm=g64,
                                     i_time_start=start)
                seen = []
                for d in agg._get_series_data():
                    if "grad_mag" in d.metric_name:
                        continue
                    out[f"{key}::{tagp}::{d.metric_name}/{region}/{d.var_name}"] = np.asarray(d.data, dtype=np.float64)
                    seen.append(d.metric_name)
                assert metrics is None or metrics == sorted(set(seen))
                metrics = sorted(set(seen))
        out[f"{key}::metrics"] = json.dumps(metrics)
    path = os.path.join(OUT, f"{tag}.npz")
    save_npz(path, out)
    assert os.path.getsize(path) < (1 << 20), os.path.getsize(path)
    print(f"{tag}: regions {regions}; {os.path.getsize(path)} bytes, saved")
    for key in ("ens", "det"):
        d = max(np.abs(out[k] - out[k.replace("ref32", "ref64")]).max() for k in out if k.startswith(f"{key}::ref32::"))
        print(f"  {key}: metrics {json.loads(out[f'{key}::metrics'])}, max |ref32 - ref64| {d:.2e}")


if __name__ == "__main__":
    torch.set_num_threads(8)
    main()
