"""Wavenumber-frequency (Wheeler-Kiladis) spectra of a tropical field, gen against target, on the device: whether a long rollout
has an MJO, whether Kelvin and equatorial Rossby waves move at the right speed, whether eastward power exceeds westward power
where it should.  The reference has nothing of the kind, and none of the other aggregators sees organised, propagating
variability: `TimeVariabilityAggregator` stops at lag 1 at a grid point, the degree spectra know nothing of time.  The
definition is `csrc/spacetime.h`: direct sums in float64 in a fixed order, so every output has the same bits in any layout,
batch, run and cut of the run into windows.

Out of scope: the smoothed background and the signal-to-background ratio, dispersion curves, plots, per-member outputs, masks,
cross-spectra between variables, ragged rank shares.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, List, Mapping, Optional, Sequence, Tuple

import torch

from ._lib import (SDY_ST_MAX_LON, SDY_ST_MAX_PAIRS, SDY_ST_MAX_SEGMENT, SdySpacetimeAppendArgs, SdySpacetimeSegmentPowerArgs,
                   check, current_stream, lib, ptr)
from .windows import FieldAccumulator, WindowLayout, fill_window, runs, whole_ics_message, window_layouts

#: the detrend modes of `sdy_spacetime_segment_power`, by name
DETREND = {"none": 0, "mean": 1, "linear": 2}
COMPONENTS = ("symmetric", "antisymmetric")
#: name -> (component, k_min, k_max, period_min_days, period_max_days); k is signed, positive meaning eastward
DEFAULT_BANDS = {
    "mjo_east": ("symmetric", 1, 3, 30.0, 96.0),
    "mjo_west": ("symmetric", -3, -1, 30.0, 96.0),
    "kelvin": ("symmetric", 1, 14, 2.5, 20.0),
    "rossby": ("symmetric", -10, -1, 10.0, 48.0),
}
#: the default largest zonal wavenumber (or W // 2 on a coarser grid)
DEFAULT_MAX_WAVENUMBER = 32
_SYMMETRY_TOLERANCE = 1e-6


def band_pairs(lats, lat_max: float = 15.0) -> Tuple[List[int], List[int]]:
    """The (north row, mirror row) pairs of the latitudes `lats` (degrees, strictly monotone, mirror-symmetric) with `0 <= lat
    <= lat_max`, in order of increasing |lat|; on an odd number of rows the equator row pairs with itself."""
    lat = [float(x) for x in lats]
    H = len(lat)
    if H < 1:
        raise ValueError("lats is empty")
    if any(math.isnan(x) for x in lat):
        raise ValueError("lats holds a NaN")
    up = all(b > a for a, b in zip(lat, lat[1:]))
    down = all(b < a for a, b in zip(lat, lat[1:]))
    if H > 1 and not (up or down):
        raise ValueError("lats must be strictly monotone")
    worst = max(abs(lat[h] + lat[H - 1 - h]) for h in range(H))
    if worst > _SYMMETRY_TOLERANCE:
        raise ValueError(f"lats must be mirror-symmetric about the equator (|lats[h] + lats[H-1-h]| <= {_SYMMETRY_TOLERANCE:g}), "
                         f"got {worst:g}")
    if not float(lat_max) >= 0.0:
        raise ValueError(f"lat_max must not be negative, got {lat_max!r}")
    north = [h for h in range(H) if lat[h] >= lat[H - 1 - h] and abs(lat[h]) <= float(lat_max)]
    north.sort(key=lambda h: abs(lat[h]))
    return north, [H - 1 - h for h in north]


def tukey_taper(N: int, p: float) -> List[float]:
    """w_n = w_{N-1-n} = 0.5 (1 - cos(pi (n + 0.5) / m)) for n < m = floor(p N / 2), 1 elsewhere; m == 0 gives all ones."""
    m = int(math.floor(p * N / 2))
    w = [1.0] * N
    for n in range(m):
        w[n] = w[N - 1 - n] = 0.5 * (1.0 - math.cos(math.pi * (n + 0.5) / m))
    return w


def circle_table(n: int) -> List[float]:
    """(cos(2 pi i / n), sin(2 pi i / n)), i = 0 .. n - 1, interleaved: the tables the two entry points take."""
    out = []
    for i in range(n):
        t = 2.0 * math.pi * i / n
        out += [math.cos(t), math.sin(t)]
    return out


class SpaceTimeSpectra:
    """What `SpaceTimeSpectrumAggregator` computes: the latitudes of the grid, the variables, the segments and the bands.

    `lats` (H, degrees) must be strictly monotone and mirror-symmetric; the band is every row with `|lat| <= lat_max`, taken as
    (north row, mirror row) pairs.  Segments of `segment_length` counted times (4 .. 1024) start every `hop` counted times
    (default `segment_length // 2`).  `max_wavenumber` defaults to `min(32, W // 2)`, resolved on the first window.  `detrend` is
    "none", "mean" or "linear"; `taper` the Tukey fraction p in [0, 1]; `timestep_hours` the spacing of the counted times.
    `bands` maps a name to `(component, k_min, k_max, period_min_days, period_max_days)`, component "symmetric" or
    "antisymmetric", k signed with positive meaning eastward (default: `DEFAULT_BANDS`)."""

    def __init__(self, lats, variables: Sequence[str], segment_length: int, hop: Optional[int] = None,
                 max_wavenumber: Optional[int] = None, lat_max: float = 15.0, detrend: str = "linear", taper: float = 0.2,
                 timestep_hours: float = 6.0, bands: Optional[Mapping[str, tuple]] = None):
        self.variables = list(variables)
        if len(self.variables) == 0:
            raise ValueError("variables=[] selects nothing")
        self.lats = [float(x) for x in (lats.tolist() if hasattr(lats, "tolist") else lats)]
        self.north, self.south = band_pairs(self.lats, lat_max)
        self.lat_max = float(lat_max)
        if len(self.north) == 0:
            raise ValueError(f"no latitude row with |lat| <= {self.lat_max:g}")
        if len(self.north) > SDY_ST_MAX_PAIRS:
            raise ValueError(f"{len(self.north)} row pairs in the band, more than {SDY_ST_MAX_PAIRS}")
        self.segment_length = int(segment_length)
        if not 4 <= self.segment_length <= SDY_ST_MAX_SEGMENT:
            raise ValueError(f"segment_length lies in 4..{SDY_ST_MAX_SEGMENT}, got {segment_length!r}")
        self.hop = self.segment_length // 2 if hop is None else int(hop)
        if not 1 <= self.hop <= self.segment_length:
            raise ValueError(f"hop lies in 1..segment_length, got {hop!r}")
        self.max_wavenumber = None if max_wavenumber is None else int(max_wavenumber)
        if self.max_wavenumber is not None and self.max_wavenumber < 0:
            raise ValueError(f"max_wavenumber must not be negative, got {max_wavenumber!r}")
        if detrend not in DETREND:
            raise ValueError(f"detrend is one of {tuple(DETREND)}, got {detrend!r}")
        self.detrend = detrend
        self.taper = float(taper)
        if not 0.0 <= self.taper <= 1.0:
            raise ValueError(f"taper lies in [0, 1], got {taper!r}")
        self.timestep_hours = float(timestep_hours)
        if not self.timestep_hours > 0.0:
            raise ValueError(f"timestep_hours must be positive, got {timestep_hours!r}")
        self.bands: Dict[str, tuple] = {}
        for name, band in (DEFAULT_BANDS if bands is None else bands).items():
            if len(band) != 5 or band[0] not in COMPONENTS:
                raise ValueError(f"band {name!r} is (component, k_min, k_max, period_min_days, period_max_days) with a component "
                                 f"of {COMPONENTS}, got {band!r}")
            comp, k_min, k_max, p_min, p_max = band
            if int(k_min) > int(k_max) or not 0.0 < float(p_min) <= float(p_max):
                raise ValueError(f"band {name!r}: k_min <= k_max and 0 < period_min_days <= period_max_days, got {band!r}")
            self.bands[name] = (comp, int(k_min), int(k_max), float(p_min), float(p_max))

    @property
    def n_pairs(self) -> int:
        return len(self.north)

    def wavenumbers(self, W: int) -> int:
        """K on a grid of W longitudes."""
        K = min(DEFAULT_MAX_WAVENUMBER, W // 2) if self.max_wavenumber is None else self.max_wavenumber
        if K > W // 2:
            raise ValueError(f"max_wavenumber {K} on {W} longitudes: at most {W // 2}")
        return K

    def frequencies(self) -> List[float]:
        """Cycles per day of nu = 0 .. N // 2."""
        N = self.segment_length
        return [nu / (N * self.timestep_hours / 24.0) for nu in range(N // 2 + 1)]

    def band_mask(self, name: str, K: int) -> torch.Tensor:
        """(N // 2 + 1, 2 K + 1) bool: the cells of a band, nu >= 1, k in range and period in range."""
        _, k_min, k_max, p_min, p_max = self.bands[name]
        freq = self.frequencies()
        mask = torch.zeros(len(freq), 2 * K + 1, dtype=torch.bool)
        for nu in range(1, len(freq)):
            if p_min <= 1.0 / freq[nu] <= p_max:
                for k in range(max(k_min, -K), min(k_max, K) + 1):
                    mask[nu, K + k] = True
        return mask


def arrange(P: torch.Tensor) -> torch.Tensor:
    """(..., N, K + 1) two-sided in frequency -> (..., N // 2 + 1, 2 K + 1) one-sided with signed wavenumber -K .. K, positive
    meaning eastward: out[nu][+k] = P[(N - nu) mod N][k], out[nu][-k] = P[nu][k], out[nu][0] their mean at k = 0."""
    N = P.shape[-2]
    nu = torch.arange(N // 2 + 1, device=P.device)
    back = (N - nu) % N
    west = P.index_select(-2, nu)[..., 1:].flip(-1)
    east = P.index_select(-2, back)[..., 1:]
    zero = (P.index_select(-2, nu)[..., :1] + P.index_select(-2, back)[..., :1]) / 2
    return torch.cat([west, zero, east], dim=-1)


class SpaceTimeSpectrumAggregator(FieldAccumulator):
    """Per variable of a `SpaceTimeSpectra` the power of gen (members pooled) and of the target as a function of zonal
    wavenumber and frequency, for the parts of an equatorial band symmetric and antisymmetric about the equator.

    Definition (csrc/spacetime.h; all float64 after the fp32 loads, every value one chain in ascending order).  Per row pair:
    `s = (x_N + x_S) / 2`, `a = (x_N - x_S) / 2`.  Per fold and `k = 0 .. K`: `c[k] = (1 / W) sum_j y[j] (cos t - i sin t)`, `t =
    2 pi ((k j) mod W) / W`: a direct sum, any W.  Counted time n goes to slot `n mod N` of a ring.  Segment s covers the counted
    times `s hop .. s hop + N - 1`; when its last time is stored every column (trajectory, pair, fold, k) is detrended
    (none / mean / least-squares line), tapered (Tukey) and transformed along time, `P_f = |X_f|^2 / (N sum w^2)`, and added over
    members and pairs.  Times after the last complete segment are left out.  There is no masking: a non-finite value in the
    band makes the affected cells NaN, for good.

    `record_batch(loss, target_data, gen_data, target_data_norm, gen_data_norm, i_time_start)` is what `run_inference` calls once
    per window: targets `(samples, time, lat, lon)`, gen `(members, samples, time, lat, lon)` (a 4-D gen is one member).  Only the
    specification's variables are read, in place, the member-stacked transposed view included.  Time 0 of a run is the initial
    condition and is not counted.  The first accepted window may start anywhere and fixes the grid and the member and sample
    counts; every later one must repeat them and start where the one before ended (`ValueError` otherwise).  The ring -- 16 bytes
    x (members x samples + samples) x N x pairs x 2 x (K + 1) per variable -- and the accumulators are allocated on the first
    window, after their bytes are compared with `max_bytes` (default: a quarter of the device's memory); a workspace of half
    the ring's size follows with the first segment.  The host cuts a window's append at segment ends, so a window may
    complete several segments.  A refused window changes nothing.  Ragged shares (flat rows with `sample_weights`) are refused.

    `get_data()` returns float64 device tensors: `gen/<var>` and `target/<var>` `(samples, 2, N // 2 + 1, 2 K + 1)` -- component 0
    symmetric, 1 antisymmetric; frequency nu = 0 .. N // 2; wavenumber -K .. K, positive eastward -- the mean over segments,
    members and pairs; `frequency` (cycles per day), `wavenumber`, `n_segments`.  `cos(2 pi (k0 j / W - f0 n / N))` lands at `(nu =
    f0, +k0)` with power 1/4.  `ValueError("No data recorded ...")` before any collective when no segment is complete.

    `get_logs(label)` returns Python floats: per band `power_gen/<band>/<var>`, `power_target/<band>/<var>` (the sum of the band's
    cells, averaged over samples) and `power_ratio/<band>/<var>`; with `mjo_east` and `mjo_west`, `east_west_ratio_gen/<var>` and
    `east_west_ratio_target/<var>`.  The raw sums and the sample counts are added over ranks in ONE `dist.reduce_sum` before any
    division; a band without a cell gives NaN."""

    accepts_sample_weights = True      # (to see, and refuse, a ragged share)
    _job_words = "member count, sample count"
    _acc_words = "float64 coefficients and accumulators"

    def __init__(self, spec: SpaceTimeSpectra, dist=None, target: str = "denorm", metadata=None,
                 max_bytes: Optional[int] = None):
        if not isinstance(spec, SpaceTimeSpectra):
            raise ValueError(f"expected a sdy_amd.SpaceTimeSpectra, got {type(spec).__name__}")
        if target not in ("norm", "denorm"):
            raise ValueError(f"target must be 'norm' or 'denorm', got {target!r}")
        super().__init__(dist=dist, metadata=metadata, max_bytes=max_bytes)      # (no time axis)
        self._spec = spec
        self._target = target
        self._K: Optional[int] = None              # resolved on the first window
        self._n_times = 0                          # counted times so far
        self._n_segments = 0
        self._next_start: Optional[int] = None     # where the next window has to start (None before the first window)
        self._tables: Dict[str, torch.Tensor] = {}

    def _statistics(self) -> Dict[str, float]:
        return {"coef": 0.0, "acc": 0.0}

    @staticmethod
    def _job(l: WindowLayout) -> tuple:
        return (l.n0, l.n1, l.H, l.W)

    def _elements(self, stat: str, job: tuple) -> int:
        M, B, _, _ = job
        N, K1 = self._spec.segment_length, self._K + 1
        if stat == "coef":
            return (M * B + B) * N * self._spec.n_pairs * 2 * K1 * 2
        return 2 * B * 2 * N * K1

    def _size_words(self, names, jobs) -> str:
        M, B, _, _ = jobs[0]
        return (f"8 bytes x ({M * B + B} trajectories x {self._spec.n_pairs} pairs x 2 parts + 2 sides x {B} samples) x 2 folds x "
                f"{self._spec.segment_length} slots x {self._K + 1} wavenumbers x {len(names)} variables")

    @property
    def n_times(self) -> int:
        """Counted times so far."""
        return self._n_times

    @property
    def n_segments(self) -> int:
        """Complete segments so far."""
        return self._n_segments

    def _table(self, key: str, values: Sequence[float], device) -> torch.Tensor:
        if key not in self._tables:
            self._tables[key] = torch.tensor(values, dtype=torch.float64).to(device)
        return self._tables[key]

    @torch.no_grad()
    def record_batch(self, loss, target_data, gen_data, target_data_norm=None, gen_data_norm=None, i_time_start: int = 0,
                     sample_weights: Optional[Sequence[float]] = None):
        del loss
        if self._target == "norm":
            target_data, gen_data = target_data_norm, gen_data_norm
        who = type(self).__name__
        ragged = sample_weights is not None or any(
            g.dim() == 4 and k in target_data and target_data[k].dim() == 4 and g.shape[0] != target_data[k].shape[0]
            for k, g in gen_data.items())
        if ragged:
            raise ValueError(whole_ics_message(who))
        start = int(i_time_start)
        if start < 0:
            raise ValueError(f"i_time_start must not be negative, got {start}")
        spec = self._spec
        names = spec.variables
        missing = [k for k in names if k not in gen_data]
        if missing:
            raise ValueError(f"no generated variable {missing[0]!r} in the window, but its space-time spectrum was asked for")
        lay = window_layouts(target_data, {k: gen_data[k] for k in names})
        if self._next_start is not None and start != self._next_start:
            raise ValueError(f"{who}: a window that starts at time {start}, where the one before ended at "
                             f"{self._next_start}: the segments need every window of a run, in order")
        H, W = lay[0].H, lay[0].W
        if any((l.H, l.W) != (H, W) for l in lay) or H != len(spec.lats):
            raise ValueError(f"{who}: the variables share the grid of the specification's {len(spec.lats)} latitudes, got "
                             f"{[(l.H, l.W) for l in lay]}")
        if W > SDY_ST_MAX_LON:
            raise ValueError(f"{who}: {W} longitudes, more than {SDY_ST_MAX_LON}")
        had = self._K
        self._K = spec.wavenumbers(W) if had is None else had
        try:
            device = self._prepare(list(names), lay)
        except Exception:
            self._K = had
            raise
        N, hop, R, K = spec.segment_length, spec.hop, spec.n_pairs, self._K
        lon_table = self._table("lon", circle_table(W), device)
        T = lay[0].T
        t = 1 if start == 0 else 0                     # the very first time of a run is the initial condition
        with torch.cuda.device(device):
            while t < T:
                end = self._n_segments * hop + N - 1   # the last counted time of the next segment to complete
                take = min(T - t, end - self._n_times + 1)
                for first, last in runs(lay, lambda l: l.extents):
                    a = SdySpacetimeAppendArgs()
                    fill_window(a.win, lay, first, last)
                    a.H, a.W, a.R, a.K = H, W, R, K
                    for p in range(R):
                        a.north[p], a.south[p] = spec.north[p], spec.south[p]
                    a.lon_table, a.t0, a.t1, a.n_first, a.N = ptr(lon_table), t, t + take, self._n_times, N
                    a.coef = self._at("coef", first)
                    check(lib.sdy_spacetime_append(C.byref(a), current_stream()), "sdy_spacetime_append")
                self._n_times += take
                t += take
                if self._n_times - 1 == end:
                    self._segment(lay, (self._n_segments * hop) % N, device)
                    self._n_segments += 1
        self._next_start = start + T

    def _segment(self, lay: List[WindowLayout], first_slot: int, device) -> None:
        spec = self._spec
        N, R, K = spec.segment_length, spec.n_pairs, self._K
        M, B = self._grids[0][:2]
        taper = self._table("taper", tukey_taper(N, spec.taper), device)
        time_table = self._table("time", circle_table(N), device)
        ws_bytes = lib.sdy_spacetime_workspace_bytes(len(lay), M, B, N, R, K)   # (a run of variables needs no more)
        if ws_bytes == 0:
            raise ValueError(f"{type(self).__name__}: the workspace of a segment is out of range")
        if "ws" not in self._tables:
            self._tables["ws"] = torch.empty(ws_bytes // 8, dtype=torch.float64, device=device)
        for first, last in runs(lay, lambda l: l.extents):
            a = SdySpacetimeSegmentPowerArgs()
            a.coef, a.nvars, a.M, a.B, a.N, a.R, a.K = self._at("coef", first), last - first, M, B, N, R, K
            a.first_slot, a.detrend = first_slot, DETREND[spec.detrend]
            a.taper, a.time_table, a.acc = ptr(taper), ptr(time_table), self._at("acc", first)
            a.ws, a.ws_bytes = ptr(self._tables["ws"]), ws_bytes
            check(lib.sdy_spacetime_segment_power(C.byref(a), current_stream()), "sdy_spacetime_segment_power")

    def _recorded(self) -> None:
        # (raised BEFORE any collective: every rank of a job must have completed at least one segment)
        if self._names is None or self._n_segments == 0:
            raise ValueError(f"No data recorded: no segment of {self._spec.segment_length} counted times is complete "
                             f"({self._n_times} counted).")

    def _power(self, i: int) -> Tuple[torch.Tensor, torch.Tensor]:
        """-> (gen, target) `(samples, 2, N // 2 + 1, 2 K + 1)` of variable i."""
        M, B = self._grids[i][:2]
        N, K1, R = self._spec.segment_length, self._K + 1, self._spec.n_pairs
        acc = self._view("acc", i, 2, B, 2, N, K1)
        return arrange(acc[0] / (self._n_segments * M * R)), arrange(acc[1] / (self._n_segments * R))

    @torch.no_grad()
    def get_data(self) -> Dict[str, torch.Tensor]:
        self._recorded()
        device = self._acc["acc"].device
        data: Dict[str, torch.Tensor] = {}
        for i, name in enumerate(self._names):
            data[f"gen/{name}"], data[f"target/{name}"] = self._power(i)
        data["frequency"] = torch.tensor(self._spec.frequencies(), dtype=torch.float64, device=device)
        data["wavenumber"] = torch.arange(-self._K, self._K + 1, dtype=torch.float64, device=device)
        data["n_segments"] = torch.tensor(float(self._n_segments), dtype=torch.float64, device=device)
        return data

    @torch.no_grad()
    def get_logs(self, label: str) -> Dict[str, float]:
        self._recorded()
        spec = self._spec
        device = self._acc["acc"].device
        bands = list(spec.bands)
        masks = {b: spec.band_mask(b, self._K).to(device) for b in bands}
        parts = []
        for i, name in enumerate(self._names):
            B = self._grids[i][1]
            sides = self._power(i)
            for b in bands:
                comp = COMPONENTS.index(spec.bands[b][0])
                parts += [(side[:, comp] * masks[b]).sum().reshape(1) for side in sides]
            parts.append(torch.tensor([float(B)], dtype=torch.float64, device=device))
        packed = self._dist.reduce_sum(torch.cat(parts)).cpu().tolist()
        logs: Dict[str, float] = {}
        nan = float("nan")
        n = 2 * len(bands) + 1
        for i, name in enumerate(self._names):
            row = packed[i * n:(i + 1) * n]
            samples = row[-1]
            power = {}
            for j, b in enumerate(bands):
                some = bool(masks[b].any())
                g, t = (row[2 * j] / samples, row[2 * j + 1] / samples) if some and samples > 0.0 else (nan, nan)
                power[b] = (g, t)
                logs[f"power_gen/{b}/{name}"] = float(g)
                logs[f"power_target/{b}/{name}"] = float(t)
                logs[f"power_ratio/{b}/{name}"] = float(g / t) if t > 0.0 else nan
            if "mjo_east" in power and "mjo_west" in power:
                for side, key in enumerate(("east_west_ratio_gen", "east_west_ratio_target")):
                    e, w = power["mjo_east"][side], power["mjo_west"][side]
                    logs[f"{key}/{name}"] = float(e / w) if w > 0.0 else nan
        return {f"{label}/{k}": v for k, v in logs.items()} if len(label) != 0 else logs


@torch.no_grad()
def space_time_spectrum(x: torch.Tensor, lats, segment_length: int, hop: Optional[int] = None,
                        max_wavenumber: Optional[int] = None, lat_max: float = 15.0, detrend: str = "linear", taper: float = 0.2,
                        timestep_hours: float = 6.0) -> Dict[str, torch.Tensor]:
    """The wavenumber-frequency power of one `(time, lat, lon)` device tensor, every time counted
    (`SpaceTimeSpectrumAggregator`'s definition and arrangement): `power` `(2, N // 2 + 1, 2 K + 1)` float64, `frequency`,
    `wavenumber`, `n_segments`."""
    if x.dim() != 3:
        raise ValueError(f"expected (time, lat, lon), got {tuple(x.shape)}")
    spec = SpaceTimeSpectra(lats, ["x"], segment_length, hop=hop, max_wavenumber=max_wavenumber, lat_max=lat_max,
                            detrend=detrend, taper=taper, timestep_hours=timestep_hours, bands={})
    if x.shape[0] < spec.segment_length:
        raise ValueError(f"No data recorded: {x.shape[0]} times do not fill a segment of {spec.segment_length}")
    agg = SpaceTimeSpectrumAggregator(spec)
    field = {"x": x[None]}
    agg.record_batch(None, field, field, i_time_start=1)       # (time 0 of a run is not counted: this is not time 0)
    data = agg.get_data()
    return {"power": data["target/x"][0], "frequency": data["frequency"], "wavenumber": data["wavenumber"],
            "n_segments": data["n_segments"]}
