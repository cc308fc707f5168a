"""The inference loop's data writer: host mirror of `DataWriterConfig` / `DataWriter`
(`src/ace_inference/inference/data_writer/main.py:19-168`), `TimeCoarsen` (`data_writer/time_coarsen.py`) and
`PredictionDataWriter` (`data_writer/prediction.py`), for `run_inference(writer=...)`.

`DataWriter` stacks a `PredictionDataWriter` and a `HistogramDataWriter` (`sdy_amd.histogram`) and wraps each in `TimeCoarsen`
when `time_coarsen` is configured, as the reference does.  The time average runs on the DEVICE, in front of everything else:
one launch per dict (`sdy_time_coarsen`, csrc/coarsen.hip) reads the window driver's tensors in place -- the member-stacked
`(members, samples, time, lat, lon)` view included -- and writes the coarsened dict into one contiguous buffer.  The
histograms behind it never leave the device; the predictions cross to the host after the average, so the bytes of the
device-to-host copy are divided by the coarsening factor.

Deviations from the reference, all on purpose:
  * the reference's `TIME_DIM = 1` (`time_coarsen.py:9`) is the time axis of `(sample, time, lat, lon)` data only; of the
    member-stacked 5-D predictions `run_inference` hands over it is the SAMPLE axis, which the reference would average.  Here
    the time axis is always the third from last, whatever leads it, so a trajectory's values do not depend on how it is stacked;
  * a tail of `batch_times` that does not fill a group is dropped like the tensors' (`unfold` drops it; xarray's
    `coarsen(...).mean()` with its default `boundary="exact"` would raise).  Objects offering `isel` / `coarsen` are driven
    through exactly the reference's calls and keep their own behaviour;
  * a first window that holds the initial condition only is passed on as it is (the reference's `unfold` of the empty remainder
    raises);
  * no xarray / netCDF4: the predictions are written as `.npy` memmaps (`PredictionDataWriter`), the histograms as
    `histograms.npz` (`sdy_amd.histogram`);
  * `save_raw_prediction_names` is documented by the reference's `DataWriterConfig` but never passed on
    (`main.py:52-62`); here `DataWriterConfig.build` passes it and `PredictionDataWriter(save_names=...)` honours it;
  * the video sub-writer (`enable_video_netcdfs`) is out of scope: `NotImplementedError`;
  * the reference attaches histograms for `n_ensemble_members == 1` only; `histogram_ensembles=True` attaches them for
    ensembles too (the device histograms pool the members of a lead time).

GPU only: `TimeCoarsen` raises on CPU tensors, like every module of this package.  `PredictionDataWriter` alone also accepts
host tensors (what `run_inference(host_outputs=True)` hands over) and writes them directly.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import json
import os
from typing import Dict, List, Mapping, Optional, Sequence, Tuple

import numpy as np
import torch

from ._lib import SdyCoarsenArgs, check, current_stream, lib, ptr
from .histogram import HistogramDataWriter
from .windows import runs, strided_layout

TIME_DIM_NAME = "time"


def _require_device(v: torch.Tensor) -> None:
    if not v.is_cuda:
        raise RuntimeError("sdy_amd.data_writer coarsens on the GPU only (no CPU fallback)")


def _launch(a: SdyCoarsenArgs, device: torch.device) -> None:
    with torch.cuda.device(device):
        check(lib.sdy_time_coarsen(C.byref(a), current_stream()), "sdy_time_coarsen")


def coarsen_tensors(tensors: Sequence[torch.Tensor], t_first: int, factor: int) -> Tuple[List[torch.Tensor], Optional[torch.Tensor]]:
    """Every tensor `(..., time, lat, lon)` with its first `t_first` times kept and the rest averaged in groups of `factor`
    (a tail is dropped): -> (outputs, the one float32 buffer they are views of).  Output i has tensor i's leading shape and
    `t_first + (T - t_first) // factor` times.  One `sdy_time_coarsen` per run of consecutive same-shaped tensors (at most
    SDY_MAX_VARS each); inputs are read in place where `sdy_hist_add` would read them in place.  `factor == 1`, `t_first == 0`
    packs the tensors unchanged, bit for bit."""
    if factor < 1:
        raise ValueError(f"coarsen factor must be 1 or greater, got {factor}")
    if not tensors:
        return [], None
    for v in tensors:
        _require_device(v)
    lay = [strided_layout(v) for v in tensors]
    device = tensors[0].device
    offsets, total = [], 0
    for (v, n0, n1, _, _, T, HW), orig in zip(lay, tensors):      # every call is checked before the first one is enqueued
        if v.device != device:
            raise ValueError(f"tensors of one dict on {device} and {v.device}")
        if min(n0, n1, T, HW) < 1:
            raise ValueError("empty tensor")
        if not 0 <= t_first <= T:
            raise ValueError(f"{t_first} initial times of a window of {T}")
        t_out = t_first + (T - t_first) // factor
        if t_out < 1:
            raise ValueError(f"a window of {T} times is shorter than one group of {factor}")
        offsets.append((total, t_out))
        total += (n0 * n1 * t_out * HW + 3) & ~3          # every output stays 16-byte aligned within the buffer
    buf = torch.empty(total, dtype=torch.float32, device=device)
    outs = [buf[o:o + n0 * n1 * t_out * HW].view(*orig.shape[:-3], t_out, *orig.shape[-2:])
            for (o, t_out), (_, n0, n1, _, _, _, HW), orig in zip(offsets, lay, tensors)]
    for first, last in runs(lay, lambda l: l[1:3] + l[5:]):      # consecutive tensors of one shape share a call
        a = SdyCoarsenArgs()
        a.nvars = last - first
        for j in range(first, last):
            v, _, _, s0, s1, _, _ = lay[j]
            a.data[j - first], a.s0[j - first], a.s1[j - first], a.out[j - first] = ptr(v), s0, s1, ptr(outs[j])
        _, a.n0, a.n1, _, _, a.T, a.HW = lay[first]
        a.t_first, a.factor = int(t_first), int(factor)
        _launch(a, device)
    return outs, buf


def _time_select(d: Mapping[str, torch.Tensor], s: slice) -> Dict[str, torch.Tensor]:
    return {k: v[..., s, :, :] for k, v in d.items()}


def _times_select(times, s: slice):
    if times is None:
        return None
    if hasattr(times, "isel"):
        return times.isel({TIME_DIM_NAME: s})
    return times[:, s]


def _times_coarsen(times, factor: int):
    """`batch_times.coarsen(time=factor).mean()`: None passes through; an object with `coarsen` is driven through that call;
    a numpy / torch array (sample, time) becomes the group means (datetime64 included), a tail dropped."""
    if times is None:
        return None
    if hasattr(times, "coarsen"):
        return times.coarsen({TIME_DIM_NAME: factor}).mean()
    n = times.shape[1] // factor
    if isinstance(times, torch.Tensor):
        g = times[:, :n * factor].reshape(times.shape[0], n, factor)
        return g.mean(dim=-1) if g.is_floating_point() else g.to(torch.float64).mean(dim=-1)
    a = np.asarray(times)
    g = a[:, :n * factor].reshape(a.shape[0], n, factor)
    if a.dtype.kind == "M":      # mean of datetimes: the group's first label plus the mean offset, in the array's own unit
        offsets = (g - g[..., :1]).astype(np.int64)
        return g[..., 0] + (offsets.sum(axis=-1) // factor).astype(g.dtype.str.replace("M8", "m8"))
    return g.mean(axis=-1)


@dataclasses.dataclass
class TimeCoarsenConfig:
    """`time_coarsen.py:27-51`.  `coarsen_factor`: an integer 1 or greater; time labels become the mean of their group's."""

    coarsen_factor: int

    def __post_init__(self):
        if self.coarsen_factor < 1:
            raise ValueError(f"coarsen_factor must be 1 or greater, got {self.coarsen_factor}")

    def build(self, data_writer) -> "TimeCoarsen":
        return TimeCoarsen(data_writer=data_writer, coarsen_factor=self.coarsen_factor)

    def n_coarsened_timesteps(self, n_timesteps: int) -> int:
        """Assumes the initial condition is in n_timesteps, and is not coarsened."""
        return ((n_timesteps - 1) // self.coarsen_factor) + 1


class TimeCoarsen:
    """`time_coarsen.py:54-137`: wraps a data writer and coarsens its arguments in time before passing them on.  One
    `sdy_time_coarsen` per source (and run of same-shaped variables) and `append_batch`; the wrapped writer receives device
    tensors that are views of one buffer per source.  The time axis is the third from last (module docstring)."""

    def __init__(self, data_writer, coarsen_factor: int):
        if coarsen_factor < 1:
            raise ValueError(f"coarsen_factor must be 1 or greater, got {coarsen_factor}")
        self._data_writer = data_writer
        self._coarsen_factor = int(coarsen_factor)

    def _coarsen(self, d: Mapping[str, torch.Tensor], t_first: int) -> Dict[str, torch.Tensor]:
        outs, _ = coarsen_tensors(list(d.values()), t_first, self._coarsen_factor)
        return dict(zip(d.keys(), outs))

    def append_batch(self, target: Mapping[str, torch.Tensor], prediction: Mapping[str, torch.Tensor], start_timestep: int,
                     start_sample: int = 0, batch_times=None) -> None:
        f = self._coarsen_factor
        if start_timestep == 0:
            # the initial condition is recorded without coarsening, then the rest of the batch: two views of one launch's output
            tgt, pred = self._coarsen(target, 1), self._coarsen(prediction, 1)
            one, rest = slice(None, 1), slice(1, None)
            self._data_writer.append_batch(_time_select(tgt, one), _time_select(pred, one), 0, start_sample,
                                           _times_select(batch_times, one))
            if all(v.shape[-3] > 1 for v in list(tgt.values()) + list(pred.values())):
                self._data_writer.append_batch(_time_select(tgt, rest), _time_select(pred, rest), 1, start_sample,
                                               _times_coarsen(_times_select(batch_times, rest), f))
            return
        self._data_writer.append_batch(self._coarsen(target, 0), self._coarsen(prediction, 0), ((start_timestep - 1) // f) + 1,
                                       start_sample, _times_coarsen(batch_times, f))

    def flush(self) -> None:
        self._data_writer.flush()


class PredictionDataWriter:
    """`prediction.py::PredictionDataWriter`: the raw targets and predictions of an inference run, as float32 `.npy` memmaps
    under `<path>/autoregressive_predictions/` (no netCDF: module docstring):
        target/<name>.npy       (n_samples, n_timesteps, lat, lon)
        prediction/<name>.npy   ([members,] n_samples, n_timesteps, lat, lon)     members axis iff n_ensemble_members > 1
        index.json              dims, coords["lat" / "lon"], units / long_name from `metadata`, the variable list
    Files are created from the first batch's shapes and filled with NaN: a variable one source never supplies, or a region never
    written, reads NaN (the reference's fill value).  `save_names` restricts the variables (the reference documents
    `save_raw_prediction_names` but never passes it on; `DataWriterConfig.build` here does).

    `append_batch` takes device tensors: one `sdy_time_coarsen` launch with factor 1 packs the selected variables of a source
    into one device buffer, one asynchronous copy on a side stream moves it into pinned host memory (two pinned buffers per
    source, used in turn), and the copy into the memmaps happens when the next batch has been enqueued, or at `flush()` -- so the
    transfer of window i overlaps the compute of window i + 1 (the pattern of `loop._DeferredHostWriter`).  Host tensors are
    written directly.  A batch outside `n_samples` / `n_timesteps` raises ValueError before anything is copied or created."""

    SOURCES = ("target", "prediction")

    def __init__(self, path: str, n_samples: int, n_timesteps: int, metadata: Optional[Mapping[str, object]] = None,
                 coords: Optional[Mapping[str, np.ndarray]] = None, save_names: Optional[Sequence[str]] = None,
                 n_ensemble_members: int = 1):
        if n_samples < 1 or n_timesteps < 1 or n_ensemble_members < 1:
            raise ValueError(f"n_samples, n_timesteps, n_ensemble_members must be positive, got {n_samples}, {n_timesteps}, "
                             f"{n_ensemble_members}")
        self.path = str(path)
        self.directory = os.path.join(self.path, "autoregressive_predictions")
        self.metadata = dict(metadata) if metadata else {}
        self.coords = dict(coords) if coords else {}
        self.save_names = None if save_names is None else list(save_names)
        self._n_samples, self._n_timesteps, self._members = int(n_samples), int(n_timesteps), int(n_ensemble_members)
        self._grid: Optional[Tuple[int, int]] = None
        self._files: Dict[Tuple[str, str], np.memmap] = {}
        self._names: List[str] = []
        self._stream: Optional[torch.cuda.Stream] = None
        self._pinned: Dict[str, List[Optional[torch.Tensor]]] = {s: [None, None] for s in self.SOURCES}
        self._turn = 0
        self._pending = None       # (event, [(source, name, host tensor), ...], start_sample, start_timestep)

    # ---- shapes and bounds
    def _selected(self, data: Mapping[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
        return {k: v for k, v in data.items() if self.save_names is None or k in self.save_names}

    def _check(self, source: str, name: str, v: torch.Tensor, start_timestep: int, start_sample: int) -> None:
        stacked = source == "prediction" and self._members > 1
        if v.dim() != (5 if stacked else 4):
            raise ValueError(f"{source} {name!r}: expected {'(members, ' if stacked else '('}samples, time, lat, lon), got "
                             f"{tuple(v.shape)}")
        if stacked and v.shape[0] != self._members:
            raise ValueError(f"{source} {name!r}: {v.shape[0]} members, the file has {self._members}")
        n, T = v.shape[-4], v.shape[-3]
        if start_sample < 0 or start_sample + n > self._n_samples:
            raise ValueError(f"Batch size {n} starting at sample {start_sample} is too large to fit in the file with sample "
                             f"dimension of length {self._n_samples}.")
        if start_timestep < 0 or start_timestep + T > self._n_timesteps:
            raise ValueError(f"timesteps {start_timestep}..{start_timestep + T - 1} outside the file's {self._n_timesteps}")
        grid = tuple(v.shape[-2:])
        if (self._grid or grid) != grid:
            raise ValueError(f"{source} {name!r}: grid {grid}, the files have {self._grid}")

    def _create(self, names: Sequence[str], grid: Tuple[int, int]) -> None:
        self._grid = grid
        for name in names:
            if name in self._names:
                continue
            self._names.append(name)
            for source in self.SOURCES:
                shape = (self._n_samples, self._n_timesteps) + grid
                if source == "prediction" and self._members > 1:
                    shape = (self._members,) + shape
                os.makedirs(os.path.join(self.directory, source), exist_ok=True)
                mm = np.lib.format.open_memmap(os.path.join(self.directory, source, f"{name}.npy"), mode="w+", dtype=np.float32,
                                               shape=shape)
                mm[...] = np.nan
                self._files[(source, name)] = mm

    # ---- the protocol
    def append_batch(self, target: Mapping[str, torch.Tensor], prediction: Mapping[str, torch.Tensor], start_timestep: int,
                     start_sample: int = 0, batch_times=None) -> None:
        del batch_times
        start_timestep, start_sample = int(start_timestep), int(start_sample)
        picked = {"target": self._selected(target), "prediction": self._selected(prediction)}
        for source, d in picked.items():           # everything is checked before anything is enqueued, created or written
            for name, v in d.items():
                self._check(source, name, v, start_timestep, start_sample)
        every = [v for d in picked.values() for v in d.values()]
        if not every:
            return
        self._create([n for d in picked.values() for n in d], tuple(every[0].shape[-2:]))
        host_now, staged, event = [], [], None
        for source, d in picked.items():
            on_device = {k: v for k, v in d.items() if v.is_cuda}
            host_now += [(source, k, v) for k, v in d.items() if not v.is_cuda]
            if not on_device:
                continue
            outs, buf = coarsen_tensors(list(on_device.values()), 0, 1)
            if self._stream is None or self._stream.device != buf.device:
                self._stream = torch.cuda.Stream(device=buf.device)
            pin = self._pinned[source][self._turn]
            if pin is None or pin.numel() < buf.numel():
                pin = self._pinned[source][self._turn] = torch.empty(buf.numel(), dtype=torch.float32, pin_memory=True)
            self._stream.wait_stream(torch.cuda.current_stream(buf.device))
            with torch.cuda.stream(self._stream):
                pin[:buf.numel()].copy_(buf, non_blocking=True)
                event = torch.cuda.Event()
                event.record(self._stream)
            buf.record_stream(self._stream)
            for name, o in zip(on_device, outs):
                offset = o.data_ptr() - buf.data_ptr()
                staged.append((source, name, pin[offset // 4:offset // 4 + o.numel()].view(o.shape)))
        self._write_pending()                       # the previous batch: its copy finished long ago
        for source, name, v in host_now:
            self._store(source, name, v, start_sample, start_timestep)
        if staged:
            self._pending = (event, staged, start_sample, start_timestep)
            self._turn ^= 1

    def _store(self, source: str, name: str, v: torch.Tensor, start_sample: int, start_timestep: int) -> None:
        a = v.detach().to(torch.float32).numpy()
        n, T = a.shape[-4], a.shape[-3]
        self._files[(source, name)][..., start_sample:start_sample + n, start_timestep:start_timestep + T, :, :] = a

    def _write_pending(self) -> None:
        if self._pending is None:
            return
        event, staged, start_sample, start_timestep = self._pending
        self._pending = None
        # the sources' copies were enqueued in order on one stream: the last event covers them all
        event.synchronize()
        for source, name, v in staged:
            self._store(source, name, v, start_sample, start_timestep)

    def flush(self) -> None:
        self._write_pending()
        for mm in self._files.values():
            mm.flush()
        if self._grid is None:
            return
        dims = {"sample": self._n_samples, "timestep": self._n_timesteps, "lat": self._grid[0], "lon": self._grid[1]}
        if self._members > 1:
            dims["member"] = self._members
        variables = {}
        for name in self._names:
            meta = self.metadata.get(name)
            variables[name] = {k: str(getattr(meta, k)) for k in ("units", "long_name") if getattr(meta, k, None) is not None}
        index = {"sources": list(self.SOURCES), "dims": dims,
                 "layout": {"target": ["sample", "timestep", "lat", "lon"],
                            "prediction": (["member"] if self._members > 1 else []) + ["sample", "timestep", "lat", "lon"]},
                 "coords": {k: np.asarray(self.coords[k], dtype=np.float64).tolist() for k in ("lat", "lon") if k in self.coords},
                 "variables": variables}
        with open(os.path.join(self.directory, "index.json"), "w") as f:
            json.dump(index, f, indent=1)


class DataWriter:
    """`main.py:65-168`: the sub-writers of an inference run behind one `append_batch` / `flush`, each wrapped in `TimeCoarsen`
    when `time_coarsen` is given (`n_timesteps` then counts coarsened steps, the initial condition kept).  `save_names`: see
    `PredictionDataWriter`.  `enable_video_netcdfs=True` is out of scope (NotImplementedError); histograms are attached for
    `n_ensemble_members == 1` as in the reference, or for ensembles too with `histogram_ensembles=True`."""

    def __init__(self, path: str, n_samples: int, n_timesteps: int, metadata: Optional[Mapping[str, object]],
                 coords: Optional[Mapping[str, np.ndarray]], enable_prediction_netcdfs: bool, enable_video_netcdfs: bool,
                 time_coarsen: Optional[TimeCoarsenConfig] = None, n_ensemble_members: int = 1,
                 save_names: Optional[Sequence[str]] = None, histogram_ensembles: bool = False):
        if enable_video_netcdfs:
            raise NotImplementedError("the video data writer is out of scope of sdy_amd (DESIGN.md section 8)")
        self._writers: List[object] = []
        if time_coarsen is not None:
            n_timesteps = time_coarsen.n_coarsened_timesteps(n_timesteps)

        def wrap(writer):
            return time_coarsen.build(writer) if time_coarsen is not None else writer

        if enable_prediction_netcdfs:
            self._writers.append(wrap(PredictionDataWriter(path=path, n_samples=n_samples, n_timesteps=n_timesteps,
                                                           metadata=metadata, coords=coords, save_names=save_names,
                                                           n_ensemble_members=n_ensemble_members)))
        if n_ensemble_members == 1 or histogram_ensembles:
            self._writers.append(wrap(HistogramDataWriter(path=path, n_timesteps=n_timesteps, metadata=metadata)))

    def append_batch(self, target: Mapping[str, torch.Tensor], prediction: Mapping[str, torch.Tensor], start_timestep: int,
                     start_sample: int = 0, batch_times=None) -> None:
        for writer in self._writers:
            writer.append_batch(target=target, prediction=prediction, start_timestep=start_timestep, start_sample=start_sample,
                                batch_times=batch_times)

    def flush(self) -> None:
        for writer in self._writers:
            writer.flush()


@dataclasses.dataclass
class DataWriterConfig:
    """`main.py:19-62`, the same four fields.  `save_raw_prediction_names` reaches the prediction writer here."""

    log_extended_video_netcdfs: bool = False
    save_prediction_files: bool = True
    save_raw_prediction_names: Optional[Sequence[str]] = None
    time_coarsen: Optional[TimeCoarsenConfig] = None

    def __post_init__(self):
        if not self.save_prediction_files and self.save_raw_prediction_names is not None:
            raise ValueError("save_raw_prediction_names provided but save_prediction_files is False")

    def build(self, experiment_dir: str, n_samples: int, n_timesteps: int, metadata: Optional[Mapping[str, object]],
              coords: Optional[Mapping[str, np.ndarray]], n_ensemble_members: int = 1) -> DataWriter:
        return DataWriter(path=experiment_dir, n_samples=n_samples, n_timesteps=n_timesteps, metadata=metadata, coords=coords,
                          enable_prediction_netcdfs=self.save_prediction_files,
                          enable_video_netcdfs=self.log_extended_video_netcdfs, time_coarsen=self.time_coarsen,
                          n_ensemble_members=n_ensemble_members, save_names=self.save_raw_prediction_names)
