"""Device-side data writers (`sdy_amd.data_writer`, kernel of csrc/coarsen.hip) against the reference's own `TimeCoarsen`
(tests/golden/fx_time_coarsen.npz, tools/gen_golden.py:gen_time_coarsen), against float64 and against a torch restatement
(`unfold(time, f, f).mean(-1)`).

Error bound, u = 2^-24: any fp32 summation order of f values followed by one division is within (f + 1) u max|x_i| of the
exact mean, for the kernel and for torch alike.  f = 1 is a copy and f = 2 one rounded add and an exact halving of normal-range
inputs (unit-scale Gaussians; checked): both bit for bit, so nothing behind a factor-2 coarsening -- a histogram's bin, a written
file -- can differ from what torch-coarsened tensors give."""
import json
import os
import types

import numpy as np
import pytest
import torch

import golden_utils as gu
from test_data_writer_host import WINDOWS, _bit_equal, exact_and_bound, expected_calls

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
TINY = float(np.finfo(np.float32).tiny)


@pytest.fixture(scope="module")
def fx():
    z = gu.load("fx_time_coarsen")
    return z, json.loads(str(z["cases"]))


class Recorder:
    def __init__(self, inner=None):
        self.calls, self.inner = [], inner

    def append_batch(self, target, prediction, start_timestep, start_sample, batch_times=None):
        self.calls.append(({k: v.clone() for k, v in target.items()}, {k: v.clone() for k, v in prediction.items()},
                           start_timestep, start_sample, batch_times))
        if self.inner is not None:
            self.inner.append_batch(target=target, prediction=prediction, start_timestep=start_timestep,
                                    start_sample=start_sample, batch_times=batch_times)

    def flush(self):
        if self.inner is not None:
            self.inner.flush()


def torch_coarsen(x, t_first, f):
    """The reference's arithmetic along the time axis (third from last), the first t_first times kept."""
    t = x.dim() - 3
    head, rest = x.narrow(t, 0, t_first), x.narrow(t, t_first, x.shape[t] - t_first)
    return torch.cat([head, rest.unfold(t, f, f).mean(-1)], dim=t)


def check_against_float64(got, x, t_first, f):
    """got, x: device tensors (..., time, lat, lon); the bound per element, bit-identity where nothing is rounded twice."""
    g = got.reshape(-1, *got.shape[-3:]).cpu().numpy()
    xs = x.reshape(-1, *x.shape[-3:]).cpu().numpy()
    assert (np.abs(xs) >= TINY).all() and np.isfinite(xs).all()
    exact, bound = exact_and_bound(xs, t_first, f)
    assert g.shape == exact.shape, (g.shape, exact.shape)
    err = np.abs(g.astype(np.float64) - exact)
    assert (err <= bound).all(), float((err - bound).max())
    assert _bit_equal(g[:, :t_first], xs[:, :t_first])
    if f <= 2:
        assert torch.equal(got, torch_coarsen(x, t_first, f))


def layouts(x):
    """A (S, T, H, W) host array on the device: contiguous, and as the member-stacked view of IC-major storage (members = 1
    and the samples taken as members)."""
    t = torch.from_numpy(x).cuda()
    yield "contiguous", t
    yield "stacked", t.view(1, *t.shape).transpose(0, 1)                      # (S, 1, ...) viewed from (1, S, ...) storage
    yield "transposed", t.transpose(0, 1).contiguous().transpose(0, 1)        # sample stride below the time stride: copied once


def test_fixture_cases_on_contiguous_and_transposed_views(fx):
    import sdy_amd

    z, cases = fx
    for case in cases:
        grid, f = case.split("_f")
        f = int(f)
        recorded, windows = expected_calls(z, case)
        for kind in ("contiguous", "stacked", "transposed"):
            rec = Recorder()
            tc = sdy_amd.TimeCoarsen(rec, f)
            for w, (t0, _) in enumerate(WINDOWS):
                tgt = {"a": dict(layouts(z[f"{grid}::w{w}::target::a"]))[kind]}
                pred = {n: dict(layouts(z[f"{grid}::w{w}::prediction::{n}"]))[kind] for n in ("a", "b")}
                tc.append_batch(tgt, pred, t0, int(z["start_sample"]), z[f"{grid}::w{w}::times"])
            assert [c[2] for c in rec.calls] == [int(c["start_timestep"]) for c in recorded]
            assert [c[3] for c in rec.calls] == [3, 3, 3]
            for (tgt, pred, *_, times), want in zip(rec.calls, recorded):
                assert np.array_equal(times, want["times"])
                for src, d in (("target", tgt), ("prediction", pred)):
                    for n, v in d.items():
                        w_ = want[f"{src}::{n}"]
                        got = v.reshape(w_.shape).cpu().numpy()      # (the stacked view carries one more axis of length 1)
                        assert v.numel() == w_.size
                        if f <= 2:
                            assert _bit_equal(got, w_), (case, kind, src, n)
            # ... and per window against float64, with the bound
            for w, (t_first, want) in enumerate(windows):
                joined = rec.calls[:2] if w == 0 else rec.calls[2:]
                for key, ref in want.items():
                    src, n = key.split("::")
                    got = np.concatenate([c[0 if src == "target" else 1][n].reshape(-1, *c[0]["a"].shape[-3:]).cpu().numpy()
                                          for c in joined], axis=1)
                    x = z[f"{grid}::w{w}::{key}"]
                    exact, bound = exact_and_bound(x, t_first, f)
                    assert got.shape == ref.shape == exact.shape
                    assert (np.abs(got.astype(np.float64) - exact) <= bound).all(), (case, kind, key)
                    assert (np.abs(ref.astype(np.float64) - exact) <= bound).all(), (case, kind, key)


@pytest.mark.parametrize("hw", [(6, 12), (5, 7)])
@pytest.mark.parametrize("factor", [1, 2, 3, 4])
@pytest.mark.parametrize("t_first", [0, 1])
def test_views_offsets_and_remainders(hw, factor, t_first):
    """HW = 72 (16-byte accesses) and 35 (scalar); storage offset by one element (misaligned pointers: scalar path); a
    member-stacked view read in place; a (time, lat, lon) block that is not contiguous (copied once); T = 7, so that every
    factor but 1 leaves a remainder for one of the two t_first."""
    from sdy_amd.data_writer import coarsen_tensors

    H, W = hw
    M, S, T = 3, 2, 7
    g = torch.Generator(device="cuda").manual_seed(100 * H + 10 * factor + t_first)
    n = M * S * T * H * W
    flat = torch.randn(n + 1, device="cuda", generator=g)
    aligned = flat[:n].view(S, M, T, H, W)
    shifted = flat[1:].view(S, M, T, H, W)
    assert aligned.data_ptr() % 16 == 0 and shifted.data_ptr() % 16 == 4
    wide = torch.randn(S, T, H, W + 3, device="cuda", generator=g)
    # (consecutive tensors of one shape share a launch, and one misaligned pointer sends the whole launch down the scalar
    #  path: the order keeps the aligned member-stacked view in a launch of its own)
    cases = {"stacked": aligned.transpose(0, 1), "rows": aligned[:, 0], "shifted": shifted.transpose(0, 1),
             "padded_rows": wide[..., :W], "time_major": aligned[0].transpose(0, 1).contiguous().transpose(0, 1)}
    assert not cases["stacked"].is_contiguous() and not cases["padded_rows"].is_contiguous()
    assert cases["time_major"].stride(1) == M * H * W
    outs, buf = coarsen_tensors(list(cases.values()), t_first, factor)
    t_out = t_first + (T - t_first) // factor
    for (kind, x), got in zip(cases.items(), outs):
        assert got.shape == x.shape[:-3] + (t_out, H, W) and got.is_contiguous(), kind
        assert got.untyped_storage().data_ptr() == buf.untyped_storage().data_ptr()
        check_against_float64(got, x, t_first, factor)


def test_97_tiny_variables_take_two_launches(monkeypatch):
    from sdy_amd import data_writer as dw

    launches = []
    real = dw._launch
    monkeypatch.setattr(dw, "_launch", lambda a, dev: (launches.append(a.nvars), real(a, dev)))
    g = torch.Generator(device="cuda").manual_seed(97)
    xs = [torch.randn(1, 5, 2, 4, device="cuda", generator=g) for _ in range(97)]
    outs, _ = dw.coarsen_tensors(xs, 1, 2)
    assert launches == [96, 1]
    for x, got in zip(xs, outs):
        assert torch.equal(got, torch_coarsen(x, 1, 2))


def test_two_shapes_mixed_in_one_dict(monkeypatch):
    from sdy_amd import data_writer as dw

    launches = []
    real = dw._launch
    monkeypatch.setattr(dw, "_launch", lambda a, dev: (launches.append((a.nvars, a.n1, a.HW)), real(a, dev)))
    g = torch.Generator(device="cuda").manual_seed(12)
    d = {"a": torch.randn(2, 7, 6, 12, device="cuda", generator=g), "b": torch.randn(2, 7, 6, 12, device="cuda", generator=g),
         "c": torch.randn(3, 7, 5, 7, device="cuda", generator=g), "d": torch.randn(2, 7, 6, 12, device="cuda", generator=g)}
    rec = Recorder()
    dw.TimeCoarsen(rec, 3).append_batch(d, {}, 7, 0)
    assert launches == [(2, 2, 72), (1, 3, 35), (1, 2, 72)]
    (tgt, pred, st, *_), = rec.calls
    assert st == 3 and pred == {} and list(tgt) == list(d)
    for n, x in d.items():
        check_against_float64(tgt[n], x, 0, 3)


def test_a_variable_larger_than_one_pass_of_the_grid():
    """48 variables share the launch's blocks (85 each, 512 work items per block): 3 x 4 x 4050 = 48600 quads per variable need
    a second, partly filled pass of the grid-stride loop; with the scalar kernel (misaligned) four times as many items."""
    from sdy_amd.data_writer import coarsen_tensors

    g = torch.Generator(device="cuda").manual_seed(48)
    big = torch.randn(48 * 3 * 7 * 90 * 180 + 1, device="cuda", generator=g)
    for off in (0, 1):
        xs = list(big[off:off + 48 * 3 * 7 * 90 * 180].view(48, 3, 7, 90, 180).unbind(0))
        outs, _ = coarsen_tensors(xs, 1, 2)
        for i in (0, 17, 47):
            assert torch.equal(outs[i], torch_coarsen(xs[i], 1, 2)), (off, i)
        assert torch.equal(torch.stack(outs), torch_coarsen(torch.stack(xs), 1, 2))


def test_histograms_behind_a_factor_two_coarsening():
    """TimeCoarsen(HistogramDataWriter) equals HistogramDataWriter fed torch-coarsened tensors: counts integer for integer,
    edges bit for bit (factor 2 is bit-exact, so no value near an edge can move)."""
    import sdy_amd

    g = torch.Generator(device="cuda").manual_seed(21)
    names = ["a", "b", "c"]
    behind, direct = sdy_amd.HistogramDataWriter(None, 7, n_bins=300), sdy_amd.HistogramDataWriter(None, 7, n_bins=300)
    tc = sdy_amd.TimeCoarsen(behind, 2)
    for t0, T, spread in ((0, 7, 1.0), (7, 6, 4.0)):
        flat = {n: torch.randn(2, 3, T, 12, 24, device="cuda", generator=g) * spread for n in names}
        tgt = {n: v[:, 0].contiguous() for n, v in flat.items()}
        pred = {n: v.transpose(0, 1) for n, v in flat.items()}
        tc.append_batch(tgt, pred, t0, 0)
        if t0 == 0:
            direct.append_batch({n: v[:, :1] for n, v in tgt.items()}, {n: v[:, :, :1] for n, v in pred.items()}, 0, 0)
            direct.append_batch({n: torch_coarsen(v[:, 1:], 0, 2) for n, v in tgt.items()},
                                {n: torch_coarsen(v[:, :, 1:], 0, 2) for n, v in pred.items()}, 1, 0)
        else:
            direct.append_batch({n: torch_coarsen(v, 0, 2) for n, v in tgt.items()},
                                {n: torch_coarsen(v, 0, 2) for n, v in pred.items()}, 4, 0)
    a, b = behind.get_dataset(), direct.get_dataset()
    for src in ("target", "prediction"):
        assert set(a[src]) == set(b[src])
        for n in names:
            assert np.array_equal(a[src][n], b[src][n]) and a[src][n].dtype == np.int64
            assert _bit_equal(a[src][f"{n}_bin_edges"], b[src][f"{n}_bin_edges"])
            assert (a[src][n].sum(axis=1) == (2 if src == "target" else 6) * 12 * 24).all()


@pytest.mark.parametrize("members", [1, 3])
def test_prediction_writer_round_trip(members, tmp_path, monkeypatch):
    import sdy_amd
    from sdy_amd import data_writer as dw

    launches = []
    real = dw._launch
    monkeypatch.setattr(dw, "_launch", lambda a, dev: (launches.append((a.nvars, a.factor)), real(a, dev)))
    g = torch.Generator(device="cuda").manual_seed(5 + members)
    S, H, W, n_samples, n_times = 2, 6, 12, 4, 10
    meta = {"a": types.SimpleNamespace(units="K", long_name="temperature")}
    wr = sdy_amd.PredictionDataWriter(str(tmp_path), n_samples, n_times, meta, {"lat": np.arange(H), "lon": np.arange(W)},
                                      save_names=["a", "forcing", "diag"], n_ensemble_members=members)
    lead = (S, members) if members > 1 else (S,)
    batches = []
    for st, T in ((0, 4), (4, 3)):
        tgt = {n: torch.randn(S, T, H, W, device="cuda", generator=g) for n in ("a", "forcing", "unsaved")}
        pred = {n: torch.randn(*lead, T, H, W, device="cuda", generator=g) for n in ("a", "diag", "unsaved")}
        if members > 1:
            pred = {n: v.transpose(0, 1) for n, v in pred.items()}       # the window driver's member-stacked view
        batches.append((st, tgt, pred))
    # out of range: ValueError with no file touched and no launch made
    for st, ss in ((8, 1), (0, 3), (-1, 1), (0, -1)):
        with pytest.raises(ValueError):
            wr.append_batch(batches[0][1], batches[0][2], st, ss)
    assert launches == [] and not (tmp_path / "autoregressive_predictions").exists()
    for st, tgt, pred in batches:
        wr.append_batch(tgt, pred, st, 1)
    assert launches == [(2, 1)] * 4                  # one packing launch per source and batch, factor 1
    with pytest.raises(ValueError):
        wr.append_batch(batches[0][1], batches[0][2], 7, 1)
    wr.flush()
    root = tmp_path / "autoregressive_predictions"
    for src in ("target", "prediction"):
        assert sorted(p.name for p in (root / src).iterdir()) == ["a.npy", "diag.npy", "forcing.npy"]
    for src, k in (("target", 1), ("prediction", 2)):
        for n in ("a", "forcing", "diag"):
            f = np.load(root / src / f"{n}.npy")
            stacked = src == "prediction" and members > 1
            assert f.dtype == np.float32 and f.shape == ((members,) if stacked else ()) + (n_samples, n_times, H, W)
            for b in batches:
                if n in b[k]:
                    x = b[k][n].cpu().numpy()
                    region = f[..., 1:3, b[0]:b[0] + x.shape[-3], :, :]
                    assert _bit_equal(np.ascontiguousarray(region), x), (src, n)
                    region[...] = np.nan
            assert np.isnan(f).all(), (src, n)        # a variable one source lacks, samples 0 and 3, times 7..9: never written
    index = json.loads((root / "index.json").read_text())
    assert index["dims"] == dict(sample=n_samples, timestep=n_times, lat=H, lon=W, **({"member": members} if members > 1 else {}))
    assert sorted(index["variables"]) == ["a", "diag", "forcing"] and index["variables"]["a"]["units"] == "K"
    # host tensors (run_inference(host_outputs=True)) are accepted and written directly
    wr2 = sdy_amd.PredictionDataWriter(str(tmp_path / "host"), n_samples, n_times, n_ensemble_members=members)
    st, tgt, pred = batches[1]
    n_before = len(launches)
    wr2.append_batch({k: v.cpu() for k, v in tgt.items()}, {k: v.cpu() for k, v in pred.items()}, st, 1)
    wr2.flush()
    assert len(launches) == n_before
    f = np.load(tmp_path / "host" / "autoregressive_predictions" / "prediction" / "unsaved.npy")
    assert _bit_equal(np.ascontiguousarray(f[..., 1:3, 4:7, :, :]), pred["unsaved"].cpu().numpy())


def _run_through_the_driver(path, members):
    import sdy_amd
    from sdy_amd import synthetic

    dev = torch.device("cuda", 0)
    n_out, n_forc, nlat, nlon, window, n_windows = 4, 2, 32, 64, 6, 3
    exp, _, _ = synthetic.build_sampler(dev, state_chans=n_out, forcing_chans=n_forc, nlat=nlat, nlon=nlon, embed=16, layers=2,
                                        horizon=6, carried_input_only_channel=True)
    stepper, names, out_names = synthetic.build_stepper(exp, n_out, n_forc, carried_input_only_channel=True)
    steps = window * n_windows
    writer = sdy_amd.DataWriter(str(path), n_samples=2, n_timesteps=steps + 1, metadata={}, coords={},
                                enable_prediction_netcdfs=True, enable_video_netcdfs=False,
                                time_coarsen=sdy_amd.TimeCoarsenConfig(2), n_ensemble_members=members, histogram_ensembles=True)
    tee = Recorder(writer)
    sdy_amd.run_inference(None, stepper, synthetic.windows(names, n_windows, window, nlat, nlon, n_ics=2, seed=5), steps, window,
                          n_ensemble_members=members, eval_device=dev, writer=tee)
    return tee.calls, writer, steps


@pytest.mark.parametrize("members", [1, 2])
def test_through_the_window_driver(members, tmp_path):
    """run_inference(writer=DataWriter(time_coarsen=2)) on the tiny synthetic stepper, three windows of six steps: the written
    files equal a torch coarsening of the full stitched timeline (recorded through a tee in front of the writer), the
    histograms equal direct adds of the same coarsened tensors."""
    import sdy_amd

    calls, writer, steps = _run_through_the_driver(tmp_path / "out", members)
    assert [c[2] for c in calls] == [0, 7, 13]
    n_coarse = steps // 2 + 1
    root = tmp_path / "out" / "autoregressive_predictions"
    hist = writer._writers[1]._data_writer.get_dataset()
    for k, src in ((0, "target"), (1, "prediction")):
        for n in calls[0][k]:
            timeline = torch.cat([c[k][n] for c in calls], dim=-3)
            assert timeline.shape[-3] == steps + 1
            want = torch_coarsen(timeline, 1, 2)
            f = np.load(root / src / f"{n}.npy")
            assert f.shape == tuple(want.shape) and f.shape[-3] == n_coarse
            assert f.shape[:-3] == ((members, 2) if (members > 1 and src == "prediction") else (2,))
            assert _bit_equal(f, want.cpu().numpy()), (src, n)
            h = sdy_amd.DynamicHistogram(n_coarse)
            h.add(want[..., :1, :, :], i_time_start=0)
            for w in range(3):
                h.add(want[..., 1 + 3 * w:4 + 3 * w, :, :], i_time_start=1 + 3 * w)
            assert np.array_equal(hist[src][n], h.counts), (src, n)
            assert _bit_equal(hist[src][f"{n}_bin_edges"], h.bin_edges), (src, n)
    assert os.path.exists(tmp_path / "out" / "histograms.npz")


def test_two_identical_runs_give_identical_files(tmp_path):
    runs = []
    for i in range(2):
        _run_through_the_driver(tmp_path / f"run{i}", 2)
        root = tmp_path / f"run{i}" / "autoregressive_predictions"
        runs.append({str(p.relative_to(root)): p.read_bytes() for p in sorted(root.rglob("*")) if p.is_file()})
    assert len(runs[0]) >= 2 * 4 + 1 and runs[0] == runs[1]
