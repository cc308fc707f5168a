"""Device histograms (`sdy_amd.histogram`, kernels of csrc/histogram.hip) against the reference's own `DynamicHistogram`
(tests/golden/fx_histogram.npz, tools/gen_golden.py:gen_histogram) and, at production size, against `np.histogram` with the
library's own read-back edges.  Everything is exact: counts integer for integer, edges bit for bit.

Expected counts at production size are built the reference's way: before each add the counts so far are merged pairwise as
often as the range doubled (the host replay of the range rules, `sdy_hist_plan_host`, is pinned to the reference by
tests/test_histogram_host.py), then the add's own histogram over the new edges is added.  For the 63-variable dict the add's
own histogram comes from `torch.bucketize` on the device (the same [e_k, e_k+1) / closed-last-bin rule, stated with exact
float32 comparisons), tied to `np.histogram` on a few variables: numpy sorts on the host, and a window's 7e8 values would
first have to be copied there (2.9 GB) -- several seconds per window."""
import ctypes as C
import json
import os
import types

import numpy as np
import pytest
import torch

import golden_utils as gu

pytestmark = pytest.mark.gpu
H, W = 180, 360


def _pooled(x):
    x = x.reshape(-1, *x.shape[-3:])
    return x.transpose(1, 0, 2, 3).reshape(x.shape[1], -1)


def _bit_equal(a, b):
    return a.dtype == b.dtype == np.float32 and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _merged(counts, n_left, n_right):
    """DynamicHistogram._double_size_left / _right on (..., n_bins) counts."""
    n = counts.shape[-1]
    for _ in range(n_left):
        new = np.zeros_like(counts)
        new[..., n // 2:] = counts[..., ::2] + counts[..., 1::2]
        counts = new
    for _ in range(n_right):
        new = np.zeros_like(counts)
        new[..., :n // 2] = counts[..., ::2] + counts[..., 1::2]
        counts = new
    return counts


def _plan(start, stop, init, vmin, vmax, n_bins):
    import sdy_amd

    ns, ne, nl, nr, fl = C.c_float(), C.c_float(), C.c_int(), C.c_int(), C.c_uint()
    assert sdy_amd.lib.sdy_hist_plan_host(start, stop, init, vmin, vmax, n_bins, ns, ne, nl, nr, fl) == 0
    assert fl.value == 0
    return ns.value, ne.value, nl.value, nr.value


def _bucket_counts(rows, edges):
    """(T, N) device values, float32 edges -> int64 (T, n_bins) on the host: bin k = [e_k, e_k+1), last bin closed."""
    e = torch.from_numpy(edges).to(rows.device)
    n = e.numel() - 1
    idx = (torch.bucketize(rows, e[:-1].contiguous(), right=True) - 1).clamp_(0, n - 1)
    inside = ((rows >= e[0]) & (rows <= e[-1])).to(torch.int64)
    return torch.zeros(rows.shape[0], n, dtype=torch.int64, device=rows.device).scatter_add_(1, idx, inside).cpu().numpy()


def _state(hset):
    """(flags, outside) per variable of a _HistogramSet, read back raw (no raising)."""
    import sdy_amd

    torch.cuda.synchronize()
    raw = np.ascontiguousarray(hset.state.cpu().numpy())
    out = []
    for i in range(len(hset.names)):
        fl, outside = C.c_uint(), C.c_ulonglong()
        assert sdy_amd.lib.sdy_hist_state_unpack_host(raw.ctypes.data_as(C.c_void_p), i, None, None, None, C.byref(fl),
                                                      C.byref(outside)) == 0
        out.append((fl.value, outside.value))
    return out


@pytest.fixture(scope="module")
def fx():
    z = gu.load("fx_histogram")
    return z, json.loads(str(z["cases"]))


def _views(x):
    """The stored input as a contiguous device tensor and as transposed views of differently laid out storage."""
    t = torch.from_numpy(x).cuda()
    yield "contiguous", t
    if t.dim() == 4:           # (S, T, H, W): stored time-major, handed over transposed
        yield "transposed", t.transpose(0, 1).contiguous().transpose(0, 1)
        # ... and as a member-stacked 5-D view (members = the samples, one sample), the window driver's unfold
        yield "stacked", t.view(1, *t.shape).transpose(0, 1)
    else:                      # (E, S, T, H, W): the driver's IC-major batch (S, E, ...) seen members-first
        yield "transposed", t.transpose(0, 1).contiguous().transpose(0, 1)


def test_fixture_cases_on_contiguous_and_transposed_views(fx):
    import sdy_amd

    z, cases = fx
    n_times = int(z["n_times"])
    for case in cases:
        n_bins, n_adds = int(z[f"{case}::n_bins"]), int(z[f"{case}::n_adds"])
        kinds = [k for k, _ in _views(z[f"{case}::in0"])]
        for kind in kinds:
            h = sdy_amd.DynamicHistogram(n_times, n_bins)
            assert h.bin_edges is None and not h.counts.any()
            for i in range(n_adds):
                v = dict(_views(z[f"{case}::in{i}"]))[kind]
                if kind != "contiguous":
                    assert not v.is_contiguous() or v.shape[0] == 1 or v.shape[1] == 1
                h.add(v, i_time_start=int(z[f"{case}::i_time_start{i}"]))
                assert _bit_equal(h.bin_edges, z[f"{case}::edges{i}"]), (case, kind, i)
            counts = h.counts
            assert counts.dtype == np.int64 and counts.shape == (n_times, n_bins)
            assert np.array_equal(counts, z[f"{case}::counts"]), (case, kind)
            assert _state(h._set) == [(0, 0)]


@pytest.mark.parametrize("shape,offset", [((3, 2, 13, 21), 0), ((2, 3, 16, 32), 1), ((2, 2, 181, 359), 3), ((2, 3, 2, 184, 360), 0)])
def test_odd_sizes_misaligned_storage_and_several_blocks_per_row(shape, offset):
    """HW not a multiple of 4 or a pointer off the 16-byte grid take the scalar-load kernels; 181 x 359 and 184 x 360 exceed
    one block's share of a row (32768 values), in either kernel."""
    import sdy_amd

    g = torch.Generator(device="cuda").manual_seed(17)
    n = int(np.prod(shape))
    T = shape[-3]
    h = sdy_amd.DynamicHistogram(T + 1, 300)
    expected = np.zeros((T + 1, 300), dtype=np.int64)
    start, stop, init = 0.0, 0.0, 0
    for spread, shift in ((1.0, 0.0), (6.0, -9.0)):
        x = (torch.randn(n + offset, device="cuda", generator=g) * spread + shift)[offset:].view(shape)
        assert (x.data_ptr() % 16 == 0) == (offset == 0)
        h.add(x, i_time_start=1)
        rows = torch.from_numpy(_pooled(x.cpu().numpy())).cuda()
        start, stop, n_left, n_right = _plan(start, stop, init, float(x.min()), float(x.max()), 300)
        init = 1
        edges = h.bin_edges
        assert _bit_equal(edges, sdy_amd.histogram.bin_edges(start, stop, 300))
        expected = _merged(expected, n_left, n_right)
        own = _bucket_counts(rows, edges)
        assert np.array_equal(own[0], np.histogram(rows[0].cpu().numpy(), bins=edges)[0])
        expected[1:] += own
        assert np.array_equal(h.counts, expected), (shape, offset, spread)
    assert n_left >= 1
    assert (expected.sum(axis=1) == [0] + [2 * n // T] * T).all()


@pytest.fixture(scope="module")
def production_windows():
    """Three windows of one variable, (25, 1, 7, 180, 360) as the strided view of an IC-major (1 x 25, 7, ...) batch, with a
    growing spread: the second exceeds the first range on both sides, the third far to the left."""
    g = torch.Generator(device="cuda").manual_seed(5)
    wins = []
    for spread, shift in ((2.0, 280.0), (5.0, 281.0), (30.0, 200.0)):
        batch = torch.randn(25, 7, H, W, device="cuda", generator=g) * spread + shift
        wins.append(batch.view(1, 25, 7, H, W).transpose(0, 1))
    return wins


def test_production_size_equals_numpy_histogram_with_the_read_back_edges(production_windows):
    import sdy_amd

    n_times, n_bins = 19, 300
    h = sdy_amd.DynamicHistogram(n_times, n_bins)
    expected = np.zeros((n_times, n_bins), dtype=np.int64)
    start, stop, init, doublings = 0.0, 0.0, 0, np.zeros(2, dtype=int)
    for w, x in enumerate(production_windows):
        assert x.shape == (25, 1, 7, H, W) and x.stride()[:3] == (7 * H * W, 25 * 7 * H * W, H * W)
        t0 = 6 * w
        h.add(x, i_time_start=t0)
        start, stop, n_left, n_right = _plan(start, stop, init, float(x.min()), float(x.max()), n_bins)
        init = 1
        doublings += [n_left, n_right]
        edges = h.bin_edges                                  # the library's own read-back
        assert _bit_equal(edges, sdy_amd.histogram.bin_edges(start, stop, n_bins))
        expected = _merged(expected, n_left, n_right)
        rows = x.permute(2, 0, 1, 3, 4).reshape(7, -1).cpu().numpy()
        for t in range(7):
            expected[t0 + t] += np.histogram(rows[t], bins=edges)[0]
        got = h.counts
        assert np.array_equal(got, expected), f"window {w}"
    assert doublings[0] >= 1 and doublings[1] >= 1
    per_time = np.zeros(n_times, dtype=np.int64)
    for w in range(3):
        per_time[6 * w:6 * w + 7] += 25 * H * W
    assert np.array_equal(got.sum(axis=1), per_time)          # every time row sums to rows x HW (windows overlap by one time)
    assert _state(h._set) == [(0, 0)]


def test_writer_on_a_63_variable_production_dict():
    import sdy_amd

    nv, members, T, n_times, n_bins = 63, 25, 7, 13, 300
    names = [f"v{i}" for i in range(nv)]
    g = torch.Generator(device="cuda").manual_seed(9)
    wr = sdy_amd.HistogramDataWriter(None, n_times)
    exp = {s: np.zeros((nv, n_times, n_bins), dtype=np.int64) for s in ("target", "prediction")}
    rng = {s: [(0.0, 0.0, 0)] * nv for s in exp}
    scale = 10.0 ** torch.linspace(-6.0, 5.0, nv, device="cuda")
    for w, (spread, shift) in enumerate(((1.0, 0.5), (3.0, -2.0))):
        pred_all = (torch.randn(nv, members, T, H, W, device="cuda", generator=g) * spread + shift) * scale.view(-1, 1, 1, 1, 1)
        tgt_all = (torch.randn(nv, 1, T, H, W, device="cuda", generator=g) * spread + shift) * scale.view(-1, 1, 1, 1, 1)
        pred = {n: pred_all[i].view(1, members, T, H, W).transpose(0, 1) for i, n in enumerate(names)}
        tgt = {n: tgt_all[i] for i, n in enumerate(names)}
        t0 = 6 * w
        wr.append_batch(target=tgt, prediction=pred, start_timestep=t0, start_sample=0)
        ds = wr.get_dataset()
        for src, data in (("target", tgt), ("prediction", pred)):
            for i, n in enumerate(names):
                x = data[n]
                start, stop, init = rng[src][i]
                start, stop, n_left, n_right = _plan(start, stop, init, float(x.min()), float(x.max()), n_bins)
                rng[src][i] = (start, stop, 1)
                edges = ds[src][f"{n}_bin_edges"]
                assert _bit_equal(edges, sdy_amd.histogram.bin_edges(start, stop, n_bins)), (src, n)
                exp[src][i] = _merged(exp[src][i], n_left, n_right)
                rows = x.movedim(-3, 0).reshape(T, -1)
                own = _bucket_counts(rows, edges)
                if i % 31 == 0 and (src == "target" or i == 0):     # the device restatement IS np.histogram
                    r = rows[3].cpu().numpy()
                    assert np.array_equal(own[3], np.histogram(r, bins=edges)[0]), (src, n)
                exp[src][i, t0:t0 + T] += own
                assert np.array_equal(ds[src][n], exp[src][i]), (w, src, n)
        del pred_all, tgt_all, pred, tgt
    for src, rows in (("target", 1), ("prediction", members)):
        sums = exp[src].sum(axis=2)
        want = np.zeros(n_times, dtype=np.int64)
        want[0:7] += rows * H * W
        want[6:13] += rows * H * W
        assert (sums == want).all()
        assert _state(wr._sets[src]) == [(0, 0)] * nv


def test_two_runs_give_identical_counts(production_windows):
    import sdy_amd

    runs = []
    for _ in range(2):
        h = sdy_amd.DynamicHistogram(8, 300)
        for x in production_windows[:2]:
            h.add(x[:5], i_time_start=1)
        runs.append((h.counts.copy(), h.bin_edges.copy()))
    assert np.array_equal(runs[0][0], runs[1][0]) and _bit_equal(runs[0][1], runs[1][1])
    assert runs[0][0].sum() == 2 * 5 * 7 * H * W


def test_bounds_and_device_are_checked_before_any_launch():
    import sdy_amd

    h = sdy_amd.DynamicHistogram(4, 8)
    x = torch.rand(2, 3, 4, 8, device="cuda")
    h.add(x, i_time_start=1)
    before, edges = h.counts.copy(), h.bin_edges.copy()
    for t0 in (2, -1, 4):
        with pytest.raises(ValueError):
            h.add(x * 100.0, i_time_start=t0)
    with pytest.raises(RuntimeError, match="GPU only"):
        h.add(x.cpu(), i_time_start=0)
    with pytest.raises(ValueError):
        h.add(x[0, 0], i_time_start=0)
    assert np.array_equal(h.counts, before) and _bit_equal(h.bin_edges, edges) and before.sum() == x.numel()
    for n_bins in (7, 0, 4096):
        with pytest.raises(ValueError):
            sdy_amd.DynamicHistogram(4, n_bins)
    # the C entry point refuses the same window by itself
    from sdy_amd._lib import SdyHistArgs, current_stream, ptr

    a = SdyHistArgs()
    a.nvars, a.n0, a.n1, a.T, a.HW, a.t_start, a.n_times, a.n_bins = 1, 1, 2, 3, 32, 2, 4, 8
    a.data[0], a.s0[0], a.s1[0] = ptr(x), 0, x.stride(0)
    a.state, a.counts = ptr(h._set.state), ptr(h._set.counts)
    assert sdy_amd.lib.sdy_hist_add(C.byref(a), current_stream()) == -1
    assert np.array_equal(h.counts, before)


def test_non_finite_values_raise_at_read_back_and_are_not_counted():
    import sdy_amd

    h = sdy_amd.DynamicHistogram(2, 8)
    x = torch.rand(2, 2, 4, 8, device="cuda")
    h.add(x)
    good = h.counts.copy()
    x[1, 1, 2, 3] = float("nan")
    h.add(x)
    with pytest.raises(sdy_amd.SdyError, match="non-finite"):
        h.counts
    (flags, outside), = _state(h._set)
    assert flags == 1 and outside == 1              # the range stayed; only the NaN itself was left out
    torch.cuda.synchronize()
    assert h._set.counts.sum().item() == 2 * good.sum() - 1


def test_variable_missing_from_one_source_is_filled_like_the_reference():
    import sdy_amd

    g = torch.Generator(device="cuda").manual_seed(3)
    tgt = {n: torch.randn(2, 3, 12, 24, device="cuda", generator=g) for n in ("a", "forcing")}
    pred = {n: torch.randn(2, 3, 12, 24, device="cuda", generator=g) for n in ("a", "diag")}
    wr = sdy_amd.HistogramDataWriter(None, 3, n_bins=8)
    wr.append_batch(tgt, pred, 0, 0)
    ds = wr.get_dataset()
    assert set(ds) == {"target", "prediction"}
    for src in ds:
        assert set(ds[src]) == {"a", "forcing", "diag", "a_bin_edges", "forcing_bin_edges", "diag_bin_edges"}
    assert not ds["prediction"]["forcing"].any() and ds["target"]["forcing"].sum() == 2 * 3 * 12 * 24
    assert not ds["target"]["diag"].any() and ds["prediction"]["diag"].sum() == 2 * 3 * 12 * 24
    assert _bit_equal(ds["prediction"]["forcing_bin_edges"], ds["target"]["forcing_bin_edges"])
    assert _bit_equal(ds["target"]["diag_bin_edges"], ds["prediction"]["diag_bin_edges"])
    assert ds["target"]["diag"].shape == (3, 8) and ds["target"]["diag"].dtype == np.int64


@pytest.mark.parametrize("members", [1, 3])
def test_through_the_window_driver(members, tmp_path):
    """run_inference(writer=tee(HistogramDataWriter, recorder)) on the tiny synthetic stepper, three windows (the later ones
    arrive without their first time): the writer's dataset is what direct DynamicHistogram.add calls on the recorded tensors
    give, and flush() leaves a readable histograms.npz."""
    import sdy_amd
    from sdy_amd import synthetic

    dev = torch.device("cuda", 0)
    n_out, n_forc, nlat, nlon, window, n_windows = 4, 2, 32, 64, 6, 3
    exp, _, _ = synthetic.build_sampler(dev, state_chans=n_out, forcing_chans=n_forc, nlat=nlat, nlon=nlon, embed=16, layers=2,
                                        horizon=6, carried_input_only_channel=True)
    stepper, names, out_names = synthetic.build_stepper(exp, n_out, n_forc, carried_input_only_channel=True)
    steps = window * n_windows
    hist = sdy_amd.HistogramDataWriter(str(tmp_path / "out"), steps + 1, metadata={"v0": types.SimpleNamespace(units="K")})
    calls = []

    class Tee:
        def append_batch(self, target, prediction, start_timestep, start_sample, batch_times=None):
            calls.append((start_timestep, {k: v.clone() for k, v in target.items()}, {k: v.clone() for k, v in prediction.items()}))
            hist.append_batch(target=target, prediction=prediction, start_timestep=start_timestep, start_sample=start_sample,
                              batch_times=batch_times)

        def flush(self):
            hist.flush()

    sdy_amd.run_inference(None, stepper, synthetic.windows(names, n_windows, window, nlat, nlon, n_ics=2, seed=5), steps, window,
                          n_ensemble_members=members, eval_device=dev, writer=Tee())
    assert [c[0] for c in calls] == [0, 7, 13]
    assert calls[0][2][out_names[0]].shape == ((members, 2, 7, nlat, nlon) if members > 1 else (2, 7, nlat, nlon))
    assert calls[1][2][out_names[0]].shape[-3] == 6
    ds = hist.get_dataset()
    assert set(ds["target"]) == set(ds["prediction"]) and set(names) <= set(ds["target"])
    for k, src in ((1, "target"), (2, "prediction")):
        for n in calls[0][k]:
            h = sdy_amd.DynamicHistogram(steps + 1)
            for c in calls:
                h.add(c[k][n], i_time_start=c[0])
            assert np.array_equal(ds[src][n], h.counts), (src, n)
            assert _bit_equal(ds[src][f"{n}_bin_edges"], h.bin_edges), (src, n)
            rows = 2 * (members if src == "prediction" else 1)
            assert (ds[src][n].sum(axis=1) == rows * nlat * nlon).all()
    path = os.path.join(str(tmp_path / "out"), "histograms.npz")
    assert os.path.exists(path)
    with np.load(path) as f:
        for src in ds:
            for key, v in ds[src].items():
                assert np.array_equal(f[f"{src}/{key}"], v)
        assert str(f["units/v0"]) == "K"
