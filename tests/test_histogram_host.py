"""Host side of the device histograms (`sdy_amd.histogram`, csrc/hist_edges.h through `sdy_hist_plan_host`,
`sdy_hist_edges_host`, `sdy_hist_bins_host`): the range rules, the edges and the bin search against the reference's own
`DynamicHistogram` (tests/golden/fx_histogram.npz, tools/gen_golden.py:gen_histogram), and `sdy_hist_add`'s argument checks.
No GPU: the kernels compile the same header, so what is pinned here is what they compute.  Everything is exact: edges bit
for bit, counts integer for integer."""
import ctypes as C
import json

import numpy as np
import pytest

import golden_utils as gu

ERR_ARG = -1


@pytest.fixture(scope="module")
def sdy():
    import sdy_amd

    return sdy_amd


@pytest.fixture(scope="module")
def fx():
    z = gu.load("fx_histogram")
    return z, json.loads(str(z["cases"]))


def _plan(lib, start, stop, init, vmin, vmax, n_bins):
    ns, ne, nl, nr, fl = C.c_float(), C.c_float(), C.c_int(), C.c_int(), C.c_uint()
    assert lib.sdy_hist_plan_host(start, stop, init, vmin, vmax, n_bins, ns, ne, nl, nr, fl) == 0
    return ns.value, ne.value, nl.value, nr.value, fl.value


def _pooled(x):
    x = x.reshape(-1, *x.shape[-3:])
    return x.transpose(1, 0, 2, 3).reshape(x.shape[1], -1)


def test_fixture_is_from_the_numpy_the_edges_are_pinned_to(fx):
    z, cases = fx
    assert len(cases) == 8 and {c.rsplit("_b", 1)[1] for c in cases} == {"300", "8"}
    assert str(z["numpy_version"]).split(".")[0] == "2"       # float32 scalars stay float32 (NEP 50): fp32 linspace


def test_range_rules_and_edges_replay_every_fixture_case(sdy, fx):
    z, cases = fx
    seen = np.zeros(2, dtype=int)
    for case in cases:
        n_bins = int(z[f"{case}::n_bins"])
        start, stop, init = 0.0, 0.0, 0
        for i in range(int(z[f"{case}::n_adds"])):
            vmin, vmax = (float(v) for v in z[f"{case}::minmax{i}"])
            start, stop, n_left, n_right, flags = _plan(sdy.lib, start, stop, init, vmin, vmax, n_bins)
            init = 1
            assert flags == 0
            assert [n_left, n_right] == z[f"{case}::doublings{i}"].tolist(), (case, i)
            seen += [n_left, n_right]
            edges = sdy.histogram.bin_edges(start, stop, n_bins)
            want = z[f"{case}::edges{i}"]
            assert edges.dtype == want.dtype == np.float32
            assert np.array_equal(edges.view(np.uint32), want.view(np.uint32)), (case, i)
    assert seen[0] >= 4 and seen[1] >= 2            # both directions, several doublings in one add among them


def test_bin_search_is_numpy_histogram_on_every_fixture_add(sdy, fx):
    """Counts of each add alone, against np.histogram with the recorded edges -- including the values planted on edges and
    the constant field's range, whose step is below float32's spacing (runs of equal edges)."""
    z, cases = fx
    corrected = 0
    for case in cases:
        n_bins = int(z[f"{case}::n_bins"])
        for i in range(int(z[f"{case}::n_adds"])):
            rows, edges = _pooled(z[f"{case}::in{i}"]), z[f"{case}::edges{i}"]
            flat = np.ascontiguousarray(rows.reshape(-1))
            bins = np.empty(flat.size, dtype=np.int32)
            assert sdy.lib.sdy_hist_bins_host(flat.ctypes.data_as(C.c_void_p), flat.size, float(edges[0]), float(edges[-1]),
                                              n_bins, bins.ctypes.data_as(C.c_void_p)) == 0
            assert bins.min() >= 0 and bins.max() < n_bins
            got = np.stack([np.bincount(b, minlength=n_bins) for b in bins.reshape(rows.shape)])
            want = np.stack([np.histogram(r, bins=edges)[0] for r in rows])
            assert np.array_equal(got, want), (case, i)
            step = (edges[-1] - edges[0]) / np.float32(n_bins)
            with np.errstate(all="ignore"):
                corrected += int((((flat - edges[0]) * (np.float32(1) / step)).astype(np.int64).clip(0, n_bins - 1) != bins).sum())
    assert corrected > 0        # the plain guess is not enough: the correction against the edges is exercised
    # outside the range and NaN: -1
    x = np.array([-1.0, 0.0, 1.0, 1.0000001, np.nan, np.inf], dtype=np.float32)
    bins = np.empty(x.size, dtype=np.int32)
    assert sdy.lib.sdy_hist_bins_host(x.ctypes.data_as(C.c_void_p), x.size, 0.0, 1.0, 8, bins.ctypes.data_as(C.c_void_p)) == 0
    assert bins.tolist() == [-1, 0, 7, -1, -1, -1]


def test_ranges_the_reference_cannot_handle_set_the_flag_instead_of_looping(sdy):
    lib = sdy.lib
    # zero-width range (a constant 1000.0: +-1e-6 does not change it in float32), as the first range and as a later one
    assert _plan(lib, 0.0, 0.0, 0, 1000.0, 1000.0, 300) == (0.0, 0.0, 0, 0, 1)
    assert _plan(lib, 5.0, 5.0, 1, 4.0, 6.0, 300) == (5.0, 5.0, 0, 0, 1)
    # non-finite min / max
    for vmin, vmax in ((float("-inf"), 1.0), (float("nan"), 1.0), (0.0, float("inf")), (0.0, float("nan"))):
        assert _plan(lib, 0.0, 1.0, 1, vmin, vmax, 300) == (0.0, 1.0, 0, 0, 1)
        assert _plan(lib, 0.0, 0.0, 0, vmin, vmax, 8)[4] == 1
    # a range that doubles out of float32: flagged, state unchanged
    assert _plan(lib, 0.0, 3.0e38, 1, -3.0e38, 1.0, 300) == (0.0, np.float32(3.0e38), 0, 0, 1)
    # and an ordinary case next to them: 0..1 doubled twice to the left reaches -3
    assert _plan(lib, 0.0, 1.0, 1, -2.5, 0.5, 8) == (-3.0, 1.0, 2, 0, 0)
    assert _plan(lib, 0.0, 1.0, 1, 0.5, 3.5, 8) == (0.0, 4.0, 0, 2, 0)
    # constant sample: widened by 1e-6 in float32
    s, e, *_ = _plan(lib, 0.0, 0.0, 0, 2.5, 2.5, 300)
    assert (np.float32(s), np.float32(e)) == (np.float32(2.5) - np.float32(1e-6), np.float32(2.5) + np.float32(1e-6))


def test_argument_validation_returns_err_arg_without_a_device(sdy):
    from sdy_amd._lib import SdyHistArgs

    lib = sdy.lib
    n_times, n_bins, T, HW = 6, 300, 3, 16
    data = np.zeros((2, T, HW), dtype=np.float32)          # host memory: a call that passed the checks would not be right
    state = np.zeros(lib.sdy_hist_state_bytes(1), dtype=np.uint8)
    counts = np.zeros((1, n_times, n_bins), dtype=np.uint64)

    def args(**kw):
        a = SdyHistArgs()
        a.nvars = 1
        a.data[0], a.s0[0], a.s1[0] = data.ctypes.data, 0, T * HW
        a.n0, a.n1, a.T, a.HW = 1, 2, T, HW
        a.t_start, a.n_times, a.n_bins = 0, n_times, n_bins
        a.state, a.counts = state.ctypes.data, counts.ctypes.data
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    bad = [dict(t_start=n_times - T + 1), dict(t_start=-1), dict(n_bins=299), dict(n_bins=0), dict(n_bins=4096),
           dict(n0=0), dict(n1=0), dict(T=0), dict(HW=0), dict(HW=-4), dict(n_times=0), dict(nvars=0), dict(nvars=97),
           dict(state=None), dict(counts=None)]
    for kw in bad:
        assert lib.sdy_hist_add(C.byref(args(**kw)), None) == ERR_ARG, kw
    assert lib.sdy_hist_add(None, None) == ERR_ARG                      # NULL table
    a = args()
    a.data[0] = None
    assert lib.sdy_hist_add(C.byref(a), None) == ERR_ARG                # NULL variable
    a = args()
    a.s1[0] = -T * HW
    assert lib.sdy_hist_add(C.byref(a), None) == ERR_ARG                # negative stride
    assert not counts.any() and not state.any()
    assert lib.sdy_hist_state_bytes(0) == 0 and lib.sdy_hist_state_bytes(3) == 3 * lib.sdy_hist_state_bytes(1)
    assert lib.sdy_hist_plan_host(0.0, 1.0, 1, 0.0, 1.0, 7, None, None, None, None, None) == ERR_ARG
    assert lib.sdy_hist_edges_host(0.0, 1.0, 8, None) == ERR_ARG


def test_python_layer_refuses_what_the_kernels_do_not_cover(sdy):
    import torch

    with pytest.raises(ValueError):
        sdy.histogram.HistogramDataWriter(None, 4, n_bins=7)
    with pytest.raises(RuntimeError, match="GPU only"):
        sdy.histogram.HistogramDataWriter(None, 4).append_batch({"a": torch.zeros(1, 2, 4, 8)}, {"a": torch.zeros(1, 2, 4, 8)}, 0, 0)
    with pytest.raises(RuntimeError, match="No data"):
        sdy.histogram.HistogramDataWriter(None, 4).get_dataset()
    assert sdy.DynamicHistogram is sdy.histogram.DynamicHistogram and sdy.HistogramDataWriter is sdy.histogram.HistogramDataWriter
