"""sdy_member_gram without a GPU: the host twin (the header the kernel compiles, the device's partition) against exact
arithmetic, exact integers, the zero-weight rule and the placement of NaN, the refusals of both entry points before anything
touches a device, the bindings, and `sdy_amd.field_scores.scores` on CPU tensors against a direct restatement from the fields.
Bounds: tests/member_gram_utils.py."""
import ctypes as C

import numpy as np
import pytest
import torch

import member_gram_utils as mg

ARG, UNSUP = -1, -2


@pytest.fixture(scope="module")
def sdy():
    import sdy_amd

    return sdy_amd


@pytest.mark.parametrize("H,W,M", [(3, 5, 2), (5, 7, 15)])
@pytest.mark.parametrize("with_clim", [False, True])
def test_host_twin_against_exact_rational_arithmetic(sdy, H, W, M, with_clim):
    target, gen, w, clim = mg.seeded_case(M, 2, 2, H, W, seed=100 * H + M)
    clim = clim if with_clim else None
    got = mg.host_gram(sdy, target, gen, w, clim)
    G, A = mg.gram_fraction(target, gen, w, clim)
    worst = mg.check_against_exact(got, G, A, H * W, what=f"{H}x{W} M={M}")
    print(f"worst error {worst:.3f} x 2^-53 sum w |a_i a_j| (bound {H * W + 4})")
    assert np.array_equal(got, np.swapaxes(got, -1, -2))


def test_scaled_integers_are_the_same_exact_arithmetic():
    """What the larger shapes of the GPU tests use instead of Fractions."""
    target, gen, w, clim = mg.seeded_case(3, 1, 2, 3, 5, seed=5)
    G, A = mg.gram_fraction(target, gen, w, clim)
    Gi, Ai = mg.gram_exact(target, gen, w, clim)
    for idx in np.ndindex(*G.shape):
        assert G[idx] * mg.EXACT_SCALE == Gi[idx] and A[idx] * mg.EXACT_SCALE == Ai[idx]


@pytest.mark.parametrize("H,W,M", [(5, 7, 0), (6, 10, 14), (6, 10, 15), (40, 72, 5)])
def test_host_twin_exact_integers(sdy, H, W, M):
    """Small integers: every entry is an integer below 2^53 whatever the order of the sums: bit for bit numpy's int64."""
    target, gen, w, clim = mg.integer_case(M, 2, 2, H, W, seed=7 + M)
    for c in (None, clim):
        got = mg.host_gram(sdy, target, gen, w, c)
        want = mg.gram_int64(target, gen, w, c)
        assert np.array_equal(got, want.astype(np.float64))
    assert (w == 0).any() and np.abs(want).max() < 2 ** 53
    if M == 0:                                        # flat rows == one stacked member
        assert np.array_equal(mg.host_gram(sdy, target, gen[None], w, clim), got)


def test_packed_index_and_unpack(sdy):
    from sdy_amd.field_scores import gram_index, unpack

    for N in (3, 16, 17, 66):
        k = 0
        for i in range(N):
            for j in range(i, N):
                assert gram_index(i, j, N) == mg.index(i, j, N) == k
                k += 1
        assert k == mg.entries(N)
        packed = np.arange(k, dtype=np.float64)
        assert np.array_equal(unpack(torch.from_numpy(packed), N).numpy(), mg.unpack(packed, N))
    with pytest.raises(ValueError):
        unpack(torch.zeros(5, dtype=torch.float64), 3)


def test_zero_weight_rule_and_nan_placement(sdy):
    M, S, T, H, W = 4, 2, 2, 6, 10
    target, gen, w, clim = mg.seeded_case(M, S, T, H, W, seed=3)
    zero = np.argwhere(w == 0)
    live = np.argwhere(w != 0)
    assert len(zero) >= 3 and len(live) >= 3
    base = mg.host_gram(sdy, target, gen, w, clim)
    # NaN and Inf under zero weight, in a member, the target and the climatology: nothing changes, bit for bit
    g2, t2, c2 = gen.copy(), target.copy(), clim.copy()
    g2[1, 0, 1, zero[0][0], zero[0][1]] = np.nan
    g2[2, 1, 0, zero[1][0], zero[1][1]] = np.inf
    t2[0, 0, zero[2][0], zero[2][1]] = np.nan
    c2[zero[0][0], zero[0][1]] = -np.inf
    assert np.array_equal(mg.host_gram(sdy, t2, g2, w, c2), base)
    # a NaN in member m under a positive weight: exactly row and column 1 + m of that (sample, time)
    m, s, t = 2, 1, 0
    g3 = gen.copy()
    g3[m, s, t, live[1][0], live[1][1]] = np.nan
    got = mg.host_gram(sdy, target, g3, w, clim)
    poisoned = np.zeros(got.shape, bool)
    poisoned[s, t, 1 + m, :] = poisoned[s, t, :, 1 + m] = True
    assert np.array_equal(np.isnan(got), poisoned)
    assert np.array_equal(got[~poisoned], base[~poisoned])
    # a NaN in the target: every member's row and the truth's, not Gamma_00
    t3 = target.copy()
    t3[s, t, live[2][0], live[2][1]] = np.nan
    got = mg.host_gram(sdy, t3, gen, w, clim)
    poisoned = np.zeros(got.shape, bool)
    poisoned[s, t, 1:, :] = poisoned[s, t, :, 1:] = True
    assert np.array_equal(np.isnan(got), poisoned) and np.array_equal(got[~poisoned], base[~poisoned])
    # the weight sum is Gamma_00, and a climatology of zeros is none
    assert np.allclose(base[..., 0, 0], w.astype(np.float64).sum(), rtol=1e-14)
    assert np.array_equal(mg.host_gram(sdy, target, gen, w, np.zeros_like(clim)), mg.host_gram(sdy, target, gen, w, None))


def test_bindings_and_workspace_bytes(sdy):
    from sdy_amd import _lib

    assert _lib.SdyMemberGramArgs in _lib.ABI_STRUCTS and _lib.SDY_GRAM_MAX_MEMBERS == 64      # tests/test_capi_cpu.py
    ws = sdy.lib.sdy_member_gram_workspace_bytes
    assert ws(2, 3, 2, 2, 2880) == 2 * 2 * 2 * 3 * 15 * 8                    # three chunks of 1024, N = 5: 15 entries
    assert ws(1, 1, 1, 1, 1) == 6 * 8 and ws(96, 64, 1, 1, 1024) == 96 * 2211 * 8 and ws(1, 64, 1, 1, 1025) == 2 * 2211 * 8
    for bad in ((0, 3, 1, 1, 10), (97, 3, 1, 1, 10), (1, 0, 1, 1, 10), (1, 65, 1, 1, 10), (1, 3, 0, 1, 10), (1, 3, 1, 0, 10),
                (1, 3, 1, 1, 0), (-1, 3, 1, 1, 10)):
        assert ws(*bad) == 0, bad
    assert sdy.FieldScoreAggregator is sdy.field_scores.FieldScoreAggregator and sdy.member_gram is sdy.field_scores.member_gram


def _fake_args(sdy, nvars=1, n0=3, n1=2, T=2, HW=35):
    """Plausible arguments whose pointers are never dereferenced: every refusal comes before any access."""
    a = sdy._lib.SdyMemberGramArgs()
    p = 1 << 20
    a.win.nvars, a.win.n0, a.win.n1, a.win.T = nvars, n0, n1, T
    a.win.gs0, a.win.gs1, a.win.ts1 = n1 * T * HW, T * HW, T * HW
    for v in range(nvars):
        a.win.gen[v], a.win.target[v] = p, 2 * p
    a.HW, a.weights, a.out, a.ws = HW, 3 * p, 4 * p, 5 * p
    a.ws_bytes = sdy.lib.sdy_member_gram_workspace_bytes(min(nvars, 96), min(n0, 64), n1, T, HW)
    return a


def test_refusals_before_anything_is_touched(sdy):
    host, dev = sdy.lib.sdy_member_gram_host, lambda a: sdy.lib.sdy_member_gram(C.byref(a), None)   # noqa: E731
    assert host(None) == ARG and sdy.lib.sdy_member_gram(None, None) == ARG

    def both(change, want):
        a = _fake_args(sdy)
        change(a)
        assert host(C.byref(a)) == want and dev(a) == want

    both(lambda a: setattr(a, "weights", None), ARG)
    both(lambda a: setattr(a, "out", None), ARG)
    both(lambda a: setattr(a, "weights", (3 << 20) + 2), ARG)
    both(lambda a: setattr(a, "out", (4 << 20) + 4), ARG)
    both(lambda a: a.climatology.__setitem__(0, (6 << 20) + 1), ARG)
    both(lambda a: setattr(a, "HW", 0), ARG)
    both(lambda a: setattr(a.win, "nvars", 0), ARG)                       # what sdy_window refuses
    both(lambda a: setattr(a.win, "nvars", 97), ARG)
    both(lambda a: setattr(a.win, "n0", 0), ARG)
    both(lambda a: setattr(a.win, "T", 0), ARG)
    both(lambda a: setattr(a.win, "gs1", -1), ARG)
    both(lambda a: a.win.gen.__setitem__(0, None), ARG)
    both(lambda a: a.win.target.__setitem__(0, None), ARG)
    both(lambda a: setattr(a.win, "n0", 65), UNSUP)                       # one member too many
    # 2^31 (sample, time, chunk) work items in a variable
    a = _fake_args(sdy, n0=1, n1=1 << 30, T=2, HW=1)
    assert host(C.byref(a)) == UNSUP and dev(a) == UNSUP
    # 2^38 elements of out and more: the grid of the second launch
    a = _fake_args(sdy, nvars=96, n0=64, n1=1 << 21, T=1, HW=1)
    assert host(C.byref(a)) == UNSUP and dev(a) == UNSUP
    # the workspace: the device entry point only (the host twin takes none)
    for change in (lambda a: setattr(a, "ws", None), lambda a: setattr(a, "ws", (5 << 20) + 4),
                   lambda a: setattr(a, "ws_bytes", a.ws_bytes - 8), lambda a: setattr(a, "ws_bytes", 0)):
        a = _fake_args(sdy)
        change(a)
        assert dev(a) == ARG
    # a climatology pointer of a variable past nvars is not looked at
    a = _fake_args(sdy, n0=65)
    a.climatology[5] = 1
    assert host(C.byref(a)) == UNSUP


@pytest.mark.parametrize("M,with_clim", [(1, False), (2, True), (7, False), (7, True)])
def test_scores_on_cpu_against_the_fields(sdy, M, with_clim):
    """`scores` of the host twin's Gram against a float64 restatement from the fields themselves.  Independent members: D_ii +
    D_jj - 2 D_ij cancels by no more than a factor of 4, so 1e-12 of the term scale sqrt(D_ii + D_jj + 2 |D_ij|) holds for the
    distances; the correlations are O(1) quantities of unit-variance fields and are held to 1e-12 absolutely."""
    from sdy_amd.field_scores import scores

    H, W = 9, 14
    target, gen, w, clim = mg.seeded_case(M, 2, 3, H, W, seed=40 + M)
    clim = clim if with_clim else None
    gram = torch.from_numpy(mg.host_gram(sdy, target, gen, w, clim))
    got = scores(gram, M, climatology=with_clim)
    want, scale = mg.scores_direct(target, gen, w, clim)
    assert set(got) == set(want)
    assert ("anomaly_correlation" in got) == with_clim and ("pattern_correlation" in got) == (not with_clim)
    for key, ref in want.items():
        x = got[key].numpy()
        assert x.shape == (2, 3) and x.dtype == np.float64
        if M == 1 and key in ("member_distance", "distance_ratio"):
            assert np.isnan(x).all()
            continue
        tol = 1e-12 * (scale[key] if key in scale else np.maximum(np.abs(ref), 1.0))
        assert (np.abs(x - ref) <= tol).all(), (key, np.abs(x - ref).max(), tol.min())
    if M == 1:
        assert np.array_equal(got["energy_score"].numpy(), got["error_distance"].numpy())


def test_scores_of_an_all_equal_ensemble_and_of_the_initial_condition(sdy):
    from sdy_amd.field_scores import scores

    target, gen, w, _ = mg.seeded_case(5, 1, 2, 6, 10, seed=9)
    same = np.broadcast_to(gen[:1], gen.shape).copy()
    got = scores(torch.from_numpy(mg.host_gram(sdy, target, same, w)), 5)
    assert (got["member_distance"] == 0).all() and (got["distance_ratio"] == 0).all()         # exactly
    assert torch.equal(got["energy_score"], got["error_distance"]) and (got["error_distance"] > 0).all()
    # (the mean of five equal correlations and the correlation of the mean error: other roundings of the same number)
    assert torch.allclose(got["pattern_correlation"], got["pattern_correlation_member_avg"], rtol=1e-14, atol=0.0)
    # every member IS the truth (an initial condition): distances exactly 0, ratios NaN, the correlation exactly 1
    truth = np.broadcast_to(target[None], gen.shape).copy()
    got = scores(torch.from_numpy(mg.host_gram(sdy, target, truth, w)), 5)
    for key in ("error_distance", "member_distance", "energy_score", "ensemble_mean_rmse"):
        assert (got[key] == 0).all(), key
    assert torch.isnan(got["distance_ratio"]).all() and (got["pattern_correlation"] == 1).all()
    # a constant truth anomaly has no variance: NaN
    flat = np.full_like(target, 2.0)
    got = scores(torch.from_numpy(mg.host_gram(sdy, flat, gen, w)), 5)
    assert torch.isnan(got["pattern_correlation"]).all() and torch.isnan(got["pattern_correlation_member_avg"]).all()
    with pytest.raises(ValueError):
        scores(torch.zeros(4, 4, dtype=torch.float64), 3)


def test_aggregator_refusals_without_gpu(sdy):
    area = torch.ones(4, 8)
    with pytest.raises(ValueError):
        sdy.FieldScoreAggregator(area, n_timesteps=0)
    with pytest.raises(ValueError):
        sdy.FieldScoreAggregator(area, n_timesteps=3, target="other")
    with pytest.raises(ValueError, match="climatology"):
        sdy.FieldScoreAggregator(area, n_timesteps=3, climatology={"a": torch.zeros(8, 4)})
    agg = sdy.FieldScoreAggregator(area, n_timesteps=3, is_ensemble=True, climatology={"zz": torch.zeros(4, 8)})
    t = {"a": torch.zeros(2, 2, 4, 8)}
    with pytest.raises(ValueError, match="member-stacked"):
        agg.record_batch(None, t, {"a": torch.zeros(6, 2, 4, 8)})
    with pytest.raises(ValueError, match="outside"):
        agg.record_batch(None, t, {"a": torch.zeros(3, 2, 2, 4, 8)}, i_time_start=2)
    with pytest.raises(ValueError, match="not generated"):
        agg.record_batch(None, t, {"a": torch.zeros(3, 2, 2, 4, 8)})
    agg = sdy.FieldScoreAggregator(area, n_timesteps=3, is_ensemble=True)
    with pytest.raises(RuntimeError, match="GPU only"):
        agg.record_batch(None, t, {"a": torch.zeros(3, 2, 2, 4, 8)})
    with pytest.raises(ValueError, match="No batches"):
        agg.get_series()
    inf = sdy.metrics.InferenceAggregator(area, n_timesteps=3, n_ensemble_members=3, field_scores=True)
    assert list(inf._aggregators)[-1] == "field_scores" and inf._aggregators["field_scores"].is_ensemble
    assert "field_scores" not in sdy.metrics.InferenceAggregator(area, n_timesteps=3)._aggregators
