"""Host side of the neighbourhood verification (no GPU): sdy_fss_accumulate_host -- the header the kernels compile
(csrc/fss.h) -- against the numpy restatement on every case, `sdy_amd.fss.scores` on CPU tensors against a brute-force float64
computation of the fractions, the two r = 0 identities against the event tables, what the entry points refuse, and what
`FractionsSkillAggregator` refuses before it touches a device.  Cases and comparisons: tests/fss_utils.py."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import event_verif_utils as eu
import fss_utils as fu
from window_utils import vp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SDY_OK, SDY_ERR_ARG, SDY_ERR_UNSUPPORTED = 0, -1, -2


@pytest.fixture(scope="module")
def sdy():
    import sdy_amd

    return sdy_amd


@pytest.fixture(scope="module")
def cases():
    return fu.cases()


@pytest.fixture(scope="module")
def wanted(cases):
    return {name: fu.restate(case, brute=True) for name, case in cases.items()}


@pytest.mark.parametrize("name", fu.SMALL)
def test_host_twin_against_restatement(sdy, cases, wanted, name):
    case = cases[name]
    got = fu.host(case)
    assert fu.same(got, wanted[name][0])
    for k in fu.event_names(case):
        assert got[k][..., 0].sum() > 0                                    # some centre is counted at every case's radii
        if case["windows"][0][0] == 0:
            assert (got[k][0] == 0).all()                                  # the initial condition is not counted


def test_host_twin_pooled_equals_the_slots_summed(sdy, cases, wanted):
    for name in ("m3_b2_5x8", "nan_m5_b2_6x8"):
        pooled = fu.host(cases[name], pool=True)
        assert fu.same(pooled, {k: v.sum(axis=0, keepdims=True) for k, v in wanted[name][0].items()})
        assert fu.same(pooled, fu.restate(cases[name], pool=True))


def test_fixture_covers_what_it_claims(cases):
    assert list(cases) == list(fu.SMALL)
    c = cases["m3_b2_5x8"]
    kinds = sorted((d, isinstance(t, np.ndarray)) for _, d, t in c["events"]["a"])
    assert kinds == [("above", False), ("above", True), ("below", False), ("below", True)]
    assert c["radii"] == (0, 1, 2) and (fu.sizes(5, 2) < 5 * 5).tolist() == [True, True, False, True, True]   # clipped at r = 2
    assert [len(c["events"].get(k, ())) for k in c["names"]] == [4, 1, 0]
    assert cases["m2_b2_4x5"]["W"] == 2 * cases["m2_b2_4x5"]["radii"][0] + 1
    assert (cases["m4_b2_5x6"]["H"] * cases["m4_b2_5x6"]["W"]) % 4 != 0
    big = cases["m25_b1_37x40"]
    assert big["H"] > 2 * 16 and big["radii"][-1] == 15 and big["M"] * 31 * 31 <= 65535
    full = cases["m64_b1_33x32_full"]
    assert full["M"] * 31 * 31 == 61504 and 61504 ** 2 < 2 ** 32 and 64 * 33 * 33 > 65535
    assert all(g.ndim == 4 for _, _, gen in cases["m1_b2_6x8"]["windows"] for g in gen.values())


def test_known_answer_at_the_bounds(sdy, cases):
    """Every member and the truth in the event everywhere, M = 64, r = 15 on 33 x 32: K = 64 n, O = n at every centre."""
    got = fu.host(cases["m64_b1_33x32_full"])["a"]
    n = fu.sizes(33, 15).astype(np.float64)
    assert n.max() == 31 * 31 and n.min() == 31 * 16
    want = np.stack([np.full(33, 32.0), 32 * 64 * n, 32 * n, 32 * (64 * n) ** 2, 32 * 64 * n * n, 32 * n * n], axis=-1)
    assert np.array_equal(got[1, 0, 0], want) and np.array_equal(got[2, 0, 0], want) and (got[0] == 0).all()


def test_nan_removes_the_centres_within_r_and_no_others(sdy):
    """One NaN target at (lat 6, lon 3) of a 13 x 12 grid, everything else in the event: at radius r the rows within r of lat 6
    lose exactly the 2r + 1 centres within r of lon 3, every other row keeps its 12.  The same for a NaN in a threshold map;
    a NaN member removes nothing."""
    H, W, M = 13, 12, 3
    for where in ("target", "map", "member"):
        y = np.ones((1, 1, H, W), np.float32)
        g = np.ones((M, 1, 1, H, W), np.float32)
        thr = np.zeros((H, W), np.float32)
        if where == "target":
            y[0, 0, 6, 3] = np.nan
        elif where == "map":
            thr[6, 3] = np.nan
        else:
            g[1, 0, 0, 6, 3] = np.nan
        case = dict(M=M, B=1, H=H, W=W, names=["a"], weights=np.ones((H, W), np.float32), n_timesteps=2, radii=(0, 1, 2, 4),
                    windows=[(1, {"a": y}, {"a": g})], events={"a": [("positive", "above", thr)]})
        got = fu.host(case)["a"][1, 0]                                      # (R, H, 6)
        assert fu.same({"a": fu.host(case)["a"]}, fu.restate(case))
        for j, r in enumerate(case["radii"]):
            lost = np.where(np.abs(np.arange(H) - 6) <= r, 2 * r + 1, 0)
            assert np.array_equal(got[j, :, 0], W - (0 * lost if where == "member" else lost)), (where, r)
            if where == "member":                                           # one member short at the points that see (6, 3)
                n = fu.sizes(H, r)
                assert np.array_equal(got[j, :, 1], W * M * n - lost)
                assert np.array_equal(got[j, :, 2], W * n)


# ---- the scores ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", fu.SMALL)
def test_scores_against_brute_force(sdy, cases, wanted, name):
    case = cases[name]
    sums, frac = wanted[name]
    w = fu.lat_weights(case)
    for k in fu.event_names(case):
        centres = np.zeros(case["n_timesteps"])
        for start, target, _ in case["windows"]:
            centres[start + (1 if start == 0 else 0):start + target[k].shape[1]] += case["B"] * case["W"]
        got = sdy.fss.scores(torch.from_numpy(sums[k]), case["M"], case["radii"], torch.from_numpy(w),
                             centres=torch.from_numpy(centres)[:, None])
        assert all(v.dtype == torch.float64 and not v.is_cuda and tuple(v.shape) == sums[k].shape[:3] for v in got.values())
        want = fu.brute_scores(frac[k])
        assert sorted(got) == sorted(want) == sorted(fu.SLOT_METRICS)
        for metric in fu.SLOT_METRICS:
            fu.close(got[metric].numpy(), want[metric], f"{name} {k} {metric}")
        empty = sums[k][..., 0].sum(axis=-1) == 0
        assert all(bool(torch.isnan(v[torch.from_numpy(empty)]).all()) for v in got.values())      # without counts: NaN
        assert not empty[1:].any()
        without = sdy.fss.scores(torch.from_numpy(sums[k]), case["M"], case["radii"], torch.from_numpy(w))
        assert bool(torch.isnan(without["counted_fraction"]).all()) and torch.equal(without["fbs"][1:], got["fbs"][1:])


def test_scores_known_values(sdy):
    """By hand: one row, r = 0 (n = 1), M = 2: four centres with (K, O) = (2, 1), (0, 0), (1, 1), (1, 0)."""
    s = torch.tensor([[[4.0, 4.0, 2.0, 6.0, 3.0, 2.0]]])
    got = sdy.fss.scores(s, 2, (0,), torch.ones(1), centres=torch.tensor(8.0))
    assert float(got["fbs"]) == 0.125 and float(got["fss"]) == 1.0 - 0.5 / 3.5
    assert float(got["base_rate"]) == 0.5 and float(got["forecast_rate"]) == 0.5 and float(got["fss_useful"]) == 0.75
    assert float(got["counted_fraction"]) == 0.5
    with pytest.raises(ValueError, match="sums are"):
        sdy.fss.scores(torch.zeros(2, 3, 5), 2, (0, 1), torch.ones(3))
    with pytest.raises(ValueError, match="sums are"):
        sdy.fss.scores(torch.zeros(2, 3, 6), 2, (0,), torch.ones(3))
    assert np.array_equal(sdy.fss.neighbourhood_sizes(5, (0, 2)).numpy(), np.stack([fu.sizes(5, 0), fu.sizes(5, 2)]))


# ---- the two identities at r = 0 -------------------------------------------------------------------------------------------
def _event_case(case):
    """The case as tests/event_verif_utils.py reads it."""
    return {k: v for k, v in case.items() if k != "radii"}


@pytest.mark.parametrize("name", ["m3_b2_5x8", "m4_b2_5x6", "m1_b2_6x8", "nan_m5_b2_6x8"])
def test_radius_zero_follows_from_the_event_table(sdy, cases, name):
    """Integer for integer from sdy_event_table_accumulate_host: count = sum table, sum K = sum k table, sum O = sum table[1],
    sum K^2 = sum k^2 table, sum K O = sum k table[1], sum O^2 = sum O.  And `fbs` is the `brier_score` of `events.scores`."""
    case = cases[name]
    assert case["radii"][0] == 0
    sums = fu.host(case)
    tables, _ = eu.host(_event_case(case))
    k = np.arange(case["M"] + 1, dtype=np.float64)
    w = torch.from_numpy(fu.lat_weights(case))
    for var in fu.event_names(case):
        t = tables[var]                                                     # (slots, E, H, 2, M + 1)
        want = np.stack([t.sum(axis=(-1, -2)), (t * k).sum(axis=(-1, -2)), t[..., 1, :].sum(axis=-1), (t * k * k).sum(axis=(-1, -2)),
                         (t[..., 1, :] * k).sum(axis=-1), t[..., 1, :].sum(axis=-1)], axis=-1)
        assert np.array_equal(sums[var][:, :, 0], want)
        fbs = sdy.fss.scores(torch.from_numpy(sums[var]), case["M"], case["radii"], w)["fbs"][..., 0]
        brier = sdy.events.scores(torch.from_numpy(t), w)["brier_score"]
        fu.close(fbs.numpy(), brier.numpy(), f"{name} {var} fbs at r = 0 against brier_score")


# ---- the entry points ------------------------------------------------------------------------------------------------------
def _small_call(M=3, pool=False, radii=(0, 1)):
    rng = np.random.default_rng(3)
    target = {"a": rng.standard_normal((2, 3, 4, 6)).astype(np.float32)}
    gen = {"a": rng.standard_normal((M, 2, 3, 4, 6)).astype(np.float32)}
    events = {"a": [("hi", "above", 0.5), ("lo", "below", np.zeros((4, 6), np.float32))]}
    case = dict(M=M, B=2, H=4, W=6, names=["a"], events=events, radii=radii)
    n_slots = 1 if pool else 5
    acc = np.full((1, n_slots, 2, len(radii), 4, 6), 7.0)
    ws = np.zeros(1 * 2 * 2 * 3 * 4 * 6 * 2 + 8, np.uint8)
    a, keep = fu.args(case, target, gen, ["a"], 1, 0, n_slots, pool, acc, ws)
    return a, keep, acc


def _codes(sdy, a):
    """The entry points that check the whole structure: the twin, and the three device ones -- refused without a device."""
    lib = sdy.lib
    return [lib.sdy_fss_accumulate_host(C.byref(a)), lib.sdy_fss_accumulate(C.byref(a), None), lib.sdy_fss_encode(C.byref(a), None),
            lib.sdy_fss_sum(C.byref(a), None)]


@pytest.mark.parametrize("field,value,code", [
    ("acc", None, SDY_ERR_ARG), ("scalars", None, SDY_ERR_ARG), ("maps", None, SDY_ERR_ARG),    # NULL pointers
    ("acc", "+4", SDY_ERR_ARG), ("ws", "+4", SDY_ERR_ARG),                                      # off an 8-byte boundary
    ("scalars", "+2", SDY_ERR_ARG), ("maps", "+2", SDY_ERR_ARG),
    ("n_events", 0, SDY_ERR_ARG), ("n_events", 9, SDY_ERR_ARG),                                 # E outside 1..8
    ("n_radii", 0, SDY_ERR_ARG), ("n_radii", 5, SDY_ERR_ARG),
    ("radii", (1, 1), SDY_ERR_ARG), ("radii", (2, 1), SDY_ERR_ARG), ("radii", (-1, 1), SDY_ERR_ARG),      # not ascending, negative
    ("radii", (0, 3), SDY_ERR_ARG),                                                             # 2r + 1 = 7 > W = 6
    ("t0", 4, SDY_ERR_ARG), ("t0", -1, SDY_ERR_ARG),                                            # the slot rules of the event table
    ("t_start", 3, SDY_ERR_ARG), ("t_start", -1, SDY_ERR_ARG), ("n_slots", 2, SDY_ERR_ARG), ("n_slots", 0, SDY_ERR_ARG),
    ("n_maps", 0, SDY_ERR_ARG), ("map_first0", 1, SDY_ERR_ARG),
    ("ws_bytes", 2 * 2 * 3 * 4 * 6 * 2 - 1, SDY_ERR_ARG),                                       # a workspace that is too small
    ("gs0", -1, SDY_ERR_ARG), ("nvars", 0, SDY_ERR_ARG), ("nvars", 97, SDY_ERR_ARG), ("H", 0, SDY_ERR_ARG), ("W", 0, SDY_ERR_ARG),
    ("gen0", None, SDY_ERR_ARG), ("target0", None, SDY_ERR_ARG),
    ("n0", 65, SDY_ERR_UNSUPPORTED),                                                            # M over the maximum
    (("W", "radii", "n0", "ws_bytes"), (64, (0, 16), 64, 1 << 40), SDY_ERR_UNSUPPORTED),        # 64 x 33^2 > 65535
    (("W", "radii", "n0", "ws_bytes"), (64, (0, 26), 25, 1 << 40), SDY_ERR_UNSUPPORTED),        # 25 x 53^2 > 65535
    (("W", "H", "radii", "n0", "ws_bytes"), (512, 1, (0, 128), 1, 1 << 40), SDY_ERR_UNSUPPORTED),         # 257^2 > 65535
])
def test_entry_points_refuse(sdy, field, value, code):
    a, keep, acc = _small_call()
    fields, values = (field, value) if isinstance(field, tuple) else ((field,), (value,))
    for f, v in zip(fields, values):
        if f == "gen0":
            a.gen[0] = None
        elif f == "target0":
            a.target[0] = None
        elif f == "map_first0":
            a.map_first[0] = v
        elif f == "radii":
            a.n_radii = len(v)
            for j, r in enumerate(v):
                a.radii[j] = r
        elif isinstance(v, str):
            setattr(a, f, getattr(a, f) + int(v))
        else:
            setattr(a, f, v)
    assert _codes(sdy, a) == [code] * 4
    assert (acc == 7.0).all()
    lib = sdy.lib
    assert [lib.sdy_fss_accumulate_host(None), lib.sdy_fss_accumulate(None, None), lib.sdy_fss_encode(None, None),
            lib.sdy_fss_sum(None, None)] == [SDY_ERR_ARG] * 4


def test_radii_at_the_bounds_are_accepted(sdy):
    """M = 64 allows r = 15 and M = 25 allows r = 25: the twin takes them (the device entry points would launch)."""
    for M, r in ((64, 15), (25, 25)):
        W = 2 * r + 1
        y = {"a": np.zeros((1, 1, 2, W), np.float32)}
        g = {"a": np.ones((M, 1, 1, 2, W), np.float32)}
        case = dict(M=M, B=1, H=2, W=W, names=["a"], events={"a": [("hi", "above", 0.5)]}, radii=(r,))
        acc = np.zeros((1, 1, 1, 1, 2, 6))
        a, keep = fu.args(case, y, g, ["a"], 0, 0, 1, False, acc)
        assert sdy.lib.sdy_fss_accumulate_host(C.byref(a)) == SDY_OK
        n = 2 * W
        assert np.array_equal(acc[0, 0, 0, 0], np.tile([W, W * M * n, 0, W * (M * n) ** 2, 0, 0], (2, 1)))


def test_the_twin_needs_no_workspace_and_the_device_does(sdy):
    a, keep, acc = _small_call()
    a.ws, a.ws_bytes = None, 0
    assert _codes(sdy, a) == [SDY_OK] + [SDY_ERR_ARG] * 3
    assert acc.sum() > 7.0 * acc.size


def test_counter_and_index_bounds(sdy):
    """One call's largest row sum reaches 2^53; n_slots x H reaches 2^40; the second kernel's LDS cannot hold 2 r_max + 1 rows
    of sums."""
    lib = sdy.lib
    # n1 W (M n_max)^2 = 2^21 x 64 x (61504)^2 > 2^53, with a workspace no smaller than its codes would be
    a, keep, acc = _small_call()
    for f, v in zip(("n0", "n1", "H", "W", "T", "t0", "n_slots"), (64, 1 << 21, 31, 64, 1, 0, 1)):
        setattr(a, f, v)
    a.n_radii, a.radii[0], a.ws_bytes = 1, 15, 1 << 62
    assert lib.sdy_fss_accumulate_host(C.byref(a)) == SDY_ERR_UNSUPPORTED and lib.sdy_fss_accumulate(C.byref(a), None) == SDY_ERR_UNSUPPORTED
    a.n1 = 1                                                               # 64 x 61504^2 < 2^53: this one is not the reason
    a.t_start, a.n_slots, a.H = 0, 1 << 30, 1 << 10                        # n_slots x H = 2^40
    a.W, a.T = 64, 1
    assert lib.sdy_fss_accumulate_host(C.byref(a)) == SDY_ERR_UNSUPPORTED and lib.sdy_fss_accumulate(C.byref(a), None) == SDY_ERR_UNSUPPORTED
    a, keep, acc = _small_call()
    a.W, a.n_radii, a.radii[0], a.n0, a.ws_bytes = 4096, 1, 3, 1, 1 << 62  # 7 rows of 4096 sums and one of 4102: over 64 KB
    assert lib.sdy_fss_accumulate_host(C.byref(a)) == SDY_ERR_UNSUPPORTED and lib.sdy_fss_sum(C.byref(a), None) == SDY_ERR_UNSUPPORTED
    assert (acc == 7.0).all()


def test_pooled_takes_one_slot_only_and_an_empty_window_is_ok(sdy):
    a, keep, acc = _small_call(pool=True)
    a.t_start = 1000                                                       # not looked at when the times are pooled
    assert sdy.lib.sdy_fss_accumulate_host(C.byref(a)) == SDY_OK
    a.n_slots = 2
    assert _codes(sdy, a) == [SDY_ERR_ARG] * 4
    a, keep, acc = _small_call()
    a.t0 = a.T                                                             # T - t0 == 0: nothing is launched, so no device needed
    assert _codes(sdy, a) == [SDY_OK] * 4 and (acc == 7.0).all()


def test_workspace_bytes(sdy):
    f = sdy.lib.sdy_fss_workspace_bytes
    assert f(1, 2, 2, 3, 4, 6) == 2 * 2 * 3 * 4 * 6 * 2 and f(63, 1, 1, 7, 180, 360) == 63 * 7 * 180 * 360 * 2
    assert f(1, 1, 1, 1, 1, 1) == 8                                        # rounded up to 8 bytes
    for bad in ((0, 1, 1, 1, 4, 6), (97, 1, 1, 1, 4, 6), (1, 0, 1, 1, 4, 6), (1, 9, 1, 1, 4, 6), (1, 1, 0, 1, 4, 6),
                (1, 1, 1, 0, 4, 6), (1, 1, 1, 1, 0, 6), (1, 1, 1, 1, 4, 0), (1, 1, 1, 2, 1 << 15, (1 << 14) + 1),
                (96, 8, (1 << 31) - 1, 1, 1 << 15, 1 << 15)):
        assert f(*bad) == 0, bad


def test_struct_is_in_the_handshake(sdy):
    from sdy_amd import _lib

    at = _lib.ABI_STRUCTS.index(_lib.SdyFssArgs)
    assert _lib.ABI_STRUCTS[at - 1] is _lib.SdyEventArgs and len(_lib.ABI_STRUCTS) == 25 and _lib.SDY_FSS_MAX_RADII == 4
    hdr = open(os.path.join(ROOT, "include", "sdy_amd.h")).read()
    assert "#define SDY_FSS_MAX_RADII 4\n" in hdr and "#define SDY_ABI_STRUCTS 25\n" in hdr


# ---- the Python class, as far as it goes without a device -----------------------------------------------------------------
def _window(M=3, B=2, T=3, H=4, W=6, names=("a", "b")):
    g = torch.Generator().manual_seed(0)
    target = {k: torch.randn(B, T, H, W, generator=g) for k in names}
    gen = {k: torch.randn(M, B, T, H, W, generator=g) for k in names}
    return target, gen


def _record(agg, target, gen, **kw):
    agg.record_batch(loss=0.0, target_data=target, gen_data=gen, target_data_norm=target, gen_data_norm=gen, **kw)


def _events(sdy, names=("a",)):
    ev = sdy.Events()
    for k in names:
        ev.add(k, "hi", above=0.5)
    return ev


def test_class_refusals_at_construction(sdy):
    w = torch.ones(4, 6)
    sdy.FractionsSkillAggregator(_events(sdy), (0, 1, 2), w * torch.arange(1.0, 5.0)[:, None], n_timesteps=3)
    for bad in ((), (0, 1, 2, 3, 4), (1, 1), (2, 1), (-1, 0), (0.5, 1)):
        with pytest.raises(ValueError, match="radii are 1 .. 4 non-negative integers, strictly ascending"):
            sdy.FractionsSkillAggregator(_events(sdy), bad, w, n_timesteps=3)
    w[2, 3] = 1.5
    with pytest.raises(ValueError, match="FractionsSkillAggregator: the area weights vary along a latitude row"):
        sdy.FractionsSkillAggregator(_events(sdy), (1,), w, n_timesteps=3)
    with pytest.raises(ValueError, match="FractionsSkillAggregator needs an sdy_amd.Events with at least one event"):
        sdy.FractionsSkillAggregator(sdy.Events(), (1,), torch.ones(4, 6), n_timesteps=3)
    with pytest.raises(ValueError, match="workspace_bytes must be positive"):
        sdy.FractionsSkillAggregator(_events(sdy), (1,), torch.ones(4, 6), n_timesteps=3, workspace_bytes=0)


def test_class_refuses_before_the_device(sdy):
    agg = sdy.FractionsSkillAggregator(_events(sdy), (0, 3), torch.ones(4, 6), n_timesteps=3)
    before = dict(vars(agg))
    with pytest.raises(ValueError, match="radius 3: a neighbourhood of 7 longitudes on a grid of 6"):
        _record(agg, *_window())
    agg = sdy.FractionsSkillAggregator(_events(sdy), (16,), torch.ones(4, 40), n_timesteps=3)
    with pytest.raises(ValueError, match=r"64 members x \(2 x 16 \+ 1\)\^2 points exceed 65535"):
        _record(agg, *_window(M=64, B=1, T=1, W=40))
    agg = sdy.FractionsSkillAggregator(_events(sdy), (1,), torch.ones(4, 6), n_timesteps=3, workspace_bytes=2 * 3 * 4 * 6 * 2 - 1)
    with pytest.raises(ValueError, match="one variable's codes need 288 bytes, more than workspace_bytes = 287"):
        _record(agg, *_window())
    agg = sdy.FractionsSkillAggregator(_events(sdy), (0, 1), torch.ones(4, 6), n_timesteps=3)
    before = dict(vars(agg))
    with pytest.raises(RuntimeError, match="GPU only"):
        _record(agg, *_window())
    assert vars(agg) == before and agg._names is None and agg._scalars is None and agg._ws is None      # nothing changed
    with pytest.raises(ValueError, match="No data recorded"):
        agg.get_logs("x")
    with pytest.raises(ValueError, match="No data recorded"):
        agg.get_data()
    target, gen = _window()
    flat = {k: v.reshape(-1, *v.shape[2:])[:5] for k, v in gen.items()}
    with pytest.raises(ValueError, match="FractionsSkillAggregator needs member-stacked"):
        _record(agg, target, flat)
    with pytest.raises(ValueError, match="times 2..4 outside the aggregator's 3"):
        _record(agg, *_window(), i_time_start=2)
    with pytest.raises(ValueError, match="at most 64 members, got 65"):
        _record(agg, *_window(M=65, B=1, T=1))


def test_class_sizes_its_accumulators(sdy):
    need = 8 * (3 * 1 * 2 * 4 * 6)                                         # (slots, E, radii, lat, 6)
    agg = sdy.FractionsSkillAggregator(_events(sdy), (0, 1), torch.ones(4, 6), n_timesteps=3, max_bytes=need - 1)
    with pytest.raises(ValueError, match=f"need {need} bytes"):
        _record(agg, *_window())


def test_inference_aggregator_option_is_off_by_default(sdy):
    w = torch.ones(4, 6)
    agg = sdy.metrics.InferenceAggregator(w, n_timesteps=3, n_ensemble_members=2, events=_events(sdy))
    assert "fss" not in agg._aggregators
    agg = sdy.metrics.InferenceAggregator(w, n_timesteps=3, n_ensemble_members=2, events=_events(sdy), event_neighbourhoods=(1, 2),
                                          event_pool_times=True)
    fss = agg._aggregators["fss"]
    assert isinstance(fss, sdy.FractionsSkillAggregator) and fss._radii == [1, 2] and fss._n_slots == 1
    assert list(agg._aggregators)[-2:] == ["events", "fss"]
    with pytest.raises(ValueError, match="event_neighbourhoods needs events="):
        sdy.metrics.InferenceAggregator(w, n_timesteps=3, n_ensemble_members=2, event_neighbourhoods=(1,))


def test_the_out_of_scope_notes_are_gone():
    for path in ("spherical-dyffusion_amd/events.py", "DESIGN.md"):
        text = " ".join(open(os.path.join(ROOT, path)).read().split())
        assert "neighbourhood (fractions-skill) scores, plots" not in text and "(fractions-skill) scores and plots are out" not in text
