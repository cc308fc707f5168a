"""Derived water-budget variables (reference src/ace_inference/inference/derived_variables.py, metrics.py:296-367): the host
side that needs no GPU -- name resolution, the reference's errors and warnings, refusal of CPU tensors, the C ABI's
argument checks, and a float64 numpy restatement of the formulas against the reference's own outputs
(tests/golden/fx_derived.npz), which pins the formulas independently of the kernel."""
import ctypes as C
import json
import logging

import numpy as np
import pytest
import torch

import golden_utils as gu

DERIVED = ["surface_pressure_due_to_dry_air", "total_water_path", "total_water_path_budget_residual"]
BUDGET = ["LHTFLsfc", "PRATEsfc", "tendency_of_total_water_path_due_to_advection"]


@pytest.fixture(scope="module")
def derived():
    import sdy_amd

    return sdy_amd.derived


def _names(K=3, budget=True):
    return [f"specific_total_water_{k}" for k in range(K)] + ["PRESsfc"] + (BUDGET if budget else [])


def test_natural_sort_and_aliases(derived):
    names = ["specific_total_water_10", "specific_total_water_2", "specific_total_water_0", "specific_total_water_1",
             "PS", "LHFLX", "surface_precipitation_rate", "tendency_of_total_water_path_due_to_advection", "TMP2m"]
    for k in range(3, 10):
        names.append(f"specific_total_water_{k}")
    plan = derived.resolve(names, 12, 12)
    assert plan.water == [f"specific_total_water_{k}" for k in range(11)]
    assert plan.surface_pressure == "PS"
    assert plan.budget == ("LHFLX", "surface_precipitation_rate", "tendency_of_total_water_path_due_to_advection")
    assert plan.outputs == DERIVED
    # the first name of each alias list wins when both are present (ClimateData._get)
    plan = derived.resolve(_names() + ["PS", "LHFLX"], 4, 4)
    assert plan.surface_pressure == "PRESsfc" and plan.budget[0] == "LHTFLsfc"
    assert derived.natural_sort(["a11", "a2", "B1", "a1"]) == ["a1", "a2", "a11", "B1"]


def test_missing_inputs_are_skipped_with_a_warning(derived, caplog):
    with caplog.at_level(logging.WARNING):
        plan = derived.resolve(_names(budget=False) + ["LHTFLsfc"], 4, 4)
    assert plan.outputs == DERIVED[:2] and plan.budget is None
    assert [r.getMessage() for r in caplog.records] == [
        "Could not compute total_water_path_budget_residual because 'precipitation_rate' is missing"]
    caplog.clear()
    with caplog.at_level(logging.WARNING):
        plan = derived.resolve(["PRESsfc"] + BUDGET, 4, 4)
    assert plan.outputs == []
    assert [r.getMessage() for r in caplog.records] == [
        f"Could not compute {n} because ['specific_total_water_'] is missing" for n in DERIVED]
    caplog.clear()
    with caplog.at_level(logging.WARNING):
        plan = derived.resolve(_names()[:3] + BUDGET, 4, 4)
    assert plan.outputs == []
    assert all("'surface_pressure' is missing" in r.getMessage() for r in caplog.records) and len(caplog.records) == 3


def test_existing_name_and_level_mismatch_raise(derived):
    for name in DERIVED:
        with pytest.raises(ValueError, match="already exists"):
            derived.resolve(_names() + [name], 4, 4)
    with pytest.raises(ValueError, match="vertical levels"):
        derived.resolve(_names(K=3), 5, 5)
    with pytest.raises(ValueError, match="vertical levels"):
        derived.resolve(_names(K=3), 4, 3)
    # a dict without the dry-air inputs never reaches the level check (the reference: KeyError -> warning first)
    assert derived.resolve(["TMP2m"], 9, 9).outputs == []


def test_cpu_tensors_are_refused_and_inputless_dicts_pass(derived):
    d = {n: torch.rand(2, 3, 4, 8) for n in _names(K=3)}
    sigma = type("S", (), {"ak": torch.zeros(4), "bk": torch.linspace(0, 1, 4)})()
    with pytest.raises(RuntimeError, match="GPU only"):
        derived.compute_derived_quantities(d, sigma)
    with pytest.raises(RuntimeError, match="GPU only"):
        derived.deriver(sigma)(d)
    other = {"TMP2m": torch.rand(2, 3, 4, 8)}
    out = derived.compute_derived_quantities(other, sigma)
    assert out == other and out is not other


def test_reexported(derived):
    import sdy_amd

    assert sdy_amd.compute_derived_quantities is derived.compute_derived_quantities
    assert callable(derived.deriver)


def test_c_abi_argument_checks(derived):
    from sdy_amd import _lib

    lib = _lib.lib
    buf = (C.c_float * 64)()
    base = (C.addressof(buf) + 15) // 16 * 16

    def call(**kw):
        a = _lib.SdyDerivedArgs()
        K = kw.pop("K", 2)
        a.K, a.n0, a.n1, a.T, a.HW, a.s0, a.s1 = K, 1, 1, 2, 8, 0, 16
        for k in range(min(K, _lib.SDY_DERIVED_MAX_LEVELS)):
            a.q[k] = base
        a.ps = a.lhf = a.prate = a.adv = base
        for k, v in kw.items():
            setattr(a, k, v)
        return lib.sdy_derived_water(C.byref(a), None)

    assert call() == 0                                   # no output requested: nothing to do
    assert call(dry=base + 1) == -1                      # misaligned output
    assert call(K=0) == -1 and call(K=17) == -1          # levels outside 1..SDY_DERIVED_MAX_LEVELS
    assert call(HW=6) == -1                              # HW not a multiple of 4
    assert call(s1=18) == -1 and call(T=0) == -1 and call(n1=0) == -1
    assert call(ps=None, twp=base) == -1                 # a required input missing
    assert call(adv=None, resid=base) == -1              # the budget inputs are required for the residual ...
    assert call(q=(C.c_void_p * 16)(*([base + 4] + [base] * 15)), twp=base) == -1     # ... misaligned input
    assert call(n0=300, n1=300, twp=base) == -2          # more than 65535 trajectories


def _restate(d, ak, bk, time_axis):
    """float64 restatement of the three formulas; the residual differenced along `time_axis`."""
    K = len(ak) - 1
    q = [d[f"specific_total_water_{k}"].astype(np.float64) for k in range(K)]
    ps = next(d[n] for n in ("PRESsfc", "PS") if n in d).astype(np.float64)
    lhf = next(d[n] for n in ("LHTFLsfc", "LHFLX") if n in d).astype(np.float64)
    pr = next(d[n] for n in ("PRATEsfc", "surface_precipitation_rate") if n in d).astype(np.float64)
    adv = d["tendency_of_total_water_path_due_to_advection"].astype(np.float64)
    ak, bk = np.asarray(ak, np.float64), np.asarray(bk, np.float64)
    twp = sum(((ak[k + 1] + ps * bk[k + 1]) - (ak[k] + ps * bk[k])) * q[k] for k in range(K)) / 9.80665
    dry = ps - 9.80665 * twp
    res = np.zeros_like(twp)
    cur = [slice(None)] * twp.ndim
    prv = list(cur)
    cur[time_axis], prv[time_axis] = slice(1, None), slice(None, -1)
    cur, prv = tuple(cur), tuple(prv)
    res[cur] = (twp[cur] - twp[prv]) / 21600.0 - (lhf[cur] / 2.5e6 - pr[cur] + adv[cur])
    return {"surface_pressure_due_to_dry_air": dry, "total_water_path": twp, "total_water_path_budget_residual": res}


def test_fixture_matches_float64_restatement():
    z = gu.load("fx_derived")
    for case in json.loads(str(z["cases"])):
        names = json.loads(str(z[f"{case}::names"]))
        d = {n: z[f"{case}::in::{n}"] for n in names}
        ak, bk = z[f"{case}::ak"], z[f"{case}::bk"]
        five = d["tendency_of_total_water_path_due_to_advection"].ndim == 5
        # the reference differences axis 1: the sample axis of a 5-D dict, the time axis of a 4-D one
        ref = _restate(d, ak, bk, time_axis=1)
        for n in DERIVED[:2]:
            got = z[f"{case}::ref::{n}"].astype(np.float64)
            assert np.abs(got - ref[n]).max() <= 2e-6 * np.abs(ref[n]).max(), (case, n)
        scale = max(np.abs(ref["total_water_path"]).max() / 21600.0,
                    max(np.abs(v).max() for k, v in d.items() if k in ("LHTFLsfc", "LHFLX")) / 2.5e6,
                    max(np.abs(v).max() for k, v in d.items() if k in ("PRATEsfc", "surface_precipitation_rate")),
                    np.abs(d["tendency_of_total_water_path_due_to_advection"]).max())
        r = DERIVED[2]
        assert np.abs(z[f"{case}::ref::{r}"] - ref[r]).max() <= 1e-5 * scale, case
        if five:
            # per member (what the port computes): the residual along time, axis 2
            per = _restate(d, ak, bk, time_axis=2)
            for n in DERIVED:
                got = z[f"{case}::member::{n}"].astype(np.float64)
                tol = 1e-5 * scale if n == r else 2e-6 * np.abs(per[n]).max()
                assert np.abs(got - per[n]).max() <= tol, (case, n)
            if d["PRESsfc" if "PRESsfc" in d else "PS"].shape[2] > 1:
                # the recorded reference value of the ensemble residual is NOT the per-member one (the quirk)
                assert np.abs(z[f"{case}::ref::{r}"] - z[f"{case}::member::{r}"]).max() > 100 * 1e-5 * scale
        if d["PRESsfc" if "PRESsfc" in d else "PS"].shape[-3] == 1:
            assert not z[f"{case}::member::{r}" if five else f"{case}::ref::{r}"].any()
