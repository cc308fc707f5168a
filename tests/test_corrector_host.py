"""Post-step state corrector (reference src/ace_inference/core/corrector.py): the side that needs no GPU.  The host entry point
`sdy_corrector_host` -- the device kernels' own per-column arithmetic and scalar solve (csrc/corrector_math.h) with the same
1024-column partition of the float64 sums -- against every case of the reference's own `Corrector`
(tests/golden/fx_corrector.npz); the float64 restatement the GPU tests use at larger sizes against the same fixture; name
resolution, errors, refusal of CPU tensors and the C ABI's argument checks.

Parity bound per corrected variable (`corrector_utils.parity_bound`):
    max|ours - ref64| <= c * max|ref32 - ref64| + 4 * 2^-24 * max|ref64|
`ref32` / `ref64` are the reference's class on float32 / float64 inputs, so the first term is the reference's own fp32 error
(it carries the cancellation in the water-path tendency) and the second the handful of fp32 roundings per element.
Measured ratio max|ours - ref64| / max|ref32 - ref64| of the host entry point over the 31 cases x their rewritten variables
(printed by test_host_matches_reference): largest 1.13 (`b2k3_zero_adv`: the advective tendency minus its mean, where both
errors are one rounding of the subtraction); recomputed advective tendency 0.31 .. 0.85 with the dry-air rule on (what is left
is the fp32 surface pressure) and 0.01 .. 0.05 without it, scaled precipitation / latent heat flux 0.01 .. 0.74, surface
pressure 0.61 .. 0.76.  The budget rule's figures are below the reference's because the water-path tendency is formed in
float64 and rounded once (csrc/corrector_math.h), which test_budget_identity_per_column needs.  The kernel on the MI355X gives
the same figures (tests/test_gpu_corrector.py).  C = 3.5, about 3 x the largest ratio."""
import ctypes as C

import pytest
import torch

import corrector_utils as cu

C_PARITY = 3.5


@pytest.fixture(scope="module")
def sdy():
    import sdy_amd

    return sdy_amd


class _Sigma:
    def __init__(self, ak, bk):
        self.ak, self.bk = ak, bk


@pytest.mark.parametrize("name", cu.case_names())
def test_restatement_matches_reference_float64(name):
    d = cu.case_data(name)
    got = cu.corrector64(d["config"], d["area"], d["ak"], d["bk"], d["d_in"], d["d_gen"])
    assert list(got) == d["written"] or sorted(got) == sorted(d["written"])
    for n, ref in d["ref64"].items():
        assert float((got[n] - ref).abs().max()) <= 1e-12 * float(ref.abs().max()), n


@pytest.mark.parametrize("name", cu.case_names())
def test_host_matches_reference(sdy, name):
    d = cu.case_data(name)
    got = cu.host_corrector(sdy, d["config"], d["ak"], d["bk"], d["area"], d["d_in"], d["d_gen"])
    for n in d["d_gen"]:
        if n not in d["written"]:
            assert torch.equal(got[n], d["d_gen"][n]), f"{n} was touched"
    for n in d["written"]:
        err = float((got[n].double() - d["ref64"][n]).abs().max())
        print(f"{name} {n}: err {err:.3e} ratio {cu.error_ratio(got[n], d['ref32'][n], d['ref64'][n]):.3f}")
        assert err <= cu.parity_bound(d["ref32"][n], d["ref64"][n], C_PARITY), n


def test_reference_itself_meets_the_bound():
    for name in cu.case_names():
        d = cu.case_data(name)
        for n in d["written"]:
            err = float((d["ref32"][n].double() - d["ref64"][n]).abs().max())
            assert err <= cu.parity_bound(d["ref32"][n], d["ref64"][n], 1.0)


@pytest.mark.parametrize("name", ["b2k8_all_advection_and_precipitation", "b2k3_all_advection_and_evaporation", "b3k2_dry"])
def test_normalised_layout_equals_plain_layout(sdy, name):
    """The stepper's layout (normalised, packed, in place) against plain tensors holding the very same physical values
    (x * std + mean formed in fp32 as the kernel forms it): only the stored form's rounding differs."""
    d = cu.case_data(name)
    stats = {n: (0.0, 1.0) for n in d["d_gen"]}
    stats.update({cu.pick(d["d_gen"], "ps"): (98000.0, 4000.0), cu.pick(d["d_gen"], "lhf"): (75.0, 40.0),
                  cu.pick(d["d_gen"], "prate"): (3.0e-5, 2.0e-5), cu.ADV: (1.0e-6, 1.5e-5)})
    for k, n in enumerate(cu.water_names(d["d_gen"])):
        stats[n] = (float(d["d_gen"][n].mean()), float(d["d_gen"][n].std()))
    phys = []
    for src in (d["d_in"], d["d_gen"]):
        x = {n: ((v.double() - stats[n][0]) / stats[n][1]).float() for n, v in src.items()}
        phys.append({n: v * torch.tensor(stats[n][1]) + torch.tensor(stats[n][0]) for n, v in x.items()})
    p_in, p_gen = phys
    plain = cu.host_corrector(sdy, d["config"], d["ak"], d["bk"], d["area"], p_in, p_gen)
    packed = cu.host_corrector(sdy, d["config"], d["ak"], d["bk"], d["area"], p_in, p_gen, stats=stats)
    ref64 = cu.corrector64(d["config"], d["area"], d["ak"], d["bk"], p_in, p_gen)
    for n in p_gen:
        if n not in d["written"]:
            assert packed[n] is p_gen[n], f"{n} was touched"
            continue
        # the stored form rounds (y - mean) / std once more: within the bound's second term
        assert float((packed[n] - plain[n].double()).abs().max()) <= 4.0 * cu.EPS32 * float(ref64[n].abs().max()), n


@pytest.mark.parametrize("name", [n for n in cu.case_names() if "_all_advection_and_" in n])
def test_budget_identity_per_column(sdy, name):
    """With a recomputed advective tendency the budget of the corrected fp32 fields closes per column, in float64, to one
    rounding of the water path (corrector_utils.budget_identity): the tendency is formed in float64 and rounded once."""
    d = cu.case_data(name)
    got = cu.host_corrector(sdy, d["config"], d["ak"], d["bk"], d["area"], d["d_in"], d["d_gen"])
    resid, bound = cu.budget_identity(got, d["d_in"], d["ak"], d["bk"])
    print(f"budget identity {name}: {resid:.3e} bound {bound:.3e}")
    assert resid <= bound


def test_partition_of_the_sums_does_not_depend_on_the_batch(sdy):
    d = cu.case_data("b2k8_all_advection_and_evaporation")
    full = cu.host_corrector(sdy, d["config"], d["ak"], d["bk"], d["area"], d["d_in"], d["d_gen"])
    for b in range(2):
        one = cu.host_corrector(sdy, d["config"], d["ak"], d["bk"], d["area"], {n: v[b:b + 1] for n, v in d["d_in"].items()},
                                {n: v[b:b + 1] for n, v in d["d_gen"].items()})
        for n in d["written"]:
            assert torch.equal(one[n][0], full[n][b]), n


# ---- names and errors ----------------------------------------------------------------------------------------------------
def _corrector(sdy, K=2, **cfg):
    ak, bk = torch.linspace(0.0, 1.0, K + 1), torch.linspace(0.0, 1.0, K + 1)
    return sdy.CorrectorConfig(**cfg).build(torch.ones(4, 6), _Sigma(ak, bk))


FULL = dict(conserve_dry_air=True, zero_global_mean_moisture_advection=True,
            moisture_budget_correction="advection_and_precipitation")


def test_config_defaults_and_reexports(sdy):
    cfg = sdy.CorrectorConfig()
    assert (cfg.conserve_dry_air, cfg.zero_global_mean_moisture_advection, cfg.moisture_budget_correction) == (False, False, None)
    corr = cfg.build(torch.ones(4, 6), _Sigma([0.0, 1.0], [0.0, 1.0]))
    assert isinstance(corr, sdy.Corrector) and not corr.enabled
    assert sdy.corrector.Corrector is sdy.Corrector


def test_name_resolution_follows_climate_data(sdy):
    corr = _corrector(sdy, K=11, **FULL)
    names = [f"specific_total_water_{k}" for k in (10, 2, 0, 1, 3, 4, 5, 6, 7, 8, 9)] + \
        ["PS", "LHFLX", "surface_precipitation_rate", cu.ADV, "TMP2m"]
    plan = corr.resolve(names, names)
    assert plan.gen_water == [f"specific_total_water_{k}" for k in range(11)] == plan.in_water
    assert (plan.gen_ps, plan.in_ps, plan.lhf, plan.prate, plan.adv) == ("PS", "PS", "LHFLX", "surface_precipitation_rate", cu.ADV)
    assert plan.written == ["PS", "surface_precipitation_rate", cu.ADV]
    # the first name of each alias list wins when both are present (ClimateData._get)
    plan = corr.resolve(names + ["PRESsfc", "LHTFLsfc"], names + ["PRESsfc", "LHTFLsfc"])
    assert plan.gen_ps == "PRESsfc" and plan.lhf == "LHTFLsfc"
    evap = _corrector(sdy, zero_global_mean_moisture_advection=True, moisture_budget_correction="evaporation")
    base = ["specific_total_water_0", "specific_total_water_1", "PRESsfc", "LHTFLsfc", "PRATEsfc", cu.ADV]
    assert evap.resolve(base, base).written == ["LHTFLsfc", cu.ADV]
    assert _corrector(sdy, zero_global_mean_moisture_advection=True).resolve([], [cu.ADV]).written == [cu.ADV]


def test_errors(sdy):
    base = ["specific_total_water_0", "specific_total_water_1", "PRESsfc", "LHTFLsfc", "PRATEsfc", cu.ADV]
    without = lambda *drop: [n for n in base if n not in drop]  # noqa: E731
    dry = _corrector(sdy, conserve_dry_air=True)
    with pytest.raises(ValueError, match="surface_pressure is required to force dry air conservation"):
        dry.resolve(without("PRESsfc"), base)
    with pytest.raises(ValueError, match="specific_total_water is required for conservation"):
        dry.resolve(base, without("specific_total_water_0", "specific_total_water_1"))
    with pytest.raises(KeyError):          # what ClimateData raises before the reference's own messages are reached
        dry.resolve(without("PRESsfc"), base)
    full = _corrector(sdy, **FULL)
    for field, name in (("latent_heat_flux", "LHTFLsfc"), ("precipitation_rate", "PRATEsfc"), (cu.ADV, cu.ADV)):
        with pytest.raises(KeyError, match=field):
            full.resolve(base, without(name))
    with pytest.raises(ValueError, match="vertical levels"):
        dry.resolve(base, base + ["specific_total_water_2"])
    for mode in ("precipitation", "evaporation", "advection_and_precipitation", "advection_and_evaporation"):
        with pytest.raises(ValueError, match="zero_global_mean_moisture_advection"):
            _corrector(sdy, moisture_budget_correction=mode)
        with pytest.raises(ValueError, match="zero_global_mean_moisture_advection"):
            _corrector(sdy, conserve_dry_air=True, moisture_budget_correction=mode)
    with pytest.raises(ValueError, match="moisture_budget_correction"):
        _corrector(sdy, zero_global_mean_moisture_advection=True, moisture_budget_correction="advection")


def test_cpu_tensors_raise(sdy):
    d = {n: torch.ones(2, 4, 6) for n in ["specific_total_water_0", "specific_total_water_1", "PRESsfc"]}
    with pytest.raises(RuntimeError, match="GPU only"):
        _corrector(sdy, conserve_dry_air=True)(d, d)


def test_stepper_needs_every_corrected_variable_in_both_packers(sdy):
    full = _corrector(sdy, **FULL)
    base = ["specific_total_water_0", "specific_total_water_1", "PRESsfc", "LHTFLsfc", "PRATEsfc", cu.ADV]
    stats = {n: 1.0 for n in base}
    sdy.MultiStepStepper(None, base, base, [], stats, stats, corrector=full)
    sdy.MultiStepStepper(None, base, base, [], stats, stats, corrector=None)
    with pytest.raises(ValueError, match="in_names and out_names"):
        sdy.MultiStepStepper(None, base[:-1], base, [], stats, stats, corrector=full)
    with pytest.raises(ValueError, match="in_names and out_names"):
        sdy.MultiStepStepper(None, base, base, ["PRATEsfc"], stats, stats, corrector=full)   # a forcing is not in the in packer
    with pytest.raises((ValueError, KeyError)):
        sdy.MultiStepStepper(None, base, base[1:], [], stats, stats, corrector=full)


# ---- the C ABI's argument checks -------------------------------------------------------------------------------------------
def _args(sdy):
    """A valid argument block on host memory: B = 2, K = 2, HW = 12, everything on, plain layout."""
    from sdy_amd import _lib

    HW, B, K = 12, 2, 2
    cfg = dict(FULL)
    ak, bk = torch.tensor([0.0, 0.5, 0.0]), torch.tensor([0.0, 0.4, 1.0])
    area = torch.ones(HW)
    a = cu.host_args(sdy, cfg, ak, bk, area, B, HW)
    buf = torch.rand(12, B, HW) + 0.5
    slots = [a.gen_q[0], a.gen_q[1], a.in_q[0], a.in_q[1], a.gen_ps, a.in_ps, a.gen_lhf, a.gen_prate, a.gen_adv]
    for i, s in enumerate(slots):
        cu._set(s, buf[i], HW)
    out = torch.zeros(4, B, HW)
    for i, s in enumerate([a.out_ps, a.out_lhf, a.out_prate, a.out_adv]):
        cu._set(s, out[i], HW)
    ws = torch.zeros(sdy.lib.sdy_corrector_workspace_bytes(B, HW) // 8 + 1, dtype=torch.float64)
    a.ws, a.ws_bytes = ws.data_ptr(), ws.numel() * 8
    return a, (area, buf, out, ws, _lib)


def test_abi_argument_checks(sdy):
    lib = sdy.lib
    a, keep = _args(sdy)
    assert lib.sdy_corrector_host(C.byref(a)) == 0
    assert lib.sdy_corrector_workspace_bytes(2, 12) == 2 * 8 * 8 + 2 * 16
    assert lib.sdy_corrector_workspace_bytes(3, 1025) == 3 * 2 * 8 * 8 + 3 * 16
    assert lib.sdy_corrector_workspace_bytes(0, 12) == 0

    def bad(mutate, code=-1, device=False):
        b, keep_b = _args(sdy)
        mutate(b)
        fn = lib.sdy_corrector if device else lib.sdy_corrector_host
        rc = fn(C.byref(b), None) if device else fn(C.byref(b))
        assert rc == code, (rc, code)

    for dev in (False, True):      # the device entry point refuses before it launches: no GPU is touched
        bad(lambda b: setattr(b.gen_ps, "channel", -1), device=dev)                 # bad index
        bad(lambda b: setattr(b.gen_q[1], "channel", 1), device=dev)                # index past the sample stride
        bad(lambda b: setattr(b.out_adv, "channel", 1), device=dev)
        bad(lambda b: setattr(b.in_ps, "stride", 11), device=dev)                   # bad stride: samples would overlap
        bad(lambda b: setattr(b.gen_lhf, "stride", -12), device=dev)
        bad(lambda b: setattr(b.out_ps, "stride", 0), device=dev)
        bad(lambda b: setattr(b, "K", 0), device=dev)                               # K out of range
        bad(lambda b: setattr(b, "K", 17), device=dev)
        bad(lambda b: setattr(b, "B", 0), device=dev)
        bad(lambda b: setattr(b, "HW", 0), device=dev)
        bad(lambda b: setattr(b, "flags", 4), device=dev)
        bad(lambda b: setattr(b, "budget", 5), device=dev)
        bad(lambda b: setattr(b, "budget", -1), device=dev)
        bad(lambda b: setattr(b, "area", None), device=dev)
        bad(lambda b: setattr(b.gen_prate, "base", None), device=dev)
        bad(lambda b: setattr(b.in_q[0], "base", None), device=dev)
        bad(lambda b: setattr(b.out_prate, "base", None), device=dev)
        bad(lambda b: setattr(b.gen_ps, "std", 0.0), device=dev)
        bad(lambda b: setattr(b.gen_adv, "mean", float("nan")), device=dev)
    # the workspace: device entry point only (the host twin keeps its sums on the stack)
    bad(lambda b: setattr(b, "ws_bytes", b.ws_bytes - 16), device=True)             # short workspace
    bad(lambda b: setattr(b, "ws", None), device=True)
    bad(lambda b: setattr(b, "ws", b.ws + 4), device=True)
    bad(lambda b: setattr(b, "B", 65536), code=-2, device=True)
    assert lib.sdy_corrector(None, None) == -1 and lib.sdy_corrector_host(None) == -1
    # what a switched-off rule would read is not required
    b, keep_b = _args(sdy)
    b.flags, b.budget = 2, 0
    b.K = 0
    for s in (b.gen_ps, b.in_ps, b.gen_q[0], b.gen_lhf):
        s.base = None
    b.out_ps.base = None
    assert lib.sdy_corrector_host(C.byref(b)) == 0
