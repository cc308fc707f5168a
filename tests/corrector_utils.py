"""Helpers of the corrector tests: the fixture of the reference's own `Corrector` (tests/golden/fx_corrector.npz, written by
tools/gen_golden.py::gen_corrector), a float64 torch restatement of its three rules (the checker at sizes the fixture cannot
hold; held to the fixture's `ref64` by tests/test_corrector_host.py), the parity bound of the issue, the conservation
diagnostics in float64, plausible random fields, and a driver of the host entry point `sdy_corrector_host`."""
import ctypes as C
import json
import re

import numpy as np
import torch

import golden_utils as gu

ADV = "tendency_of_total_water_path_due_to_advection"
ALIASES = {"ps": ["PRESsfc", "PS"], "lhf": ["LHTFLsfc", "LHFLX"], "prate": ["PRATEsfc", "surface_precipitation_rate"],
           "adv": [ADV]}
WATER = "specific_total_water_"
GRAVITY, LATENT_HEAT, TIMESTEP = 9.80665, 2.5e6, 21600.0
EPS32 = 2.0 ** -24
BUDGET_CODE = {None: 0, "precipitation": 1, "evaporation": 2, "advection_and_precipitation": 3, "advection_and_evaporation": 4}


def natural(names):
    return sorted(names, key=lambda s: [int(c) if c.isdigit() else c.lower() for c in re.split("([0-9]+)", s)])


def pick(d, what):
    return next(n for n in ALIASES[what] if n in d)


def water_names(d):
    return natural([n for n in d if n.startswith(WATER)])


_Z = None


def fixture():
    global _Z
    if _Z is None:
        z = gu.load("fx_corrector")
        _Z = (z, json.loads(str(z["cases"])))
    return _Z


def case_names():
    return [c["name"] for c in fixture()[1]]


def case_data(name):
    """-> dict(config, ak, bk, area, d_in, d_gen, ref32, ref64, written): CPU tensors, inputs under the case's names."""
    z, cases = fixture()
    c = next(c for c in cases if c["name"] == name)
    s, rn = c["set"], c["rename"]
    names = json.loads(str(z[f"{s}::names"]))
    t = lambda k: torch.from_numpy(z[k])  # noqa: E731
    return dict(config=c["config"], ak=t(f"{s}::ak"), bk=t(f"{s}::bk"), area=t(f"{s}::area"), written=c["written"],
                d_in={rn.get(n, n): t(f"{s}::in::{n}") for n in names},
                d_gen={rn.get(n, n): t(f"{s}::gen::{n}") for n in names},
                ref32={n: t(f"{name}::ref32::{n}") for n in c["written"]},
                ref64={n: t(f"{name}::ref64::{n}") for n in c["written"]})


# ---- float64 restatement -------------------------------------------------------------------------------------------------
def wmean(x, area):
    w = area.to(x.dtype)
    return (x * w).sum(dim=(-2, -1)) / w.sum()


def _levels(d, dtype=torch.float64):
    return torch.stack([d[n].to(dtype) for n in water_names(d)], dim=-1)


def twp64(d, ak, bk, dtype=torch.float64):
    ps = d[pick(d, "ps")].to(dtype)
    dp = (ak.to(dtype) + ps[..., None] * bk.to(dtype)).diff(dim=-1)
    return (dp * _levels(d, dtype)).sum(-1) / GRAVITY


def dry64(d, ak, bk, dtype=torch.float64):
    return d[pick(d, "ps")].to(dtype) - GRAVITY * twp64(d, ak, bk, dtype)


def corrector64(config, area, ak, bk, d_in, d_gen, dtype=torch.float64):
    """The reference's three rules in float64 torch, written from the issue's formulas: -> {name: corrected tensor} of the
    rewritten variables.  dtype=torch.float32: the same evaluated in float32 (sums included), the stand-in for the reference's
    fp32 error at sizes the fixture cannot hold."""
    gen = {k: v.to(dtype) for k, v in d_gen.items()}
    out = {}
    budget = config.get("moisture_budget_correction")
    if config.get("conserve_dry_air"):
        q = _levels(gen, dtype)
        dry = dry64(gen, ak, bk, dtype)
        err = wmean(dry, area) - wmean(dry64(d_in, ak, bk, dtype), area)
        a = (ak.to(dtype).diff() * q).sum(-1)
        b = (bk.to(dtype).diff() * q).sum(-1)
        n = pick(gen, "ps")
        gen[n] = out[n] = (dry - err[..., None, None] + a) / (1.0 - b)
    if config.get("zero_global_mean_moisture_advection"):
        gen[ADV] = out[ADV] = gen[ADV] - wmean(gen[ADV], area)[..., None, None]
    if budget is not None:
        tend = (twp64(gen, ak, bk, dtype) - twp64(d_in, ak, bk, dtype)) / TIMESTEP
        lhf, pr = pick(gen, "lhf"), pick(gen, "prate")
        evap = gen[lhf] / LATENT_HEAT
        m_t, m_e, m_p = wmean(tend, area), wmean(evap, area), wmean(gen[pr], area)
        if budget.endswith("precipitation"):
            gen[pr] = out[pr] = gen[pr] * ((m_e - m_t) / m_p)[..., None, None]
        else:
            evap = evap * ((m_t + m_p) / m_e)[..., None, None]
            gen[lhf] = out[lhf] = evap * LATENT_HEAT
        if budget.startswith("advection"):
            gen[ADV] = out[ADV] = tend - (gen[lhf] / LATENT_HEAT - gen[pr])
    return out


def budget_identity(got, d_in, ak, bk):
    """Per-column budget identity of the `advection_and_*` modes, float64 from the corrected fp32 fields `got`:
    -> (max |adv - (tend - (evap - prate))|, bound), bound = 2^-24 * max|twp| / 21600 plus the fp32 roundings of the three
    rate terms (each term's rounding, through the two subtractions that combine them)."""
    twp = twp64(got, ak, bk)
    tend = (twp - twp64(d_in, ak, bk)) / TIMESTEP
    evap, prate = got[pick(got, "lhf")].double() / LATENT_HEAT, got[pick(got, "prate")].double()
    resid = (got[ADV].double() - (tend - (evap - prate))).abs()
    bound = EPS32 * float(twp.abs().max()) / TIMESTEP + \
        2.0 * EPS32 * float(tend.abs().max() + evap.abs().max() + prate.abs().max())
    return float(resid.max()), bound


def parity_bound(ref32, ref64, c):
    """`c * max|ref32 - ref64| + 4 * 2^-24 * max|ref64|` of one corrected variable."""
    return c * float((ref32.double() - ref64).abs().max()) + 4.0 * EPS32 * float(ref64.abs().max())


def error_ratio(ours, ref32, ref64):
    """Our error over the reference's own fp32 error (both against ref64), the figure `c` is set from; the second term of the
    bound is left out of it."""
    ref_err = float((ref32.double() - ref64).abs().max())
    return float((ours.double() - ref64).abs().max()) / ref_err if ref_err > 0 else float("nan")


# ---- plausible fields at any size ---------------------------------------------------------------------------------------
def levels_for(K):
    ak8 = [3.0, 5238.4, 11815.8, 17263.1, 19929.5, 17023.4, 8970.5, 1537.5, 0.0]
    bk8 = [0.0, 0.0, 0.0115, 0.0781, 0.2034, 0.4004, 0.6513, 0.9065, 1.0]
    assert K == 8
    return torch.tensor(ak8), torch.tensor(bk8)


def area_for(H, W, seed=5):
    g = torch.Generator().manual_seed(seed)
    lat = (torch.arange(H, dtype=torch.float64) + 0.5) / H * np.pi - np.pi / 2
    return (torch.cos(lat)[:, None] * (1.0 + 0.1 * torch.rand(H, W, generator=g, dtype=torch.float64))).float()


def fields(lead, K, H, W, seed):
    """(d_in, d_gen) of fp32 CPU tensors (*lead, H, W) with the magnitudes of the fixture (gen_corrector)."""
    g = torch.Generator().manual_seed(seed)
    q_scale = torch.logspace(-6, -2, K)
    d_in, d_gen = {}, {}
    r = lambda: torch.rand(*lead, H, W, generator=g)  # noqa: E731
    n = lambda: torch.randn(*lead, H, W, generator=g)  # noqa: E731
    for k in range(K):
        d_in[f"{WATER}{k}"] = q_scale[k] * (1.0 + r())
        d_gen[f"{WATER}{k}"] = d_in[f"{WATER}{k}"] * (1.0 + 0.05 * n())
    d_in["PRESsfc"] = 1.0e5 + 3.0e3 * n()
    d_gen["PRESsfc"] = d_in["PRESsfc"] + 15.0 + 200.0 * n()
    for d in (d_in, d_gen):
        d["LHTFLsfc"] = 80.0 + 30.0 * n()
        d["PRATEsfc"] = 6.0e-5 * r()
        d[ADV] = 3.0e-6 + 1.0e-5 * n()
        d["TMP2m"] = 280.0 + n()
    return d_in, d_gen


# ---- the host entry point ----------------------------------------------------------------------------------------------
def host_args(sdy, config, ak, bk, area, B, HW):
    from sdy_amd import _lib

    a = _lib.SdyCorrectorArgs()
    a.B, a.HW, a.K = B, HW, len(ak) - 1
    a.flags = (1 if config.get("conserve_dry_air") else 0) | (2 if config.get("zero_global_mean_moisture_advection") else 0)
    a.budget = BUDGET_CODE[config.get("moisture_budget_correction")]
    for k in range(len(ak)):
        a.ak[k], a.bk[k] = float(ak[k]), float(bk[k])
    a.area = area.data_ptr()
    return a


def _set(slot, t, stride, channel=0, mean=0.0, std=1.0):
    slot.base, slot.stride, slot.channel = t.data_ptr(), stride, channel
    if hasattr(slot, "mean"):
        slot.mean, slot.std = mean, std


def host_corrector(sdy, config, ak, bk, area, d_in, d_gen, stats=None, expect=0):
    """`sdy_corrector_host` on CPU tensors (B, H, W) per variable -> {name: corrected fp32 tensor} of every gen variable
    (untouched ones included, for the bit-for-bit check).  stats = {name: (mean, std)}: the same data normalised and packed as
    the stepper holds it, `(B, n, HW)` per side, corrected in place and denormalised again in float64."""
    names = list(d_gen)
    ps = pick(d_gen, "ps")
    B, H, W = d_gen[ps].shape
    HW = H * W
    area = area.contiguous()
    a = host_args(sdy, config, ak, bk, area, B, HW)
    keep = [area]
    wat = water_names(d_gen)
    slots = [(a.gen_q[k], a.in_q[k], None, n) for k, n in enumerate(wat)]
    slots += [(a.gen_ps, a.in_ps, a.out_ps, ps), (a.gen_lhf, None, a.out_lhf, pick(d_gen, "lhf")),
              (a.gen_prate, None, a.out_prate, pick(d_gen, "prate")), (a.gen_adv, None, a.out_adv, ADV)]
    if stats is None:
        res = {n: d_gen[n].clone() for n in names}
        ins = {n: d_in[n].contiguous() for n in names}
        gens = {n: d_gen[n].contiguous() for n in names}
        keep += [ins, gens]
        for g_slot, i_slot, o_slot, n in slots:
            _set(g_slot, gens[n], HW)
            if i_slot is not None:
                _set(i_slot, ins[n], HW)
            if o_slot is not None:
                _set(o_slot, res[n], HW)
        assert sdy.lib.sdy_corrector_host(C.byref(a)) == expect
        return res
    norm = lambda d: torch.stack([((d[n].double() - stats[n][0]) / stats[n][1]).float() for n in names], 1).contiguous()  # noqa: E731
    g_pack, i_pack = norm(d_gen), norm(d_in)
    before = g_pack.clone()
    for g_slot, i_slot, o_slot, n in slots:
        ch = names.index(n)
        _set(g_slot, g_pack, len(names) * HW, ch, *stats[n])
        if i_slot is not None:
            _set(i_slot, i_pack, len(names) * HW, ch, *stats[n])
        if o_slot is not None:
            _set(o_slot, g_pack, len(names) * HW, ch)
    assert sdy.lib.sdy_corrector_host(C.byref(a)) == expect
    res = {}
    for ch, n in enumerate(names):
        if torch.equal(g_pack[:, ch], before[:, ch]):
            res[n] = d_gen[n]
        else:
            res[n] = g_pack[:, ch].double() * stats[n][1] + stats[n][0]
    return res
