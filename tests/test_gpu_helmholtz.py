"""Vorticity, divergence, streamfunction and velocity potential on the device (csrc/helmholtz.hip; sdy_amd.helmholtz): the
kernel against the library's host twin BIT FOR BIT, `helmholtz` end to end against the float64 restatement within the derived
bound of tests/helmholtz_utils.py, solid-body rotation, exact power-of-two scaling, independence of layout, chunking and company,
magnitude, NaN containment, truncation, the deriver, and through run_inference.  Every shape is tiny but one 180 x 360 case of 16
winds, which runs the 360-point FFT kernels."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

import helmholtz_utils as hu
import vector_spectrum_utils as vu
from sdy_amd.helmholtz import OUTPUTS, deriver, helmholtz

pytestmark = pytest.mark.gpu

GUARD = 4096


def _cuda(x):
    return torch.from_numpy(np.array(x)).cuda()          # a copy: the shared references are read-only


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ---- the kernel --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", hu.CASES, ids=lambda c: c.id)
def test_kernel_against_the_host_twin(case):
    import sdy_amd
    from sdy_amd._lib import current_stream

    cd, cm, scale, factor = hu.random_inputs(case)
    cd, cm, scale = hu.aligned_copy(cd), hu.aligned_copy(cm), hu.aligned_copy(scale)
    _, want, _ = hu.guarded_out(case)
    assert hu.host_run(case, cd, cm, scale, factor, want) == 0
    d = [None if x is None else _cuda(x) for x in (cd, cm, scale, factor)]
    n = want.size
    raw = torch.full((n + 2 * GUARD,), float("nan"), dtype=torch.float32, device="cuda")
    out = raw[GUARD:GUARD + n]
    assert all(x is None or x.data_ptr() % 16 == 0 for x in (*d, out))
    a = hu.fill_args(case, *[None if x is None else x.data_ptr() for x in d], out.data_ptr())
    assert sdy_amd.lib.sdy_helmholtz_coefficients(C.byref(a), current_stream()) == 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(raw[:GUARD]).all()) and bool(torch.isnan(raw[-GUARD:]).all())
    got = out.cpu().numpy().reshape(want.shape)
    assert not np.isnan(got).any(), "a padding field or an entry with m > l was read, or a field of out was not written"
    assert hu.bits_equal(got, want)


# ---- end to end against float64 ----------------------------------------------------------------------------------------------
def _check(got, want, bnd, what):
    worst = 0.0
    for name in got:
        g = got[name].cpu().numpy().astype(np.float64)
        assert g.shape == want[name].shape and got[name].dtype == torch.float32 and got[name].is_contiguous(), name
        err = np.abs(g - want[name])
        ratio = float((err / bnd[name].clip(1e-300)).max())
        worst = max(worst, ratio)
        print(f"{what} {name}: largest |error| / bound = {ratio:.4f}, largest |value| {np.abs(want[name]).max():.3e}")
        assert (err <= bnd[name]).all(), (what, name)
    print(f"{what}: largest observed ratio of error to bound {worst:.4f}")


@pytest.mark.parametrize("n,nlat,nlon,grid", [(4, 12, 24, "equiangular"), (4, 12, 24, "legendre-gauss"),
                                              (16, 180, 360, "equiangular")])
def test_helmholtz_against_float64(n, nlat, nlon, grid):
    u, v, want, bnd = hu.reference(n, nlat, nlon, grid)
    got = helmholtz(_cuda(u), _cuda(v), grid=grid)
    assert tuple(got) == OUTPUTS
    _check(got, want, bnd, f"{nlat} x {nlon} {grid}")


@pytest.mark.parametrize("grid", vu.GRIDS)
def test_solid_body_rotation_on_the_device(grid):
    """Degrees up to nlat - 2, as in tests/test_helmholtz_host.py::test_solid_body_rotation (the alias at l = nlat - 1 of the
    equiangular grid).  Against the float64 restatement within the derived bound, and against the closed form with that bound
    on top of the restatement's own 1e-12."""
    nlat, nlon, U, a = 12, 24, 30.0, hu.RADIUS
    u64, v64, lat = hu.solid_body(nlat, nlon, grid, U)
    u, v = u64.astype(np.float32), v64.astype(np.float32)
    got = helmholtz(_cuda(u), _cuda(v), grid=grid, truncate=nlat - 2)
    want, bnd = hu.helmholtz64(u, v, grid, truncate=nlat - 2), hu.bound(u, v, grid, truncate=nlat - 2)
    _check(got, want, bnd, f"solid body {grid}")
    closed = {"vorticity": 2.0 * U * np.sin(lat) / a, "streamfunction": -a * U * np.sin(lat)}
    scale = {"vorticity": 2.0 * U / a, "divergence": 2.0 * U / a, "streamfunction": a * U, "velocity_potential": a * U}
    for name in OUTPUTS:
        g = got[name].cpu().numpy().astype(np.float64)
        ref = closed[name][:, None] if name in closed else 0.0
        # the input's own rounding to fp32 moves the closed form by at most 2^-24 of the scale
        assert (np.abs(g - ref) <= bnd[name] + (1e-12 + 2.0 ** -23) * scale[name]).all(), name
    zeta = got["vorticity"].cpu().numpy()
    assert (zeta[lat > 0.1] > 0).all() and (zeta[lat < -0.1] < 0).all()          # positive in the northern hemisphere
    psi = got["streamfunction"].cpu().numpy()
    assert (psi[lat > 0.1] < 0).all() and (psi[lat < -0.1] > 0).all()


def test_truncation_against_float64():
    u, v, want, bnd = hu.reference(4, 12, 24, "equiangular", truncate=5)
    full = hu.reference(4, 12, 24, "equiangular")[2]
    assert np.abs(full["vorticity"] - want["vorticity"]).max() > 100.0 * bnd["vorticity"].max()      # the cases differ
    _check(helmholtz(_cuda(u), _cuda(v), truncate=5), want, bnd, "truncate 5")


# ---- exactness ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [-20, 20])
def test_a_power_of_two_in_the_units_scales_exactly(k):
    u, v, _, _ = hu.reference(4, 12, 24, "equiangular")
    u, v = _cuda(u), _cuda(v)
    one, two = helmholtz(u, v), helmholtz(u * 2.0 ** k, v * 2.0 ** k)
    for name in OUTPUTS:
        assert bool((one[name] != 0).any()) and _same_bits(one[name] * 2.0 ** k, two[name]), name


def test_layout_chunks_and_company_do_not_change_a_bit():
    from sdy_amd.sht import ShtPlan
    from sdy_amd.spectrum import _SLACK

    nlat, nlon = 12, 24
    u, v = hu.winds(2 * 3 * 4, nlat, nlon, "equiangular", "layout")
    base_u, base_v = _cuda(u).view(2, 3, 4, nlat, nlon), _cuda(v).view(2, 3, 4, nlat, nlon)
    # the member-stacked view of the window driver: (members, samples, time) out of (samples, members, time + 1)
    view_u, view_v = base_u.transpose(0, 1)[:, :, 1:], base_v.transpose(0, 1)[:, :, 1:]
    assert not view_u.is_contiguous()
    cont = helmholtz(view_u.contiguous(), view_v.contiguous())
    strided = helmholtz(view_u, view_v)
    for name in OUTPUTS:
        assert strided[name].shape == (3, 2, 3, nlat, nlon) and strided[name].is_contiguous()
        assert _same_bits(strided[name], cont[name]), name
    # chunks of four winds: 18 winds in five chunks
    plan = ShtPlan.get(nlat, nlon, nlat, nlon // 2 + 1, "equiangular", torch.cuda.current_device(), "f32")
    per_x, per_cs = nlat * nlon + plan.mtr * nlat * 2, plan.lmax * plan.mtr * 2
    per_wind = 2 * (per_x + 2 * per_cs + 1) + 4 * (per_cs + plan.mtr * nlat * 2 + nlat * nlon)
    chunked = helmholtz(view_u, view_v, max_workspace_bytes=16 * per_wind + _SLACK)
    for name in OUTPUTS:
        assert _same_bits(chunked[name], cont[name]), name
    with pytest.raises(ValueError, match="max_workspace_bytes"):
        helmholtz(view_u, view_v, max_workspace_bytes=16 * per_wind + _SLACK - 1)
    # a wind alone, and with fewer outputs
    alone = helmholtz(view_u[1, 1, 2], view_v[1, 1, 2], outputs=("velocity_potential", "vorticity"))
    assert tuple(alone) == ("velocity_potential", "vorticity") and alone["vorticity"].shape == (nlat, nlon)
    for name in alone:
        assert _same_bits(alone[name], cont[name][1, 1, 2]), name


def test_magnitude_of_a_real_wind_needs_no_fp16_range():
    import sdy_amd

    nlat, nlon = 12, 24
    u64, v64, _ = hu.solid_body(nlat, nlon, "equiangular", U=100.0)
    wu, wv = hu.winds(4, nlat, nlon, "equiangular", "magnitude")
    u = _cuda((u64[None] + 10.0 * wu).astype(np.float32))
    v = _cuda((10.0 * wv).astype(np.float32))
    sdy_amd.ops.status_flags(reset=True)
    got = helmholtz(u, v)
    flags = sdy_amd.ops.status_flags(reset=True)
    assert flags & 2 == 0, f"SDY_FLAG_F16_RANGE was raised (flags {flags})"
    psi = got["streamfunction"]
    print(f"largest |psi| {float(psi.abs().max()):.3e} m^2/s")
    assert all(bool(torch.isfinite(x).all()) for x in got.values())
    assert 1e8 <= float(psi.abs().max()) <= 1e10


def test_a_nan_stays_in_its_wind():
    u, v, _, _ = hu.reference(4, 12, 24, "equiangular")
    u, v = _cuda(u), _cuda(v)
    clean = helmholtz(u, v)
    u2 = u.clone()
    u2[1, 5, 7] = float("nan")
    dirty = helmholtz(u2, v)
    for name in OUTPUTS:
        for i in (0, 2, 3):
            assert _same_bits(dirty[name][i], clean[name][i]), (name, i)
        assert not bool(torch.isfinite(dirty[name][1]).any()), name


# ---- the deriver -------------------------------------------------------------------------------------------------------------
NAMES = ["eastward_wind_0", "TMP2m", "northward_wind_0", "UGRD10m", "VGRD10m", "eastward_wind_1", "northward_wind_1",
         "eastward_wind_7"]


def _dict(shape, key):
    g = torch.Generator(device="cpu").manual_seed(key)
    return {n: torch.randn(*shape, 12, 24, generator=g).cuda() for n in NAMES}


@pytest.mark.parametrize("shape", [(2, 3), (3, 2, 3)])
def test_deriver_names_order_and_values(shape):
    data = _dict(shape, len(shape))
    out = deriver(NAMES)(data)
    assert list(out) == NAMES + ["vorticity_0", "divergence_0", "vorticity_10m", "divergence_10m", "vorticity_1", "divergence_1"]
    assert all(out[n] is data[n] for n in NAMES) and list(data) == NAMES
    for k, (un, vn) in (("0", NAMES[0:3:2]), ("10m", NAMES[3:5]), ("1", NAMES[5:7])):
        direct = helmholtz(data[un], data[vn], outputs=("vorticity", "divergence"))
        for name in direct:
            assert out[f"{name}_{k}"].shape == shape + (12, 24) and _same_bits(out[f"{name}_{k}"], direct[name]), (name, k)
    four = deriver(NAMES, outputs=OUTPUTS, levels=[1, "10m"], truncate=6)(data)
    assert list(four) == NAMES + [f"{o}_{k}" for k in ("10m", "1") for o in OUTPUTS]
    direct = helmholtz(data["eastward_wind_1"], data["northward_wind_1"], truncate=6)
    assert all(_same_bits(four[f"{o}_1"], direct[o]) for o in OUTPUTS)
    with pytest.raises(ValueError, match="divergence_10m already exists"):
        deriver(NAMES)({**data, "divergence_10m": data["TMP2m"]})
    part = {n: t for n, t in data.items() if n != "VGRD10m"}                      # a pair with a missing component is skipped
    assert list(deriver(NAMES)(part)) == list(part) + ["vorticity_0", "divergence_0", "vorticity_1", "divergence_1"]


def test_chain_with_the_water_budget_deriver():
    import sdy_amd

    data = _dict((2, 3), 7)
    g = torch.Generator(device="cpu").manual_seed(8)
    for n in ("specific_total_water_0", "specific_total_water_1"):
        data[n] = (1e-3 * torch.rand(2, 3, 12, 24, generator=g)).cuda()
    data["PRESsfc"] = (1e5 + 1e3 * torch.randn(2, 3, 12, 24, generator=g)).cuda()
    sigma = types.SimpleNamespace(ak=torch.tensor([0.0, 5000.0, 0.0]), bk=torch.tensor([0.0, 0.5, 1.0]))
    water, wind = sdy_amd.derived.deriver(sigma), deriver(list(data))
    both = sdy_amd.derived.chain(water, wind)(data)
    w, h = water(data), wind(data)
    new_w, new_h = [n for n in w if n not in data], [n for n in h if n not in data]
    assert len(new_w) >= 2 and len(new_h) == 6
    assert list(both) == list(data) + new_w + new_h
    assert all(torch.equal(both[n], w[n]) for n in new_w) and all(_same_bits(both[n], h[n]) for n in new_h)


def test_through_run_inference():
    """run_inference(derive=deriver(...)) on the tiny synthetic sampler with wind names: the derived names reach the aggregator
    and the writer, they equal `helmholtz` applied to the window's winds, and what a run without `derive` hands over is
    unchanged bit for bit."""
    import sdy_amd
    from sdy_amd import synthetic

    dev = torch.device("cuda", 0)
    n_forc, nlat, nlon, window, n_windows, members = 2, 32, 64, 6, 2, 2
    out_names = ["eastward_wind_0", "northward_wind_0", "UGRD10m", "VGRD10m"]
    forcing = [f"f{i}" for i in range(n_forc)]
    names = ["HGTsfc"] + out_names + forcing
    steps = window * n_windows
    derived = [f"{o}_{k}" for k in ("0", "10m") for o in ("vorticity", "velocity_potential")]

    class Record:
        def __init__(self):
            self.batches, self.written = [], []

        def record_batch(self, loss, target_data, gen_data, target_data_norm=None, gen_data_norm=None, i_time_start=0):
            self.batches.append(({k: v.clone() for k, v in target_data.items()}, {k: v.clone() for k, v in gen_data.items()}))

        def append_batch(self, target, prediction, start_timestep, start_sample, batch_times=None):
            self.written.append(({k: v.clone() for k, v in target.items()}, {k: v.clone() for k, v in prediction.items()}))

        def flush(self):
            pass

    runs = {}
    for on in (False, True):
        # a fresh sampler per run: the interpolator's dropout stream counts its calls
        exp, _, _ = synthetic.build_sampler(dev, state_chans=4, forcing_chans=n_forc, nlat=nlat, nlon=nlon, embed=16, layers=2,
                                            horizon=6, carried_input_only_channel=True)
        stepper = sdy_amd.MultiStepStepper(exp, names, out_names, forcing, {n: 0.0 for n in names}, {n: 1.0 for n in names}, None)
        rec = Record()
        sdy_amd.run_inference(rec, stepper, synthetic.windows(names, n_windows, window, nlat, nlon, n_ics=2, seed=5), steps,
                              window, n_ensemble_members=members, eval_device=dev, writer=rec,
                              derive=deriver(out_names, outputs=("vorticity", "velocity_potential")) if on else None)
        runs[on] = rec
    plain, full = runs[False], runs[True]
    assert len(full.batches) == len(plain.batches) == n_windows and len(full.written) == len(plain.written) >= n_windows
    for kind in ("batches", "written"):
        for (t0, g0), (t1, g1) in zip(getattr(plain, kind), getattr(full, kind)):
            for d0, d1 in ((t0, t1), (g0, g1)):
                assert list(d1) == list(d0) + derived, kind
                assert all(_same_bits(d0[n].cpu(), d1[n].cpu()) for n in d0), kind          # nothing existing changed
                for k, (un, vn) in (("0", out_names[:2]), ("10m", out_names[2:])):
                    direct = helmholtz(d1[un].to(dev), d1[vn].to(dev), outputs=("vorticity", "velocity_potential"))
                    for o, x in direct.items():
                        assert _same_bits(d1[f"{o}_{k}"].to(dev), x), (kind, o, k)
