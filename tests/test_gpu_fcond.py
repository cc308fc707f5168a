"""DYffusion forward conditioning on the device (reference src/diffusion/dyffusion.py:299-355): the forecaster's input group
a * x_0 + s * eps generated inside the input concat, its noise stream, shard invariance, and the production shape.

Reference pins: tests/golden/fx_sample_fcond_*.npz, written by tools/gen_golden.py from the reference's own
`MultiHorizonForecastingDYffusion`.  They store seeds and checksums instead of weights, inputs and the torch.randn_like draws of
the pass; the rebuilt draws are injected into the product forecaster call by call (`noise_injector`)."""
import json
import math

import numpy as np
import pytest
import torch

import golden_utils as gu
from conftest import rel_l2
from helpers import make_pair
from oracle.philox import philox4x32
from oracle.sfno import SFNOConfig
from test_gpu_golden import TOL_TIGHT, _net

pytestmark = pytest.mark.gpu
N_FORC = 2


def _digest(*ts):
    return np.array([float(t.double().abs().sum()) for t in ts] + [float((t.double() ** 2).sum()) for t in ts])


def _seeded(z):
    """Weights, inputs and noise of a seeded fixture, rebuilt with the generators tools/gen_golden.py used and checked against
    the checksums the generating run stored (a drift of torch's CPU generator cannot pass as a parity failure)."""
    from oracle.sfno import make_state_dict

    fcfg = SFNOConfig(**json.loads(str(z["fcfg"])))
    icfg = SFNOConfig(**json.loads(str(z["icfg"])))
    nets = []
    for cfg, key in ((fcfg, "f"), (icfg, "i")):
        sd = make_state_dict(cfg, seed=int(z[f"seed_{key}"]))
        dig = np.array([float(sum(v.double().abs().sum() for v in sd.values())),
                        float(sum((v.double() ** 2).sum() for v in sd.values()))])
        assert np.allclose(dig, z[f"{key}_digest"], rtol=1e-9), "make_state_dict(seed) no longer reproduces the fixture's weights"
        nets.append(_net(cfg, cfg.in_chans - N_FORC, N_FORC, sd))
    B, cs, H, W = int(z["batch"]), 6 + int(z["hack"]), fcfg.nlat, fcfg.nlon
    g = torch.Generator(device="cpu").manual_seed(int(z["seed_x"]))
    x0 = torch.randn(B, cs, H, W, generator=g)
    if "input_keys" in z.files:           # one sampling pass: x0, then its condition
        keys = json.loads(str(z["input_keys"]))
        shape = {"static_condition": (B, N_FORC, H, W), "dynamical_condition": (B, 7, N_FORC, H, W)}
        inputs = {k: torch.randn(*shape[k], generator=g) for k in keys}
    else:                                 # two windows: x0, then one dynamical condition per window
        inputs = {f"dynamical_condition{w}": torch.randn(B, 7, N_FORC, H, W, generator=g) for w in range(2)}
    assert np.allclose(_digest(x0, *inputs.values()), z["inputs_digest"], rtol=1e-9), \
        "the seeded inputs no longer reproduce the fixture's"
    eps = []
    if "n_eps" in z.files and int(z["n_eps"]) > 0:
        ge = torch.Generator(device="cpu").manual_seed(int(z["seed_eps"]))
        eps = [torch.randn(x0.shape, generator=ge) for _ in range(int(z["n_eps"]))]
        assert np.allclose(_digest(*eps), z["eps_digest"], rtol=1e-9), "the seeded noise no longer reproduces the reference's"
    return fcfg, icfg, nets[0], nets[1], x0, inputs, eps


@pytest.mark.parametrize("name", ["fx_sample_fcond_data", "fx_sample_fcond_data_hack", "fx_sample_fcond_v1",
                                  "fx_sample_fcond_v2", "fx_sample_fcond_v1_k2"])
def test_conditioned_sampler_vs_reference(name):
    import sdy_amd

    z = gu.load(name)
    fcfg, icfg, fnet, inet, x0, inputs, eps = _seeded(z)
    extra = json.loads(str(z["diffusion_extra"]))
    hack = bool(int(z["hack"]))
    if extra["forward_conditioning"].startswith("data+noise"):
        assert eps, "the reference drew noise"
        fnet.noise_injector = lambda call: eps[call]      # one draw per forecaster call, in call order
    else:
        assert not eps
    trace = []
    for tag, net in (("F", fnet), ("I", inet)):
        def hook(fwd, tag=tag):
            def run(inputs, time=None, **kw):
                rpc = kw.get("rows_per_call") or len(time)      # a stacked forward: its calls in row order
                for k in range(len(time) // rpc):
                    trace.append([tag, float(time[k * rpc])])
                return fwd(inputs, time=time, **kw)
            return run
        net.forward = hook(net.forward)
    ipol = sdy_amd.InterpolationExperiment(inet, horizon=6)
    inet.set_min_max_time(icfg.min_time, icfg.max_time)      # (opened to [0, 5] for artificial steps, as in the fixture)
    exp = sdy_amd.MultiHorizonForecastingDYffusion(
        fnet, ipol, horizon=6,
        diffusion_config=dict(hack_for_imprecise_interpolation=hack, **{"enable_interpolator_dropout": False, **extra}))
    out = exp.model.sample(x0.cuda(), **{k: v.cuda() for k, v in inputs.items()})
    assert trace == json.loads(str(z["trace"])), "network call order / times differ from the reference's"
    if eps:
        assert fnet._call == len(eps)
    ref = {k[5:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("out::")}
    assert sorted(out) == sorted(ref)
    for k in ref:
        err = rel_l2(out[k], ref[k])
        assert err < TOL_TIGHT, f"{name}/{k}: rel L2 {err:.3e}"


def test_conditioned_windows_vs_reference():
    """Two autoregressive windows through get_preds_at_t_for_batch with "data": x_0 of window 2 is window 1's forecast (the
    fixture holds window 1's last prediction and all of window 2)."""
    import sdy_amd

    z = gu.load("fx_sample_fcond_windows")
    _, _, fnet, inet, x0, inputs, _ = _seeded(z)
    exp = sdy_amd.MultiHorizonForecastingDYffusion(
        fnet, sdy_amd.InterpolationExperiment(inet, horizon=6), horizon=6,
        diffusion_config=dict(enable_interpolator_dropout=False, **json.loads(str(z["diffusion_extra"]))))
    x = x0.cuda()
    for w in range(2):
        dyn = inputs[f"dynamical_condition{w}"].cuda()
        res = {}
        for h in range(1, 7):
            res.update(exp.get_preds_at_t_for_batch({"dynamics": x, "dynamical_condition": dyn}, horizon=h,
                                                    prepare_inputs=False))
        ref = {k[6:]: torch.from_numpy(z[k]) for k in z.files if k.startswith(f"out{w}::")}
        assert set(ref) <= set(res) and (w == 0 or sorted(res) == sorted(ref))
        for k in ref:
            err = rel_l2(res[k], ref[k])
            assert err < TOL_TIGHT, f"window {w} {k}: rel L2 {err:.3e}"
        x = res["t6_preds_normed"]


# ---- the noise stream --------------------------------------------------------------------------------------------------
def _fill(seed, call, batch_offset, rows_per_call, B, C, HW):
    from sdy_amd._lib import check, current_stream, lib, ptr

    out = torch.empty(B, C, HW, dtype=torch.float32, device="cuda")
    check(lib.sdy_cond_noise_fill(seed, call, batch_offset, rows_per_call, B, C, HW, ptr(out), current_stream()),
          "sdy_cond_noise_fill")
    return out


def _numpy_noise(seed, call, batch_offset, rows_per_call, B, C, HW):
    """include/sdy_amd.h "Forward-conditioning noise stream", in float64 from oracle.philox words."""
    n = rows_per_call or B
    b = np.arange(B, dtype=np.uint64)[:, None, None]
    c = np.arange(C, dtype=np.uint64)[None, :, None]
    q = np.arange(HW // 4, dtype=np.uint64)[None, None, :]
    traj = (b % np.uint64(n)) + np.uint64(batch_offset)
    cl = np.uint64(call) + b // np.uint64(n)
    shape = (B, C, HW // 4)
    w = philox4x32(np.broadcast_to(q, shape).astype(np.uint32), np.broadcast_to(traj * np.uint64(C) + c, shape).astype(np.uint32),
                   np.uint32(0x2000), np.broadcast_to(cl, shape).astype(np.uint32), np.uint32(seed & 0xFFFFFFFF),
                   np.uint32(seed >> 32))
    u = [((np.asarray(x, dtype=np.uint64) >> np.uint64(8)) + np.uint64(1)).astype(np.float64) * 2.0 ** -24 for x in w]
    r0, r1 = np.sqrt(-2 * np.log(u[0])), np.sqrt(-2 * np.log(u[2]))
    e = np.stack([r0 * np.cos(2 * np.pi * u[1]), r0 * np.sin(2 * np.pi * u[1]),
                  r1 * np.cos(2 * np.pi * u[3]), r1 * np.sin(2 * np.pi * u[3])], axis=-1)
    return e.reshape(B, C, HW)


def test_noise_stream_matches_its_definition():
    """sdy_cond_noise_fill against the numpy restatement, with stacked calls and a batch offset.  Tolerance 1e-5 absolute: the
    device evaluates log, sqrt and sincospi in fp32 (a few ulp each) on |eps| <= sqrt(-2 ln 2^-24) = 5.77, where one fp32
    ulp is 4.8e-7; the counters, words and uniforms are exact on both sides."""
    seed = 0x0123456789ABCDEF
    for call, boff, rpc, B, C, HW in ((0, 0, 0, 2, 6, 32 * 64), (7, 5, 2, 4, 3, 180 * 360 // 20), (2 ** 31 + 3, 1000, 1, 3, 2, 64)):
        got = _fill(seed, call, boff, rpc, B, C, HW).cpu().double().numpy()
        want = _numpy_noise(seed, call, boff, rpc, B, C, HW)
        assert np.isfinite(got).all()
        err = np.abs(got - want).max()
        assert err < 1e-5, f"max |device - float64 restatement| {err:.3e}"
    # stacked calls = consecutive calls: row b of a (n rows per call) fill is row b % n of call + b // n
    a = _fill(seed, 3, 8, 2, 6, 4, 256)
    for k in range(3):
        assert torch.equal(a[2 * k:2 * k + 2], _fill(seed, 3 + k, 8, 0, 2, 4, 256))


def test_noise_stream_statistics():
    """>= 10^7 draws: mean, variance and the Kolmogorov-Smirnov distance to N(0, 1) within 5-sigma-class bounds, nothing
    non-finite, and no correlation between neighbouring channels, rows (trajectories) or calls."""
    B, C, HW = 4, 40, 180 * 360
    e = _fill(99, 11, 0, 0, B, C, HW)
    e2 = _fill(99, 12, 0, 0, B, C, HW)
    N = e.numel()
    assert N >= 10 ** 7 and bool(torch.isfinite(e).all())
    x = e.double()
    mean, var = float(x.mean()), float(x.var())
    assert abs(mean) < 5 / math.sqrt(N), mean
    assert abs(var - 1) < 5 * math.sqrt(2 / N), var
    s = torch.sort(x.reshape(-1))[0].cpu()
    cdf = torch.special.ndtr(s)
    i = torch.arange(1, N + 1, dtype=torch.float64)
    ks = float(torch.maximum(i / N - cdf, cdf - (i - 1) / N).max())
    assert ks < 2.5 / math.sqrt(N), f"KS distance {ks:.3e}"     # (P[D > 2.5 / sqrt(N)] ~ 8e-6)

    def corr(a, b):
        a, b = a.reshape(-1).double(), b.reshape(-1).double()
        return float(((a - a.mean()) * (b - b.mean())).mean() / (a.std() * b.std()))
    bound = lambda n: 5 / math.sqrt(n)   # noqa: E731
    assert abs(corr(x[:, :-1], x[:, 1:])) < bound(x[:, 1:].numel())          # neighbouring channels
    assert abs(corr(x[:-1], x[1:])) < bound(x[1:].numel())                   # neighbouring rows
    assert abs(corr(x, e2)) < bound(N)                                       # neighbouring calls
    assert abs(corr(x[..., :-1], x[..., 1:])) < bound(x[..., 1:].numel())    # neighbouring pixels


def _tiny(mode, seed_i=4242):
    import sdy_amd

    C, H, W, E, L = 6, 32, 64, 16, 2
    fcfg = SFNOConfig(in_chans=2 * C + N_FORC, out_chans=C, nlat=H, nlon=W, embed_dim=E, num_layers=L, with_time_emb=True,
                      min_time=0.0, max_time=5.0)
    icfg = SFNOConfig(in_chans=2 * C + N_FORC, out_chans=C, nlat=H, nlon=W, embed_dim=E, num_layers=L, with_time_emb=True,
                      dropout_mlp=0.1, drop_path_rate=0.1, min_time=1.0, max_time=5.0)
    fnet, fora, _ = make_pair(fcfg, C, C + N_FORC, seed=11, net_seed=777)
    inet, _, _ = make_pair(icfg, 2 * C, N_FORC, seed=22, net_seed=seed_i)
    exp = sdy_amd.MultiHorizonForecastingDYffusion(fnet, sdy_amd.InterpolationExperiment(inet, horizon=6), horizon=6,
                                                   diffusion_config=dict(forward_conditioning=mode))
    return exp, fnet, fora


def test_forward_draws_the_stream_it_documents():
    """The Philox draw inside the forward equals the injected eps of sdy_cond_noise_fill (same call, trajectory) bit for bit,
    and "data" is the plain concat of x_0 (a = 1, s = 0: nothing drawn)."""
    exp, fnet, _ = _tiny("data+noise-v1")
    g = torch.Generator(device="cpu").manual_seed(5)
    x, x0 = torch.randn(3, 6, 32, 64, generator=g).cuda(), torch.randn(3, 6, 32, 64, generator=g).cuda()
    dyn = torch.randn(3, N_FORC, 32, 64, generator=g).cuda()
    t = torch.full((3,), 2.0).cuda()
    fnet.batch_offset, fnet._call = 4, 9
    y = fnet(x, time=t, condition=dyn, forward_condition=(x0, 0.25, 0.75))
    eps = _fill(fnet.seed, 9, 4, 0, 3, 6, 32 * 64).reshape(3, 6, 32, 64)
    fnet._call = 9
    fnet.noise_injector = lambda call: eps
    assert torch.equal(y, fnet(x, time=t, condition=dyn, forward_condition=(x0, 0.25, 0.75)))
    fnet.noise_injector = None
    # "data": exactly the network on the explicit concat
    y_data = fnet(x, time=t, condition=dyn, forward_condition=(x0, 1.0, 0.0))
    y_cat = fnet(x, time=t, condition=torch.cat([x0, dyn], dim=1))
    assert torch.equal(y_data, y_cat)
    with pytest.raises(ValueError):
        fnet(x, time=t, condition=dyn, forward_condition=(x0, 1.0, 0.0), reuse_encoder=True)


def test_shard_invariance_of_a_noise_conditioned_rollout():
    """A 4-member "data+noise-v1" sampling pass as one batch == as two unit ranges (batch_offset 0 and 2, the call counters
    restored between them) == the forecaster's rows as stacked calls, bit for bit."""
    g = torch.Generator(device="cpu").manual_seed(8)
    x0 = torch.randn(4, 6, 32, 64, generator=g).cuda()
    dyn = torch.randn(4, 7, N_FORC, 32, 64, generator=g).cuda()
    exp, fnet, _ = _tiny("data+noise-v1")
    whole = exp.model.sample(x0, dynamical_condition=dyn)
    exp2, fnet2, _ = _tiny("data+noise-v1")
    state = exp2.dropout_calls()
    parts = []
    for r0 in (0, 2):
        exp2.set_dropout_calls(state)
        exp2.set_batch_offset(r0)
        parts.append(exp2.model.sample(x0[r0:r0 + 2], dynamical_condition=dyn[r0:r0 + 2]))
    assert sorted(whole) == sorted(parts[0])
    for k in whole:
        assert torch.equal(whole[k], torch.cat([p[k] for p in parts])), k
    assert exp.dropout_calls() == exp2.dropout_calls()
    # the noise matters: "data" gives another result
    exp3, _, _ = _tiny("data")
    assert not torch.equal(exp3.model.sample(x0, dynamical_condition=dyn)["t1_preds"], whole["t1_preds"])
    # stacked calls: 2 calls x 2 rows in one forward == the two forwards one after the other
    x = torch.randn(2, 6, 32, 64, generator=g).cuda()
    t = torch.full((2,), 1.0).cuda()
    c = dyn[:2, 0]
    fnet._call, fnet.batch_offset = 20, 0
    one = [fnet(x, time=t, condition=c, forward_condition=(x0[:2], 0.4, 0.6)) for _ in range(2)]
    fnet._call = 20
    two = fnet(torch.cat([x, x]), time=torch.cat([t, t]), condition=torch.cat([c, c]),
               forward_condition=(torch.cat([x0[:2], x0[:2]]), 0.4, 0.6), rows_per_call=2)
    assert fnet._call == 22
    assert torch.equal(two, torch.cat(one))


def test_production_shape_conditioned_forecaster_vs_oracle():
    """180 x 360, E = 256, 6 blocks, 63 + 63 + 2 = 128 input channels (the forecaster of a "data+noise-v1" checkpoint at the
    production shape): parity with the oracle forward fed the same eps through the injection hook, and the launches of the
    fused paths by the stage timer -- one concat, fused encoder / decoder pairs, the fused MLP, dh_h3, leg_par, fft360."""
    import sdy_amd

    layers, C, H, W = 6, 63, 180, 360
    cfg = SFNOConfig(in_chans=2 * C + N_FORC, out_chans=C, nlat=H, nlon=W, embed_dim=256, num_layers=layers,
                     with_time_emb=True, min_time=0.0, max_time=5.0)
    net, ora, _ = make_pair(cfg, C, C + N_FORC, seed=4321)
    g = torch.Generator(device="cpu").manual_seed(3)
    x, x0 = torch.randn(2, C, H, W, generator=g), torch.randn(2, C, H, W, generator=g)
    dyn = torch.randn(2, N_FORC, H, W, generator=g)
    a = torch.tensor([0.4, 0.8])          # per-row coefficients (data+noise-v1 at t = 2 and t = 4 of horizon 6)
    s = 1 - a
    t = torch.tensor([2.0, 4.0])
    eps = _fill(net.seed, 0, 0, 0, 2, C, H * W).reshape(2, C, H, W)
    net.noise_injector = lambda call: eps
    with sdy_amd.ops.stage_timer() as st:
        y = net(x.cuda(), time=t.cuda(), condition=dyn.cuda(), forward_condition=(x0.cuda(), a, s))
    net.noise_injector = None
    n = {k: v[0] for k, v in st.stages.items()}
    assert n.get("concat") == 1
    assert n.get("encoder (fused pair)") == 1 and n.get("decoder (fused pair)") == 1
    assert n.get("mlp fused") == layers and "mlp fc1" not in n and "mlp fc2" not in n
    assert n.get("dhconv") == layers and n.get("rfft (lon)") == layers and n.get("legendre analysis") == layers
    assert "encoder.0 conv" not in n and "decoder.0 conv" not in n
    gen = a.view(2, 1, 1, 1) * x0 + s.view(2, 1, 1, 1) * eps.cpu()
    ref = ora(x, time=t, condition=torch.cat([gen, dyn], dim=1))
    assert torch.isfinite(y).all()
    err = rel_l2(y, ref)
    assert err < TOL_TIGHT, f"conditioned forecaster at full size vs oracle: rel L2 {err:.3e}"
    # the in-kernel draw of the same call: bit-identical to the injected one
    net._call = 0
    assert torch.equal(y, net(x.cuda(), time=t.cuda(), condition=dyn.cuda(), forward_condition=(x0.cuda(), a, s)))
