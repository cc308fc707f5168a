"""Every switch of `DYffusion.sample_loop` outside the shipped configuration, held to the reference and to the oracle.

Against the REFERENCE (tests/golden/fx_sample_sw_*.npz, written by tools/gen_golden.py::gen_sample_switches from the reference's
own DYffusion.sample on the networks and inputs of fx_sample_tiny / fx_sample_tiny_hack): output keys, every lead time within
the bounds the other sampler fixtures are held to (tests/test_gpu_golden.py TOL, TOL_TIGHT), and the network call trace.
Across the sampler's four interpolation paths (stacked 2B pair with shared inputs, stacked copies, two forwards with encoder
reuse, plain calls): bit-identical results, dropout off and on.  Against the ORACLE (oracle/dyffusion.py): the switches the
reference cannot run or that no fixture isolates, at the tolerance of tests/test_gpu_dyffusion.py::test_sample_matches_oracle.

Two known divergences from the reference are pinned as refusals: `time_encoding="continuous"` (the reference accepts it; not
implemented here) and the carried input-only channel with a cold autoregressive init (the reference fails there too, later)."""
import contextlib
import json

import pytest
import torch

import golden_utils as gu
import test_gpu_golden as tg
from conftest import rel_l2
from helpers import make_pair
from oracle.dyffusion import OracleDYffusion
from oracle.sfno import SFNOConfig
from test_gpu_dyffusion import TOL as TOL_ORACLE          # test_sample_matches_oracle's bound

pytestmark = pytest.mark.gpu

HORIZON, C_OUT, N_FORC = 6, 6, 2
LAST_AR = dict(use_cold_sampling_for_last_step=False, use_cold_sampling_for_init_of_ar_step=True)

# name: (carried input-only channel, diffusion options, interpolator's minimal time) -- the seven fixtures' configurations
# (tools/gen_golden.py SWITCH_CASES; test_fixture_configurations_are_the_ones_listed_here ties the two), then the oracle-only ones
CONFIGS = {
    "mid": (True, dict(use_cold_sampling_for_intermediate_steps=False), 1.0),
    "discrete_k2": (True, dict(time_encoding="discrete", additional_interpolation_steps=2), 0.0),
    "cond0": (False, dict(dynamic_cond_from_t="0"), 1.0),
    "plus3": (True, dict(additional_interpolation_steps=2, sampling_schedule="only_dynamics_plus3"), 0.0),
    "short": (True, dict(sampling_schedule=[0, 1, 2, 3]), 1.0),
    "refine_pt": (True, dict(refine_intermediate_predictions=True, prediction_timesteps=[1, 2.5, 4]), 1.0),
    "last_ar": (False, dict(LAST_AR), 1.0),
    "cond_t": (False, dict(dynamic_cond_from_t="t"), 1.0),
    "discrete_k0": (True, dict(time_encoding="discrete"), 1.0),
}
ORACLE_ONLY = ["cond_t", "cond0", "discrete_k0", "last_ar"]

# the sampler's interpolation paths (dyffusion.py sample_loop: q_sample_pair, q_sample_two, q_sample)
PATHS = {
    "stacked pair, shared inputs": dict(fuse=8, share=True, reuse=True),
    "stacked pair, stacked copies": dict(fuse=8, share=False, reuse=True),
    "two forwards, encoder reused": dict(fuse=0, share=True, reuse=True),
    "plain calls": dict(fuse=0, share=True, reuse=False),
}


def _set_path(sampler, fuse, share, reuse):
    sampler.fuse_interpolator_pair_max_batch = fuse
    sampler.share_pair_inputs = share
    sampler.reuse_interpolator_encoder = reuse


def _experiment(fnet, inet, hack, extra, ipol_min_time, dropout=False):
    import sdy_amd

    ipol = sdy_amd.InterpolationExperiment(inet, horizon=HORIZON)
    # (the experiment pins the interpolator's valid times to the data steps [1, 5] like the reference's; the generator opened
    #  the range for the fixtures with artificial steps -- tools/gen_golden.py, build_experiments)
    inet.set_min_max_time(ipol_min_time, HORIZON - 1.0)
    return sdy_amd.MultiHorizonForecastingDYffusion(
        fnet, ipol, horizon=HORIZON,
        diffusion_config=dict(hack_for_imprecise_interpolation=hack, enable_interpolator_dropout=dropout, **extra))


def _pairs(hack, extra, ipol_min_time, nlat, nlon, dropout):
    """(product forecaster, product interpolator, oracle forecaster, oracle interpolator) with the fixtures' seeds."""
    cs = C_OUT + int(hack)
    discrete_extra = extra.get("additional_interpolation_steps", 0) if extra.get("time_encoding") == "discrete" else 0
    fcfg = SFNOConfig(in_chans=cs + N_FORC, out_chans=C_OUT, nlat=nlat, nlon=nlon, embed_dim=16, num_layers=2,
                      with_time_emb=True, min_time=0.0, max_time=HORIZON - 1.0 + discrete_extra)
    icfg = SFNOConfig(in_chans=2 * cs + N_FORC, out_chans=C_OUT, nlat=nlat, nlon=nlon, embed_dim=16, num_layers=2,
                      with_time_emb=True, dropout_mlp=0.1 if dropout else 0.0, drop_path_rate=0.1 if dropout else 0.0,
                      min_time=ipol_min_time, max_time=HORIZON - 1.0)
    fnet, fora, _ = make_pair(fcfg, cs, N_FORC, seed=11)
    inet, iora, _ = make_pair(icfg, 2 * cs, N_FORC, seed=22, net_seed=4242)
    return fnet, inet, fora, iora


def _inputs(hack, B, nlat, nlon, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    x0 = torch.randn(B, C_OUT + int(hack), nlat, nlon, generator=g)
    if hack:
        return x0, {"static_condition": torch.randn(B, N_FORC, nlat, nlon, generator=g)}
    return x0, {"dynamical_condition": torch.randn(B, HORIZON + 1, N_FORC, nlat, nlon, generator=g)}


def _oracle(fora, iora, hack, extra):
    return OracleDYffusion(
        lambda x, time, condition=None, static_condition=None: fora(x, time=time, condition=condition,
                                                                    static_condition=static_condition),
        lambda x, time, condition=None, static_condition=None: iora(x, time=time, condition=condition,
                                                                    static_condition=static_condition),
        timesteps=HORIZON, hack_for_imprecise_interpolation=hack, enable_interpolator_dropout=False, **extra)


@contextlib.contextmanager
def _forwards(**nets):
    """Records every forward of the given networks while active: (tag, time of row 0, rows, shared_inputs, reuse_encoder)."""
    seen, originals = [], {}
    for tag, net in nets.items():
        originals[tag] = net.forward

        def run(inputs, time=None, _tag=tag, _fwd=net.forward, **kw):
            seen.append((_tag, float(time[0]), int(time.shape[0]), bool(kw.get("shared_inputs")), bool(kw.get("reuse_encoder"))))
            return _fwd(inputs, time=time, **kw)
        net.forward = run
    try:
        yield seen
    finally:
        for tag, net in nets.items():
            net.forward = originals[tag]


def _sample_loop(exp, x0, kw):
    """-> predictions plus sample_loop's first return value (which `sample` drops) under "final_state"."""
    with torch.inference_mode():
        final, preds = exp.model.sample_loop(x0, **kw)
    assert "final_state" not in preds
    return dict(preds, final_state=final)


def test_fixture_configurations_are_the_ones_listed_here():
    for name in gu.SWITCH_FIXTURES:
        case = gu.switch_case(name)
        hack, extra, tmin = CONFIGS[name[len("fx_sample_sw_"):]]
        assert (case["hack"], case["extra"], case["ipol_min_time"]) == (hack, extra, tmin), name


@pytest.mark.parametrize("name", gu.SWITCH_FIXTURES)
def test_sampler_switches_vs_reference(name):
    """One switch per fixture, against the reference's own DYffusion.sample (src/diffusion/dyffusion.py):
      mid          use_cold_sampling_for_intermediate_steps=False: intermediate lead times are the interpolations (:527-531)
      discrete_k2  time_encoding="discrete" with two artificial steps: the forecaster sees the diffusion steps 0..7 (:287-288)
      cond0        dynamic_cond_from_t="0": the forecaster's condition is the first time of the window (:338-339)
      plus3        schedule "only_dynamics_plus3": fractional diffusion steps 0.75, 1.5, 2.25 (:391-397)
      short        schedule [0, 1, 2, 3]: four lead times, and sample_loop returns the state, not the forecast (:565-567)
      refine_pt    refining sweep over prediction_timesteps=[1, 2.5, 4]: a "t2.5_preds" key (:550-564)
      last_ar      last step not cold, cold state kept as "preds_autoregressive_init" (:505-512; the reference runs this
                   configuration without the carried channel, so the fixture is the reference's, not the oracle's alone)
    Values with the default path (B = 2: the stacked pair) and again with plain calls, whose (network, time) trace must be the
    reference's recorded one."""
    case = gu.switch_case(name)
    zb, hack, extra = case["base"], case["hack"], case["extra"]
    fcfg = SFNOConfig(**json.loads(str(zb["fcfg"])))
    icfg = SFNOConfig(**json.loads(str(zb["icfg"])))
    fnet = tg._net(fcfg, fcfg.in_chans - N_FORC, N_FORC, gu.state_dict(zb, "f::"))
    inet = tg._net(icfg, icfg.in_chans - N_FORC, N_FORC, gu.state_dict(zb, "i::"))
    exp = _experiment(fnet, inet, hack, extra, case["ipol_min_time"])
    x0, kw = case["x0"].cuda(), {k: v.cuda() for k, v in case["kw"].items()}
    ref = case["ref"]
    if name == "fx_sample_sw_last_ar":
        assert "preds_autoregressive_init" in ref
    if name == "fx_sample_sw_refine_pt":
        assert "t2.5_preds" in ref
    if name == "fx_sample_sw_short":
        assert sorted(ref) == [f"t{i}_preds" for i in range(1, 5)] and case["final_state"] is not None
    for path in ("stacked pair, shared inputs", "plain calls"):
        _set_path(exp.model, **PATHS[path])
        exp.set_dropout_calls((0, 0))
        with _forwards(F=fnet, I=inet) as seen:
            out = _sample_loop(exp, x0, kw)
        final = out.pop("final_state")
        assert sorted(out) == sorted(ref), f"{name} ({path}): keys {sorted(out)} != {sorted(ref)}"
        errs = {k: rel_l2(out[k], ref[k]) for k in ref}
        print(f"[switches] {name} ({path}): worst lead time {max(errs.values()):.3e}")
        for k, err in errs.items():
            assert out[k].shape == ref[k].shape
            assert err < tg.TOL, f"{name}/{k} ({path}): rel L2 {err:.3e}"
            assert err < tg.TOL_TIGHT, f"{name}/{k} ({path}): rel L2 {err:.3e}"
        assert fnet._call + inet._call == len(case["trace"])
        if path == "plain calls":
            assert [[tag, t] for tag, t, *_ in seen] == case["trace"], "network call order / times differ from the reference's"
        if case["final_state"] is not None:
            assert final.shape == case["final_state"].shape
            err = rel_l2(final, case["final_state"])
            assert err < tg.TOL_TIGHT, f"{name} ({path}): returned state rel L2 {err:.3e}"


@pytest.mark.parametrize("config", ORACLE_ONLY)
def test_sampler_switches_vs_oracle(config):
    """Against oracle/dyffusion.py, at test_sample_matches_oracle's tolerance:
      cond_t       dynamic_cond_from_t="t": the forecaster's condition is dyn[:, int(t)], the window's time at the forecaster's
                   input step.  The REFERENCE RAISES here (IndexError: slice_time indexes with the float time tensor,
                   src/diffusion/dyffusion.py:343,357-361), so this behaviour is pinned to the oracle alone.
      cond0        "0" with a dynamical condition (also a reference fixture above)
      discrete_k0  time_encoding="discrete" without artificial steps (the times equal the "dynamics" ones)
      last_ar      last step not cold + cold AR init (also a reference fixture above)
    sample_loop's returned state is compared too."""
    hack, extra, tmin = CONFIGS[config]
    fnet, inet, fora, iora = _pairs(hack, extra, tmin, 32, 64, dropout=False)
    exp = _experiment(fnet, inet, hack, extra, tmin)
    x0, kw = _inputs(hack, 2, 32, 64, seed=1234)
    want_final, want = _oracle(fora, iora, hack, extra).sample_loop(x0, **kw)
    got = _sample_loop(exp, x0.cuda(), {k: v.cuda() for k, v in kw.items()})
    final = got.pop("final_state")
    assert sorted(got) == sorted(want)
    if config == "last_ar":
        assert "preds_autoregressive_init" in got
    for k in want:
        err = rel_l2(got[k], want[k])
        assert got[k].shape == want[k].shape and err < TOL_ORACLE, f"{config}/{k}: rel L2 {err:.3e}"
    assert final.shape == want_final.shape and rel_l2(final, want_final) < TOL_ORACLE
    if config == "cond_t":          # the condition's time matters: "h" gives other fields
        other = _experiment(fnet, inet, hack, {}, tmin).model.sample(x0.cuda(), **{k: v.cuda() for k, v in kw.items()})
        assert rel_l2(other["t3_preds"], want["t3_preds"]) > 1e-3


@pytest.mark.parametrize("dropout", [False, "always"], ids=["dropout-off", "dropout-always"])
@pytest.mark.parametrize("config", list(CONFIGS))
def test_interpolation_paths_agree(config, dropout):
    """The four interpolation paths give the same samples bit for bit (the promise of
    tests/test_gpu_dyffusion.py::test_fused_interpolator_pair_equals_two_calls and
    ::test_interpolator_pair_with_shared_encoder_equals_two_full_forwards, here for every switch): predictions, keys and the
    state sample_loop returns; B = 2 at 32 x 64 and B = 3 at 20 x 40 (`out[B:]` of a stacked pair then starts at an odd row, and
    800 pixels are no multiple of the 64-pixel tiles).  With dropout "always" the interpolator has dropout 0.1 / drop path 0.1
    and draws from the product's own stream: every path starts at the same call counter with the same batch_offset and must end
    at the same counter.  Each path is also checked to have taken its branch: 2B-row forwards, shared inputs, encoder reuse
    (the last two only without a time-dependent condition).  At 20 x 40, dropout off, the result is held to the oracle too."""
    hack, extra, tmin = CONFIGS[config]
    for B, nlat, nlon in ((2, 32, 64), (3, 20, 40)):
        fnet, inet, fora, iora = _pairs(hack, extra, tmin, nlat, nlon, dropout=bool(dropout))
        exp = _experiment(fnet, inet, hack, extra, tmin, dropout=dropout)
        x0, kw = _inputs(hack, B, nlat, nlon, seed=77)
        x0c, kwc = x0.cuda(), {k: v.cuda() for k, v in kw.items()}
        exp.set_batch_offset(5)
        outs, calls = {}, {}
        for path, setting in PATHS.items():
            _set_path(exp.model, **setting)
            exp.set_dropout_calls((0, 0))
            with _forwards(I=inet) as seen:
                outs[path] = _sample_loop(exp, x0c, kwc)
            calls[path] = exp.dropout_calls()
            rows = {r for _, _, r, _, _ in seen}
            stacked, shared, reused = 2 * B in rows, any(s for *_, s, _ in seen), any(r for *_, r in seen)
            where = f"{config}, B = {B}, {path}"
            assert stacked == (setting["fuse"] > 0), where
            assert shared == (setting["fuse"] > 0 and setting["share"] and hack), where
            assert reused == (setting["fuse"] == 0 and setting["reuse"] and hack), where
        base = outs["plain calls"]
        for path, out in outs.items():
            assert sorted(out) == sorted(base), f"{config}, B = {B}: keys of '{path}'"
            assert calls[path] == calls["plain calls"], f"{config}, B = {B}: call counters after '{path}'"
            for k in base:
                assert torch.equal(out[k], base[k]), \
                    f"{config}, B = {B}, {k}: '{path}' differs from plain calls by {float((out[k] - base[k]).abs().max()):.3e}"
        if dropout:      # the stream is on: the same pass from another call counter is another sample
            exp.set_dropout_calls((0, 100))
            again = _sample_loop(exp, x0c, kwc)
            assert not torch.equal(again["t3_preds"], base["t3_preds"])
        elif (nlat, nlon) != (32, 64):
            want_final, want = _oracle(fora, iora, hack, extra).sample_loop(x0, **kw)
            got = dict(base)
            assert rel_l2(got.pop("final_state"), want_final) < TOL_ORACLE
            assert sorted(got) == sorted(want)
            for k in want:
                err = rel_l2(got[k], want[k])
                assert err < TOL_ORACLE, f"{config}, {nlat} x {nlon}, {k}: rel L2 {err:.3e} against the oracle"


def test_refused_configurations_launch_nothing():
    """`time_encoding="continuous"`: the reference accepts it (t / num_timesteps, src/diffusion/dyffusion.py:289-290), this
    sampler refuses it at construction -- a known divergence, out of scope.  Carried channel + last step not cold + cold AR
    init: the reference fails on 7 + 6 channels at its last step (:508); here sample_loop raises before the first network call
    (the pointwise update once read past the forecast's end in this configuration)."""
    hack, tmin = True, 1.0
    fnet, inet, _, _ = _pairs(hack, {}, tmin, 32, 64, dropout=False)
    with pytest.raises(ValueError, match="time_encoding"):
        _experiment(fnet, inet, hack, dict(time_encoding="continuous"), tmin)
    exp = _experiment(fnet, inet, hack, dict(LAST_AR), tmin)
    x0, kw = _inputs(hack, 2, 32, 64, seed=3)
    with pytest.raises(RuntimeError, match="use_cold_sampling_for_init_of_ar_step"):
        exp.model.sample(x0.cuda(), **{k: v.cuda() for k, v in kw.items()})
    assert exp.dropout_calls() == (0, 0)
