"""DYffusion forward conditioning ("data", "data+noise-v1", "data+noise-v2"; reference src/diffusion/dyffusion.py:299-355):
host-side logic that needs no GPU -- constructor, per-row coefficients, channel accounting, and the noise stream's place in
the Philox counter space."""
import json
import os
import re
from contextlib import nullcontext

import numpy as np
import pytest
import torch

import golden_utils as gu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sdy():
    import sdy_amd

    return sdy_amd


class _FakeIpol:
    window = 1

    def __init__(self, horizon=6):
        self.true_horizon = horizon


def _sampler(sdy, **kw):
    return sdy.DYffusion(model=None, interpolator=_FakeIpol(), timesteps=6, **kw)


@pytest.mark.parametrize("mode", ["data", "none", "data+noise-v1", "data+noise-v2"])
def test_constructor_accepts_the_reference_values(sdy, mode):
    s = _sampler(sdy, forward_conditioning=mode)
    assert s.hparams.forward_conditioning == mode
    assert _sampler(sdy).hparams.forward_conditioning == "none"       # the project's default stays


@pytest.mark.parametrize("mode", ["data|noise", "data+noise", "Data", ""])
def test_constructor_rejects_other_values(sdy, mode):
    with pytest.raises(ValueError, match="forward_conditioning"):
        _sampler(sdy, forward_conditioning=mode)


def _reference_coefs(mode, t, num_timesteps):
    """The reference's tensor arithmetic (dyffusion.py:316-330): fp32 t / (num_timesteps - 1), then (f, 1 - f)."""
    tt = torch.full((1,), t, dtype=torch.float32)
    f = tt / (num_timesteps - 1)
    if mode == "data+noise-v1":
        return float(f[0]), float((1 - f)[0])
    return float((1 - f)[0]), float(f[0])


@pytest.mark.parametrize("k", [0, 2])
def test_coefficients_follow_the_reference_formula(sdy, k):
    ipol = _FakeIpol(horizon=6)
    for mode in ("data+noise-v1", "data+noise-v2"):
        s = sdy.DYffusion(model=None, interpolator=ipol, timesteps=6, forward_conditioning=mode,
                          additional_interpolation_steps=k)
        assert s.num_timesteps == 6 + k
        for t in range(s.num_timesteps):
            assert s.forward_condition_coefs(t) == _reference_coefs(mode, t, 6 + k), (mode, k, t)
    assert sdy.DYffusion(model=None, interpolator=ipol, timesteps=6, forward_conditioning="data",
                         additional_interpolation_steps=k).forward_condition_coefs(3) == (1.0, 0.0)
    assert sdy.DYffusion(model=None, interpolator=ipol, timesteps=6,
                         additional_interpolation_steps=k).forward_condition_coefs(3) is None


def test_predict_x_last_hands_the_condition_to_the_network(sdy):
    seen = []

    class Net:
        min_time = max_time = None

        def predict_forward(self, x, time=None, condition=None, **kw):
            seen.append((condition, kw.get("forward_condition")))
            return x

    x0, xt = torch.zeros(2, 3, 4, 8), torch.ones(2, 3, 4, 8)
    for mode, want in (("none", None), ("data", (1.0, 0.0)), ("data+noise-v1", (0.4, 0.6)), ("data+noise-v2", (0.6, 0.4))):
        s = sdy.DYffusion(model=Net(), interpolator=_FakeIpol(), timesteps=6, forward_conditioning=mode)
        s.predict_x_last(x0, xt, t=2)
        cond, fc = seen[-1]
        assert cond is None
        if want is None:
            assert fc is None
        else:
            assert fc[0] is x0 and fc[1:] == pytest.approx(want, abs=1e-7)


FIXTURES = ["fx_sample_fcond_data", "fx_sample_fcond_data_hack", "fx_sample_fcond_v1", "fx_sample_fcond_v2",
            "fx_sample_fcond_v1_k2", "fx_sample_fcond_windows", "fx_sample_tiny", "fx_sample_tiny_hack"]


@pytest.mark.parametrize("name", FIXTURES)
def test_channel_accounting_matches_the_reference_networks(sdy, monkeypatch, name):
    """module_from_state builds the forecaster with exactly the input width the reference's
    `_base_experiment.num_conditional_channels` gave the network in the fixture (tools/gen_golden.py asserts it there)."""
    from sdy_amd import checkpoint

    z = gu.load(name)
    fcfg = json.loads(str(z["fcfg"]))
    extra = json.loads(str(z["diffusion_extra"])) if "diffusion_extra" in z.files else {}
    hack = bool(int(z["hack"]))
    cs, n_forc = 6 + int(hack), 2
    built = []

    class FakeNet:
        def __init__(self, n_in, n_cond):
            self.in_chans, self.model = n_in + n_cond, self

        def set_min_max_time(self, min_time, max_time):
            pass

    def fake_build(mc, n_in, n_out, n_cond, spatial, weights, **kw):
        built.append(FakeNet(n_in, n_cond))
        return built[-1]

    monkeypatch.setattr(checkpoint, "_build_net", fake_build)
    monkeypatch.setattr(checkpoint, "module_weights", lambda *a, **k: ({}, {}))
    monkeypatch.setattr(checkpoint.torch.cuda, "device", lambda d: nullcontext())
    dm = dict(in_names=[f"v{i}" for i in range(cs)], out_names=[f"v{i}" for i in range(cs - 6, cs)],
              forcing_names=["f0", "f1"], window=1, horizon=6)
    dc = dict(timesteps=6, hack_for_imprecise_interpolation=hack, **extra)
    state = {"hyper_parameters": {"datamodule_config": dm, "diffusion_config": dc, "model_config": {}}}
    istate = {"hyper_parameters": {"model_config": {}}}
    checkpoint.module_from_state(state, istate, (32, 64), device="cpu")
    assert built[0].in_chans == fcfg["in_chans"]
    assert built[1].in_chans == 2 * cs + n_forc
    # the reference's rule itself: "" / "none" add nothing, "data|noise" twice the window, every other value once
    for mode, n in (("", 0), ("none", 0), ("data", cs), ("data+noise-v1", cs), ("data+noise-v2", cs), ("data|noise", 2 * cs)):
        assert checkpoint.forward_conditioning_channels({"forward_conditioning": mode}, 1, cs) == n
    assert checkpoint.forward_conditioning_channels({}, 1, cs) == 0
    assert checkpoint.forward_conditioning_channels({"forward_conditioning": "data"}, 2, cs) == 2 * cs


def _define(name):
    src = open(os.path.join(ROOT, "spherical-dyffusion_amd", "csrc", "common.h")).read()
    return int(re.search(rf"#define {name} (0x[0-9A-Fa-f]+)u?", src).group(1), 16)


def test_noise_stream_counters_are_disjoint_from_the_dropout_streams():
    """Every counter (c0, c1, stream, call) the forward-conditioning noise can use differs from every counter of the element
    dropout (stream = 2 * layer + kind) and of drop path (stream = 0x1000 + layer) in the stream word, for all layer counts the
    network takes (sdy_sfno_config: <= 32 layers), any E / hidden width, batch <= 128 and any call number; and within the noise
    stream, distinct (trajectory, channel) planes get distinct c1 words over the ranges a forward can use."""
    noise = _define("SDY_NOISE_STREAM")
    assert noise == 0x2000
    L_MAX = 32
    dropout_words = {2 * layer + kind for layer in range(L_MAX) for kind in (0, 1)}
    drop_path_words = {0x1000 + layer for layer in range(L_MAX)}
    assert noise not in dropout_words | drop_path_words
    # (the time MLP and every GEMM epilogue draw with these two families only: the stream ids the library passes)
    capi = open(os.path.join(ROOT, "spherical-dyffusion_amd", "csrc", "capi.hip")).read()
    assert set(re.findall(r"stream_(?:fc[12]|id) = ([^;]+);", capi)) <= {"2u * i", "2u * i + 1u", "a->stream_id"}
    # c1 = trajectory * C + c is injective for trajectories < 2^32 / C: B <= 128 rows, batch offsets of large ensembles,
    # C <= 4 * 64 channels of a window
    for C in (6, 7, 63, 64, 256):
        traj = np.arange(0, 128 + 100_000, dtype=np.uint64)
        c1 = (traj[:, None] * np.uint64(C) + np.arange(C, dtype=np.uint64)[None, :]).reshape(-1)
        assert c1.max() < 2 ** 32 and np.unique(c1).size == c1.size
