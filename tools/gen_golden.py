#!/usr/bin/env python3
"""Generate golden vectors by RUNNING THE REFERENCE'S OWN CLASSES on CPU (build container only).

    python tools/gen_golden.py            # writes tests/golden/*.npz (+ fx_trace.json)

The reference is imported from /root/reference through tools/ref_shims.py (stubs for the packages this image lacks;
`torch_harmonics` is supplied by oracle/sht.py -- see the shim header).  Nothing here is needed at test time: the
fixtures are plain data (inputs, weights, expected outputs, recorded dropout masks).

Weights are "trained-like" (oracle.sfno.make_state_dict) and are loaded into the reference network with
strict=True, which also pins the state_dict contract (names + shapes) of SURVEY.md Appendix B.
"""
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import ref_shims  # noqa: E402

ref_shims.install()
from ref_shims import AttrDict  # noqa: E402

from oracle.sfno import SFNOConfig, make_state_dict  # noqa: E402
from src.models.modules.drop_path import DropPath  # noqa: E402
from src.models.sfno.sfnonet import SphericalFourierNeuralOperatorNet as RefSFNO  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
os.makedirs(OUT, exist_ok=True)


def np_sd(sd):
    return {"sd::" + k: v.detach().cpu().numpy() for k, v in sd.items()}


def pack(mask: torch.Tensor) -> np.ndarray:
    return np.packbits(mask.detach().cpu().numpy().astype(bool).reshape(-1))


def ref_net(cfg: SFNOConfig, n_in: int, n_cond: int, seed: int):
    net = RefSFNO(
        num_input_channels=n_in, num_output_channels=cfg.out_chans, num_conditional_channels=n_cond,
        spatial_shape_in=(cfg.nlat, cfg.nlon), spatial_shape_out=(cfg.nlat, cfg.nlon), loss_function=None,
        embed_dim=cfg.embed_dim, num_layers=cfg.num_layers, operator_type="dhconv", filter_type="linear",
        scale_factor=1, use_mlp=True, mlp_ratio=cfg.mlp_ratio, dropout_mlp=cfg.dropout_mlp,
        drop_path_rate=cfg.drop_path_rate, normalization_layer="instance_norm", with_time_emb=cfg.with_time_emb,
        data_grid=cfg.data_grid, big_skip=cfg.big_skip, pos_embed=cfg.pos_embed, verbose=False,
    )
    sd = make_state_dict(cfg, seed=seed)
    missing, unexpected = net.load_state_dict(sd, strict=False)
    # non-persistent SHT buffers are the only thing allowed to be absent
    assert not unexpected, unexpected
    assert all(".weights" in k or ".pct" in k for k in missing), missing
    ref_keys = {k for k in net.state_dict().keys() if ".weights" not in k and ".pct" not in k}
    assert ref_keys == set(sd.keys()), (sorted(ref_keys ^ set(sd.keys())))
    if cfg.with_time_emb:
        net.set_min_max_time(cfg.min_time, cfg.max_time)
    net.eval()
    return net, sd


class MaskRecorder:
    """Records the keep-masks the reference's nn.Dropout / DropPath layers actually drew (out != 0)."""

    def __init__(self, net):
        self.records = []
        self.handles = []
        for name, m in net.named_modules():
            if isinstance(m, torch.nn.Dropout):
                self.handles.append(m.register_forward_hook(self._hook(name, "elem")))
            elif isinstance(m, DropPath):
                self.handles.append(m.register_forward_hook(self._hook(name, "path")))

    def _hook(self, name, kind):
        def fn(mod, inp, out):
            if not mod.training:
                return
            if kind == "elem":
                self.records.append((name, (out != 0) | (inp[0] == 0)))
            else:
                keep = (out.flatten(1) != 0).any(dim=1) | (inp[0].flatten(1) == 0).all(dim=1)
                self.records.append((name, keep))
        return fn

    def remove(self):
        for h in self.handles:
            h.remove()


def gen_sfno(tag, cfg, n_in, n_cond, B, times, seed, with_masks):
    net, sd = ref_net(cfg, n_in, n_cond, seed)
    g = torch.Generator(device="cpu").manual_seed(1234)
    x = torch.randn(B, n_in, cfg.nlat, cfg.nlon, generator=g)
    cond = torch.randn(B, n_cond, cfg.nlat, cfg.nlon, generator=g) if n_cond else None
    t = torch.tensor(times, dtype=torch.float32) if cfg.with_time_emb else None
    blk_io = {}
    h = net.blocks[0].register_forward_hook(
        lambda m, i, o: blk_io.update(x=i[0].detach().clone(), y=o.detach().clone()))
    with torch.no_grad():
        y, trepr = net(x, time=t, condition=cond, return_time_emb=True)
    h.remove()
    out = dict(np_sd(sd), x=x.numpy(), y=y.numpy(), block0_in=blk_io["x"].numpy(), block0_out=blk_io["y"].numpy(),
               cfg=json.dumps({**cfg.__dict__, "n_in": n_in, "n_cond": n_cond}))
    if cond is not None:
        out["cond"] = cond.numpy()
    if t is not None:
        out["time"] = t.numpy()
        out["t_repr"] = trepr.numpy()
    if with_masks:
        net.enable_inference_dropout()       # _base_model.py:288-290 -> utils.enable_inference_dropout
        rec = MaskRecorder(net)
        torch.manual_seed(777)
        with torch.no_grad():
            yd = net(x, time=t, condition=cond)
        rec.remove()
        net.disable_inference_dropout()
        out["y_dropout"] = yd.numpy()
        out["mask_names"] = json.dumps([n for n, _ in rec.records])
        for i, (_, m) in enumerate(rec.records):
            out[f"mask{i}"] = pack(m)
            out[f"mask{i}_shape"] = np.array(m.shape)
    np.savez_compressed(os.path.join(OUT, f"{tag}.npz"), **out)
    print(f"{tag}: y std {float(y.std()):.4f}, saved")


def _weights_digest(sd):
    """Checksum of a seeded state_dict (the full-width fixtures store the SEED, not 100+ MB of weights): the test refuses
    to compare if its own make_state_dict(seed) does not reproduce these numbers."""
    return np.array([float(sum(v.double().abs().sum() for v in sd.values())),
                     float(sum((v.double() ** 2).sum() for v in sd.values()))])


def gen_sfno_full(tag="fx_sfno_full"):
    """The REFERENCE network at production width on the production grid: 180 x 360, E = 256, hidden 512, 68 + 2 -> 34
    channels, ALL 8 blocks (BASELINE.json configs[1] = the interpolator, whole): the first (equiangular -> Legendre-Gauss), six inner
    (LG -> LG) and the last (LG -> equiangular), time embedding, B = 1, dropout off.  These
    sizes reach every production kernel (`mlp_h3`, `conv_h3`, `dh_h3`, `leg_par`, `fft360`, `pair_h3`); the small fixtures
    above only reach the generic tile kernels.  Stored: seeds, checksums of the seeded weights / inputs, and the
    34 x 180 x 360 output of the reference (8.8 MB)."""
    cfg = SFNOConfig(in_chans=70, out_chans=34, nlat=180, nlon=360, embed_dim=256, num_layers=8, with_time_emb=True,
                     min_time=1.0, max_time=5.0)
    seed_w, seed_x = 4321, 1234
    net, sd = ref_net(cfg, 68, 2, seed_w)
    g = torch.Generator(device="cpu").manual_seed(seed_x)
    x = torch.randn(1, 68, cfg.nlat, cfg.nlon, generator=g)
    cond = torch.randn(1, 2, cfg.nlat, cfg.nlon, generator=g)
    t = torch.tensor([3.0])
    with torch.no_grad():
        y = net(x, time=t, condition=cond)
    np.savez_compressed(os.path.join(OUT, f"{tag}.npz"), y=y.numpy(), time=t.numpy(), seed_w=np.array(seed_w),
                        seed_x=np.array(seed_x), weights_digest=_weights_digest(sd),
                        inputs_digest=np.array([float(x.double().abs().sum()), float(cond.double().abs().sum())]),
                        cfg=json.dumps({**cfg.__dict__, "n_in": 68, "n_cond": 2}))
    print(f"{tag}: y std {float(y.std()):.4f}, |y| max {float(y.abs().max()):.3f}, saved")


def gen_sfno_wide_masks(tag="fx_sfno_wide_masks"):
    """The reference network at production WIDTH (E = 256, hidden 512: the fused MLP kernel's shape) on the small grid, with
    dropout and drop path ON and the masks its nn.Dropout / DropPath layers drew recorded -- injected into the product, they
    drive the fused `mlp_h3` kernel with the reference's own random decisions (no Philox on either side).  3 blocks, B = 2."""
    cfg = SFNOConfig(in_chans=10, out_chans=6, nlat=32, nlon=64, embed_dim=256, num_layers=3, with_time_emb=True,
                     dropout_mlp=0.1, drop_path_rate=0.3, min_time=0.0, max_time=5.0)
    seed_w, seed_x = 4321, 1234
    net, sd = ref_net(cfg, 8, 2, seed_w)
    g = torch.Generator(device="cpu").manual_seed(seed_x)
    x = torch.randn(2, 8, cfg.nlat, cfg.nlon, generator=g)
    cond = torch.randn(2, 2, cfg.nlat, cfg.nlon, generator=g)
    t = torch.tensor([1.0, 4.0])
    with torch.no_grad():
        y = net(x, time=t, condition=cond)
    net.enable_inference_dropout()
    rec = MaskRecorder(net)
    torch.manual_seed(777)
    with torch.no_grad():
        yd = net(x, time=t, condition=cond)
    rec.remove()
    out = dict(y=y.numpy(), y_dropout=yd.numpy(), time=t.numpy(), seed_w=np.array(seed_w), seed_x=np.array(seed_x),
               weights_digest=_weights_digest(sd),
               inputs_digest=np.array([float(x.double().abs().sum()), float(cond.double().abs().sum())]),
               cfg=json.dumps({**cfg.__dict__, "n_in": 8, "n_cond": 2}), mask_names=json.dumps([n for n, _ in rec.records]))
    for i, (_, m) in enumerate(rec.records):
        out[f"mask{i}"] = pack(m)
        out[f"mask{i}_shape"] = np.array(m.shape)
    np.savez_compressed(os.path.join(OUT, f"{tag}.npz"), **out)
    print(f"{tag}: y std {float(y.std()):.4f}, dropout changes y by {float((yd - y).norm() / y.norm()):.3f}, "
          f"{len(rec.records)} masks, saved")


def build_experiments(C, n_forc, H, W, E, L, hack, dropout, seed_f, seed_i, extra=None, ipol_min_time=1.0):
    import src.experiment_types._base_experiment as be
    from src.experiment_types.forecasting_multi_horizon import MultiHorizonForecastingDYffusion
    from src.experiment_types.interpolation import InterpolationExperiment

    be.get_dims_of_dataset = lambda dc: {"input": len(dc.in_names), "output": len(dc.out_names), "spatial_in": (H, W),
                                          "spatial_out": (H, W), "conditional": len(dc.forcing_names)}
    cs = C + (1 if hack else 0)
    dm = AttrDict(_target_="src.datamodules.fv3gfs_ensemble.FV3GFSEnsembleDataModule",
                  in_names=[f"v{i}" for i in range(cs)], out_names=[f"v{i}" for i in range(cs - C, cs)],
                  forcing_names=[f"f{i}" for i in range(n_forc)], window=1, horizon=6)

    def mcfg(**kw):
        return AttrDict(_target_="src.models.sfno.sfnonet.SphericalFourierNeuralOperatorNet", embed_dim=E, num_layers=L,
                        operator_type="dhconv", filter_type="linear", scale_factor=1, use_mlp=True, mlp_ratio=2.0,
                        normalization_layer="instance_norm", with_time_emb=True, data_grid="equiangular",
                        loss_function=None, verbose=False, **kw)

    ipol = InterpolationExperiment(model_config=mcfg(dropout_mlp=0.1 if dropout else 0.0,
                                                     drop_path_rate=0.1 if dropout else 0.0),
                                   datamodule_config=dm, enable_inference_dropout=True, verbose=False)
    icfg = SFNOConfig(in_chans=2 * cs + n_forc, out_chans=C, nlat=H, nlon=W, embed_dim=E, num_layers=L,
                      with_time_emb=True, dropout_mlp=0.1 if dropout else 0.0, drop_path_rate=0.1 if dropout else 0.0,
                      min_time=ipol_min_time, max_time=5.0)
    if ipol_min_time != 1.0:
        # InterpolationExperiment.__init__ pins the network's valid time range to the data time steps [1, horizon - 1]
        # (src/experiment_types/interpolation.py:24-25,27-31) and the network asserts it (sfnonet.py:780-782): sampling with
        # artificial steps (interpolation times in (0, 1)) needs an interpolator whose range was opened, as a user with a
        # continuous-time interpolator would do
        ipol.model.set_min_max_time(min_time=ipol_min_time, max_time=5.0)
    assert ipol.model.in_chans == icfg.in_chans and ipol.model.out_chans == C
    isd = make_state_dict(icfg, seed=seed_i)
    ipol.model.load_state_dict(isd, strict=False)
    dcfg = AttrDict(_target_="src.diffusion.dyffusion.DYffusion", timesteps=6, forward_conditioning="none",
                    interpolator=ipol, interpolator_local_checkpoint_path=None, time_encoding="dynamics",
                    hack_for_imprecise_interpolation=hack, enable_interpolator_dropout=bool(dropout))
    dcfg.update(extra or {})     # (`extra` may set forward_conditioning)
    fc = MultiHorizonForecastingDYffusion(model_config=mcfg(), datamodule_config=dm, diffusion_config=dcfg,
                                          verbose=False)
    # forward conditioning widens the forecaster by window * n_input channels (_base_experiment.py:207-225)
    n_fwd = 0 if dcfg["forward_conditioning"] == "none" else cs
    fcfg = SFNOConfig(in_chans=cs + n_fwd + n_forc, out_chans=C, nlat=H, nlon=W, embed_dim=E, num_layers=L,
                      with_time_emb=True, min_time=0.0, max_time=5.0)
    assert fc.model.model.in_chans == fcfg.in_chans
    fsd = make_state_dict(fcfg, seed=seed_f)
    fc.model.model.load_state_dict(fsd, strict=False)
    fc.eval()
    ipol.eval()
    return fc, ipol, fcfg, icfg, fsd, isd, cs


def save_npz_fixed(path, arrays):
    """np.savez_compressed, but every archive member carries one fixed timestamp (np.savez stamps the time of writing): the
    same arrays give the same bytes, so a regenerated fixture can be compared with the committed one by checksum."""
    import zipfile

    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for k, v in arrays.items():
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            with zf.open(info, "w", force_zip64=True) as f:
                np.lib.format.write_array(f, np.asanyarray(v), allow_pickle=False)


def sample_case_digest(fsd, isd, inputs):
    """Checksums of a sampler case's weights and inputs (x0, then the condition): what a fixture that stores only outputs keeps
    of them, asserted against the base fixture that stores them whole."""
    return dict(f_digest=_weights_digest(fsd), i_digest=_weights_digest(isd), inputs_digest=_digest(*inputs))


def gen_sample(tag, hack, dropout, extra=None, ipol_min_time=1.0, base=None, keep_final=False):
    """One DYffusion.sample of the reference on the tiny networks.  `base`: the name of a fixture with the same networks and
    inputs -- the new fixture then stores the outputs, the trace and the configuration only, with checksums of weights and
    inputs that are asserted against `base` here, and is written with fixed timestamps.  `keep_final`: also store what
    `sample_loop` returns first (the final state)."""
    C, n_forc, H, W, E, L = 6, 2, 32, 64, 16, 2
    fc, ipol, fcfg, icfg, fsd, isd, cs = build_experiments(C, n_forc, H, W, E, L, hack, dropout, 11, 22, extra,
                                                           ipol_min_time=ipol_min_time)
    g = torch.Generator(device="cpu").manual_seed(1234)
    B = 2
    x0 = torch.randn(B, cs, H, W, generator=g)
    if hack:
        kw = {"static_condition": torch.randn(B, n_forc, H, W, generator=g)}
    else:
        kw = {"dynamical_condition": torch.randn(B, 7, n_forc, H, W, generator=g)}
    trace = []
    f_net, i_net = fc.model.model, ipol.model
    hf = f_net.register_forward_pre_hook(lambda m, a, k: trace.append(["F", float(k["time"][0])]), with_kwargs=True)
    # (the third entry -- is the interpolator's dropout on for this call -- only where a fixture switches it per call)
    per_call_dropout = (extra or {}).get("enable_interpolator_dropout") == "except_dynamical_steps"
    hi = i_net.register_forward_pre_hook(
        lambda m, a, k: trace.append(["I", float(k["time"][0])] + ([bool(m.blocks[0].mlp.fwd[2].training)] if per_call_dropout else [])),
        with_kwargs=True)
    rec = MaskRecorder(i_net) if dropout else None
    final = {}
    if keep_final:      # `sample` drops sample_loop's first return value (dyffusion.py:565-572): record it on the way
        loop = fc.model.sample_loop

        def recording_loop(*a, **k):
            final["state"], intermediates = loop(*a, **k)
            return final["state"], intermediates
        fc.model.sample_loop = recording_loop
    torch.manual_seed(4242)
    res = fc.model.sample(x0, **kw)     # DYffusion.sample (dyffusion.py:569-572)
    hf.remove()
    hi.remove()
    if base is not None:
        assert not dropout, "a fixture that leans on a base fixture stores no masks"
        zb = np.load(os.path.join(OUT, f"{base}.npz"), allow_pickle=False)
        dig = sample_case_digest(fsd, isd, [x0] + list(kw.values()))
        want = sample_case_digest({k[3:]: torch.from_numpy(zb[k]) for k in zb.files if k.startswith("f::")},
                                  {k[3:]: torch.from_numpy(zb[k]) for k in zb.files if k.startswith("i::")},
                                  [torch.from_numpy(zb["x0"])] + [torch.from_numpy(zb[k]) for k in kw])
        for k in dig:
            assert np.array_equal(dig[k], want[k]), f"{tag}: {k} differs from {base}'s"
        assert int(zb["hack"]) == int(hack)
        out = dict(base=base, hack=np.array(int(hack)), dropout=np.array(0), trace=json.dumps(trace),
                   diffusion_extra=json.dumps(extra or {}), ipol_min_time=np.array(float(ipol_min_time)), **dig)
        for k, v in res.items():
            out["out::" + k] = v.numpy()
        if keep_final:
            out["final_state"] = final["state"].numpy()
        save_npz_fixed(os.path.join(OUT, f"{tag}.npz"), out)
        print(f"{tag}: keys {sorted(res.keys())}, {len(trace)} network calls, "
              f"{os.path.getsize(os.path.join(OUT, f'{tag}.npz'))} bytes, saved")
        return trace
    out = dict(x0=x0.numpy(), hack=np.array(int(hack)), dropout=np.array(int(dropout)),
               fcfg=json.dumps(fcfg.__dict__), icfg=json.dumps(icfg.__dict__), trace=json.dumps(trace))
    if extra:
        out["diffusion_extra"] = json.dumps(extra)
    out.update({"f::" + k: v.numpy() for k, v in fsd.items()})
    out.update({"i::" + k: v.numpy() for k, v in isd.items()})
    for k, v in kw.items():
        out[k] = v.numpy()
    for k, v in res.items():
        out["out::" + k] = v.numpy()
    if rec is not None:
        rec.remove()
        out["mask_names"] = json.dumps([n for n, _ in rec.records])
        for i, (_, m) in enumerate(rec.records):
            out[f"mask{i}"] = pack(m)
            out[f"mask{i}_shape"] = np.array(m.shape)
    np.savez_compressed(os.path.join(OUT, f"{tag}.npz"), **out)
    print(f"{tag}: keys {sorted(res.keys())}, {len(trace)} network calls, saved")
    return trace

    # also exercise the stepper-facing surface once (get_preds_at_t_for_batch), results must equal sample()


class RandnRecorder:
    """Records every torch.randn_like draw while active (the reference's forward-conditioning noise)."""

    def __enter__(self):
        self.draws, self._orig = [], torch.randn_like

        def rec(*a, **k):
            e = self._orig(*a, **k)
            self.draws.append(e.detach().clone())
            return e
        torch.randn_like = rec
        return self.draws

    def __exit__(self, *exc):
        torch.randn_like = self._orig


def _digest(*ts):
    return np.array([float(t.double().abs().sum()) for t in ts] + [float((t.double() ** 2).sum()) for t in ts])


def _seeded_sample_head(fcfg, icfg, fsd, isd, extra, hack, seeds, inputs):
    """The part every seeded forward-conditioning fixture shares: configs, seeds and checksums instead of weights / inputs."""
    return dict(hack=np.array(int(hack)), dropout=np.array(0), fcfg=json.dumps(fcfg.__dict__), icfg=json.dumps(icfg.__dict__),
                diffusion_extra=json.dumps(extra), seed_f=np.array(seeds[0]), seed_i=np.array(seeds[1]),
                seed_x=np.array(seeds[2]), f_digest=_weights_digest(fsd), i_digest=_weights_digest(isd),
                inputs_digest=_digest(*inputs))


def gen_sample_fcond_seeded(tag, hack, extra, ipol_min_time=1.0, B=1):
    """One DYffusion.sample with forward conditioning, stored SEEDED (tests rebuild weights, inputs and noise from the seeds
    and refuse to compare unless the checksums agree): the trace, the outputs, and for the noise modes the checksum of every
    torch.randn_like draw of the pass.  The draws are the only use of torch's global generator in the pass (no dropout), so
    after torch.manual_seed(seed_eps) they are torch.randn(x0.shape) one after the other -- asserted here."""
    C, n_forc, H, W, E, L = 6, 2, 32, 64, 16, 2
    seeds = (11, 22, 1234)
    fc, ipol, fcfg, icfg, fsd, isd, cs = build_experiments(C, n_forc, H, W, E, L, hack, False, *seeds[:2], extra,
                                                           ipol_min_time=ipol_min_time)
    g = torch.Generator(device="cpu").manual_seed(seeds[2])
    x0 = torch.randn(B, cs, H, W, generator=g)
    if hack:
        kw = {"static_condition": torch.randn(B, n_forc, H, W, generator=g)}
    else:
        kw = {"dynamical_condition": torch.randn(B, 7, n_forc, H, W, generator=g)}
    trace = []
    f_net, i_net = fc.model.model, ipol.model
    hf = f_net.register_forward_pre_hook(lambda m, a, k: trace.append(["F", float(k["time"][0])]), with_kwargs=True)
    hi = i_net.register_forward_pre_hook(lambda m, a, k: trace.append(["I", float(k["time"][0])]), with_kwargs=True)
    seed_eps = 4242
    torch.manual_seed(seed_eps)
    with RandnRecorder() as eps:       # the forward-conditioning noise (dyffusion.py:321-330), in call order
        res = fc.model.sample(x0, **kw)     # DYffusion.sample (dyffusion.py:569-572)
    hf.remove()
    hi.remove()
    ge = torch.Generator(device="cpu").manual_seed(seed_eps)
    for e in eps:
        assert torch.equal(e, torch.randn(x0.shape, generator=ge)), "the noise draws are not the seeded sequence"
    out = _seeded_sample_head(fcfg, icfg, fsd, isd, extra, hack, seeds, [x0] + list(kw.values()))
    out.update(trace=json.dumps(trace), input_keys=json.dumps(list(kw)), batch=np.array(B), seed_eps=np.array(seed_eps),
               n_eps=np.array(len(eps)), eps_digest=_digest(*eps) if eps else np.zeros(0))
    for k, v in res.items():
        out["out::" + k] = v.numpy()
    np.savez_compressed(os.path.join(OUT, f"{tag}.npz"), **out)
    print(f"{tag}: keys {sorted(res.keys())}, {len(trace)} network calls, {len(eps)} noise draws, saved")


def gen_sample_fcond():
    """DYffusion forward conditioning (src/diffusion/dyffusion.py:299-355; the forecaster sees [x_t | forward inputs |
    dynamical condition | static condition], _base_model.py:166-192): "data" with a dynamical condition, "data" with the carried
    channel and a static condition (four groups), both noise variants, v1 with two artificial steps (f = t / 7), and two
    autoregressive windows through get_preds_at_t_for_batch (x_0 changes between them).  Seeded (small files)."""
    gen_sample_fcond_seeded("fx_sample_fcond_data", False, dict(forward_conditioning="data"))
    gen_sample_fcond_seeded("fx_sample_fcond_data_hack", True, dict(forward_conditioning="data"))
    gen_sample_fcond_seeded("fx_sample_fcond_v1", False, dict(forward_conditioning="data+noise-v1"))
    gen_sample_fcond_seeded("fx_sample_fcond_v2", False, dict(forward_conditioning="data+noise-v2"))
    gen_sample_fcond_seeded("fx_sample_fcond_v1_k2", True, dict(forward_conditioning="data+noise-v1",
                                                                additional_interpolation_steps=2), ipol_min_time=0.0)
    gen_fcond_windows()


def gen_fcond_windows(tag="fx_sample_fcond_windows", B=1):
    """Two autoregressive windows of get_preds_at_t_for_batch (forecasting_multi_horizon.py:331-381, the stepper's
    prepare_inputs=False form) with forward_conditioning="data": window 2 starts from window 1's last prediction.  Seeded;
    stored: window 1's last prediction (window 2's x_0) and every prediction of window 2."""
    C, n_forc, H, W, E, L = 6, 2, 32, 64, 16, 2
    extra = dict(forward_conditioning="data")
    seeds = (11, 22, 4321)
    fc, ipol, fcfg, icfg, fsd, isd, cs = build_experiments(C, n_forc, H, W, E, L, False, False, *seeds[:2], extra)
    g = torch.Generator(device="cpu").manual_seed(seeds[2])
    x0 = torch.randn(B, cs, H, W, generator=g)
    dyns = [torch.randn(B, 7, n_forc, H, W, generator=g) for _ in range(2)]
    out = _seeded_sample_head(fcfg, icfg, fsd, isd, extra, False, seeds, [x0] + dyns)
    out["batch"] = np.array(B)
    x = x0
    for w, dyn in enumerate(dyns):
        res = {}
        for h in range(1, 7):
            batch = {"dynamics": x, "dynamical_condition": dyn}     # (read at h = 1 only; the reference pops from it)
            res.update(fc.get_preds_at_t_for_batch(batch, horizon=h, split="predict", prepare_inputs=False))
        x = res["t6_preds_normed"]
        for k, v in res.items():
            if w == 1 or k == "t6_preds_normed":
                out[f"out{w}::" + k] = v.numpy()
    np.savez_compressed(os.path.join(OUT, f"{tag}.npz"), **out)
    print(f"{tag}: keys {sorted(res.keys())}, saved")


def gen_sample_refine():
    """`refine_intermediate_predictions=True` (src/diffusion/dyffusion.py:551-563: a second interpolator sweep from the last
    forecast) with the carried input-only channel; 6 + 10 + 5 network calls."""
    return gen_sample("fx_sample_tiny_refine", hack=True, dropout=False, extra=dict(refine_intermediate_predictions=True))


def gen_sample_artificial():
    """The sampler OUTSIDE the shipped k = 0 configuration (src/diffusion/dyffusion.py:134-188 step map, :226-235 per-call
    dropout rule, :363-455 named schedules, :467-520 loop): additional_interpolation_steps = 2 puts two artificial diffusion
    steps (interpolation times 1/3, 2/3) in front of the first data step.
      fx_sample_tiny_k2          full schedule [0 .. 7], dropout "except_dynamical_steps" (on only for the calls of a step that
                                 lands on an artificial time), masks recorded
      fx_sample_tiny_k2_every2nd the same with sampling_schedule="every2nd" (artificial step 1 of [1, 2] joins)
      fx_sample_tiny_naive       sampling_type="naive", one artificial step, dropout always on, masks recorded"""
    k2 = dict(additional_interpolation_steps=2, enable_interpolator_dropout="except_dynamical_steps")
    t1 = gen_sample("fx_sample_tiny_k2", hack=True, dropout=True, extra=k2, ipol_min_time=0.0)
    t2 = gen_sample("fx_sample_tiny_k2_every2nd", hack=True, dropout=True, extra=dict(k2, sampling_schedule="every2nd"),
                    ipol_min_time=0.0)
    t3 = gen_sample("fx_sample_tiny_naive", hack=True, dropout=True,
                    extra=dict(additional_interpolation_steps=1, sampling_type="naive"), ipol_min_time=0.0)
    return t1, t2, t3


SWITCH_CASES = {
    # tag: (hack, extra diffusion options, interpolator's minimal time, keep sample_loop's final state)
    "fx_sample_sw_mid": (True, dict(use_cold_sampling_for_intermediate_steps=False), 1.0, False),
    "fx_sample_sw_discrete_k2": (True, dict(time_encoding="discrete", additional_interpolation_steps=2), 0.0, False),
    "fx_sample_sw_cond0": (False, dict(dynamic_cond_from_t="0"), 1.0, False),
    "fx_sample_sw_plus3": (True, dict(additional_interpolation_steps=2, sampling_schedule="only_dynamics_plus3"), 0.0, False),
    "fx_sample_sw_short": (True, dict(sampling_schedule=[0, 1, 2, 3]), 1.0, True),
    "fx_sample_sw_refine_pt": (True, dict(refine_intermediate_predictions=True, prediction_timesteps=[1, 2.5, 4]), 1.0, False),
    "fx_sample_sw_last_ar": (False, dict(use_cold_sampling_for_last_step=False, use_cold_sampling_for_init_of_ar_step=True),
                             1.0, False),
}


def gen_sample_switches():
    """The sampler's switches outside the shipped configuration, one reference pass each (src/diffusion/dyffusion.py:286-297
    time encoding, :333-345 dynamic_cond_from_t, :367-455 schedules, :495-534 cold-sampling switches, :546-567 refining sweep
    with prediction_timesteps and the final state of a schedule that ends early).  Networks and inputs are those of
    fx_sample_tiny (no carried channel: dynamical condition) / fx_sample_tiny_hack (carried channel: static condition), so
    only outputs, trace and configuration are stored (gen_sample, `base`).  Dropout off everywhere.
    Two configurations the reference cannot run are asserted to fail as recorded in NOTEBOOK.md:
      dynamic_cond_from_t="t"                                    IndexError (slice_time indexes with a float tensor, :343,360)
      carried channel + last step not cold + cold AR init        RuntimeError (7-channel state + 6-channel forecast, :508)"""
    traces = {}
    for tag, (hack, extra, ipol_min_time, keep_final) in SWITCH_CASES.items():
        traces[tag] = gen_sample(tag, hack=hack, dropout=False, extra=extra, ipol_min_time=ipol_min_time,
                                 base="fx_sample_tiny_hack" if hack else "fx_sample_tiny", keep_final=keep_final)
    for hack, extra, error in ((False, dict(dynamic_cond_from_t="t"), IndexError),
                               (True, dict(use_cold_sampling_for_last_step=False, use_cold_sampling_for_init_of_ar_step=True),
                                RuntimeError)):
        C, n_forc, H, W = 6, 2, 32, 64
        fc, _, _, _, _, _, cs = build_experiments(C, n_forc, H, W, 16, 2, hack, False, 11, 22, extra)
        g = torch.Generator(device="cpu").manual_seed(1234)
        x0 = torch.randn(2, cs, H, W, generator=g)
        kw = {"static_condition": torch.randn(2, n_forc, H, W, generator=g)} if hack else \
            {"dynamical_condition": torch.randn(2, 7, n_forc, H, W, generator=g)}
        try:
            fc.model.sample(x0, **kw)
        except error as e:
            print(f"reference with {extra}: {type(e).__name__}: {str(e)[:100]}")
        else:
            raise AssertionError(f"the reference no longer raises {error.__name__} with {extra}")
    return traces


def gen_stepper(tag="fx_stepper_tiny"):
    """The reference's own `run_on_batch_multistep` (src/ace_inference/core/stepper_multistep.py:298-466): normalise, pack,
    autoregressive loop over n_forward_steps with the DYffusion module, prescriber, denormalise."""
    from src.ace_inference.core.normalizer import StandardNormalizer
    from src.ace_inference.core.optimization import NullOptimization
    from src.ace_inference.core.prescriber import Prescriber
    from src.ace_inference.core.stepper_multistep import run_on_batch_multistep
    from src.ace_inference.training.utils.darcy_loss import LpLoss
    from src.utilities.packer import Packer

    C, n_forc, H, W, E, L = 6, 2, 32, 64, 16, 2
    fc, ipol, fcfg, icfg, fsd, isd, cs = build_experiments(C, n_forc, H, W, E, L, True, False, 11, 22)
    in_names = ["HGTsfc"] + [f"v{i}" for i in range(1, cs)]     # HGTsfc is input-only (the "imprecise" case)
    out_names = in_names[1:]
    forcing_names = [f"f{i}" for i in range(n_forc)]
    mask_name = "ocean_fraction"
    n_steps, B = 8, 2
    g = torch.Generator(device="cpu").manual_seed(2024)
    names = in_names + forcing_names
    means = {n: torch.randn((), generator=g) * 3.0 for n in names}
    stds = {n: torch.rand((), generator=g) * 2.0 + 0.5 for n in names}
    data = {n: torch.randn(B, n_steps + 1, H, W, generator=g) * stds[n] + means[n] for n in names}
    data[mask_name] = torch.rand(B, n_steps + 1, H, W, generator=g)
    pres = Prescriber(prescribed_name="v2", mask_name=mask_name, mask_value=1, interpolate=False)

    class _NullAgg:
        def record_batch(self, *a, **k):
            pass

    axis = -3
    stepped = run_on_batch_multistep(
        data={k: v.clone() for k, v in data.items()}, module=fc, normalizer=StandardNormalizer(means, stds),
        in_packer=Packer(in_names, axis=axis), out_packer=Packer(out_names, axis=axis),
        forcings_packer=Packer(forcing_names, axis=axis), optimization=NullOptimization(), loss_obj=LpLoss(),
        prescriber=pres, aggregator=_NullAgg(), n_forward_steps=n_steps)
    out = dict(in_names=json.dumps(in_names), out_names=json.dumps(out_names), forcing_names=json.dumps(forcing_names),
               prescriber=json.dumps(pres.get_state()), n_steps=np.array(n_steps),
               fcfg=json.dumps(fcfg.__dict__), icfg=json.dumps(icfg.__dict__))
    out.update({"f::" + k: v.numpy() for k, v in fsd.items()})
    out.update({"i::" + k: v.numpy() for k, v in isd.items()})
    out.update({"data::" + k: v.numpy() for k, v in data.items()})
    out.update({"mean::" + k: v.numpy() for k, v in means.items()})
    out.update({"std::" + k: v.numpy() for k, v in stds.items()})
    out.update({"gen::" + k: v.numpy() for k, v in stepped.gen_data.items()})
    out.update({"gen_norm::" + k: v.numpy() for k, v in stepped.gen_data_norm.items()})
    out.update({"metric::" + k: np.asarray(float(v)) for k, v in stepped.metrics.items()})
    np.savez_compressed(os.path.join(OUT, f"{tag}.npz"), **out)
    print(f"{tag}: loss {float(stepped.metrics['loss']):.5f}, gen vars {sorted(stepped.gen_data)[:3]}..., saved")


def gen_loop(tag="fx_loop_tiny"):
    """The reference's own window driver `run_inference` + `WindowStitcher` (src/ace_inference/inference/loop.py:26-264):
    two windows of 6 steps, 2 samples, 2 ensemble members (dropout off: the fixture pins the stitching / carry-over /
    stacking logic, the stochastic part is covered by the device-vs-oracle tests)."""
    import types

    import src.ace_inference.inference.loop as L
    from src.ace_inference.core.aggregator.null import NullAggregator
    from src.ace_inference.core.normalizer import StandardNormalizer
    from src.ace_inference.core.prescriber import Prescriber
    from src.ace_inference.core.stepper_multistep import run_on_batch_multistep
    from src.ace_inference.training.utils.darcy_loss import LpLoss
    from src.utilities.packer import Packer

    C, n_forc, H, W, E, Lr = 6, 2, 32, 64, 16, 2
    fc, ipol, fcfg, icfg, fsd, isd, cs = build_experiments(C, n_forc, H, W, E, Lr, True, False, 11, 22)
    in_names = ["HGTsfc"] + [f"v{i}" for i in range(1, cs)]
    out_names = in_names[1:]
    forcing_names = [f"f{i}" for i in range(n_forc)]
    mask_name = "ocean_fraction"
    n_total, n_mem_steps, B, members = 12, 6, 2, 2
    g = torch.Generator(device="cpu").manual_seed(777)
    names = in_names + forcing_names
    means = {n: torch.randn((), generator=g) * 3.0 for n in names}
    stds = {n: torch.rand((), generator=g) * 2.0 + 0.5 for n in names}
    series = {n: torch.randn(B, n_total + 1, H, W, generator=g) * stds[n] + means[n] for n in names}
    series[mask_name] = torch.rand(B, n_total + 1, H, W, generator=g)
    pres = Prescriber(prescribed_name="v2", mask_name=mask_name, mask_value=1, interpolate=False)
    axis = -3

    class _Stepper:   # what run_inference needs of MultiStepStepper: .module and .run_on_batch
        module = fc

        def run_on_batch(self, data, optimization, n_forward_steps=1, aggregator=None):
            return run_on_batch_multistep(
                data=data, module=fc, normalizer=StandardNormalizer(means, stds), in_packer=Packer(in_names, axis=axis),
                out_packer=Packer(out_names, axis=axis), forcings_packer=Packer(forcing_names, axis=axis),
                optimization=optimization, loss_obj=LpLoss(), prescriber=pres,
                aggregator=aggregator if aggregator is not None else NullAggregator(), n_forward_steps=n_forward_steps)

    class _Times:   # the only thing the loop does with xr.DataArray times: .isel(time=slice(1, None))
        def __init__(self, idx):
            self.idx = list(idx)

        def isel(self, time):
            return _Times(self.idx[time])

    windows = [types.SimpleNamespace(data={k: v[:, i * n_mem_steps:(i + 1) * n_mem_steps + 1].clone() for k, v in series.items()},
                                     times=_Times(range(i * n_mem_steps, (i + 1) * n_mem_steps + 1)))
               for i in range(n_total // n_mem_steps)]
    data = types.SimpleNamespace(loader=windows, sigma_coordinates=None)
    rec = []

    class _Writer:
        def append_batch(self, target, prediction, start_timestep, start_sample, batch_times=None):
            rec.append((int(start_timestep), {k: v.clone() for k, v in prediction.items()},
                        {k: v.clone() for k, v in target.items()}))

    losses = []

    class _Agg:   # (with the reference's NullAggregator an ensemble run dies on `stepped.metrics["loss"]`, loop.py:145,209)
        def record_batch(self, loss, target_data, gen_data, target_data_norm, gen_data_norm, i_time_start=0):
            losses.append((float(loss), int(i_time_start)))

    L.compute_derived_quantities = lambda d, s: d     # derived variables are outside the fixture's scope
    L.run_inference(_Agg(), _Stepper(), data, n_total, n_mem_steps, members, "cpu", writer=_Writer())
    out = dict(in_names=json.dumps(in_names), out_names=json.dumps(out_names), forcing_names=json.dumps(forcing_names),
               prescriber=json.dumps(pres.get_state()), n_total=np.array(n_total), n_mem_steps=np.array(n_mem_steps),
               members=np.array(members), fcfg=json.dumps(fcfg.__dict__), icfg=json.dumps(icfg.__dict__),
               starts=np.array([r[0] for r in rec]), losses=np.array([l[0] for l in losses]),
               i_time_starts=np.array([l[1] for l in losses]))
    # network weights: identical to fx_stepper_tiny.npz (same build_experiments seeds), not stored twice
    out.update({"series::" + k: v.numpy() for k, v in series.items()})
    out.update({"mean::" + k: v.numpy() for k, v in means.items()})
    out.update({"std::" + k: v.numpy() for k, v in stds.items()})
    for w, (st, pred, tgt) in enumerate(rec):
        out.update({f"pred{w}::" + k: v.numpy() for k, v in pred.items()})
    np.savez_compressed(os.path.join(OUT, f"{tag}.npz"), **out)
    print(f"{tag}: writer calls at {[r[0] for r in rec]}, prediction shapes "
          f"{[tuple(next(iter(r[1].values())).shape) for r in rec]}, saved")


def gen_ckpt_layout(tag="fx_ckpt_layout"):
    """What a Lightning checkpoint of the two reference experiments looks like (no tensors: key names and
    hyper-parameters only): `state_dict` keys of `MultiHorizonForecastingDYffusion` / `InterpolationExperiment`, the
    `LitEma` buffer name of every parameter (src/models/modules/ema.py:20-27) and the `hyper_parameters` dictionaries
    (`_base_experiment.py:75-100`).  The weights of the matching fixture are those of fx_stepper_tiny."""
    from src.models.modules.ema import LitEma

    fc, ipol, fcfg, icfg, fsd, isd, cs = build_experiments(6, 2, 32, 64, 16, 2, True, True, 11, 22)

    def clean(o):
        if isinstance(o, dict):
            return {k: clean(v) for k, v in o.items() if k != "interpolator"}
        if isinstance(o, (list, tuple)):
            return [clean(v) for v in o]
        if isinstance(o, (int, float, str, bool)) or o is None:
            return o
        return None

    def ema_map(handle):
        e = LitEma(handle, decay=0.9999)
        return dict(e.m_name2s_name)

    out = {
        "forecaster": {"hyper_parameters": clean(dict(fc.hparams)),
                       "state_dict_keys": [k for k in fc.state_dict().keys() if not k.startswith("model.interpolator")],
                       "ema_names": ema_map(fc.model), "ema_extra": ["decay", "num_updates"]},
        "interpolator": {"hyper_parameters": clean(dict(ipol.hparams)), "state_dict_keys": list(ipol.state_dict().keys()),
                         "ema_names": ema_map(ipol.model), "ema_extra": ["decay", "num_updates"]},
    }
    with open(os.path.join(OUT, f"{tag}.json"), "w") as f:
        json.dump(out, f, indent=1)
    print(f"{tag}: {len(out['forecaster']['state_dict_keys'])} + {len(out['interpolator']['state_dict_keys'])} keys, saved")


def gen_metrics(tag="fx_metrics"):
    """The reference's own ensemble diagnostics (src/ace_inference/core/metrics.py) on a small ensemble."""
    from src.ace_inference.core import metrics as M

    g = torch.Generator(device="cpu").manual_seed(31)
    E, S, T, H, W = 5, 2, 3, 16, 32
    lats = torch.linspace(-84.375, 84.375, H)
    w = M.spherical_area_weights(lats, W)
    truth = torch.randn(S, T, H, W, generator=g) * 2.0 + 1.0
    pred = truth[None] + torch.randn(E, S, T, H, W, generator=g) * 0.7 + 0.1
    dim = (-2, -1)
    out = dict(lats=lats.numpy(), weights=w.numpy(), truth=truth.numpy(), pred=pred.numpy(),
               rmse=M.root_mean_squared_error(truth, pred.mean(0), w, dim=dim).numpy(),
               spread=M.ensemble_spread(pred, w, dim=dim).numpy(),
               spread_skill_ratio=M.spread_skill_ratio(truth, pred, w, dim=dim).numpy(),
               crps=M.weighted_crps(truth, pred, w, dim=dim).numpy(),
               bias=M.weighted_mean_bias(truth, pred.mean(0), w, dim=dim).numpy())
    np.savez_compressed(os.path.join(OUT, f"{tag}.npz"), **out)
    print(f"{tag}: crps[0] {out['crps'][0]}, saved")


def gen_time_mean(tag="fx_time_mean"):
    """The reference's own TimeMeanAggregator (src/ace_inference/core/aggregator/inference/time_mean.py) fed two windows of
    an ensemble run the way run_inference feeds it (loop.py:133-149): time-mean maps, their RMSE and bias."""
    from src.ace_inference.core import metrics as M
    from src.ace_inference.core.aggregator.inference.time_mean import TimeMeanAggregator

    class NoDist:            # single process: reduce_mean is the identity (core/distributed.py)
        def reduce_mean(self, t):
            return t

    g = torch.Generator(device="cpu").manual_seed(41)
    E, S, T, H, W = 3, 2, 4, 16, 32
    names = ["a", "b"]
    lats = torch.linspace(-84.375, 84.375, H)
    w = M.spherical_area_weights(lats, W)
    out = dict(lats=lats.numpy(), names=json.dumps(names))
    for is_ens in (True, False):
        agg = TimeMeanAggregator(w, dist=NoDist(), is_ensemble=is_ens)
        key = "ens" if is_ens else "det"
        for win, (i_time_start, nt) in enumerate(((0, T + 1), (T + 1, T))):
            tgt = {n: torch.randn(S, nt, H, W, generator=g) * 2.0 + 1.0 for n in names}
            shp = (E, S, nt, H, W) if is_ens else (S, nt, H, W)
            gen = {n: (tgt[n][None] if is_ens else tgt[n]) + torch.randn(*shp, generator=g) * 0.5 + 0.2 for n in names}
            agg.record_batch(loss=0.0, target_data=tgt, gen_data=gen, target_data_norm=tgt, gen_data_norm=gen,
                             i_time_start=i_time_start)
            for n in names:
                out[f"{key}::tgt{win}::{n}"] = tgt[n].numpy()
                out[f"{key}::gen{win}::{n}"] = gen[n].numpy()
            out[f"{key}::i_time_start{win}"] = i_time_start
        for pr in agg._get_target_gen_pairs():
            out[f"{key}::gen_map::{pr.name}"] = pr.gen.numpy()
            out[f"{key}::target_map::{pr.name}"] = pr.target.numpy()
            out[f"{key}::rmse::{pr.name}"] = pr.rmse(weights=w)
            out[f"{key}::bias::{pr.name}"] = pr.weighted_mean_bias(weights=w)
    np.savez_compressed(os.path.join(OUT, f"{tag}.npz"), **out)
    print(f"{tag}: ens rmse a {out['ens::rmse::a']}, saved")


def gen_mean_series(tag="fx_mean_series"):
    """The reference's own MeanAggregator (src/ace_inference/core/aggregator/inference/reduced.py:144-266: the per-timestep
    series of area-weighted metrics) fed three windows the way run_inference feeds it (loop.py:133-149), ensemble and
    deterministic.  The gradient-magnitude metric is not stored (out of the build's scope)."""
    from src.ace_inference.core import metrics as M
    from src.ace_inference.core.aggregator.inference.reduced import MeanAggregator

    class NoDist:            # single process: reduce_mean is the identity (core/distributed.py)
        def reduce_mean(self, t):
            return t

    g = torch.Generator(device="cpu").manual_seed(43)
    E, S, T, H, W = 4, 2, 3, 16, 32
    names = ["a", "b"]
    lats = torch.linspace(-84.375, 84.375, H)
    w = M.spherical_area_weights(lats, W)
    n_timesteps = 1 + 3 * T
    out = dict(lats=lats.numpy(), names=json.dumps(names), n_timesteps=n_timesteps)
    for is_ens in (True, False):
        agg = MeanAggregator(w, target="denorm", n_timesteps=n_timesteps, is_ensemble=is_ens, dist=NoDist(),
                             device=torch.device("cpu"))
        key = "ens" if is_ens else "det"
        i_time = 0
        for win in range(3):
            nt = T + 1 if win == 0 else T           # the first window keeps its initial condition (loop.py:133-141)
            tgt = {n: torch.randn(S, nt, H, W, generator=g) * 2.0 + 1.0 for n in names}
            shp = (E, S, nt, H, W) if is_ens else (S, nt, H, W)
            gen = {n: (tgt[n][None] if is_ens else tgt[n]) + torch.randn(*shp, generator=g) * 0.5 + 0.2 for n in names}
            agg.record_batch(loss=0.0, target_data=tgt, gen_data=gen, target_data_norm=tgt, gen_data_norm=gen,
                             i_time_start=i_time)
            for n in names:
                out[f"{key}::tgt{win}::{n}"] = tgt[n].numpy()
                out[f"{key}::gen{win}::{n}"] = gen[n].numpy()
            out[f"{key}::i_time_start{win}"] = i_time
            i_time += nt
        metrics = []
        for d in agg._get_series_data():
            if "grad_mag" in d.metric_name:
                continue
            out[f"{key}::series::{d.metric_name}/{d.var_name}"] = np.asarray(d.data, dtype=np.float64)
            metrics.append(d.metric_name)
        out[f"{key}::metrics"] = json.dumps(sorted(set(metrics)))
    np.savez_compressed(os.path.join(OUT, f"{tag}.npz"), **out)
    print(f"{tag}: ens weighted_crps/a {out['ens::series::weighted_crps/a'][:3]}, saved")


def gen_mean_series_grad(tag="fx_mean_series_grad"):
    """The reference's own inference MeanAggregator (reduced.py:144-266) and one-step MeanAggregator
    (one_step/reduced.py:35-147) WITH weighted_grad_mag_percent_diff (metrics.py:210-241), fed three windows the way
    run_inference feeds them (loop.py:133-149), ensemble and deterministic, on a 16x32 and an odd 7x10 grid.  The truth has
    spatial structure; prediction "a" is a smoothed truth (negative percent difference), "b" a noisier one (positive).  The
    one-step aggregator's target time lies inside the second window."""
    from src.ace_inference.core import metrics as M
    from src.ace_inference.core.aggregator.inference.reduced import MeanAggregator
    from src.ace_inference.core.aggregator.one_step.reduced import MeanAggregator as OneStepMeanAggregator

    class NoDist:            # single process: reduce_mean is the identity (core/distributed.py)
        def reduce_mean(self, t):
            return t

    g = torch.Generator(device="cpu").manual_seed(47)
    E, S, T = 5, 2, 2
    names = ["a", "b"]
    target_time = 4                                # windows cover times 0-2, 3-4, 5-6
    n_timesteps = 1 + 3 * T

    def field(shape, H, W):                        # a few large-scale waves with random phases + small-scale noise
        lat = torch.linspace(0, np.pi, H)[:, None]
        lon = torch.linspace(0, 2 * np.pi, W + 1)[:-1][None, :]
        ph = torch.rand(*shape, 3, 1, 1, generator=g) * 2 * np.pi
        x = (torch.sin(2 * lat + ph[..., 0, :, :]) * torch.cos(lon + ph[..., 1, :, :])
             + 0.5 * torch.cos(3 * lon + 2 * lat + ph[..., 2, :, :]))
        return 2.0 * x + 1.0 + 0.3 * torch.randn(*shape, H, W, generator=g)

    def smooth(x):                                 # 3-point box filter along both axes, edges replicated
        xp = torch.nn.functional.pad(x.reshape(-1, 1, *x.shape[-2:]), (1, 1, 1, 1), mode="replicate")
        return torch.nn.functional.avg_pool2d(xp, 3, stride=1).reshape(x.shape)

    out = dict(names=json.dumps(names), n_timesteps=n_timesteps, target_time=target_time, shapes=json.dumps([]))
    shapes = []
    for H, W in ((16, 32), (7, 10)):
        shp_tag = f"{H}x{W}"
        shapes.append(shp_tag)
        lats = torch.linspace(-84.375, 84.375, H) if H == 16 else torch.linspace(-80.0, 80.0, H)
        w = M.spherical_area_weights(lats, W)
        out[f"{shp_tag}::lats"] = lats.numpy()
        for is_ens in (True, False):
            key = f"{shp_tag}::{'ens' if is_ens else 'det'}"
            agg = MeanAggregator(w, target="denorm", n_timesteps=n_timesteps, is_ensemble=is_ens, dist=NoDist(),
                                 device=torch.device("cpu"))
            one = OneStepMeanAggregator(w, target_time=target_time, is_ensemble=is_ens, dist=NoDist(),
                                        device=torch.device("cpu"))
            i_time = 0
            for win in range(3):
                nt = T + 1 if win == 0 else T       # the first window keeps its initial condition (loop.py:133-141)
                tgt = {n: field((S, nt), H, W) for n in names}
                mshp = (E, S, nt) if is_ens else (S, nt)
                base = {n: tgt[n][None] if is_ens else tgt[n] for n in names}
                gen = {"a": smooth(base["a"].expand(*mshp, H, W).clone()) + 0.1 * torch.randn(*mshp, H, W, generator=g),
                       "b": base["b"] + 0.6 * torch.randn(*mshp, H, W, generator=g) + 0.1}
                loss = 0.25 * (win + 1)
                for a in (agg, one):
                    a.record_batch(loss=loss, target_data=tgt, gen_data=gen, target_data_norm=tgt, gen_data_norm=gen,
                                   i_time_start=i_time)
                for n in names:
                    out[f"{key}::tgt{win}::{n}"] = tgt[n].numpy()
                    out[f"{key}::gen{win}::{n}"] = gen[n].numpy()
                out[f"{key}::i_time_start{win}"] = i_time
                out[f"{key}::loss{win}"] = loss
                i_time += nt
            metrics = []
            for d in agg._get_series_data():
                out[f"{key}::series::{d.metric_name}/{d.var_name}"] = np.asarray(d.data, dtype=np.float64)
                metrics.append(d.metric_name)
            out[f"{key}::metrics"] = json.dumps(sorted(set(metrics)))
            logs = one.get_logs("one")
            for k, v in logs.items():
                out[f"{key}::one_step::{k[len('one/'):]}"] = np.float64(v)
            out[f"{key}::one_step_keys"] = json.dumps(sorted(k[len("one/"):] for k in logs))
            gm = [out[f"{key}::series::weighted_grad_mag_percent_diff/{n}"] for n in names]
            assert (gm[0] < 0).all() and (gm[1] > 0).all(), gm      # both signs of the percent difference occur
    out["shapes"] = json.dumps(shapes)
    path = os.path.join(OUT, f"{tag}.npz")
    np.savez_compressed(path, **out)
    print(f"{tag}: 16x32 ens grad_mag a {out['16x32::ens::series::weighted_grad_mag_percent_diff/a'][:3]}, "
          f"b {out['16x32::ens::series::weighted_grad_mag_percent_diff/b'][:3]}; {os.path.getsize(path)} bytes, saved")

def gen_derived(tag="fx_derived"):
    """The reference's own `compute_derived_quantities` (inference/derived_variables.py, metrics.py:296-367) on
    function-level cases, and its own `run_inference` (inference/loop.py:158-264) with it on the tiny stepper of gen_loop.

    Function level: 4-D (samples, time, lat, lon) and 5-D member-stacked (members, samples, time, lat, lon) dicts on a 7 x 12
    grid, K = 4, 8 and 12 levels (12 inserted out of order, with the aliases PS / LHFLX / surface_precipitation_rate),
    T = 1, FV3GFS-like magnitudes.  5-D cases also record the reference applied to each member alone (`member::`): the
    values the port computes, since the reference differences the 5-D residual over samples.

    Loop: fx_loop_tiny's series and network with the six generated variables renamed to specific_total_water_0 / _1
    (K = 2), PRESsfc, LHTFLsfc, PRATEsfc and tendency_of_total_water_path_due_to_advection, two windows of 6 steps, 2 initial
    conditions, run with 1 member and with 3.  Recorded: the derived arrays the writer received (those the aggregator
    receives are the same dicts), on a spatial subsample [..., ::4, ::8] plus per-plane sums in fp64; and the reference
    applied member by member to the 3-member predictions."""
    import types

    import src.ace_inference.inference.loop as L
    from src.ace_inference.core.aggregator.null import NullAggregator
    from src.ace_inference.core.data_loading.data_typing import SigmaCoordinates
    from src.ace_inference.core.normalizer import StandardNormalizer
    from src.ace_inference.core.prescriber import Prescriber
    from src.ace_inference.core.stepper_multistep import run_on_batch_multistep
    from src.ace_inference.inference.derived_variables import compute_derived_quantities
    from src.ace_inference.training.utils.darcy_loss import LpLoss
    from src.utilities.packer import Packer

    derived = ["surface_pressure_due_to_dry_air", "total_water_path", "total_water_path_budget_residual"]
    g = torch.Generator(device="cpu").manual_seed(4711)
    ak8 = [3.0, 5238.4, 11815.8, 17263.1, 19929.5, 17023.4, 8970.5, 1537.5, 0.0]
    bk8 = [0.0, 0.0, 0.0115, 0.0781, 0.2034, 0.4004, 0.6513, 0.9065, 1.0]
    levels = {4: (ak8[::2], bk8[::2]), 8: (ak8, bk8),
              12: ([3.0 + 1700.0 * k * (12 - k) / 3.0 for k in range(13)], [(k / 12.0) ** 1.8 for k in range(13)])}
    H, W = 7, 12
    out = dict(derived=json.dumps(derived))
    cases = []

    def fields(lead, K, aliases):
        q_scale = torch.logspace(-2, -6, K)                   # moist near the surface, dry aloft
        d = {}
        order = list(range(K))
        if K > 10:
            order = order[::-1]                                 # insertion order != natural order (_10 after _2)
        for k in order:
            d[f"specific_total_water_{k}"] = q_scale[k] * torch.rand(*lead, H, W, generator=g) * 2.0
        ps_name, lhf_name, pr_name = ("PS", "LHFLX", "surface_precipitation_rate") if aliases else \
            ("PRESsfc", "LHTFLsfc", "PRATEsfc")
        d[ps_name] = 1.0e5 + 2.5e3 * torch.randn(*lead, H, W, generator=g)
        d[lhf_name] = 90.0 + 60.0 * torch.randn(*lead, H, W, generator=g)
        d[pr_name] = 3.0e-5 * torch.rand(*lead, H, W, generator=g) * 2.0
        d["tendency_of_total_water_path_due_to_advection"] = 2.0e-5 * torch.randn(*lead, H, W, generator=g)
        d["TMP2m"] = 280.0 + torch.randn(*lead, H, W, generator=g)           # an unrelated variable passes through
        return d

    for name, lead, K, aliases in (("det_k4", (2, 3), 4, False), ("ens_k8", (3, 2, 4), 8, False),
                                   ("det_k12_alias", (2, 3), 12, True), ("det_k8_t1", (2, 1), 8, False),
                                   ("ens_k4_t1", (2, 2, 1), 4, True)):
        ak, bk = levels[K]
        sigma = SigmaCoordinates(ak=torch.tensor(ak), bk=torch.tensor(bk))
        d = fields(lead, K, aliases)
        res = compute_derived_quantities(d, sigma)
        assert list(res)[-3:] == derived, list(res)
        cases.append(name)
        out[f"{name}::names"] = json.dumps(list(d))
        out[f"{name}::ak"], out[f"{name}::bk"] = np.asarray(ak, np.float32), np.asarray(bk, np.float32)
        out.update({f"{name}::in::{k}": v.numpy() for k, v in d.items()})
        out.update({f"{name}::ref::{k}": res[k].numpy() for k in derived})
        if len(lead) == 3:
            per = [compute_derived_quantities({k: v[m] for k, v in d.items()}, sigma) for m in range(lead[0])]
            out.update({f"{name}::member::{k}": torch.stack([p[k] for p in per]).numpy() for k in derived})
    out["cases"] = json.dumps(cases)

    # ---- the reference's window driver with the real compute_derived_quantities (the tiny stepper of gen_loop)
    C, n_forc, Hl, Wl, E, Lr = 6, 2, 32, 64, 16, 2
    fc, ipol, fcfg, icfg, fsd, isd, cs = build_experiments(C, n_forc, Hl, Wl, E, Lr, True, False, 11, 22)
    old_in = ["HGTsfc"] + [f"v{i}" for i in range(1, cs)]
    rename = dict(zip(old_in[1:], ["specific_total_water_0", "specific_total_water_1", "PRESsfc", "LHTFLsfc", "PRATEsfc",
                                   "tendency_of_total_water_path_due_to_advection"]))
    assert len(rename) == len(old_in) - 1
    rn = lambda n: rename.get(n, n)  # noqa: E731
    in_names = [rn(n) for n in old_in]
    out_names = in_names[1:]
    forcing_names = [f"f{i}" for i in range(n_forc)]
    mask_name = "ocean_fraction"
    n_total, n_mem_steps, B = 12, 6, 2
    g = torch.Generator(device="cpu").manual_seed(777)      # gen_loop's series, draw for draw
    names = old_in + forcing_names
    means = {rn(n): torch.randn((), generator=g) * 3.0 for n in names}
    stds = {rn(n): torch.rand((), generator=g) * 2.0 + 0.5 for n in names}
    series = {rn(n): torch.randn(B, n_total + 1, Hl, Wl, generator=g) * stds[rn(n)] + means[rn(n)] for n in names}
    series[mask_name] = torch.rand(B, n_total + 1, Hl, Wl, generator=g)
    pres = Prescriber(prescribed_name=rn("v2"), mask_name=mask_name, mask_value=1, interpolate=False)
    axis = -3
    ak, bk = [0.0, 0.5, 0.0], [0.0, 0.4, 1.0]
    sigma = SigmaCoordinates(ak=torch.tensor(ak), bk=torch.tensor(bk))
    out["loop::ak"], out["loop::bk"] = np.float32(ak), np.float32(bk)
    out["loop::rename"] = json.dumps(rename)

    class _Stepper:
        module = fc

        def run_on_batch(self, data, optimization, n_forward_steps=1, aggregator=None):
            return run_on_batch_multistep(
                data=data, module=fc, normalizer=StandardNormalizer(means, stds), in_packer=Packer(in_names, axis=axis),
                out_packer=Packer(out_names, axis=axis), forcings_packer=Packer(forcing_names, axis=axis),
                optimization=optimization, loss_obj=LpLoss(), prescriber=pres,
                aggregator=aggregator if aggregator is not None else NullAggregator(), n_forward_steps=n_forward_steps)

    per_member = []           # 5-D (member-stacked) calls of the loop: the reference applied to each member alone

    def recording(data, sigma_coordinates):
        any_v = next(iter(data.values()))
        if any_v.dim() == 5:
            per = [compute_derived_quantities({k: v[m] for k, v in data.items()}, sigma_coordinates)
                   for m in range(any_v.shape[0])]
            per_member.append({k: torch.stack([p[k] for p in per]) for k in derived})
        return compute_derived_quantities(data, sigma_coordinates)

    L.compute_derived_quantities = recording
    sub = (Ellipsis, slice(None, None, 4), slice(None, None, 8))
    for members in (1, 3):
        windows = [types.SimpleNamespace(
            data={k: v[:, i * n_mem_steps:(i + 1) * n_mem_steps + 1].clone() for k, v in series.items()},
            times=types.SimpleNamespace(isel=lambda time: None)) for i in range(n_total // n_mem_steps)]
        rec = []

        class _Writer:
            def append_batch(self, target, prediction, start_timestep, start_sample, batch_times=None):
                rec.append((int(start_timestep), {k: v.clone() for k, v in prediction.items()},
                            {k: v.clone() for k, v in target.items()}))

        class _Agg:
            def record_batch(self, loss, target_data, gen_data, target_data_norm, gen_data_norm, i_time_start=0):
                assert all(k in target_data and k in gen_data for k in derived)

        L.run_inference(_Agg(), _Stepper(), types.SimpleNamespace(loader=windows, sigma_coordinates=sigma), n_total,
                        n_mem_steps, members, "cpu", writer=_Writer())
        key = f"loop::m{members}"
        out[f"{key}::starts"] = np.array([r[0] for r in rec])
        for w, (st, pred, tgt) in enumerate(rec):
            assert list(pred)[-3:] == derived and list(tgt)[-3:] == derived
            for kind, dct in (("pred", pred), ("tgt", tgt)):
                for k in derived:
                    out[f"{key}::{kind}{w}::{k}"] = dct[k][sub].numpy()
                    out[f"{key}::{kind}{w}::{k}::sum"] = dct[k].double().sum(dim=(-2, -1)).numpy()
            if members > 1:       # per member, with the first time dropped as the writer sees it (loop.py:133-141)
                for k in derived:
                    x = per_member[w][k][:, :, 1:] if w > 0 else per_member[w][k]
                    assert x.shape == pred[k].shape
                    out[f"{key}::member{w}::{k}"] = x[sub].numpy()
                    out[f"{key}::member{w}::{k}::sum"] = x.double().sum(dim=(-2, -1)).numpy()
        assert len(per_member) == (len(rec) if members > 1 else 0)
        per_member.clear()
    path = os.path.join(OUT, f"{tag}.npz")
    np.savez_compressed(path, **out)
    r = out["ens_k8::ref::total_water_path_budget_residual"]
    print(f"{tag}: cases {cases}; ens_k8 residual ref (sample-axis) |max| {np.abs(r).max():.3e} vs per-member "
          f"{np.abs(out['ens_k8::member::total_water_path_budget_residual']).max():.3e}; {os.path.getsize(path)} bytes, "
          "saved")


def gen_corrector(tag="fx_corrector"):
    """The reference's own `Corrector` (core/corrector.py) on CPU, per sample set and configuration.

    Three sample sets (inputs stored once each): `b3k2` B = 3, K = 2 on 6 x 12; `b2k8` B = 2, K = 8 on 19 x 36; `b2k3` B = 2,
    K = 3 on 7 x 9 (HW = 63: no multiple of 4).  Plausible fields, so that no global mean is near zero: ps 1e5 +- 3e3, q from
    1e-6 aloft to 2e-2 at the surface, prate > 0 with mean 3e-5, lhf of order 80, adv of order 1e-5 with a non-zero mean; gen
    is the input plus a step-sized change (a 15 Pa mean pressure drift), so the water-path tendency is the small difference
    of large numbers it is in a rollout.  Configurations: each option alone (a budget mode alone is what the reference's class
    accepts, its docstring notwithstanding), conserve_dry_air + zero advection + each of the four budget modes, all on every
    set; and the full `advection_and_precipitation` combination once on `b3k2` under the alias names.  Recorded per case: the
    rewritten variables as the reference returns them in float32 (`ref32`) and from float64 inputs (`ref64`)."""
    from src.ace_inference.core.corrector import CorrectorConfig
    from src.ace_inference.core.data_loading.data_typing import SigmaCoordinates

    g = torch.Generator(device="cpu").manual_seed(90210)
    ak8 = [3.0, 5238.4, 11815.8, 17263.1, 19929.5, 17023.4, 8970.5, 1537.5, 0.0]
    bk8 = [0.0, 0.0, 0.0115, 0.0781, 0.2034, 0.4004, 0.6513, 0.9065, 1.0]
    levels = {2: (ak8[::4], bk8[::4]), 3: ([ak8[i] for i in (0, 3, 6, 8)], [bk8[i] for i in (0, 3, 6, 8)]), 8: (ak8, bk8)}
    adv_name = "tendency_of_total_water_path_due_to_advection"
    plain = dict(ps="PRESsfc", lhf="LHTFLsfc", prate="PRATEsfc")
    alias = dict(ps="PS", lhf="LHFLX", prate="surface_precipitation_rate")

    def fields(B, K, H, W, names):
        q_scale = torch.logspace(-6, -2, K) if K > 1 else torch.tensor([1e-2])
        d_in, d_gen = {}, {}
        for k in range(K):
            d_in[f"specific_total_water_{k}"] = q_scale[k] * (1.0 + torch.rand(B, H, W, generator=g))
            d_gen[f"specific_total_water_{k}"] = d_in[f"specific_total_water_{k}"] * (1.0 + 0.05 * torch.randn(B, H, W, generator=g))
        d_in[names["ps"]] = 1.0e5 + 3.0e3 * torch.randn(B, H, W, generator=g)
        d_gen[names["ps"]] = d_in[names["ps"]] + 15.0 + 200.0 * torch.randn(B, H, W, generator=g)
        for d in (d_in, d_gen):
            d[names["lhf"]] = 80.0 + 30.0 * torch.randn(B, H, W, generator=g)
            d[names["prate"]] = 6.0e-5 * torch.rand(B, H, W, generator=g)
            d[adv_name] = 3.0e-6 + 1.0e-5 * torch.randn(B, H, W, generator=g)
            d["TMP2m"] = 280.0 + torch.randn(B, H, W, generator=g)              # an unrelated variable passes through
        return d_in, d_gen

    out = {}
    sets = {}
    for sname, (B, K, H, W) in (("b3k2", (3, 2, 6, 12)), ("b2k8", (2, 8, 19, 36)), ("b2k3", (2, 3, 7, 9))):
        lat = (torch.arange(H, dtype=torch.float64) + 0.5) / H * np.pi - np.pi / 2
        area = (torch.cos(lat)[:, None] * (1.0 + 0.1 * torch.rand(H, W, generator=g, dtype=torch.float64))).float()
        d_in, d_gen = fields(B, K, H, W, plain)
        sets[sname] = (K, area, d_in, d_gen)
        ak, bk = levels[K]
        out[f"{sname}::ak"], out[f"{sname}::bk"] = np.asarray(ak, np.float32), np.asarray(bk, np.float32)
        out[f"{sname}::area"] = area.numpy()
        out[f"{sname}::names"] = json.dumps(list(d_gen))
        out.update({f"{sname}::in::{k}": v.numpy() for k, v in d_in.items()})
        out.update({f"{sname}::gen::{k}": v.numpy() for k, v in d_gen.items()})
    modes = ["precipitation", "evaporation", "advection_and_precipitation", "advection_and_evaporation"]
    configs = [("dry", dict(conserve_dry_air=True)), ("zero_adv", dict(zero_global_mean_moisture_advection=True))]
    configs += [(f"only_{m}", dict(moisture_budget_correction=m)) for m in modes]
    configs += [(f"all_{m}", dict(conserve_dry_air=True, zero_global_mean_moisture_advection=True,
                                  moisture_budget_correction=m)) for m in modes]
    cases = []

    def run(case, sname, cfg, rename):
        K, area, d_in, d_gen = sets[sname]
        rn = lambda n: rename.get(n, n)  # noqa: E731
        ak, bk = out[f"{sname}::ak"], out[f"{sname}::bk"]
        res = {}
        for tagp, dt in (("ref32", torch.float32), ("ref64", torch.float64)):
            sigma = SigmaCoordinates(ak=torch.tensor(ak).to(dt), bk=torch.tensor(bk).to(dt))
            corr = CorrectorConfig(**cfg).build(area.to(dt), sigma)
            i = {rn(k): v.to(dt) for k, v in d_in.items()}
            o = {rn(k): v.to(dt) for k, v in d_gen.items()}
            r = corr(i, o)
            assert list(r) == list(o)
            res[tagp] = {k: v for k, v in r.items() if v is not o[k]}
            assert all(v.dtype == dt for v in res[tagp].values())
        assert list(res["ref32"]) == list(res["ref64"]) and res["ref32"], case
        cases.append(dict(name=case, set=sname, config=cfg, rename=rename, written=list(res["ref32"])))
        for tagp, vals in res.items():
            out.update({f"{case}::{tagp}::{k}": v.numpy() for k, v in vals.items()})

    for sname in sets:
        for cname, cfg in configs:
            run(f"{sname}_{cname}", sname, cfg, {})
    run("b3k2_alias", "b3k2", dict(conserve_dry_air=True, zero_global_mean_moisture_advection=True,
                                   moisture_budget_correction="advection_and_precipitation"),
        {plain[k]: alias[k] for k in plain})
    out["cases"] = json.dumps(cases)
    path = os.path.join(OUT, f"{tag}.npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < (1 << 20), os.path.getsize(path)


def gen_histogram(tag="fx_histogram"):
    """The reference's own `DynamicHistogram` (src/ace_inference/core/histogram.py; numpy only) fed the way
    `_HistogramAggregator.record_batch` feeds it (data_writer/histograms.py:32-45: `transpose(1, 0, 2, 3).reshape(n_times,
    -1)` of a (samples, time, lat, lon) array).  That class itself cannot be imported here (its module imports xarray), so the
    two lines are restated below.  Per case and n_bins (300 and 8) a sequence of adds on a 12 x 24 grid:
      grow      a first narrow window, one that exceeds the range on the right, one that exceeds it on the left by more
                than 4x (several doublings in one add);
      edges     a second add whose values sit exactly on interior edges and on the last edge;
      constant  a constant field (range +-1e-6: a step below float32's spacing, runs of equal edges), then a wide one;
      stacked   member-stacked 5-D predictions (members, samples, time, lat, lon); expected counts from the pooled reshape.
    Stored: inputs, i_time_start, the (min, max) fed at each add, the edges after each add, the doublings each add made,
    the final counts, numpy's version."""
    from src.ace_inference.core.histogram import DynamicHistogram

    class Counting(DynamicHistogram):
        n_left = n_right = 0

        def _double_size_left(self):
            self.n_left += 1
            super()._double_size_left()

        def _double_size_right(self):
            self.n_right += 1
            super()._double_size_right()

    def pooled(x):          # (..., samples, time, lat, lon) -> (time, everything else): record_batch's reshape, members pooled
        x = x.reshape(-1, *x.shape[-3:])
        return x.transpose(1, 0, 2, 3).reshape(x.shape[1], -1)

    rng = np.random.default_rng(20240607)
    H, W, S, n_times = 12, 24, 2, 6
    f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)  # noqa: E731
    out = dict(numpy_version=np.__version__, n_times=n_times)
    cases = []
    for n_bins in (300, 8):
        def run(case, adds):
            """adds: list of (array or callable(histogram) -> array, i_time_start)"""
            key = f"{case}_b{n_bins}"
            cases.append(key)
            h = Counting(n_times=n_times, n_bins=n_bins)
            for i, (x, t0) in enumerate(adds):
                x = f32(x(h) if callable(x) else x)
                left, right = h.n_left, h.n_right
                v = pooled(x)
                h.add(v, i_time_start=t0)
                assert h.bin_edges.dtype == np.float32
                out[f"{key}::in{i}"] = x
                out[f"{key}::i_time_start{i}"] = t0
                out[f"{key}::minmax{i}"] = np.array([v.min(), v.max()], dtype=np.float32)
                out[f"{key}::edges{i}"] = h.bin_edges.copy()
                out[f"{key}::doublings{i}"] = np.array([h.n_left - left, h.n_right - right])
            out[f"{key}::n_adds"] = len(adds)
            out[f"{key}::n_bins"] = n_bins
            out[f"{key}::counts"] = h.counts.copy()
            assert h.counts.sum() == sum(out[f"{key}::in{i}"].size for i in range(len(adds)))
            return h

        h = run("grow", [(280.0 + 2.0 * rng.standard_normal((S, 3, H, W)), 0),
                         (283.0 + 4.0 * rng.standard_normal((S, 2, H, W)), 3),
                         (250.0 + 25.0 * rng.standard_normal((S, 3, H, W)), 1)])
        assert h.n_left >= 2 and h.n_right >= 1

        def on_edges(h):
            e = h.bin_edges
            x = rng.uniform(e[0], e[-1], size=(S, 2, H, W)).astype(np.float32).clip(e[0], e[-1])
            flat = x.reshape(-1)
            picks = rng.integers(1, n_bins, size=200)
            flat[:200] = e[picks]                 # exactly on interior edges: the bin to the right owns them
            flat[200:260] = e[-1]                 # exactly on the last edge: the last bin is closed
            flat[260:300] = e[0]
            return rng.permutation(flat).reshape(x.shape)

        run("edges", [(rng.uniform(-1.0, 1.0, size=(S, 3, H, W)), 0), (on_edges, 2), (on_edges, 4)])
        h = run("constant", [(np.full((S, 2, H, W), 2.5), 0), (np.full((S, 1, H, W), 2.5), 4),
                             (2.5 + 3.0 * rng.standard_normal((S, 3, H, W)), 2)])
        assert h.n_left + h.n_right >= 20
        E = 3
        run("stacked", [(1.0e5 + 2.5e3 * rng.standard_normal((E, S, 4, H, W)), 0),
                        (1.0e5 + 4.0e3 * rng.standard_normal((E, S, 2, H, W)), 4)])
    out["cases"] = json.dumps(cases)
    path = os.path.join(OUT, f"{tag}.npz")
    np.savez_compressed(path, **out)
    print(f"{tag}: {len(cases)} cases, {os.path.getsize(path)} bytes, saved")


def gen_time_coarsen(tag="fx_time_coarsen"):
    """The reference's own `TimeCoarsen` (src/ace_inference/inference/data_writer/time_coarsen.py) around a recording writer.
    Per grid -- 6 x 12 (HW = 72) and 5 x 7 (HW = 35) -- two windows of 2 samples as `run_inference` hands them over: 1 + 6
    times at start_timestep 0, then 6 times at start_timestep 7; targets {a}, predictions {a, b}; unit-scale Gaussians (normal
    range, no subnormals).  Per factor 1, 2, 3, 4 (six times by 4: one group and a dropped tail) every call the wrapped writer
    receives is stored: tensors, start_timestep, start_sample, times.  `batch_times` is a stand-in with the two xarray calls
    the reference makes (`isel`, `coarsen(...).mean()`) on a (sample, time) float64 array; like the tensors' unfold it drops a
    tail that does not fill a group (xarray's boundary="trim"; its default would refuse the factor 4 case)."""
    from src.ace_inference.inference.data_writer.time_coarsen import TimeCoarsen

    class Times:
        def __init__(self, values):
            self.values = np.asarray(values)

        def isel(self, indexers):
            return Times(self.values[:, indexers["time"]])

        def coarsen(self, windows):
            f, v = windows["time"], self.values
            n = v.shape[1] // f
            grouped = v[:, :n * f].reshape(v.shape[0], n, f)
            return types.SimpleNamespace(mean=lambda: Times(grouped.mean(axis=-1)))

    class Recorder:
        def __init__(self):
            self.calls = []

        def append_batch(self, target, prediction, start_timestep, start_sample, batch_times):
            self.calls.append(({k: v.clone().numpy() for k, v in target.items()},
                               {k: v.clone().numpy() for k, v in prediction.items()}, start_timestep, start_sample,
                               batch_times.values.copy()))

        def flush(self):
            pass

    g = torch.Generator(device="cpu").manual_seed(20240917)
    S, start_sample = 2, 3
    windows = ((0, 7), (7, 6))            # (start_timestep, times)
    factors = (1, 2, 3, 4)
    out = dict(factors=np.array(factors), start_sample=start_sample, window_starts=np.array([w[0] for w in windows]))
    cases = []
    for H, W in ((6, 12), (5, 7)):
        grid = f"g{H}x{W}"
        data = []
        for w, (t0, T) in enumerate(windows):
            target = {"a": torch.randn(S, T, H, W, generator=g)}
            prediction = {n: torch.randn(S, T, H, W, generator=g) for n in ("a", "b")}
            times = np.arange(t0, t0 + T, dtype=np.float64)[None, :] * 6.0 + np.array([[0.0], [1000.0]])
            data.append((target, prediction, t0, times))
            for src, d in (("target", target), ("prediction", prediction)):
                for n, v in d.items():
                    assert np.isfinite(v.numpy()).all() and (np.abs(v.numpy()) >= np.finfo(np.float32).tiny).all()
                    out[f"{grid}::w{w}::{src}::{n}"] = v.numpy()
            out[f"{grid}::w{w}::times"] = times
        for f in factors:
            case = f"{grid}_f{f}"
            cases.append(case)
            rec = Recorder()
            tc = TimeCoarsen(rec, f)
            for target, prediction, t0, times in data:
                tc.append_batch(target, prediction, t0, start_sample, Times(times))
            out[f"{case}::n_calls"] = len(rec.calls)
            for j, (tgt, pred, st, ss, bt) in enumerate(rec.calls):
                for src, d in (("target", tgt), ("prediction", pred)):
                    for n, v in d.items():
                        assert v.dtype == np.float32
                        out[f"{case}::call{j}::{src}::{n}"] = v
                out[f"{case}::call{j}::start_timestep"] = st
                out[f"{case}::call{j}::start_sample"] = ss
                out[f"{case}::call{j}::times"] = bt
    out["cases"] = json.dumps(cases)
    path = os.path.join(OUT, f"{tag}.npz")
    np.savez_compressed(path, **out)
    print(f"{tag}: {len(cases)} cases, {os.path.getsize(path)} bytes, saved")


class NoDist:
    """One process: the reductions over ranks are identities."""

    def reduce_mean(self, t):
        return t

    reduce_min = reduce_max = reduce_mean


FIELD_T, FIELD_MEMBERS = 3, 3


def _field_cases():
    """The inputs `gen_video` and `gen_zonal_mean` share, from one seed: per case a list of windows
    (i_time_start, target {name: (S, T, H, W)}, gen {name: (S, T, H, W)}), fed the way `run_inference` feeds an aggregator --
    the first window holds T + 1 times (the initial condition), later ones T, n_timesteps = 1 + 3T, T = 3 -- followed by a second
    pass with fresh data over the first two windows' times, so times 0 .. 2T get n_batches = 2 and the rest 1.  S = 1, 2, 3
    samples on a 16 x 32 grid (one variable) and on an odd 7 x 10 grid (two variables; HW % 4 != 0).  Unit-scale Gaussians with
    a per-variable offset, so bias, variance and zonal structure are all non-trivial."""
    g = torch.Generator(device="cpu").manual_seed(20241017)
    T = FIELD_T
    starts = ((0, T + 1), (T + 1, T), (2 * T + 1, T), (0, T + 1), (T + 1, T))
    cases = {}
    for (H, W), names in (((16, 32), ("a",)), ((7, 10), ("a", "b"))):
        for S in (1, 2, 3):
            lat = torch.linspace(-1.0, 1.0, H)[None, None, :, None]
            windows = []
            for t0, n in starts:
                target = {k: torch.randn(S, n, H, W, generator=g) + 3.0 * j + lat for j, k in enumerate(names)}
                gen = {k: target[k] + 0.5 * torch.randn(S, n, H, W, generator=g) + 0.25 for k in names}
                windows.append((t0, target, gen))
            cases[f"g{H}x{W}_s{S}"] = windows
    return cases, 1 + 3 * T


def _field_digest(windows):
    return sum(float(v.double().abs().sum()) for _, target, gen in windows for d in (target, gen) for v in d.values())


def _strip(label):
    return label.strip("/")


def gen_video(tag="fx_video"):
    """The reference's own `VideoAggregator` (src/ace_inference/core/aggregator/inference/video.py), with and without
    `enable_extended_videos`, on `_field_cases()` -- whose inputs and i_time_starts fx_zonal_mean.npz holds (the float64
    videos fill this file; the inputs are not stored twice, a digest of them is) --: every array of `_get_data("")` (labels without
    the leading slash; the pair as `<name>::gen` / `<name>::target`).  The plain aggregator's pair is checked here to be the
    extended one's, bit for bit, and stored once.  `min_err` / `max_err` are stored as the float32 they are (checked).
    Plus one "pooled" case: E = 3 members x S = 2 samples on the 7 x 10 grid, fed to the reference as flat (E * S, T, H, W) gen
    (member-major) with the target repeated E times -- what a member-stacked (E, S, T, H, W) gen must reproduce."""
    from src.ace_inference.core.aggregator.inference.video import VideoAggregator

    cases, n_timesteps = _field_cases()
    out = dict(n_timesteps=n_timesteps, members=FIELD_MEMBERS)

    def run(case, windows):
        ext = VideoAggregator(n_timesteps, True, dist=NoDist())
        plain = VideoAggregator(n_timesteps, False, dist=NoDist())
        for t0, target, gen in windows:
            for agg in (ext, plain):
                agg.record_batch(loss=0.0, target_data=target, gen_data=gen, i_time_start=t0)
        data, pdata = ext._get_data(""), plain._get_data("")
        assert [k for k in data if k in pdata] == list(pdata)
        labels = []
        for label, d in data.items():
            key = _strip(label)
            labels.append(key)
            assert d.gen.dtype == torch.float64
            if d.target is not None:
                assert torch.equal(d.gen, pdata[label].gen) and torch.equal(d.target, pdata[label].target)
                out[f"{case}::out::{key}::gen"] = d.gen.numpy()
                out[f"{case}::out::{key}::target"] = d.target.numpy()
            elif key.startswith(("min_err/", "max_err/")):
                a = d.gen.numpy()
                assert np.array_equal(a.astype(np.float32).astype(np.float64), a)
                out[f"{case}::out::{key}"] = a.astype(np.float32)
            else:
                out[f"{case}::out::{key}"] = d.gen.numpy()
        out[f"{case}::labels"] = json.dumps(labels)

    for case, windows in cases.items():
        out[f"{case}::inputs_digest"] = _field_digest(windows)
        run(case, windows)
    # pooled: member-stacked inputs are stored; the reference sees them flat
    g = torch.Generator(device="cpu").manual_seed(20241018)
    E, S, H, W = FIELD_MEMBERS, 2, 7, 10
    case, windows, flat = "pooled", [], []
    for t0, n in ((0, FIELD_T + 1), (FIELD_T + 1, FIELD_T), (2 * FIELD_T + 1, FIELD_T)):
        target = {k: torch.randn(S, n, H, W, generator=g) + j for j, k in enumerate(("a", "b"))}
        gen = {k: target[k][None] + 0.5 * torch.randn(E, S, n, H, W, generator=g) for k in target}
        windows.append((t0, target, gen))
        flat.append((t0, {k: v.repeat(E, 1, 1, 1) for k, v in target.items()},
                     {k: v.reshape(E * S, n, H, W) for k, v in gen.items()}))
    out[f"{case}::starts"] = np.array([w[0] for w in windows])
    out[f"{case}::names"] = json.dumps(["a", "b"])
    for i, (t0, target, gen) in enumerate(windows):
        for k in target:
            out[f"{case}::w{i}::target::{k}"] = target[k].numpy()
            out[f"{case}::w{i}::gen::{k}"] = gen[k].numpy()
    run(case, flat)
    out["cases"] = json.dumps(list(cases) + [case])
    path = os.path.join(OUT, f"{tag}.npz")
    np.savez_compressed(path, **out)
    print(f"{tag}: {len(cases) + 1} cases, {os.path.getsize(path)} bytes, saved")


def gen_zonal_mean(tag="fx_zonal_mean"):
    """The reference's own `ZonalMeanAggregator` (src/ace_inference/core/aggregator/inference/zonal_mean.py) on the inputs of
    `_field_cases()`, stored here for this fixture and for fx_video.npz (windows `<case>::w<i>::<target|gen>::<name>`,
    `<case>::starts`): per case and variable the two (n_timesteps, lat) arrays `get_logs` hands to `wandb.Image`, with its transpose-and-flip for the picture undone."""
    from src.ace_inference.core.aggregator.inference import zonal_mean as ref

    class Images:
        @staticmethod
        def Image(data, caption=None):
            return data.flip(dims=[0]).t().contiguous()       # back from the picture's orientation to (time, lat)

    ref.wandb = Images
    cases, n_timesteps = _field_cases()
    out = dict(n_timesteps=n_timesteps)
    for case, windows in cases.items():
        agg = ref.ZonalMeanAggregator(n_timesteps, dist=NoDist())
        out[f"{case}::starts"] = np.array([w[0] for w in windows])
        out[f"{case}::names"] = json.dumps(list(windows[0][1]))
        out[f"{case}::inputs_digest"] = _field_digest(windows)
        for i, (t0, target, gen) in enumerate(windows):
            for k in target:
                out[f"{case}::w{i}::target::{k}"] = target[k].numpy()
                out[f"{case}::w{i}::gen::{k}"] = gen[k].numpy()
            agg.record_batch(loss=0.0, target_data=target, gen_data=gen, target_data_norm=target, gen_data_norm=gen,
                             i_time_start=t0)
        for label, a in agg.get_logs("").items():
            assert a.dtype == torch.float32 and tuple(a.shape) == (n_timesteps, next(iter(windows[0][1].values())).shape[2])
            out[f"{case}::out::{_strip(label)}"] = a.numpy()
    out["cases"] = json.dumps(list(cases))
    path = os.path.join(OUT, f"{tag}.npz")
    np.savez_compressed(path, **out)
    print(f"{tag}: {len(cases)} cases, {os.path.getsize(path)} bytes, saved")


if __name__ == "__main__":
    torch.set_num_threads(8)
    if len(sys.argv) > 1:      # regenerate selected fixtures only: python tools/gen_golden.py gen_time_mean
        for fn in sys.argv[1:]:
            globals()[fn]()
        sys.exit(0)
    # C1: one block, 32x64, 8 channels (BASELINE.json configs[0])
    gen_sfno("fx_block_c1", SFNOConfig(in_chans=8, out_chans=8, nlat=32, nlon=64, embed_dim=8, num_layers=1,
                                       with_time_emb=True, min_time=0.0, max_time=5.0), 8, 0, 2, [1.0, 4.0], 4321, False)
    # tiny full network with conditioning, time embedding, dropout + drop path (interpolator-like)
    gen_sfno("fx_sfno_tiny", SFNOConfig(in_chans=10, out_chans=6, nlat=32, nlon=64, embed_dim=16, num_layers=3,
                                        with_time_emb=True, dropout_mlp=0.1, drop_path_rate=0.3, min_time=0.0,
                                        max_time=5.0), 8, 2, 3, [0.0, 2.0, 5.0], 4321, True)
    gen_sfno("fx_sfno_tiny_lg", SFNOConfig(in_chans=4, out_chans=4, nlat=32, nlon=64, embed_dim=8, num_layers=2,
                                           with_time_emb=False, data_grid="legendre-gauss", big_skip=False,
                                           pos_embed=False), 4, 0, 2, None, 99, False)
    t1 = gen_sample("fx_sample_tiny", hack=False, dropout=False)
    gen_sample("fx_sample_tiny_hack", hack=True, dropout=False)
    gen_sample("fx_sample_tiny_masks", hack=True, dropout=True)
    gen_sample_refine()
    gen_sample_artificial()
    gen_sample_switches()
    gen_sample_fcond()
    with open(os.path.join(OUT, "fx_trace.json"), "w") as f:
        json.dump(t1, f)
    gen_stepper()
    gen_loop()
    gen_ckpt_layout()
    gen_metrics()
    gen_time_mean()
    gen_mean_series()
    gen_mean_series_grad()
    gen_derived()
    gen_corrector()
    gen_histogram()
    gen_time_coarsen()
    gen_video()
    gen_zonal_mean()
    gen_sfno_wide_masks()
    gen_sfno_full()
    sizes = {n: os.path.getsize(os.path.join(OUT, n)) for n in sorted(os.listdir(OUT))}
    print(sizes)
