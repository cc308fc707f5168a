"""Shared builders for the parity tests: a product network and an oracle network with the same weights."""
import torch

from oracle.philox import drop_path_keep, element_keep_mask, element_keep_mask_torch
from oracle.dyffusion import OracleDYffusion
from oracle.sfno import OracleSFNO, SFNOConfig, make_state_dict


def make_pair(cfg: SFNOConfig, n_in: int, n_cond: int, seed: int = 4321, net_seed: int = 99, gemm_mode=None):
    """(product net on cuda, oracle net) sharing a 'trained-like' state_dict.  `gemm_mode`: the product network's kernel
    family ("h3" | "f32"); None keeps the network's own default ($SDY_GEMM_MODE or "h3")."""
    import sdy_amd

    assert n_in + n_cond == cfg.in_chans
    sd = make_state_dict(cfg, seed=seed)
    net = sdy_amd.SphericalFourierNeuralOperatorNet(
        num_input_channels=n_in, num_output_channels=cfg.out_chans, num_conditional_channels=n_cond,
        spatial_shape_in=(cfg.nlat, cfg.nlon), embed_dim=cfg.embed_dim, num_layers=cfg.num_layers,
        mlp_ratio=cfg.mlp_ratio, dropout_mlp=cfg.dropout_mlp, drop_path_rate=cfg.drop_path_rate,
        with_time_emb=cfg.with_time_emb, data_grid=cfg.data_grid, big_skip=cfg.big_skip, pos_embed=cfg.pos_embed,
        seed=net_seed, time_dim_mult=cfg.time_dim_mult, gemm_mode=gemm_mode,
    )
    net.load_state_dict(sd, strict=True)
    if cfg.with_time_emb:
        net.set_min_max_time(cfg.min_time, cfg.max_time)
    return net, OracleSFNO(cfg, sd), sd


class PhiloxMasks:
    """Oracle-side mask provider reproducing the device dropout stream (include/sdy_amd.h, 'Dropout stream')."""

    def __init__(self, cfg: SFNOConfig, seed: int, batch_offset: int = 0):
        self.cfg, self.seed, self.batch_offset = cfg, seed, batch_offset
        self.call = 0
        self.rows = None      # optional: global trajectory index of every batch row (overrides batch_offset + b)
        self.device = None    # "cuda": evaluate the (torch restatement of the) stream on the GPU -- full-size, full-depth tests

    def __call__(self, kind, layer, shape):
        c = self.cfg
        if kind == "drop_path":
            keep = drop_path_keep(self.seed, self.call, layer, c.drop_path_rates[layer], shape[0], self.batch_offset,
                                  self.rows)
            return torch.from_numpy(keep).reshape(-1, 1, 1, 1)
        B, C, H, W = shape
        k = 0 if kind == "mlp_hidden" else 1
        if self.device is not None:
            return element_keep_mask_torch(self.seed, self.call, layer, k, c.dropout_mlp, B, C, H, W, self.batch_offset,
                                           self.rows, device=self.device)
        return torch.from_numpy(element_keep_mask(self.seed, self.call, layer, k, c.dropout_mlp, B, C, H, W,
                                                  self.batch_offset, self.rows))


class SliceErrors:
    """Relative L2 error of a batched result per slice -- (batch row, channel) for fields, (batch row, degree) for spectral
    tensors -- next to the global one.  A global relative L2 over B rows divides the error of one wrong row by about sqrt(B);
    the worst slice does not.  Chunks of rows are added in order (`rows`: their batch indices, default consecutive), the
    sums are float64 on the tensors' device."""

    def __init__(self, keep=(0, 1), what="(row, channel)"):
        self.keep, self.what = keep, what
        self.d2, self.r2, self.rows = [], [], []

    def add(self, got, ref, rows=None):
        got = torch.view_as_real(got) if got.is_complex() else got
        ref = torch.view_as_real(ref) if ref.is_complex() else ref
        g, r = got.to(ref.device, torch.float64), ref.to(torch.float64)
        dims = [d for d in range(r.dim()) if d not in self.keep]
        self.d2.append(((g - r) ** 2).sum(dims).cpu())
        self.r2.append((r * r).sum(dims).cpu())
        n0 = sum(len(x) for x in self.rows)
        self.rows.append(list(range(n0, n0 + r.shape[0])) if rows is None else list(rows))

    def result(self):
        """(global relative L2, worst slice's relative L2, index of the worst slice with its batch row)"""
        d2, r2 = torch.cat(self.d2), torch.cat(self.r2)
        rows = [b for x in self.rows for b in x]
        per = (d2 / r2.clamp_min(1e-300)).sqrt()
        i = int(per.reshape(-1).argmax())
        idx = [int(v) for v in torch.unravel_index(torch.tensor(i), per.shape)]
        idx[0] = rows[idx[0]]
        return float((d2.sum() / r2.sum().clamp_min(1e-300)).sqrt()), float(per.max()), tuple(idx)

    def check(self, name, tol_global, tol_slice):
        glob, worst, idx = self.result()
        print(f"[slices] {name}: global {glob:.3e}, worst {self.what} slice {worst:.3e} at {idx}")
        assert glob < tol_global, f"{name}: global rel L2 {glob:.3e} >= {tol_global:.1e} (worst slice {worst:.3e} at {idx})"
        assert worst < tol_slice, f"{name}: worst {self.what} slice {idx}: rel L2 {worst:.3e} >= {tol_slice:.1e} " \
                                  f"(global {glob:.3e})"
        return glob, worst


def oracle_sampling_chain(fcfg: SFNOConfig, fsd, icfg: SFNOConfig, isd, dropout_seed: int, x0, forc, dtype, horizon: int):
    """One DYffusion sampling pass of the oracle's op sequence in `dtype`, evaluated by torch on the GPU
    (OracleSFNO(device="cuda")): forecaster weights `fsd`, interpolator weights `isd` replaying the Philox dropout stream of
    `dropout_seed` (call number = interpolator call index), initial condition `x0` and static forcing `forc`.  float64 is the
    yardstick of the chain-error tests.  Returns {"t<k>_preds": CPU tensor}."""
    fora, iora = OracleSFNO(fcfg, fsd, dtype=dtype, device="cuda"), OracleSFNO(icfg, isd, dtype=dtype, device="cuda")
    masks = PhiloxMasks(icfg, seed=dropout_seed)
    masks.device = "cuda"
    n = {"i": 0}

    def ora_i(x, time, condition=None, static_condition=None):
        masks.call = n["i"]
        n["i"] += 1
        return iora(x, time=time, condition=condition, static_condition=static_condition, mask_fn=masks)

    o = OracleDYffusion(lambda x, time, condition=None, static_condition=None: fora(
        x, time=time, condition=condition, static_condition=static_condition), ora_i, timesteps=horizon)
    out = {k: v.cpu() for k, v in o.sample(x0.cuda().to(dtype), static_condition=forc.cuda()).items()}
    del fora, iora
    torch.cuda.empty_cache()
    return out
