"""Helpers of the dry-air conservation tests: the fixture of the reference's own functions (tests/golden/fx_conservation.npz,
written by tools/gen_golden_conservation.py), a float64 torch restatement of the series (the checker at sizes the fixture cannot
hold; held to the fixture's `ref64` by tests/test_conservation_host.py), timelines with the fixture's magnitudes at any size, and
a driver of the host entry point `sdy_dry_air_series_host`.  The parity rule is the corrector's: corrector_utils.parity_bound."""
import ctypes as C
import json

import torch

import corrector_utils as cu
import golden_utils as gu

WATER = cu.WATER
AK8 = [3.0, 5238.4, 11815.8, 17263.1, 19929.5, 17023.4, 8970.5, 1537.5, 0.0]
BK8 = [0.0, 0.0, 0.0115, 0.0781, 0.2034, 0.4004, 0.6513, 0.9065, 1.0]
LEVELS = {1: (AK8[::8], BK8[::8]), 2: (AK8[::4], BK8[::4]), 8: (AK8, BK8)}
LOG_KEYS = ["one_step/surface_pressure_due_to_dry_air/target", "one_step/surface_pressure_due_to_dry_air/gen"]


class Sigma:
    def __init__(self, ak, bk):
        self.ak, self.bk = ak, bk


_Z = None


def fixture():
    global _Z
    if _Z is None:
        z = gu.load("fx_conservation")
        _Z = (z, json.loads(str(z["sets"])), json.loads(str(z["facts"])))
    return _Z


def set_names():
    return [s["name"] for s in fixture()[1]]


def set_data(name):
    """-> dict(meta, ak, bk, area, gen, target, ref32, ref64): CPU tensors; ref*[side] = dict(gm, absdiff, mean), and
    ref*["dry_air_loss" | "conservation_loss" | "logs"]."""
    z, sets, _ = fixture()
    meta = next(s for s in sets if s["name"] == name)
    t = lambda k: torch.from_numpy(z[k])  # noqa: E731
    d = dict(meta=meta, ak=t(f"{name}::ak"), bk=t(f"{name}::bk"), area=t(f"{name}::area"))
    for side in ("gen", "target"):
        d[side] = {n: t(f"{name}::{side}::{n}") for n in meta["names"]}
    for ref in ("ref32", "ref64"):
        d[ref] = {side: {k: t(f"{name}::{side}::{ref}::{k}") for k in ("gm", "absdiff", "mean")} for side in ("gen", "target")}
        d[ref]["dry_air_loss"] = t(f"{name}::{ref}::dry_air_loss")
        d[ref]["conservation_loss"] = t(f"{name}::{ref}::conservation_loss")
        d[ref]["logs"] = {k: t(f"{name}::{ref}::logs::{k}") for k in LOG_KEYS}
    return d


def batches(d):
    """The two batches the fixture's aggregator saw: [(lo, hi), (lo, hi)]."""
    B, split = d["meta"]["B"], d["meta"]["split"]
    return [(0, split), (split, B)] if B > 1 else [(0, 1), (0, 1)]


# ---- float64 restatement -------------------------------------------------------------------------------------------------
def series64(data, area, ak, bk, dtype=torch.float64):
    """(gm (B, T), absdiff (T - 1,), mean) of `(B, T, H, W)` data, written from the issue's formulas; dtype=torch.float32: the
    same evaluated in float32, sums included (the stand-in for the reference's fp32 error at sizes the fixture cannot hold)."""
    gm = cu.wmean(cu.dry64(data, torch.as_tensor(ak), torch.as_tensor(bk), dtype), area)
    absdiff = gm.diff(dim=-1).abs().mean(dim=0)
    return gm, absdiff, absdiff.mean()


def levels_for(K):
    ak, bk = LEVELS[K]
    return torch.tensor(ak), torch.tensor(bk)


def timeline(B, T, K, H, W, seed, drift=15.0):
    """fp32 CPU tensors (B, T, H, W) with the magnitudes of corrector_utils.fields: every step adds `drift` Pa and 200 Pa of
    noise to PRESsfc and changes the water by 5 %."""
    g = torch.Generator().manual_seed(seed)
    q_scale = torch.logspace(-6, -2, K) if K > 1 else torch.tensor([1e-2])
    d = {}
    for k in range(K):
        steps = [q_scale[k] * (1.0 + torch.rand(B, H, W, generator=g))]
        for _ in range(T - 1):
            steps.append(steps[-1] * (1.0 + 0.05 * torch.randn(B, H, W, generator=g)))
        d[f"{WATER}{k}"] = torch.stack(steps, dim=1)
    steps = [1.0e5 + 3.0e3 * torch.randn(B, H, W, generator=g)]
    for _ in range(T - 1):
        steps.append(steps[-1] + drift + 200.0 * torch.randn(B, H, W, generator=g))
    d["PRESsfc"] = torch.stack(steps, dim=1)
    return d


# ---- the host entry point ----------------------------------------------------------------------------------------------
def var(slot, t, channel=0, mean=0.0, std=1.0):
    """`t`: (B, T, H, W), any strides along B and T."""
    slot.base, slot.stride_b, slot.stride_t = t.data_ptr(), t.stride(0), t.stride(1)
    slot.channel, slot.mean, slot.std = channel, mean, std


def host_args(water, ps, area, ak, bk, stats=None, channels=None):
    """-> (args, outputs (gm (B, T), absdiff (T - 1,), mean (1,)), keep): a complete argument block on host memory."""
    from sdy_amd import _lib

    B, T, H, W = ps.shape
    a = _lib.SdyDryAirArgs()
    a.B, a.T, a.HW, a.K = B, T, H * W, len(water)
    for k in range(len(ak)):
        a.ak[k], a.bk[k] = float(ak[k]), float(bk[k])
    area = area.contiguous()
    a.area = area.data_ptr()
    for i, t in enumerate(list(water) + [ps]):
        var(a.q[i] if i < len(water) else a.ps, t, 0 if channels is None else channels[i], *((0.0, 1.0) if stats is None else stats[i]))
    gm = torch.full((B, T), float("nan"), dtype=torch.float64)
    absdiff = torch.full((max(T - 1, 0),), float("nan"), dtype=torch.float64)
    mean = torch.full((1,), float("nan"), dtype=torch.float64)
    a.gm, a.absdiff, a.mean_absdiff = gm.data_ptr(), absdiff.data_ptr() if T > 1 else None, mean.data_ptr()
    return a, (gm, absdiff, mean), (area, water, ps)


def host_series(sdy, data, area, ak, bk, expect=0):
    """`sdy_dry_air_series_host` on a dict of CPU tensors (B, T, H, W) -> (gm, absdiff, mean (1,))."""
    water = [data[n] for n in cu.water_names(data)]
    a, out, keep = host_args(water, data[cu.pick(data, "ps")], area, ak, bk)
    assert sdy.lib.sdy_dry_air_series_host(C.byref(a)) == expect
    return out


def check_parity(ours, ref32, ref64, c, label):
    """`ours`, `ref32`, `ref64`: dict(gm, absdiff, mean); prints every figure before it asserts.  -> largest error ratio."""
    worst = 0.0
    for k in ("gm", "absdiff", "mean"):
        o = torch.as_tensor(ours[k]).double().reshape(ref64[k].shape)
        err = float((o - ref64[k]).abs().max())
        ratio = cu.error_ratio(o, ref32[k], ref64[k])
        bound = cu.parity_bound(ref32[k], ref64[k], c)
        print(f"{label} {k}: err {err:.3e} ref32 err {float((ref32[k].double() - ref64[k]).abs().max()):.3e} ratio {ratio:.3f} "
              f"bound {bound:.3e}")
        assert err <= bound, (label, k)
        worst = max(worst, ratio) if ratio == ratio else worst
    return worst
