"""Shared by tests/test_field_stats_host.py and tests/test_gpu_field_stats.py: the fixtures of the reference's VideoAggregator /
ZonalMeanAggregator (tests/golden/fx_video.npz, fx_zonal_mean.npz; tools/gen_golden.py), the library's _host entry points
driven from numpy, a float64 restatement of both aggregators, and the comparison bounds.

Bounds (u = 2^-24; the device and host paths sum fp32 inputs in float64, the reference sums in fp32):
  * a mean over n rows: (n + 2) u max|x|, the worst case of the reference's own fp32 summation;
  * err_var, compared as rmse^2 = err_var / n_batches: (n + 2) u max(e^2);
  * the mean squares enter the reference's output only through gen_var = Vg / Vt, V = E[x^2] - E[x]^2.  With
    dE2 = (n + 2) u max(x^2) and dE = (n + 2) u max|x| per source: dV = dE2 + 2 max|x| dE, and to first order
    |d(Vg / Vt)| <= (dVg + |Vg / Vt| dVt) / (|Vt| - dVt); where |Vt| <= 2 dVt (one sample: Vt is rounding noise or 0 / 0) the
    ratio carries no information in either computation and is not compared;
  * a zonal mean: (W + 2) u max|x|; the error row is gen - target, so both bounds add;
  * against the float64 restatement: 1e-12 max|statistic|.
"""
import ctypes as C
import json

import numpy as np

import golden_utils as gu
from window_utils import fill_window, vp

U = 2.0 ** -24
VIDEO_STATS = ("gen_mean", "target_mean", "gen_sq", "target_sq", "err_var", "err_min", "err_max")


def cases():
    """-> {case: dict(names, windows=[(t_start, target {name: array}, gen {name: array})], n_timesteps, out={label: array},
    zonal={label: array} or None, labels=the reference's `_get_data("")` keys in its order)}; the pooled case holds
    member-stacked (E, S, T, H, W) gen."""
    zv, zz = gu.load("fx_video"), gu.load("fx_zonal_mean")
    out = {}
    for case in json.loads(str(zv["cases"])):
        src = zv if f"{case}::starts" in zv.files else zz
        names = json.loads(str(src[f"{case}::names"]))
        windows = [(int(t0), {k: src[f"{case}::w{i}::target::{k}"] for k in names},
                    {k: src[f"{case}::w{i}::gen::{k}"] for k in names}) for i, t0 in enumerate(src[f"{case}::starts"])]
        digest = sum(float(np.abs(v.astype(np.float64)).sum()) for _, t, g in windows for d in (t, g) for v in d.values())
        if src is zz:
            assert np.isclose(digest, float(zv[f"{case}::inputs_digest"]), rtol=1e-12), "fx_video was made from other inputs"
        pre = f"{case}::out::"
        video = {k[len(pre):]: zv[k] for k in zv.files if k.startswith(pre)}
        zonal = {k[len(pre):]: zz[k] for k in zz.files if k.startswith(pre)} or None
        out[case] = dict(names=names, windows=windows, n_timesteps=int(zv["n_timesteps"]), out=video, zonal=zonal,
                         labels=json.loads(str(zv[f"{case}::labels"])))
    return out


def video_args(target, gen, names, t_start, n_timesteps, acc):
    """SdyVideoArgs over contiguous numpy arrays (gen 4-D or member-stacked 5-D) and the accumulators `acc` (stat -> float64
    (nvars, n_timesteps, HW), missing = NULL); -> (args, keep-alive list)."""
    from sdy_amd._lib import SdyVideoArgs

    a = SdyVideoArgs()
    keep, (H, W) = fill_window(a.win, target, gen, names)
    a.HW, a.t_start, a.n_timesteps = H * W, t_start, n_timesteps
    for stat, buf in acc.items():
        setattr(a, stat, vp(buf))
    return a, keep


def zonal_args(target, gen, names, t_start, n_timesteps, gen_acc, target_acc):
    from sdy_amd._lib import SdyZonalArgs

    a = SdyZonalArgs()
    keep, (a.H, a.W) = fill_window(a.win, target, gen, names)
    a.t_start, a.n_timesteps = t_start, n_timesteps
    a.gen_acc, a.target_acc = vp(gen_acc), vp(target_acc)
    return a, keep


def new_video_acc(nvars, n_timesteps, HW, extended=True):
    acc = {s: np.zeros((nvars, n_timesteps, HW)) for s in (VIDEO_STATS if extended else VIDEO_STATS[:2])}
    if extended:
        acc["err_min"][:] = np.inf
        acc["err_max"][:] = -np.inf
    return acc


def host_video(case, extended=True):
    """The case through sdy_video_accumulate_host -> (acc, n_batches)."""
    import sdy_amd

    names, nt = case["names"], case["n_timesteps"]
    H, W = case["windows"][0][1][names[0]].shape[-2:]
    acc = new_video_acc(len(names), nt, H * W, extended)
    n_batches = np.zeros(nt)
    for t0, target, gen in case["windows"]:
        a, keep = video_args(target, gen, names, t0, nt, acc)
        assert sdy_amd.lib.sdy_video_accumulate_host(C.byref(a)) == 0
        n_batches[t0:t0 + a.T] += 1
    return acc, n_batches


def host_zonal(case):
    import sdy_amd

    names, nt = case["names"], case["n_timesteps"]
    S, _, H, W = case["windows"][0][1][names[0]].shape
    gen_acc, target_acc = np.zeros((len(names), S, nt, H)), np.zeros((len(names), S, nt, H))
    n_batches = np.zeros(nt)
    for t0, target, gen in case["windows"]:
        a, keep = zonal_args(target, gen, names, t0, nt, gen_acc, target_acc)
        assert sdy_amd.lib.sdy_zonal_accumulate_host(C.byref(a)) == 0
        n_batches[t0:t0 + a.T] += 1
    return gen_acc, target_acc, n_batches


def restate_video(case):
    """Both aggregators' accumulators restated in float64 numpy from the inputs: the definition the kernels are held to."""
    names, nt = case["names"], case["n_timesteps"]
    H, W = case["windows"][0][1][names[0]].shape[-2:]
    acc = new_video_acc(len(names), nt, H * W)
    for t0, target, gen in case["windows"]:
        for j, k in enumerate(names):
            t32, g32 = target[k], gen[k]
            T = t32.shape[1]
            e = (g32 - t32).astype(np.float64).reshape(-1, T, H * W)          # one fp32 subtraction (the target broadcasts)
            g, t = g32.astype(np.float64).reshape(-1, T, H * W), t32.astype(np.float64).reshape(-1, T, H * W)
            sl = slice(t0, t0 + T)
            acc["gen_mean"][j, sl] += g.mean(0)
            acc["target_mean"][j, sl] += t.mean(0)
            acc["gen_sq"][j, sl] += (g * g).mean(0)
            acc["target_sq"][j, sl] += (t * t).mean(0)
            with np.errstate(invalid="ignore", divide="ignore"):
                acc["err_var"][j, sl] += e.var(0, ddof=1) if e.shape[0] > 1 else np.full(e.shape[1:], np.nan)
            acc["err_min"][j, sl] = np.minimum(acc["err_min"][j, sl], e.min(0))
            acc["err_max"][j, sl] = np.maximum(acc["err_max"][j, sl], e.max(0))
    return acc


def restate_zonal(case):
    names, nt = case["names"], case["n_timesteps"]
    S, _, H, W = case["windows"][0][1][names[0]].shape
    gen_acc, target_acc = np.zeros((len(names), S, nt, H)), np.zeros((len(names), S, nt, H))
    for t0, target, gen in case["windows"]:
        for j, k in enumerate(names):
            T = target[k].shape[1]
            g = gen[k].astype(np.float64).mean(-1)
            gen_acc[j, :, t0:t0 + T] += g if g.ndim == 3 else g.mean(0)
            target_acc[j, :, t0:t0 + T] += target[k].astype(np.float64).mean(-1)
    return gen_acc, target_acc


def video_outputs(acc, n_batches, names, H, W):
    """The labels of VideoAggregator.get_data() from accumulators, as numpy (the pair as `<name>::gen` / `<name>::target`)."""
    n = n_batches[:, None]
    out = {}
    with np.errstate(invalid="ignore", divide="ignore"):
        for j, k in enumerate(names):
            sh = (len(n_batches), H, W)
            gen, target = acc["gen_mean"][j] / n, acc["target_mean"][j] / n
            out[f"{k}::gen"], out[f"{k}::target"] = gen.reshape(sh), target.reshape(sh)
            if "err_var" in acc:
                out[f"bias/{k}"] = (gen - target).reshape(sh)
                out[f"rmse/{k}"] = np.sqrt(acc["err_var"][j] / n).reshape(sh)
                out[f"min_err/{k}"], out[f"max_err/{k}"] = acc["err_min"][j].reshape(sh), acc["err_max"][j].reshape(sh)
                out[f"gen_var/{k}"] = ((acc["gen_sq"][j] / n - gen ** 2) / (acc["target_sq"][j] / n - target ** 2)).reshape(sh)
    return out


def zonal_outputs(gen_acc, target_acc, n_batches, names):
    n = n_batches[None, :, None]
    out = {}
    for j, k in enumerate(names):
        out[f"gen/{k}"] = (gen_acc[j] / n).mean(0)
        out[f"error/{k}"] = ((gen_acc[j] - target_acc[j]) / n).mean(0)
    return out


def _within(got, want, bound, what):
    """|got - want| <= bound where bound is finite; NaN exactly where the reference has NaN."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    bound = np.broadcast_to(np.asarray(bound, np.float64), want.shape)
    cmp = np.isfinite(bound)
    assert np.array_equal(np.isnan(got[cmp]), np.isnan(want[cmp])), f"{what}: NaN pattern differs"
    ok = cmp & ~np.isnan(want)
    if ok.any():
        err = np.abs(got[ok] - want[ok])
        worst = float((err / bound[ok]).max())
        print(f"{what}: max |diff| {float(err.max()):.3e}, {worst:.3f} of the bound")
        assert worst <= 1.0, f"{what}: {worst:.3f} of the bound"


def check_video_against_reference(case, got, tag):
    """`got`: labels as video_outputs() gives them plus target_variance(), from the host or the device path."""
    names, ref = case["names"], case["out"]
    for k in names:
        g = np.concatenate([w[2][k].astype(np.float64).ravel() for w in case["windows"]])
        t = np.concatenate([w[1][k].astype(np.float64).ravel() for w in case["windows"]])
        e2 = max(float(((w[2][k] - w[1][k]).astype(np.float64) ** 2).max()) for w in case["windows"])
        first = case["windows"][0]
        n = int(np.prod(first[2][k].shape[:-3]))      # generated rows: samples, or members x samples
        nt = first[1][k].shape[0]
        dg, dt = (n + 2) * U * np.abs(g).max(), (nt + 2) * U * np.abs(t).max()
        _within(got[f"{k}::gen"], ref[f"{k}::gen"], dg, f"{tag} {k} gen")
        _within(got[f"{k}::target"], ref[f"{k}::target"], dt, f"{tag} {k} target")
        _within(got[f"bias/{k}"], ref[f"bias/{k}"], dg + dt, f"{tag} bias/{k}")
        assert np.array_equal(got[f"min_err/{k}"], ref[f"min_err/{k}"].astype(np.float64)), f"{tag} min_err/{k}"
        assert np.array_equal(got[f"max_err/{k}"], ref[f"max_err/{k}"].astype(np.float64)), f"{tag} max_err/{k}"
        _within(got[f"rmse/{k}"] ** 2, ref[f"rmse/{k}"] ** 2, (n + 2) * U * e2, f"{tag} rmse^2/{k}")
        if n == 1:
            assert np.isnan(got[f"rmse/{k}"]).all() and np.isnan(ref[f"rmse/{k}"]).all()
        # gen_var = Vg / Vt (module docstring)
        dVg = (n + 2) * U * (g ** 2).max() + 2 * np.abs(g).max() * dg
        dVt = (nt + 2) * U * (t ** 2).max() + 2 * np.abs(t).max() * dt
        ratio, Vt = ref[f"gen_var/{k}"], got[f"_Vt/{k}"]       # (Vt: target_variance() of the path under test)
        with np.errstate(invalid="ignore", divide="ignore"):
            bound = np.where(np.abs(Vt) > 2 * dVt, (dVg + np.abs(ratio) * dVt) / (np.abs(Vt) - dVt), np.inf)
        _within(got[f"gen_var/{k}"], ratio, bound, f"{tag} gen_var/{k}")


def target_variance(acc, n_batches, names, H, W):
    """`_Vt/<name>` entries for check_video_against_reference: E[t^2] - E[t]^2 of the path under test."""
    n = n_batches[:, None]
    with np.errstate(invalid="ignore", divide="ignore"):
        return {f"_Vt/{k}": (acc["target_sq"][j] / n - (acc["target_mean"][j] / n) ** 2).reshape(len(n_batches), H, W)
                for j, k in enumerate(names)}


def check_zonal_against_reference(case, got, tag):
    for k in case["names"]:
        g = max(float(np.abs(w[2][k]).max()) for w in case["windows"])
        t = max(float(np.abs(w[1][k]).max()) for w in case["windows"])
        W = case["windows"][0][1][k].shape[-1]
        _within(got[f"gen/{k}"], case["zonal"][f"gen/{k}"], (W + 2) * U * g, f"{tag} gen/{k}")
        _within(got[f"error/{k}"], case["zonal"][f"error/{k}"], (W + 2) * U * (g + t), f"{tag} error/{k}")


def check_close(got, want, what, rel=1e-12):
    """|got - want| <= rel * max|want| over the finite entries; the same non-finite pattern."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    fin = np.isfinite(want)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got[~fin & ~np.isnan(want)],
                                                                             want[~fin & ~np.isnan(want)]), what
    if fin.any():
        scale = float(np.abs(want[fin]).max())
        err = float(np.abs(got[fin] - want[fin]).max())
        print(f"{what}: max |diff| {err:.3e} at scale {scale:.3e}")
        assert err <= rel * scale, f"{what}: {err:.3e} > {rel} * {scale:.3e}"
