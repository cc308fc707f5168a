"""Plain torch restatements of the stepper / aggregator kernels of csrc/pointwise.hip, from the formulas in include/sdy_amd.h
and the comments next to the kernels.  Shared by tests/test_gpu_window_kernels.py (float64 references on the device's inputs)
and tests/test_window_kernels_host.py (the float32 yardsticks below, checked on the CPU).

Reductions are compared relative to the float64 sum of the ABSOLUTE values of a sum's terms, so that a signed sum (bias) is
held as tightly as a positive one.  The coefficient is not chosen: YARD[(kernel, M)] is the error, in that measure, of a torch
float32 restatement of the kernel's per-pixel arithmetic in the kernel's own order (sequential member loop, sequential pair
loop; pixels summed in float64, as the kernels do) against the same arithmetic in float64, measured on the CPU on exactly the
cases the GPU tests run (`measure_yardsticks()`: the largest value over the two shapes, every plane and every sum of the
kernel, rounded UP to two digits).  A kernel gets KERNEL_FACTOR = 4 times that: the factor covers FMA contraction of the
per-pixel arithmetic and another order of the float64 partial sums.  tests/test_window_kernels_host.py re-measures and fails
if a restatement leaves its own yardstick."""
import functools

import torch

U = 2.0 ** -24                      # unit roundoff of fp32: one operation errs by at most U * |its exact result|
KERNEL_FACTOR = 4.0
SHAPES = ((5, 12), (9, 116), (67, 248))       # HW4 = 15 | 261 = one workgroup + 5 threads | 16616 px = 65 workgroups of 256
ENS_SHAPES = SHAPES[1:]
ENS_M = (1, 2, 25, 64)
B, T1 = 3, 4
N_SAMPLE, T_ENS = 2, 3
MEANS = (0.3, -2.0, 250.0, 1.1, -40.0)
STDS = (1.7, 0.01, 40.0, 0.5, 3.0)

# Measured by measure_yardsticks() (`python tests/window_kernels_utils.py`, torch CPU, the cases of this file; NOTEBOOK.md 7j):
#   lp_rel_terms                     2.307e-08
#   metrics = series = grad   M = 1  5.155e-09    M = 2  6.936e-09    M = 25  2.312e-08    M = 64  5.085e-08
# (the three ensemble entry points share their worst sum, one of the first four).  Each constant is the measured value rounded
# UP to two digits; a kernel is allowed KERNEL_FACTOR times it.
YARD = {("lp", 0): 2.4e-08}
for _k in ("metrics", "series", "grad"):
    YARD.update({(_k, 1): 5.2e-09, (_k, 2): 7.0e-09, (_k, 25): 2.4e-08, (_k, 64): 5.1e-08})
N_SUMS = {"metrics": 4, "series": 8, "grad": 10}


def f32(v):
    """The float32 value of a Python number, as a float64 scalar tensor (what the kernel receives in its argument structure)."""
    return torch.tensor(v, dtype=torch.float32).double()


# ---- LpLoss terms -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def lp_case(H, W, nvars=3):
    """gen (B, nvars, HW) normalised prediction, data[v] (B, T1, HW) denormalised targets: independent normals (0.3, 1.7) in the
    normalised space, so no term (gen - target_norm)^2 is a difference of nearly equal numbers."""
    g = torch.Generator(device="cpu").manual_seed(1000 + H * W)
    gen = 0.3 + 1.7 * torch.randn(B, nvars, H * W, generator=g)
    data = [(0.3 + 1.7 * torch.randn(B, T1, H * W, generator=g)) * STDS[v] + MEANS[v] for v in range(nvars)]
    return gen, data


def lp_terms(gen, data, t, dtype):
    """(B, nvars, HW, 2) float64: (gen - y)^2 and y^2 with y = (x - mean) / std and d = gen - y evaluated in `dtype`, the
    squares in float64 (lp_terms_kernel: `(double)d * d`)."""
    out = []
    for v, x in enumerate(data):
        m, s = torch.tensor(MEANS[v], dtype=torch.float32).to(dtype), torch.tensor(STDS[v], dtype=torch.float32).to(dtype)
        y = (x[:, t].to(dtype) - m) / s
        d = gen[:, v].to(dtype) - y
        out.append(torch.stack([d.double() ** 2, y.double() ** 2], dim=-1))
    return torch.stack(out, dim=1)


def lp_sums(terms):
    """terms (B, nvars, HW, 2) -> (B, 2) sums; all terms are squares, so the sums are their own absolute sums."""
    return terms.sum(dim=(1, 2))


# ---- ensemble diagnostics -----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ens_case(M, H, W):
    """pred (M, n_sample, T, H, W), truth (n_sample, T, H, W): independent normals (0.3, 1.7); weights (H, W) non-uniform."""
    g = torch.Generator(device="cpu").manual_seed(77 * M + H * W)
    pred = 0.3 + 1.7 * torch.randn(M, N_SAMPLE, T_ENS, H, W, generator=g)
    truth = 0.3 + 1.7 * torch.randn(N_SAMPLE, T_ENS, H, W, generator=g)
    w = 0.2 + torch.rand(H, W, generator=g)
    return pred, truth, w


def gradient_magnitude(x):
    """|grad x| over the last two axes as torch.gradient defines it with unit spacing and edge_order 1 (include/sdy_amd.h):
    (x[i+1] - x[i-1]) / 2 inside, x[1] - x[0] and x[n-1] - x[n-2] at the edges, longitude not periodic; in x's dtype."""
    gy, gx = torch.empty_like(x), torch.empty_like(x)
    gy[..., 1:-1, :] = (x[..., 2:, :] - x[..., :-2, :]) * 0.5
    gy[..., 0, :] = x[..., 1, :] - x[..., 0, :]
    gy[..., -1, :] = x[..., -1, :] - x[..., -2, :]
    gx[..., :, 1:-1] = (x[..., :, 2:] - x[..., :, :-2]) * 0.5
    gx[..., :, 0] = x[..., :, 1] - x[..., :, 0]
    gx[..., :, -1] = x[..., :, -1] - x[..., :, -2]
    return torch.sqrt(gy * gy + gx * gx)


def ens_terms(pred, truth, w, dtype):
    """Per-pixel terms of the ten sums of sdy_ensemble_series_grad, (n_sample, T, H, W, 10) float64 (the first four are those of
    sdy_ensemble_metrics, the first eight those of sdy_ensemble_series):
      w (mean - t)^2 | w var (unbiased; 0 for M = 1) | w fair CRPS (= mean |x - t| for M = 1) | w (mean - t) | w mean | w mean^2 |
      w t | w t^2 | w |grad t| | w sum_m |grad x_m|
    mean, var, CRPS and the gradient magnitudes are evaluated in `dtype` in the kernels' order -- members summed one after the
    other, the pairs (m, n > m) one after the other into ONE accumulator --, the products with w in float64 as the kernels do."""
    M = pred.shape[0]
    x, t = pred.to(dtype), truth.to(dtype)
    mean = torch.zeros_like(t)
    gsum = torch.zeros_like(t)
    for m in range(M):
        mean = mean + x[m]
        gsum = gsum + gradient_magnitude(x[m])
    mean = mean / torch.tensor(float(M), dtype=dtype)
    var, skill, pair = torch.zeros_like(t), torch.zeros_like(t), torch.zeros_like(t)
    for m in range(M):
        d = x[m] - mean
        var = var + d * d
        skill = skill + (x[m] - t).abs()
        for n in range(m + 1, M):
            pair = pair + (x[m] - x[n]).abs()
    if M > 1:
        var = var / torch.tensor(float(M - 1), dtype=dtype)
        crps = skill / torch.tensor(float(M), dtype=dtype) - pair / torch.tensor(float(M * (M - 1)), dtype=dtype)
    else:
        var, crps = torch.zeros_like(t), skill
    e = mean - t
    wd = w.double()
    e, var, crps, mean, gsum, gt, t = (v.double() for v in (e, var, crps, mean, gsum, gradient_magnitude(t), t))
    return torch.stack([wd * e * e, wd * var, wd * crps, wd * e, wd * mean, wd * (mean * mean), wd * t, wd * (t * t), wd * gt,
                        wd * gsum], dim=-1)


def ens_sums(terms):
    """terms (n_sample, T, H, W, 10) -> ((n_sample, T, 10) sums, (n_sample, T, 10) sums of absolute values)."""
    return terms.sum(dim=(2, 3)), terms.abs().sum(dim=(2, 3))


@functools.lru_cache(maxsize=None)
def ens_reference(M, H, W):
    """(sums, absolute sums) of the float64 restatement on ens_case(M, H, W): the expected values of all three entry points."""
    pred, truth, w = ens_case(M, H, W)
    return ens_sums(ens_terms(pred, truth, w, torch.float64))


@functools.lru_cache(maxsize=None)
def ens_restated32(M, H, W):
    """The same sums with the per-pixel arithmetic in float32: the yardstick's subject."""
    pred, truth, w = ens_case(M, H, W)
    return ens_sums(ens_terms(pred, truth, w, torch.float32))[0]


# ---- the yardsticks -------------------------------------------------------------------------------------------------------
def lp_yardstick():
    worst = 0.0
    for H, W in SHAPES:
        gen, data = lp_case(H, W)
        for t in (0, T1 - 1):
            s64, s32 = lp_sums(lp_terms(gen, data, t, torch.float64)), lp_sums(lp_terms(gen, data, t, torch.float32))
            worst = max(worst, float(((s32 - s64).abs() / s64).max()))
    return worst


def ens_yardstick(kernel, M):
    nq, worst = N_SUMS[kernel], 0.0
    for H, W in ENS_SHAPES:
        s64, a64 = ens_reference(M, H, W)
        s32 = ens_restated32(M, H, W)
        rel = (s32 - s64).abs()[..., :nq] / a64[..., :nq].clamp_min(1e-300)
        worst = max(worst, float(rel.max()))
    return worst


def measure_yardsticks():
    out = {("lp", 0): lp_yardstick()}
    for M in ENS_M:
        for kernel in N_SUMS:
            out[(kernel, M)] = ens_yardstick(kernel, M)
    return out


if __name__ == "__main__":      # python tests/window_kernels_utils.py: the table of NOTEBOOK.md section 7j
    for k, v in measure_yardsticks().items():
        print(k, f"{v:.3e}")
