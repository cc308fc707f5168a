"""Cases, float64 references, a CPU restatement and the bounds of the InstanceNorm statistics chain of the fused forward.
Shared by tests/test_gpu_instnorm.py (the kernels) and tests/test_instnorm_host.py (the restatement alone);
`python tests/instnorm_utils.py` prints the restatement's table (NOTEBOOK.md 7o).

The chain: a producer stores a tensor and leaves (S, S2) = (sum, sum of squares) over HW of every stored (image, channel)
plane in float64; a consumer turns them into the coefficients of xn = a x + d (include/sdy_amd.h):
    mean = S / HW,  var = max(S2 / HW - mean^2, 0),  rstd = 1 / sqrt(var + eps)
    a = gamma rstd (1 + scale),  d = (beta - mean gamma rstd)(1 + scale) + shift

Everything below is derived, nothing is tuned.  u = 2^-24 is float32's unit roundoff.

PRODUCERS.  The reference is the float64 sum of the kernel's own stored plane v, read back: the accuracy of the GEMM or
FFT in front of the store plays no part.  Every producer sums in float32 inside a small group and in float64 across groups;
a stored value meets at most G float32 roundings on its way into the float64 accumulator, so
    |S - S64| <= G_sum u sum |v|,      |S2 - S2_64| <= G_sq u sum v^2      (+ ACC64 = 1e-13 relative for the float64 adds)
and for the quantity the network uses, var = S2 / HW - (S / HW)^2,
    |var - var64| <= dS2 / HW + 2 |mean| dS / HW + (dS / HW)^2.
G per producer, counted from the code (`G_TABLE`; tests/test_instnorm_host.py recomputes it from `ACCUM`):
    quad   (mlp_h3.hip, pair_h3.hip, pointwise.hip gelu_stats_kernel / affine_copy_stats_kernel)
           sum:   `(v.x + v.y) + (v.z + v.w)` (common.h sdy_quad_sum; pair_h3.hip writes it out)            2 adds
           sumsq: `fmaf(v.x, v.x, v.y * v.y) + fmaf(v.z, v.z, v.w * v.w)` (sdy_quad_sumsq): product, fma, add   3
           then `psum[i] += (double)...` / `s += (double)...`: float64 from there on.
    row64  (conv_h3.hip) `row16_sum(c_ok ? (v.x + v.y) + (v.z + v.w) : 0.0f)`: the quad's 2 adds + the 4 DPP adds of
           common.h row16_sum = 6;  `(v.x * v.x + v.y * v.y) + (v.z * v.z + v.w * v.w)`: product + 2 adds + 4 = 7
           (one 64-pixel tile row = 16 lanes x 4 pixels), then `__hip_atomic_fetch_add(st, (double)s1, ...)`.
    row128 (fft360.hip, the act epilogue) `qs = sdy_quad_sum(v)` 2, `qs += sdy_quad_sum(u)` (the ring's pixels 256 .. 359 on the
           lanes < 26) 1, `row16_sum(qs)` 4 = 7;  sumsq 3 + 1 + 4 = 8 (up to 16 x 8 = 128 values), then `(double)row16_sum`.
The bound is loose against rounding (the restatement stays below 0.12 of it) and tight against structure: a pixel that is
missed, counted twice or taken from the padding of a tile moves S by |v_j| and S2 by v_j^2, about 1 / HW >= 1.2e-4 of the sums
at these grids, against G u <= 4.8e-7.

CONSUMERS (pointwise.hip instnorm_from_stats_kernel / instnorm_from_partials_kernel / instnorm_coeffs_kernel, the same
statements in all three).  The test writes exact doubles, so the reference is the formula above in exact rational
arithmetic up to the square root.  Forward error, statement by statement (u64 = 2^-53):
    `mean = S / HW; var = S2 / HW - mean * mean;`    four float64 roundings: |dvar| <= 4 u64 (S2 / HW + mean^2)
    `rstd = (float)(1.0 / sqrt(var + (double)eps));`  e_r = (1 - dvar / (var + eps))^-1/2 (1 + 3 u64)(1 + u) - 1
    `a = gamma[c] * rstd;`                            e_a0 = (1 + e_r)(1 + u) - 1
    `sc = ss[...] + 1.0f;  a = a * sc;`               e_a = (1 + e_a0)(1 + u)^2 - 1              |da| <= e_a |a|
    `d = beta[c] - (float)mean * a;`   p = mean a0:   dp <= |p| ((1 + u)^2 (1 + e_a0) - 1) + dmean |a0| (1 + u)^2 (1 + e_a0)
                                                      dd0 <= dp + u (|beta| + |p| + dp)          (fused or not)
    `d = d * sc + sh_;`                               dd <= (|sc| (dd0 (1 + u)^2 + |d0| ((1 + u)^2 - 1)))(1 + u) + u (|d0 sc| + |shift|)
Errors of the inputs (dS, dS2: a producer's bound, or float64 accumulation for sdy_instnorm_coeffs, which reads x itself and
sums in float64 throughout: ACC64 relative) enter through dvar and dmean = dS / HW.
"""
import functools
import math
import zlib
from fractions import Fraction
from typing import NamedTuple

import numpy as np

U = 2.0 ** -24
U64 = 2.0 ** -53
ACC64 = 1e-13
EPS = 1e-6
G_CAP = 12
TARGETS = (0.0, 10.0, 100.0, 1000.0)        # mean / std targets the channels cycle through
CONST_VALUE = 3.25                          # the exactly constant channel
GELU_OFF = -30.0                            # GELU(-30) = 0: a plane of zeros
GRIDS = ((8, 40), (6, 36), (45, 64), (87, 96))      # HW = 320 (5 tiles), 216 (3.375), 2880 (45), 8352 (130.5)
SDY_ERR_ARG, SDY_ERR_UNSUPPORTED, SDY_ERR_ALIGN = -1, -2, -3
FLAG_NONFINITE = 1

# accumulation structure: values of one quad, DPP lanes whose quads meet in float32, a second quad added on the lane first
ACCUM = {"quad": dict(lanes=1, tail=0), "row64": dict(lanes=16, tail=0), "row128": dict(lanes=16, tail=1)}
# (G_sum, G_sq): see the module docstring, each counted at the source line quoted there
G_TABLE = {"quad": (2, 3), "row64": (6, 7), "row128": (7, 8)}
PRODUCER_ACCUM = {"conv_h3": "row64", "mlp_h3": "quad", "pair_h3": "quad", "gelu_stats": "quad", "affine_copy": "quad",
                  "irfft_lon_act": "row128"}
# gelu_erf of common.h (Abramowitz & Stegun 7.1.26, |erfc error| <= 1.5e-7, halved by the 0.5 of GELU) plus its float32 Horner
# chain, products and blend (<= 4 u): |gelu_erf(x) - GELU(x)| <= GELU_ERF_REL |x|.  Used where a test compares the fft360
# epilogue with a host GELU of sdy_irfft_lon's output.
GELU_ERF_REL = 0.75e-7 + 4 * U


def g_from_structure(kind):
    a = ACCUM[kind]
    gs = 2 + a["tail"] + int(math.log2(a["lanes"]))
    return gs, gs + 1


# ---- cases ------------------------------------------------------------------------------------------------------------------
class Case(NamedTuple):
    producer: str
    grid: tuple          # (H, W)
    B: int
    C: int               # output channels
    form: str = ""       # conv_h3: "skip" | "enc";  gelu_stats: "nchw" | "tiled"
    cin: int = 0
    drop: float = 0.0

    @property
    def HW(self):
        return self.grid[0] * self.grid[1]

    @property
    def id(self):
        extra = "".join(f"-{k}{v}" for k, v in (("", self.form), ("cin", self.cin), ("p", self.drop)) if v)
        return f"{self.producer}-{self.grid[0]}x{self.grid[1]}-B{self.B}-C{self.C}{extra}"

    @property
    def gelu(self):
        return self.producer in ("gelu_stats", "irfft_lon_act") or self.form == "skip"


PRODUCER_CASES = (
    Case("conv_h3", (8, 40), 3, 256, "skip", 256), Case("conv_h3", (87, 96), 2, 256, "skip", 256),
    Case("conv_h3", (6, 36), 3, 256, "enc", 65), Case("conv_h3", (45, 64), 2, 256, "enc", 256),
    Case("conv_h3", (87, 96), 1, 256, "enc", 321),
    Case("mlp_h3", (6, 36), 3, 256, drop=0.0), Case("mlp_h3", (45, 64), 1, 256, drop=0.1),
    Case("mlp_h3", (87, 96), 2, 256, drop=0.1),
    Case("pair_h3", (6, 36), 3, 256, cin=65), Case("pair_h3", (87, 96), 2, 256, cin=65),
    Case("gelu_stats", (6, 36), 3, 6, "nchw"), Case("gelu_stats", (87, 96), 2, 6, "nchw"),
    Case("gelu_stats", (6, 36), 2, 6, "tiled"), Case("gelu_stats", (87, 96), 3, 6, "tiled"),
    Case("affine_copy", (8, 40), 3, 6), Case("affine_copy", (87, 96), 2, 6),
    Case("irfft_lon_act", (18, 360), 3, 48), Case("irfft_lon_act", (19, 360), 1, 16), Case("irfft_lon_act", (20, 360), 2, 16),
    Case("irfft_lon_act", (19, 360), 2, 48),
)


def roles(C, gelu):
    """(offset target per channel, index of the constant channel, index of the zero channel or None)."""
    off = np.array([TARGETS[c % 4] for c in range(C)])
    return off, C - 1, (C - 2 if gelu else None)


def gen(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def gelu64(x):
    import torch

    x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64))
    return (0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))).numpy()


@functools.lru_cache(maxsize=None)
def synthetic_planes(case: Case, C=8):
    """(B, C, HW) float32 planes with the case's grid and channel roles: N(target, 1) (through GELU for the GELU producers),
    the constant channel, the zero channel -- what the restatement is run on where no GPU is."""
    off, const, zero = roles(C, case.gelu)
    z = gen("planes", case.id).standard_normal((case.B, C, case.HW)) + off[None, :, None]
    v = gelu64(z) if case.gelu else z
    v[:, const] = CONST_VALUE
    if zero is not None:
        v[:, zero] = 0.0
    return v.astype(np.float32)


# ---- the CPU restatement of the accumulation --------------------------------------------------------------------------------
def _quad(v, fma):
    """v (..., n, 4) float32 -> float32 (sum, sumsq) of each quad as the kernels form them."""
    v0, v1, v2, v3 = (v[..., i] for i in range(4))
    s = (v0 + v1) + (v2 + v3)
    if fma:    # fmaf(a, a, b * b): the exact product (48 bits, exact in float64) plus the rounded one, rounded once
        d = np.float64
        q = ((v0.astype(d) * v0 + (v1 * v1).astype(d)).astype(np.float32) +
             (v2.astype(d) * v2 + (v3 * v3).astype(d)).astype(np.float32))
    else:
        q = (v0 * v0 + v1 * v1) + (v2 * v2 + v3 * v3)
    return s, q


def _tree16(x):
    """float32 butterfly of row16_sum over the last axis (16): pairs, quads, halves, the row."""
    for _ in range(4):
        x = x[..., 0::2] + x[..., 1::2]
    return x[..., 0]


def emulate(kind, v, nlon=360):
    """(..., HW) float32 planes -> (..., 2) float64 (S, S2) by the documented accumulation of `kind`."""
    v = np.ascontiguousarray(v, dtype=np.float32)
    lead, HW = v.shape[:-1], v.shape[-1]
    assert HW % 4 == 0
    if kind == "quad":
        s, q = _quad(v.reshape(*lead, HW // 4, 4), fma=True)
        return np.stack([s.astype(np.float64).sum(-1), q.astype(np.float64).sum(-1)], -1)
    if kind == "row64":     # one tile row = 16 lanes x 4 pixels; lanes past a ragged tile's edge contribute zeros
        pad = (-HW) % 64
        vp = np.concatenate([v, np.zeros(lead + (pad,), np.float32)], -1).reshape(*lead, -1, 16, 4)
        s, q = _quad(vp, fma=False)
        return np.stack([_tree16(s).astype(np.float64).sum(-1), _tree16(q).astype(np.float64).sum(-1)], -1)
    if kind == "row128":    # one ring = 64 lanes x 4 pixels + 26 lanes x 4 more; 16-lane rows in float32, float64 from there
        assert nlon == 360 and HW % nlon == 0
        r = v.reshape(*lead, HW // nlon, nlon)
        s, q = _quad(r[..., :256].reshape(*lead, -1, 64, 4), fma=True)
        st, qt = _quad(r[..., 256:].reshape(*lead, -1, 26, 4), fma=True)
        s, q = s.copy(), q.copy()
        s[..., :26] += st
        q[..., :26] += qt
        out = []
        for x in (s, q):
            rows = _tree16(x.reshape(*lead, -1, 4, 16)).astype(np.float64)
            ring = (rows[..., 0] + rows[..., 1]) + (rows[..., 2] + rows[..., 3])      # shfl_xor 16, then 32
            tot = np.zeros(lead)
            for k in range(ring.shape[-1]):                                             # instnorm_from_partials: in order of k
                tot = tot + ring[..., k]
            out.append(tot)
        return np.stack(out, -1)
    raise KeyError(kind)


# ---- producer bounds --------------------------------------------------------------------------------------------------------
class Sums(NamedTuple):
    S: np.ndarray
    S2: np.ndarray
    dS: np.ndarray
    dS2: np.ndarray
    var: np.ndarray
    dvar: np.ndarray
    mean: np.ndarray


def plane_sums(v, kind, HW=None):
    """float64 reference sums of the stored planes v (..., HW) and the bounds of `kind`."""
    v = np.asarray(v, dtype=np.float64)
    HW = HW or v.shape[-1]
    gs, gq = G_TABLE[kind]
    S, S2 = v.sum(-1), (v * v).sum(-1)
    sa = np.abs(v).sum(-1)
    dS, dS2 = (gs * U + ACC64) * sa, (gq * U + ACC64) * S2
    mean = S / HW
    var = S2 / HW - mean * mean
    dvar = dS2 / HW + 2 * np.abs(mean) * dS / HW + (dS / HW) ** 2
    return Sums(S, S2, dS, dS2, var, dvar, mean)


def stats_ratios(got, ref: Sums, HW):
    """(|dS| / bound, |dS2| / bound, |dvar| / bound) per slot; a zero bound with a zero error counts as 0."""
    got = np.asarray(got, dtype=np.float64)
    var = got[..., 1] / HW - (got[..., 0] / HW) ** 2

    def ratio(err, bound):
        err = np.abs(err)
        return np.where(err == 0, 0.0, err / np.maximum(bound, 1e-300))

    return ratio(got[..., 0] - ref.S, ref.dS), ratio(got[..., 1] - ref.S2, ref.dS2), ratio(var - ref.var, ref.dvar)


def check_stats(got, planes, kind, what, offsets=None):
    """Assert the three producer bounds for statistics `got` (..., 2) of stored planes (..., HW); prints and returns the worst
    |error| / bound per offset target {target: (sum, sumsq, var)} when `offsets` (per channel, the last leading axis) is given."""
    HW = planes.shape[-1]
    ref = plane_sums(planes, kind)
    assert np.isfinite(np.asarray(got)).all(), f"{what}: a statistic is not finite"
    rs, rq, rv = stats_ratios(got, ref, HW)
    table = {}
    if offsets is not None:
        for t in sorted(set(offsets.tolist())):
            m = offsets == t
            table[t] = (float(rs[..., m].max()), float(rq[..., m].max()), float(rv[..., m].max()))
    worst = (float(rs.max()), float(rq.max()), float(rv.max()))
    print(f"{what}: worst |err| / bound  sum {worst[0]:.3f}  sumsq {worst[1]:.3f}  var {worst[2]:.3f}" +
          "".join(f"  [{t:g}: {a:.3f} {b:.3f} {c:.3f}]" for t, (a, b, c) in table.items()))
    for name, r in (("sum", rs), ("sumsq", rq), ("variance", rv)):
        if not (r <= 1.0).all():
            i = np.unravel_index(np.argmax(r), r.shape)
            raise AssertionError(f"{what}: {name} of slot {tuple(int(x) for x in i)} is {float(r[i]):.3g} x its bound "
                                 f"(got {np.asarray(got)[i]}, float64 {ref.S[i]:.17g} {ref.S2[i]:.17g})")
    return table or worst


# ---- consumer reference and bound ---------------------------------------------------------------------------------------------
def consumer_ref(S, S2, HW, gamma, beta, scale=None, shift=None, eps=EPS, dS=None, dS2=None):
    """(a, d, bound_a, bound_d) as float64 arrays of S's shape (B, C): the header's formula with the variance in exact rational
    arithmetic, and the forward error bound of the module docstring.  gamma, beta (C); scale, shift (B, C) or None."""
    S, S2 = np.asarray(S, dtype=np.float64), np.asarray(S2, dtype=np.float64)
    B, Cc = S.shape
    a, d, ba, bd = (np.zeros((B, Cc)) for _ in range(4))
    epsq = Fraction(float(np.float32(eps)))
    for b in range(B):
        for c in range(Cc):
            mean_q = Fraction(float(S[b, c])) / HW
            ms_q = Fraction(float(S2[b, c])) / HW
            var_q = max(ms_q - mean_q * mean_q, Fraction(0))
            t = float(var_q + epsq)
            mean = float(mean_q)
            rstd = 1.0 / math.sqrt(t)
            g, be = float(gamma[c]), float(beta[c])
            a0 = g * rstd
            d0 = be - mean * a0
            ds = 0.0 if dS is None else float(dS[b, c])
            ds2 = 0.0 if dS2 is None else float(dS2[b, c])
            dmean = ds / HW + U64 * abs(mean)
            dvar = 4 * U64 * (float(ms_q) + mean * mean) + ds2 / HW + 2 * abs(mean) * ds / HW + (ds / HW) ** 2
            et = dvar / t
            e_r = (1.0 / math.sqrt(1.0 - et) if et < 1.0 else math.inf) * (1 + 3 * U64) * (1 + U) - 1
            e_a0 = (1 + e_r) * (1 + U) - 1
            p = abs(mean * a0)
            dp = p * ((1 + U) ** 2 * (1 + e_a0) - 1) + dmean * abs(a0) * (1 + U) ** 2 * (1 + e_a0)
            dd0 = dp + U * (abs(be) + p + dp)
            if scale is None:
                a[b, c], d[b, c], ba[b, c], bd[b, c] = a0, d0, e_a0 * abs(a0), dd0
            else:
                sc, sh = 1.0 + float(scale[b, c]), float(shift[b, c])
                a[b, c], d[b, c] = a0 * sc, d0 * sc + sh
                ba[b, c] = ((1 + e_a0) * (1 + U) ** 2 - 1) * abs(a0 * sc)
                bd[b, c] = abs(sc) * (dd0 * (1 + U) ** 2 + abs(d0) * ((1 + U) ** 2 - 1)) * (1 + U) + U * (abs(d0 * sc) + abs(sh))
    return a, d, ba, bd


def check_coeffs(a_got, d_got, ref, what):
    """|a - a_ref| <= bound_a and |d - d_ref| <= bound_d for ref = consumer_ref(...); prints and returns the worst ratios."""
    a, d, ba, bd = ref
    a_got, d_got = np.asarray(a_got, dtype=np.float64).reshape(a.shape), np.asarray(d_got, dtype=np.float64).reshape(d.shape)
    assert np.isfinite(a_got).all() and np.isfinite(d_got).all(), f"{what}: a coefficient is not finite"
    ea, ed = np.abs(a_got - a), np.abs(d_got - d)
    ra = np.where(ea == 0, 0.0, ea / np.maximum(ba, 1e-300))
    rd = np.where(ed == 0, 0.0, ed / np.maximum(bd, 1e-300))
    print(f"{what}: worst |da| / bound {float(ra.max()):.3f}, |dd| / bound {float(rd.max()):.3f}, "
          f"worst |da / a| {float((ea / np.maximum(np.abs(a), 1e-300)).max()):.2e}")
    for name, r in (("a", ra), ("d", rd)):
        if not (r <= 1.0).all():
            i = np.unravel_index(np.argmax(r), r.shape)
            raise AssertionError(f"{what}: {name} of slot {tuple(int(x) for x in i)} is {float(r[i]):.3g} x its bound "
                                 f"(a {a_got[i]!r} vs {a[i]!r}, d {d_got[i]!r} vs {d[i]!r})")
    return float(ra.max()), float(rd.max())


def exact_sums(x):
    """Correctly rounded float64 (S, S2) of float32 planes x (B, C, HW) (math.fsum; the squares of floats are exact doubles)."""
    x = np.asarray(x, dtype=np.float64)
    B, Cc, _ = x.shape
    S = np.array([[math.fsum(x[b, c]) for c in range(Cc)] for b in range(B)])
    S2 = np.array([[math.fsum(x[b, c] * x[b, c]) for c in range(Cc)] for b in range(B)])
    return S, S2


# ---- what the network sees: a x + d ----------------------------------------------------------------------------------------
def norm_error(stats, x):
    """Relative L2 error of a x + d (a, d from `stats` by the float64 formula, rounded to float32, gamma = 1, beta = 0, the
    product in float32) against the float64 normalisation of the float32 planes x (..., HW)."""
    x64 = np.asarray(x, dtype=np.float64)
    HW = x64.shape[-1]

    def coeffs(S, S2):
        mean = S / HW
        rstd = 1.0 / np.sqrt(np.maximum(S2 / HW - mean * mean, 0.0) + float(np.float32(EPS)))
        return rstd, -mean * rstd

    a64, d64 = coeffs(x64.sum(-1), (x64 * x64).sum(-1))
    want = a64[..., None] * x64 + d64[..., None]
    a, d = coeffs(np.asarray(stats)[..., 0], np.asarray(stats)[..., 1])
    got = (a.astype(np.float32)[..., None] * np.asarray(x, np.float32) + d.astype(np.float32)[..., None]).astype(np.float64)
    return np.sqrt(((got - want) ** 2).sum(-1) / (want ** 2).sum(-1))


def torch_instance_norm_error(x):
    """The same number for torch's float32 instance_norm on the CPU (what the reference network runs)."""
    import torch

    xt = torch.from_numpy(np.asarray(x, np.float32))
    lead = xt.shape[:-1]
    got = torch.nn.functional.instance_norm(xt.reshape(1, -1, xt.shape[-1]), eps=EPS).reshape(*lead, -1).double().numpy()
    x64 = np.asarray(x, dtype=np.float64)
    mean = x64.mean(-1, keepdims=True)
    want = (x64 - mean) / np.sqrt(x64.var(-1, keepdims=True) + float(np.float32(EPS)))
    return np.sqrt(((got - want) ** 2).sum(-1) / (want ** 2).sum(-1))


def offset_planes(HW, n=8):
    """(4, n, HW) float32 planes N(target, 1) for the four mean / std targets (the a x + d table)."""
    z = gen("offset planes", HW).standard_normal((1, n, HW))
    return (z + np.array(TARGETS)[:, None, None]).astype(np.float32)


# ---- device buffers ---------------------------------------------------------------------------------------------------------
GUARD = 20480     # elements of NaN on both sides: more than one 64-pixel tile of 256 channels, or two rings of 48 channels


class Buf:
    """A device tensor `t` of `shape` and `dtype` inside a larger allocation with GUARD elements of NaN on both sides
    (`offset` more in front: a pointer `offset` elements off its natural boundary that is still in bounds).  `fill`: None
    (NaN: an output), a number, or a CPU tensor / array to copy."""

    def __init__(self, shape, fill=None, dtype=None, offset=0):
        import torch

        dtype = dtype or torch.float32
        n = math.prod(shape)
        self.raw = torch.full((n + 2 * GUARD + offset,), float("nan"), dtype=dtype, device="cuda")
        self.lo, self.hi = GUARD + offset, GUARD + offset + n
        self.t = self.raw[self.lo:self.hi].view(shape)
        if fill is not None:
            if isinstance(fill, (int, float)):
                self.t.fill_(fill)
            else:
                self.t.copy_(torch.as_tensor(fill).reshape(shape).to(dtype))
        self.before = self.t.clone()

    @property
    def ptr(self):
        return self.t.data_ptr()

    def guards_intact(self):
        import torch

        return bool(torch.isnan(self.raw[:self.lo]).all()) and bool(torch.isnan(self.raw[self.hi:]).all())

    def unchanged(self):
        return self.guards_intact() and bits_equal(self.t, self.before)


def bits_equal(a, b):
    import torch

    it = torch.int64 if a.dtype == torch.float64 else torch.int32
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(it).cpu(), b.contiguous().view(it).cpu())


def untile(zt, C, HW):
    """tile-major (B, ceil(HW / 64), C, 64) -> ((B, C, HW), the padding past HW of the last tile (B, C, pad))."""
    B, T = zt.shape[0], zt.shape[1]
    full = zt.permute(0, 2, 1, 3).reshape(B, C, T * 64)
    return full[:, :, :HW], full[:, :, HW:]


# ---- the restatement's table ------------------------------------------------------------------------------------------------
def restatement_table():
    """{case id: {target: worst (sum, sumsq, var) |error| / bound}} of the restatement on the synthetic planes."""
    out = {}
    for case in PRODUCER_CASES:
        kind = PRODUCER_ACCUM[case.producer]
        v = synthetic_planes(case)
        off, _, _ = roles(v.shape[1], case.gelu)
        ref = plane_sums(v, kind)
        rs, rq, rv = stats_ratios(emulate(kind, v, case.grid[1]), ref, case.HW)
        out[case.id] = {t: (float(rs[:, off == t].max()), float(rq[:, off == t].max()), float(rv[:, off == t].max()))
                        for t in TARGETS}
    return out


if __name__ == "__main__":
    print("restatement, worst |error| / bound per mean / std target (sum sumsq var):")
    for cid, row in restatement_table().items():
        print(f"  {cid:44s}" + "".join(f"  {t:g}: {a:.3f} {b:.3f} {c:.3f}" for t, (a, b, c) in row.items()))
    print("relative L2 error of a x + d against float64 (worst of 8 planes), restatement | torch float32 instance_norm:")
    for kind, HW in (("quad", 320), ("row64", 320), ("quad", 8352), ("row64", 8352), ("row128", 19 * 360), ("quad", 64800),
                     ("row64", 64800), ("row128", 64800)):
        x = offset_planes(HW)
        e = norm_error(emulate(kind, x), x).max(-1)
        r = torch_instance_norm_error(x).max(-1)
        print(f"  {kind:7s} HW {HW:6d}" + "".join(f"  {t:g}: {e[i]:.1e} | {r[i]:.1e}" for i, t in enumerate(TARGETS)))
