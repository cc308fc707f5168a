"""Shared by tests/test_member_gram_host.py and tests/test_gpu_member_gram.py: a driver of sdy_member_gram_host from numpy, the
Gram matrix in EXACT arithmetic on the fp32 inputs (fractions.Fraction, and the same in scaled Python integers for the larger
shapes), int64 and float64 restatements, a direct float64 restatement of the field scores from the fields (not through the
Gram), and the bounds.

Bound of a computed entry against the exact one.  Every a_i is exact in float64 (a difference of two fp32 values).  A term
w a_i a_j takes two roundings (w a_i, then times a_j; each at most u = 2^-53 relative), and a sum of HW terms in ANY order adds
at most (HW - 1) u (1 + O(HW u)) times the sum of the absolute terms; the padding points and the waves' and chunks' partial
sums are part of that "any order".  So for the device and for the host twin alike
    |Gamma_hat[i][j] - Gamma[i][j]| <= (HW + 4) 2^-53 sum_p w |a_i a_j|,
and two computed values differ by at most twice that."""
import ctypes as C
from fractions import Fraction

import numpy as np

from window_utils import fill_window, vp


def entries(N):
    return N * (N + 1) // 2


def index(i, j, N):
    """sdy_gram_index of csrc/member_gram.h, restated."""
    return i * N - i * (i - 1) // 2 + (j - i)


def unpack(packed, N):
    """(..., N (N + 1) / 2) -> (..., N, N) symmetric."""
    packed = np.asarray(packed)
    full = np.zeros(packed.shape[:-1] + (N, N), packed.dtype)
    iu = np.triu_indices(N)                                   # row-major in (i, j >= i)
    full[..., iu[0], iu[1]] = packed
    full[..., iu[1], iu[0]] = packed
    return full


def members_of(gen):
    g = np.asarray(gen)
    return g if g.ndim == 5 else g[None]


def seeded_case(M, S, T, H, W, seed, zero_fraction=0.2):
    """target (S, T, H, W), gen (M, S, T, H, W) (M == 0: (S, T, H, W)) with INDEPENDENT members, weights (H, W) >= 0 with some
    exact zeros, climatology (H, W); all fp32."""
    rng = np.random.default_rng(seed)
    target = (0.5 + rng.standard_normal((S, T, H, W))).astype(np.float32)
    shape = (M, S, T, H, W) if M else (S, T, H, W)
    gen = (0.5 + rng.standard_normal(shape)).astype(np.float32)
    lat = (np.arange(H) + 0.5) / H * np.pi - np.pi / 2
    w = np.broadcast_to(np.cos(lat)[:, None], (H, W)) * (0.5 + rng.random((H, W)))
    w = np.where(rng.random((H, W)) < zero_fraction, 0.0, w).astype(np.float32)
    clim = (0.4 + 0.3 * rng.standard_normal((H, W))).astype(np.float32)
    return target, gen, w, clim


def integer_case(M, S, T, H, W, seed):
    """Small integers as fp32: |values| <= 8, weights 0 .. 3 (some 0); every member its own, non-symmetric pattern."""
    rng = np.random.default_rng(seed)
    target = rng.integers(-8, 9, (S, T, H, W)).astype(np.float32)
    shape = (M, S, T, H, W) if M else (S, T, H, W)
    gen = rng.integers(-8, 9, shape).astype(np.float32)
    w = rng.integers(0, 4, (H, W)).astype(np.float32)
    clim = rng.integers(-8, 9, (H, W)).astype(np.float32)
    return target, gen, w, clim


def vectors(target, gen, w, clim, dtype=np.float64):
    """a (N, S, T, HW) with the zero-weight rule applied (a select), and w (HW,), in `dtype`."""
    y = np.asarray(target, dtype)
    g = members_of(gen).astype(dtype)
    S, T, H, Wd = y.shape
    c = np.zeros((H, Wd), dtype) if clim is None else np.asarray(clim, dtype)
    a = np.concatenate([np.ones((1,) + y.shape, dtype), g - y, (y - c)[None]]).reshape(-1, S, T, H * Wd)
    wf = np.asarray(w, dtype).reshape(-1)
    return np.where(wf != 0, a, np.zeros((), dtype)), wf


def gram_int64(target, gen, w, clim):
    """(S, T, N, N) int64 of integer-valued inputs."""
    a, wf = vectors(target, gen, w, clim, np.int64)
    return np.einsum("p,istp,jstp->stij", wf, a, a)


def gram_float64(target, gen, w, clim):
    """-> ((S, T, N, N) float64 restatement, the same with |a_i a_j|: sum_p w |a_i a_j|)."""
    with np.errstate(invalid="ignore"):
        a, wf = vectors(target, gen, w, clim)
        wa = a * wf
        return np.einsum("istp,jstp->stij", wa, a), np.einsum("istp,jstp->stij", np.abs(wa), np.abs(a))


def gram_fraction(target, gen, w, clim):
    """(S, T, N, N) object arrays of Fractions: the exact Gram and the exact sum_p w |a_i a_j|, from fractions.Fraction of the
    fp32 inputs (small shapes: a Python loop)."""
    y = np.asarray(target, np.float32)
    g = members_of(gen).astype(np.float32)
    M, (S, T, H, Wd) = g.shape[0], y.shape
    N, HW = M + 2, H * Wd
    wf = [Fraction(float(x)) for x in np.asarray(w, np.float32).reshape(-1)]
    cf = [Fraction(0)] * HW if clim is None else [Fraction(float(x)) for x in np.asarray(clim, np.float32).reshape(-1)]
    G, A = np.empty((S, T, N, N), object), np.empty((S, T, N, N), object)
    for s in range(S):
        for t in range(T):
            yy = [Fraction(float(x)) for x in y[s, t].reshape(-1)]
            rows = [[Fraction(1)] * HW]
            rows += [[Fraction(float(x)) - yy[p] for p, x in enumerate(g[m, s, t].reshape(-1))] for m in range(M)]
            rows.append([yy[p] - cf[p] for p in range(HW)])
            for i in range(N):
                for j in range(i, N):
                    terms = [wf[p] * rows[i][p] * rows[j][p] for p in range(HW) if wf[p] != 0]
                    G[s, t, i, j] = G[s, t, j, i] = sum(terms, Fraction(0))
                    A[s, t, i, j] = A[s, t, j, i] = sum((abs(x) for x in terms), Fraction(0))
    return G, A


def gram_exact(target, gen, w, clim):
    """The same exact arithmetic in scaled Python integers (numpy object arrays), for the larger shapes: every a_i and w is a
    multiple of 2^-149, so a_i 2^149 is an integer that float64 holds exactly.  -> (G, A) as integers scaled by 2^(3 * 149)."""
    a, wf = vectors(target, gen, w, clim)
    to_int = np.frompyfunc(int, 1, 1)
    ai = to_int(np.ldexp(a, 149))                                             # (N, S, T, HW) Python integers
    wi = to_int(np.ldexp(wf, 149))
    N, S, T, _ = ai.shape
    G, A = np.empty((S, T, N, N), object), np.empty((S, T, N, N), object)
    for s in range(S):
        for t in range(T):
            x = ai[:, s, t]
            G[s, t] = np.dot(x * wi, x.T)
            A[s, t] = np.dot(np.abs(x) * wi, np.abs(x).T)
    return G, A


EXACT_SCALE = 2 ** (3 * 149)


def check_against_exact(got, G, A, HW, scale=1, factor=1, what=""):
    """Every entry of `got` (S, T, N, N) float64 within factor * (HW + 4) 2^-53 A of G (exact, both divided by `scale`)."""
    got = np.asarray(got)
    assert got.shape == G.shape, (got.shape, G.shape)
    worst = Fraction(0)
    for idx in np.ndindex(*G.shape):
        assert np.isfinite(got[idx]), (what, idx, got[idx])
        err = abs(Fraction(float(got[idx])) * scale - G[idx])
        bound = Fraction(factor * (HW + 4), 2 ** 53) * A[idx]
        assert err <= bound, (what, idx, float(got[idx]), float(Fraction(G[idx]) / scale), float(err / scale), float(bound / scale))
        if A[idx]:
            worst = max(worst, err / (Fraction(1, 2 ** 53) * A[idx]))
    return float(worst)                                                       # in units of 2^-53 sum w |a_i a_j|


def make_args(sdy, target, gen, w, clim, names):
    """sdy_member_gram_args of host arrays: target / gen dicts over names, w (H, W), clim {name: (H, W)} or None.
    -> (args, keep-alive, out (nvars, S, T, entries) float64)."""
    a = sdy._lib.SdyMemberGramArgs()
    keep, (H, Wd) = fill_window(a.win, target, gen, names)
    wf = np.ascontiguousarray(w, np.float32)
    keep.append(wf)
    a.HW, a.weights = H * Wd, vp(wf)
    for k, name in enumerate(names):
        if clim is not None and name in clim:
            c = np.ascontiguousarray(clim[name], np.float32)
            keep.append(c)
            a.climatology[k] = vp(c)
    out = np.full((len(names), a.win.n1, a.win.T, entries(a.win.n0 + 2)), np.nan)
    keep.append(out)
    a.out = vp(out)
    return a, keep, out


def host_gram(sdy, target, gen, w, clim=None):
    """One field through sdy_member_gram_host -> (S, T, N, N) float64."""
    a, keep, out = make_args(sdy, {"x": target}, {"x": gen}, w, None if clim is None else {"x": clim}, ["x"])
    rc = sdy.lib.sdy_member_gram_host(C.byref(a))
    assert rc == 0, rc
    return unpack(out[0], a.win.n0 + 2)


def scores_direct(target, gen, w, clim=None):
    """The field scores of one field from the FIELDS, float64 numpy, not through the Gram -> ({key: (S, T)}, {key: term scale
    (S, T)} for the distances).  Weighted means over the points with w != 0."""
    y = np.asarray(target, np.float64)
    g = members_of(gen).astype(np.float64)
    M = g.shape[0]
    wf = np.asarray(w, np.float64)
    wn = wf / wf.sum()
    mean = lambda x: (x * wn).sum(axis=(-2, -1))                              # noqa: E731
    c = np.zeros_like(wf) if clim is None else np.asarray(clim, np.float64)
    e = g - y
    rms = np.sqrt(mean(e * e))                                                # (M, S, T)
    out = {"error_distance": rms.mean(axis=0)}
    scale = {"error_distance": rms.max(axis=0) * np.sqrt(2.0)}
    if M > 1:
        pairs, pscale = [], []
        for i in range(M):
            for j in range(i + 1, M):
                d = g[i] - g[j]
                pairs.append(np.sqrt(mean(d * d)))
                # sqrt(D_ii + D_jj + 2 |D_ij|): what the Gram's form of the distance is made of
                pscale.append(np.sqrt(mean(e[i] * e[i]) + mean(e[j] * e[j]) + 2.0 * np.abs(mean(e[i] * e[j]))))
        out["member_distance"] = np.mean(pairs, axis=0)
        scale["member_distance"] = np.max(pscale, axis=0)
        out["energy_score"] = out["error_distance"] - 0.5 * out["member_distance"]
        scale["energy_score"] = scale["error_distance"] + scale["member_distance"]
    else:
        out["member_distance"] = np.full(y.shape[:2], np.nan)
        out["energy_score"] = out["error_distance"].copy()
        scale["energy_score"] = scale["error_distance"]
    with np.errstate(invalid="ignore", divide="ignore"):
        out["distance_ratio"] = out["member_distance"] / out["error_distance"]
    em = e.mean(axis=0)
    out["ensemble_mean_rmse"] = np.sqrt(mean(em * em))
    scale["ensemble_mean_rmse"] = scale["error_distance"]

    def corr(f, ya):
        fc, yc = f - mean(f)[..., None, None], ya - mean(ya)[..., None, None]
        return mean(fc * yc) / np.sqrt(mean(fc * fc) * mean(yc * yc))

    ya = y - c
    key = "anomaly_correlation" if clim is not None else "pattern_correlation"
    out[key] = corr(ya + em, ya)
    out[key + "_member_avg"] = np.mean([corr(ya + e[m], ya) for m in range(M)], axis=0)
    return out, scale


def check_two_computed(x, y, A, HW, scale=1, what=""):
    """Two computed Grams (the device's and the host twin's), each within the bound of the exact one: twice the bound apart."""
    x, y = np.asarray(x), np.asarray(y)
    assert x.shape == y.shape == A.shape, (x.shape, y.shape, A.shape)
    for idx in np.ndindex(*A.shape):
        err = abs(Fraction(float(x[idx])) - Fraction(float(y[idx]))) * scale
        assert err <= Fraction(2 * (HW + 4), 2 ** 53) * A[idx], (what, idx, float(x[idx]), float(y[idx]))
