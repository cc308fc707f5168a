"""Shared by tests/test_eddy_host.py and tests/test_gpu_eddy.py: seeded cases, the library's _host entry points driven from
numpy, a float64 numpy restatement of the state, the maps, the weighted sums and the logs, exact rational arithmetic on the fp32
inputs, and the comparison bounds.  The reference has nothing of the kind: the yardstick is exact arithmetic on the inputs.

A group is an ordered set of K variables (2 <= K <= 4).  State of one trajectory (a member of a sample, or a sample's target) at
one grid point, counted times x_k,1 .. x_k,n (fp32):
  c_k = x_k,1, d_k,t = (double)x_k,t - (double)c_k, S_k = sum_t d_k,t, P_ij = sum_t d_i,t d_j,t for i <= j in the pair order
  (0,0), (0,1), .., (0,K-1), (1,1), ..,
every term added to the running value in ascending time (csrc/time_covariance.h).  The groups of one K form a block: `sums`
float64 `(G, K, M B + B, H, W)` -- row i0 B + i1 is member i0 of sample i1, rows M B + i1 are the targets -- `products` float64
`(G, NP, M B + B, H, W)` and `origins` float32 like `sums`.  A state is {K: block}.

Bounds (u = 2^-53; n counted times).
  * Device state against the _host twin's, the _host twin's against the restatement (`restate_state`, which adds in the same
    order), device maps against _host maps: the same bits.
  * Covariance against exact rational arithmetic (`exact_point`):
      |cov - exact| <= 2 (n + 3) u sqrt((P_ii / n + m_i^2)(P_jj / n + m_j^2)),
    the variance bound of variability_utils with Cauchy-Schwarz over the pair; at i = j it is that bound.  Derivation: the
    deviations are exact in float64.  cov = (P_ij - S_i m_j) / n with m_j = S_j / n; exactly it is P_ij / n - m_i m_j.  A raw
    sum is a recursive float64 sum of n terms, each the exact d or a product rounded once: |computed - exact| <= (n + 1) u sum
    |terms| (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2).  With a_k = sqrt(P_kk / n): sum_t |d_i,t
    d_j,t| <= sqrt(P_ii P_jj) = n a_i a_j, so the P_ij / n part carries, with the roundings of the subtraction and of the
    division, (n + 2) u a_i a_j.  |dS_k| <= (n - 1) u sum_t |d_k,t| <= (n - 1) u sqrt(n P_kk) = (n - 1) u n a_k, so S_i S_j / n^2
    moves by (n - 1) u (|m_j| a_i + |m_i| a_j), and the division S_j / n, the product S_i m_j, the subtraction and the division
    by n add 4 u |m_i m_j|.  Every factor is at most n + 3, so the total is at most (n + 3) u (a_i + |m_i|)(a_j + |m_j|) <=
    2 (n + 3) u sqrt((a_i^2 + m_i^2)(a_j^2 + m_j^2)); on the diagonal the clamp at 0 only moves towards the exact value.
  * Device `stats` against _host `stats` and against the restatement (another summation order): 1e-12 x term scale x total
    weight, total weight = B sum(w), the project's `check_raw` rule.  Term scales: the largest |cov| (slots 0, 1), the largest
    (mean_m cov_gen - cov_target)^2 (slot 2), 1 for the correlation slots (|corr| <= 1) and the weight slot.
  * Logs, the propagation rules of variability_utils.check_logs: a mean covariance is a raw sum over the total weight: 1e-12 x
    its term scale, `cov_bias` twice that; `cov_rmse` compared as its square, 1e-12 x the slot-2 scale; a mean correlation is
    slot / weight slot and moves by 2e-12 / (defined fraction), `corr_bias` by twice that; `corr_defined_fraction` by 1e-12;
    the variances as the covariances of the diagonal pairs, `eke` as the mean of two of them, and `eke_ratio` = a / b by (da +
    ratio db) / b.
"""
import ctypes as C
from fractions import Fraction

import numpy as np

from variability_utils import U, cut, rows_of, within  # noqa: F401  (cut and within: used through this module)
from window_utils import fill_window, vp

SLOTS = 6
PAIR_KEYS = ("cov_gen", "cov_target", "cov_bias", "cov_rmse", "corr_gen", "corr_target", "corr_bias", "corr_defined_fraction")
#: the most independent times a thread of time_covariance_kernel requests at once (Shape<2>::kTimes, csrc/time_covariance.hip;
#: 4 at K = 3 and 2 at K = 4); the windowing case has a window of IN_FLIGHT + 1 counted times, one more than the longest batch
IN_FLIGHT = 6
SPLIT = [1, 1, 1, 3, IN_FLIGHT + 1]       # the initial condition alone, then windows of 1, 1, 3 and 7 counted times


def n_pairs(K):
    return K * (K + 1) // 2


def pair_index(K, i, j):
    return i * K - i * (i - 1) // 2 + (j - i)


def seeded_groups(M, B, H, W, S, groups, seed, means=None, std=3.0, phi=0.6, bias=0.5, spread=20.0):
    """-> dict(M, B, H, W, S, groups {label: {short: variable}}, names (the variables, in first use), weights (H, W) float32,
    target {name: (B, S + 1, H, W)}, gen {name: (M, B, S + 1, H, W)}, loading {name: lambda}): AR(1) series along time as in
    variability_utils.seeded_series (coefficient phi, stationary standard deviation std, around a climatology means[name] +-
    spread; default mean 280), float32; time 0 is the initial condition.  Every variable is lambda x (a factor common to all
    variables of the trajectory) + sqrt(1 - lambda^2) x (its own), so two variables correlate with lambda_a lambda_b."""
    rng = np.random.default_rng(seed)
    lat = (np.arange(H) + 0.5) / H * np.pi - np.pi / 2
    weights = (np.cos(lat)[:, None] * (1.0 + 0.1 * rng.random((H, W)))).astype(np.float32)
    names = list(dict.fromkeys(v for g in groups.values() for v in g.values()))
    means = {} if means is None else means

    def ar1(shape):                      # time on axis -3
        e = rng.standard_normal(shape)
        x = np.empty(shape)
        x[..., 0, :, :] = e[..., 0, :, :]
        for t in range(1, shape[-3]):
            x[..., t, :, :] = phi * x[..., t - 1, :, :] + np.sqrt(1.0 - phi * phi) * e[..., t, :, :]
        return x

    common_t, common_g = ar1((B, S + 1, H, W)), ar1((M, B, S + 1, H, W))
    loading = {k: lam for k, lam in zip(names, np.resize([0.8, -0.7, 0.6, 0.9, -0.5, 0.75], len(names)))}
    target, gen = {}, {}
    for k in names:
        lam, own = loading[k], np.sqrt(1.0 - loading[k] ** 2)
        clim = means.get(k, 280.0) + spread * rng.standard_normal((H, W))
        target[k] = (clim + std * (lam * common_t + own * ar1((B, S + 1, H, W)))).astype(np.float32)
        gen[k] = (clim + bias + 0.8 * std * (lam * common_g + own * ar1((M, B, S + 1, H, W)))).astype(np.float32)
    return dict(M=M, B=B, H=H, W=W, S=S, groups={l: dict(g) for l, g in groups.items()}, names=names, weights=weights,
                target=target, gen=gen, loading=loading)


def blocks_of(groups):
    """{K: [labels]} in ascending K, the labels in the groups' order: what one launch takes."""
    return {K: [l for l, g in groups.items() if len(g) == K] for K in sorted({len(g) for g in groups.values()})}


def empty_state(case, fill=0.0):
    rows, H, W = case["M"] * case["B"] + case["B"], case["H"], case["W"]
    return {K: dict(labels=labels, sums=np.full((len(labels), K, rows, H, W), fill),
                    products=np.full((len(labels), n_pairs(K), rows, H, W), fill),
                    origins=np.full((len(labels), K, rows, H, W), fill, np.float32))
            for K, labels in blocks_of(case["groups"]).items()}


def same_state(a, b):
    """The same bits (NaNs in the same places)."""
    return list(a) == list(b) and all(np.array_equal(a[K][k], b[K][k], equal_nan=True)
                                      for K in a for k in ("sums", "products", "origins"))


def restate_state(case, windows):
    """-> (state, n): float64 numpy, every counted time's term added to the running value in ascending time -- the order
    csrc/time_covariance.h fixes, so these are the bits."""
    st = empty_state(case)
    n = 0
    for start, target, gen in windows:
        t0 = 1 if start == 0 else 0
        T = next(iter(target.values())).shape[1]
        for K, blk in st.items():
            for g, label in enumerate(blk["labels"]):
                x = [rows_of(target[v], gen[v]) for v in case["groups"][label].values()]
                if n == 0 and T > t0:
                    for k in range(K):
                        blk["origins"][g, k] = x[k][:, t0]
                c = blk["origins"][g].astype(np.float64)
                for t in range(t0, T):
                    d = [x[k][:, t].astype(np.float64) - c[k] for k in range(K)]
                    for k in range(K):
                        blk["sums"][g, k] = blk["sums"][g, k] + d[k]
                    for i in range(K):
                        for j in range(i, K):
                            q = pair_index(K, i, j)
                            blk["products"][g, q] = blk["products"][g, q] + d[i] * d[j]
        n += T - t0
    return st, n


def accumulate_args(case, K, labels, target, gen, t0, first, blk):
    """SdyTimeCovarianceArgs of the groups `labels` (all of K variables) over contiguous numpy arrays; -> (args, keep-alive)."""
    from sdy_amd._lib import SdyTimeCovarianceArgs

    unique = list(dict.fromkeys(v for l in labels for v in case["groups"][l].values()))
    a = SdyTimeCovarianceArgs()
    keep, (H, W) = fill_window(a.win, target, gen, unique)
    a.HW, a.t0, a.first, a.K, a.n_groups = H * W, t0, int(first), K, len(labels)
    for g, l in enumerate(labels):
        for k, v in enumerate(case["groups"][l].values()):
            a.members[g][k] = unique.index(v)
    a.sums, a.products, a.origins = vp(blk["sums"]), vp(blk["products"]), vp(blk["origins"])
    return a, keep


def host_state(case, windows):
    """The windows through sdy_time_covariance_accumulate_host -> (state, n), shaped as restate_state gives them."""
    import sdy_amd

    st = empty_state(case)
    n = 0
    for start, target, gen in windows:
        t0 = 1 if start == 0 else 0
        T = next(iter(target.values())).shape[1]
        if T - t0 < 1:
            continue
        for K, blk in st.items():
            a, keep = accumulate_args(case, K, blk["labels"], target, gen, t0, n == 0, blk)
            assert sdy_amd.lib.sdy_time_covariance_accumulate_host(C.byref(a)) == 0
        n += T - t0
    return st, n


def restate_maps(blk, g, i, j, n):
    """-> (cov, corr, V_i, V_j) of pair i <= j of group g of a block, `(rows, H, W)`: the operations of sdy_tc_finish in its order."""
    K = blk["sums"].shape[1]
    n = float(n)
    with np.errstate(invalid="ignore", divide="ignore"):
        def V(k):
            s, pp = blk["sums"][g, k], blk["products"][g, pair_index(K, k, k)]
            v = pp - s * (s / n)
            return np.where(v < 0.0, 0.0, v)

        vi, vj = V(i), V(j)
        c = vi if i == j else blk["products"][g, pair_index(K, i, j)] - blk["sums"][g, i] * (blk["sums"][g, j] / n)
        cov = c / n
        rho = c / np.sqrt(vi * vj)
        rho = np.where(rho > 1.0, 1.0, rho)
        rho = np.where(rho < -1.0, -1.0, rho)
        corr = np.where((n >= 2.0) & (vi > 0.0) & (vj > 0.0), rho, np.nan)
    return cov, corr, vi, vj


def maps_args(blk, g, i, j, n, cov, corr):
    from sdy_amd._lib import SdyTimeCovarianceMapsArgs

    K, n_elems = blk["sums"].shape[1], int(np.prod(blk["sums"].shape[2:]))
    a = SdyTimeCovarianceMapsArgs()
    a.sums, a.products = vp(blk["sums"]) + 8 * g * K * n_elems, vp(blk["products"]) + 8 * g * n_pairs(K) * n_elems
    a.K, a.i, a.j, a.n_elems, a.n_times = K, i, j, n_elems, float(n)
    a.cov, a.corr = vp(cov), vp(corr)
    return a


def host_maps(blk, g, i, j, n):
    """sdy_time_covariance_maps_host -> (cov, corr), `(rows, H, W)`."""
    import sdy_amd

    cov, corr = np.full(blk["sums"].shape[2:], 7.0), np.full(blk["sums"].shape[2:], 7.0)
    assert sdy_amd.lib.sdy_time_covariance_maps_host(C.byref(maps_args(blk, g, i, j, n, cov, corr))) == 0
    return cov, corr


def restate_stats(blk, weights, n, M, B):
    """-> (raw (G, NP, 6) weighted sums as sdy_time_covariance_stats defines them, scales (G, NP, 6): the slots' term scales)."""
    G, K, _, H, W = blk["sums"].shape
    w = weights.astype(np.float64)
    raw, scales = np.zeros((G, n_pairs(K), SLOTS)), np.zeros((G, n_pairs(K), SLOTS))
    for g in range(G):
        for i in range(K):
            for j in range(i, K):
                cov, corr, _, _ = restate_maps(blk, g, i, j, n)
                gcov, tcov = cov[:M * B].reshape(M, B, H, W), cov[M * B:]
                gcorr, tcorr = corr[:M * B].reshape(M, B, H, W), corr[M * B:]
                mean_cov = gcov.sum(axis=0) / M
                diff = mean_cov - tcov
                defined = (n >= 2) & ~np.isnan(tcorr) & ~np.isnan(gcorr).any(axis=0)
                with np.errstate(invalid="ignore"):
                    mean_corr = np.where(defined, gcorr.sum(axis=0) / M, 0.0)
                q = pair_index(K, i, j)
                raw[g, q] = [(w * mean_cov).sum(), (w * tcov).sum(), (w * (diff * diff)).sum(), (w * mean_corr).sum(),
                             (w * np.where(defined, tcorr, 0.0)).sum(), (w * defined).sum()]
                cov_scale = float(np.nanmax(np.abs(cov)))
                scales[g, q] = [cov_scale, cov_scale, float(np.nanmax(diff * diff)), 1.0, 1.0, 1.0]
    return raw, scales


def stats_args(blk, weights, n, M, B, out):
    from sdy_amd._lib import SdyTimeCovarianceStatsArgs

    G, K, _, H, W = blk["sums"].shape
    a = SdyTimeCovarianceStatsArgs()
    a.K, a.n_groups, a.M, a.n1, a.HW = K, G, M, B, H * W
    w = np.ascontiguousarray(weights, np.float32)
    a.sums, a.products, a.weights, a.n_times, a.out = vp(blk["sums"]), vp(blk["products"]), vp(w), float(n), vp(out)
    return a, [w]


def host_stats(blk, weights, n, M, B):
    """sdy_time_covariance_stats_host -> raw (G, NP, 6)."""
    import sdy_amd

    G, K = blk["sums"].shape[:2]
    out = np.full((G, n_pairs(K), SLOTS), np.nan)
    a, keep = stats_args(blk, weights, n, M, B, out)
    assert sdy_amd.lib.sdy_time_covariance_stats_host(C.byref(a)) == 0
    return out


def weight_total(case):
    return case["B"] * float(case["weights"].astype(np.float64).sum())


def per_group(case, st, per_block):
    """{label: per_block[K][g]} in the groups' order."""
    return {l: per_block[len(case["groups"][l])][st[len(case["groups"][l])]["labels"].index(l)] for l in case["groups"]}


def log_keys(groups):
    """The keys of EddyCovarianceAggregator.get_logs(""), in order."""
    keys = []
    for label, g in groups.items():
        shorts = list(g)
        keys += [f"{key}/{label}/{a}_{b}" for i, a in enumerate(shorts) for b in shorts[i + 1:] for key in PAIR_KEYS]
        keys += [f"{key}/{label}/{a}" for a in shorts for key in ("time_variance_gen", "time_variance_target")]
        if "u" in shorts and "v" in shorts:
            keys += [f"eke_gen/{label}", f"eke_target/{label}", f"eke_ratio/{label}"]
    return keys


def logs_from_raw(raw, groups, total):
    """EddyCovarianceAggregator.get_logs("") from the raw sums {label: (NP, 6)} and the total weight, in float64 numpy."""
    logs = {}
    for label, g in groups.items():
        shorts, K, s = list(g), len(g), raw[label]
        with np.errstate(invalid="ignore", divide="ignore"):
            for i in range(K):
                for j in range(i + 1, K):
                    q = s[pair_index(K, i, j)]
                    cg, ct = q[0] / total, q[1] / total
                    rg, rt = (q[3] / q[5], q[4] / q[5]) if q[5] > 0.0 else (np.nan, np.nan)
                    vals = [cg, ct, cg - ct, np.sqrt(q[2] / total), rg, rt, rg - rt, q[5] / total]
                    logs.update({f"{key}/{label}/{shorts[i]}_{shorts[j]}": float(v) for key, v in zip(PAIR_KEYS, vals)})
            for i in range(K):
                q = s[pair_index(K, i, i)]
                logs[f"time_variance_gen/{label}/{shorts[i]}"] = float(q[0] / total)
                logs[f"time_variance_target/{label}/{shorts[i]}"] = float(q[1] / total)
            if "u" in shorts and "v" in shorts:
                qu, qv = s[pair_index(K, shorts.index("u"), shorts.index("u"))], s[pair_index(K, shorts.index("v"), shorts.index("v"))]
                eg, et = 0.5 * (qu[0] + qv[0]) / total, 0.5 * (qu[1] + qv[1]) / total
                logs.update({f"eke_gen/{label}": float(eg), f"eke_target/{label}": float(et),
                             f"eke_ratio/{label}": float(eg / et) if et > 0.0 else float("nan")})
    return logs


def check_raw(got, want, scales, total, what, rel=1e-12):
    """Raw weighted sums of two paths (G, NP, 6): |diff| <= rel x term scale x total weight."""
    for g in range(want.shape[0]):
        for q in range(want.shape[1]):
            for slot in range(SLOTS):
                assert np.isfinite(got[g, q, slot]), f"{what} group {g} pair {q} slot {slot}"
                within(float(got[g, q, slot]), float(want[g, q, slot]), rel * scales[g, q, slot] * total,
                       f"{what} group {g} pair {q} slot {slot}")


def check_logs(logs, want, groups, scales, what, rel=1e-12):
    """`logs` against the restatement's `want`: keys in order, Python floats, and the bounds of the module docstring.  scales:
    {label: (NP, 6)}."""
    assert list(logs) == list(want) == log_keys(groups), list(logs)
    assert all(type(v) is float for v in logs.values())
    for label, g in groups.items():
        shorts, K, sc = list(g), len(g), scales[label]
        for i in range(K):
            for j in range(i + 1, K):
                name, q = f"{label}/{shorts[i]}_{shorts[j]}", pair_index(K, i, j)
                got = lambda key: logs[f"{key}/{name}"]      # noqa: E731
                ref = lambda key: want[f"{key}/{name}"]      # noqa: E731
                d_cov = rel * sc[q][0]
                within(got("cov_gen"), ref("cov_gen"), d_cov, f"{what} cov_gen/{name}")
                within(got("cov_target"), ref("cov_target"), d_cov, f"{what} cov_target/{name}")
                within(got("cov_bias"), ref("cov_bias"), 2.0 * d_cov, f"{what} cov_bias/{name}")
                within(got("cov_rmse") ** 2, ref("cov_rmse") ** 2, rel * sc[q][2], f"{what} (cov_rmse/{name})^2")
                frac = ref("corr_defined_fraction")
                within(got("corr_defined_fraction"), frac, rel, f"{what} corr_defined_fraction/{name}")
                for key, mult in (("corr_gen", 2.0), ("corr_target", 2.0), ("corr_bias", 4.0)):
                    within(got(key), ref(key), mult * rel / frac, f"{what} {key}/{name}")
        d_var = {a: rel * sc[pair_index(K, i, i)][0] for i, a in enumerate(shorts)}
        for a in shorts:
            for key in ("time_variance_gen", "time_variance_target"):
                within(logs[f"{key}/{label}/{a}"], want[f"{key}/{label}/{a}"], d_var[a], f"{what} {key}/{label}/{a}")
        if "u" in shorts and "v" in shorts:
            d_eke = 0.5 * (d_var["u"] + d_var["v"])
            within(logs[f"eke_gen/{label}"], want[f"eke_gen/{label}"], d_eke, f"{what} eke_gen/{label}")
            within(logs[f"eke_target/{label}"], want[f"eke_target/{label}"], d_eke, f"{what} eke_target/{label}")
            ratio = want[f"eke_ratio/{label}"]
            within(logs[f"eke_ratio/{label}"], ratio, (d_eke + abs(ratio) * d_eke) / want[f"eke_target/{label}"],
                   f"{what} eke_ratio/{label}")


# ---- exact rational arithmetic ------------------------------------------------------------------------------------------------
def exact_point(xs):
    """xs: per variable of a group the counted fp32 values of one trajectory at one grid point, in run order -> dict of exact
    Fractions: s[k], p[(i, j)], m[k] = S_k / n, cov[(i, j)] = P_ij / n - m_i m_j for i <= j."""
    K, n = len(xs), len(xs[0])
    d = [[Fraction(float(v)) - Fraction(float(x[0])) for v in x] for x in xs]
    s = [sum(dk) for dk in d]
    p = {(i, j): sum(a * b for a, b in zip(d[i], d[j])) for i in range(K) for j in range(i, K)}
    m = [sk / n for sk in s]
    return dict(n=n, s=s, p=p, m=m, cov={ij: p[ij] / n - m[ij[0]] * m[ij[1]] for ij in p})


def check_point_exact(xs, cov, what):
    """cov: {(i, j): the float64 covariance under test}, against exact arithmetic on the fp32 values `xs`: the bound of the
    module docstring; -> {(i, j): (exact covariance as float, the bound)}."""
    e = exact_point(xs)
    n, out = e["n"], {}
    for (i, j), got in cov.items():
        scale2 = (e["p"][(i, i)] / n + e["m"][i] ** 2) * (e["p"][(j, j)] / n + e["m"][j] ** 2)
        bound = 2.0 * (n + 3) * U * float(scale2) ** 0.5
        within(float(abs(Fraction(float(got)) - e["cov"][(i, j)])), 0.0, bound, f"{what} cov[{i}, {j}] vs exact")
        out[(i, j)] = (float(e["cov"][(i, j)]), bound)
    return out
