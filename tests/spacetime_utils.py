"""What the tests of the wavenumber-frequency spectra share: the numpy float64 restatement of the definition (written from its
text with direct sums: explicit cos / sin matrices, no FFT), its cross-check formulation with np.fft, the data builders, the
argument structures of the host twins, a host-side run that cuts the appends at segment ends, and the tolerance.

Tolerance against the restatement: 1e-12 * scale * n_contributions with scale = 25 A^2 (sum |w_n|)^2 / (N sum w_n^2), A the
largest |x| in the band of the run.  1e-12 is the project's constant for float64 chains (member_mean, region_series); the 25
covers the detrended values (a line fitted to data bounded by A stays below 2.5 A on the segment, and |X_f| <= sum |w_n| |z~_n|).
The outputs of `get_data` are means over their contributions: n_contributions = 1 there; a raw accumulator cell holds
n_segments x members x pairs of them."""
import ctypes as C

import numpy as np

GRIDS = ((8, 16), (9, 10), (6, 18))        # 16-byte loads; odd H (an equator row), scalar loads; K = W / 2 at its limit
MEMBERS = (1, 3)
SAMPLES = 2
NAMES = ("a", "b")
SEGMENTS = (8, 9, 12)
DETRENDS = ("none", "mean", "linear")
DETREND_CODE = {"none": 0, "mean": 1, "linear": 2}
TAPERS = (0.0, 0.2, 1.0)
LAT_MAX = 40.0                             # of the small grids: two or three row pairs


def hops(N):
    return (N, N // 2, 5)


def lats_of(H):
    """Cell centres of an equiangular grid, north to south."""
    return 90.0 - (np.arange(H) + 0.5) * 180.0 / H


def k_of(W):
    return W // 2 if W == 18 else min(5, W // 2)


# ---- the restatement --------------------------------------------------------------------------------------------------------
def band(lats, lat_max):
    """-> (north rows, south rows): every row with 0 <= lat <= lat_max (an equator row of an odd grid included), by |lat|."""
    lats = np.asarray(lats, np.float64)
    H = lats.size
    rows = [h for h in range(H) if (lats[h] >= 0 or 2 * h == H - 1) and abs(lats[h]) <= lat_max]
    rows.sort(key=lambda h: abs(lats[h]))
    return rows, [H - 1 - h for h in rows]


def taper(N, p):
    m = int(np.floor(p * N / 2))
    w = np.ones(N)
    for n in range(m):
        w[n] = w[N - 1 - n] = 0.5 * (1.0 - np.cos(np.pi * (n + 0.5) / m))
    return w


def circle(n):
    t = 2.0 * np.pi * np.arange(n) / n
    return np.stack([np.cos(t), np.sin(t)], axis=-1).copy()            # (n, 2)


def lon_coefficients(x, north, south, K):
    """x (..., H, W) -> (..., R, 2, K + 1) complex: c[k] = (1 / W) sum_j y[j] (cos t - i sin t), t = 2 pi ((k j) mod W) / W."""
    x = np.asarray(x, np.float32).astype(np.float64)
    W = x.shape[-1]
    xn, xs = x[..., north, :], x[..., south, :]
    y = np.stack([(xn + xs) / 2, (xn - xs) / 2], axis=-2)              # (..., R, 2, W)
    t = 2.0 * np.pi * ((np.arange(K + 1)[:, None] * np.arange(W)[None, :]) % W) / W
    return (y @ np.cos(t).T - 1j * (y @ np.sin(t).T)) / W


def detrended(z, detrend, w):
    """z (N, ...) complex, the times of a segment in order -> w_n z~_n."""
    N = z.shape[0]
    shape = (N,) + (1,) * (z.ndim - 1)
    d = (np.arange(N) - (N - 1) / 2).reshape(shape)
    y = z
    if detrend != "none":
        y = y - z.sum(axis=0) / N
    if detrend == "linear":
        y = y - d * ((d * z).sum(axis=0) / (d * d).sum())
    return w.reshape(shape) * y


def segment_power(z, detrend, w):
    """z (N, ...) complex -> P (N, ...): P_f = |sum_n w_n z~_n (cos u - i sin u)|^2 / (N sum w^2), u = 2 pi ((f n) mod N) / N."""
    N = z.shape[0]
    y = detrended(z, detrend, w)
    u = 2.0 * np.pi * ((np.arange(N)[:, None] * np.arange(N)[None, :]) % N) / N
    X = np.tensordot(np.cos(u) - 1j * np.sin(u), y, axes=1)
    return (X.real ** 2 + X.imag ** 2) / (N * (w * w).sum())


def segment_power_fft(x, north, south, K, detrend, w):
    """The same through np.fft: x (N, ..., H, W) fp32 -> P (N, ..., R, 2, K + 1)."""
    x = np.asarray(x, np.float32).astype(np.float64)
    xn, xs = x[..., north, :], x[..., south, :]
    y = np.stack([(xn + xs) / 2, (xn - xs) / 2], axis=-2)
    c = np.fft.fft(y, axis=-1)[..., :K + 1] / x.shape[-1]
    X = np.fft.fft(detrended(c, detrend, w), axis=0)
    return np.abs(X) ** 2 / (x.shape[0] * (w * w).sum())


def arrange(P):
    """(..., N, K + 1) -> (..., N // 2 + 1, 2 K + 1): out[nu][+k] = P[(N - nu) mod N][k], out[nu][-k] = P[nu][k], k = 0 their mean."""
    N, K = P.shape[-2], P.shape[-1] - 1
    out = np.empty(P.shape[:-2] + (N // 2 + 1, 2 * K + 1))
    for nu in range(N // 2 + 1):
        back = (N - nu) % N
        for k in range(1, K + 1):
            out[..., nu, K + k] = P[..., back, k]
            out[..., nu, K - k] = P[..., nu, k]
        out[..., nu, K] = (P[..., nu, 0] + P[..., back, 0]) / 2
    return out


def raw_sums(gen, target, lats, N, hop, K, lat_max, detrend, p):
    """gen (M, B, n, H, W), target (B, n, H, W), every time counted -> (acc (2, B, 2, N, K + 1) raw sums over segments, members and
    pairs, n_segments)."""
    north, south = band(lats, lat_max)
    w = taper(N, p)
    n = target.shape[1]
    n_segments = 0 if n < N else (n - N) // hop + 1
    M, B = gen.shape[:2]
    acc = np.zeros((2, B, 2, N, K + 1))
    cg = lon_coefficients(gen, north, south, K)                        # (M, B, n, R, 2, K1)
    ct = lon_coefficients(target, north, south, K)                     # (B, n, R, 2, K1)
    for s in range(n_segments):
        Pg = segment_power(np.moveaxis(cg[:, :, s * hop:s * hop + N], 2, 0), detrend, w)      # (N, M, B, R, 2, K1)
        Pt = segment_power(np.moveaxis(ct[:, s * hop:s * hop + N], 1, 0), detrend, w)         # (N, B, R, 2, K1)
        acc[0] += Pg.sum(axis=(1, 3)).transpose(1, 2, 0, 3)
        acc[1] += Pt.sum(axis=2).transpose(1, 2, 0, 3)
    return acc, n_segments


def want(gen, target, lats, N, hop, K, lat_max, detrend, p):
    """-> {"gen", "target": (B, 2, N // 2 + 1, 2 K + 1), "n_segments"}: what `get_data` returns per variable."""
    acc, n_segments = raw_sums(gen, target, lats, N, hop, K, lat_max, detrend, p)
    R = len(band(lats, lat_max)[0])
    return {"gen": arrange(acc[0] / (n_segments * gen.shape[0] * R)), "target": arrange(acc[1] / (n_segments * R)),
            "n_segments": n_segments}


def scale(gen, target, lats, N, lat_max, p):
    north, south = band(lats, lat_max)
    rows = sorted(set(north + south))
    A = max(np.abs(np.asarray(gen)[..., rows, :]).max(), np.abs(np.asarray(target)[..., rows, :]).max())
    w = taper(N, p)
    return 25.0 * float(A) ** 2 * np.abs(w).sum() ** 2 / (N * (w * w).sum())


def tolerance(gen, target, lats, N, lat_max, p, n_contributions=1):
    return 1e-12 * scale(gen, target, lats, N, lat_max, p) * n_contributions


def same_bits(a, b):
    """float64 arrays equal bit for bit, NaN matching NaN."""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    if a.shape != b.shape:
        return False
    return bool(((a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))).all())


# ---- data -------------------------------------------------------------------------------------------------------------------
def make_data(M, B, n, H, W, seed=0, amplitude=3.0, mean=0.0):
    """-> (gen (M, B, n, H, W), target (B, n, H, W)) fp32: noise around `mean`, a drift in time and a propagating wave."""
    rng = np.random.default_rng(seed + 1000 * M + 10 * n + W)
    t = np.arange(n).reshape(1, 1, n, 1, 1)
    j = np.arange(W).reshape(1, 1, 1, 1, W)
    x = amplitude * rng.standard_normal((M + 1, B, n, H, W)) + 0.05 * amplitude * t
    x = x + amplitude * np.cos(2 * np.pi * (2 * j / W - t / 6.0)) + mean
    x = x.astype(np.float32)
    return x[:M], x[M]


# ---- the host twins ---------------------------------------------------------------------------------------------------------
def append_args(coef, target, gen, north, south, K, N, t0, t1, n_first, lon_table):
    """One variable: gen (M, B, T, H, W), target (B, T, H, W) fp32 C-contiguous, coef (n_traj, N, R, 2, K + 1, 2) float64."""
    from sdy_amd import _lib

    M, B, T, H, W = gen.shape
    a = _lib.SdySpacetimeAppendArgs()
    a.nvars, a.gen[0], a.target[0] = 1, gen.ctypes.data, target.ctypes.data
    a.win.n0, a.win.n1, a.win.T, a.gs0, a.gs1, a.ts1 = M, B, T, B * T * H * W, T * H * W, T * H * W
    a.H, a.W, a.R, a.K = H, W, len(north), K
    for p in range(len(north)):
        a.north[p], a.south[p] = north[p], south[p]
    a.lon_table, a.t0, a.t1, a.n_first, a.N, a.coef = lon_table.ctypes.data, t0, t1, n_first, N, coef.ctypes.data
    return a, (coef, target, gen, lon_table)


def power_args(coef, M, B, N, R, K, first_slot, detrend, w, time_table, acc):
    from sdy_amd import _lib

    a = _lib.SdySpacetimeSegmentPowerArgs()
    a.coef, a.nvars, a.M, a.B, a.N, a.R, a.K = coef.ctypes.data, 1, M, B, N, R, K
    a.first_slot, a.detrend = first_slot, DETREND_CODE[detrend]
    a.taper, a.time_table, a.acc = w.ctypes.data, time_table.ctypes.data, acc.ctypes.data
    a.ws, a.ws_bytes = None, 0
    return a, (coef, w, time_table, acc)


def host_run(gen, target, lats, N, hop, K, lat_max, detrend, p, cuts=None, keep_coef=False):
    """The whole of a run through the host twins, every time counted: appends cut at segment ends (and at `cuts`, window
    lengths), a segment launch when a segment's last time is stored.  -> (acc (2, B, 2, N, K + 1), n_segments[, coef])."""
    import sdy_amd

    gen, target = np.ascontiguousarray(gen, np.float32), np.ascontiguousarray(target, np.float32)
    M, B, n, H, W = gen.shape
    north, south = band(lats, lat_max)
    R = len(north)
    coef = np.zeros((M * B + B, N, R, 2, K + 1, 2))
    acc = np.zeros((2, B, 2, N, K + 1))
    lon_table, time_table, w = circle(W), circle(N), taper(N, p)
    n_times = n_segments = 0
    start = 0
    for length in (cuts or (n,)):
        g, t = np.ascontiguousarray(gen[:, :, start:start + length]), np.ascontiguousarray(target[:, start:start + length])
        at = 0
        while at < length:
            end = n_segments * hop + N - 1
            take = min(length - at, end - n_times + 1)
            a, keep = append_args(coef, t, g, north, south, K, N, at, at + take, n_times, lon_table)
            assert sdy_amd.lib.sdy_spacetime_append_host(C.byref(a)) == 0
            n_times += take
            at += take
            if n_times - 1 == end:
                a, keep = power_args(coef, M, B, N, R, K, (n_segments * hop) % N, detrend, w, time_table, acc)
                assert sdy_amd.lib.sdy_spacetime_segment_power_host(C.byref(a)) == 0
                n_segments += 1
        start += length
    return (acc, n_segments, coef) if keep_coef else (acc, n_segments)


def host_spectrum(x, lats, N, hop, K, lat_max, detrend, p):
    """One (time, lat, lon) field through the host twins -> (2, N // 2 + 1, 2 K + 1), the arrangement of `get_data`."""
    x = np.asarray(x, np.float32)
    acc, n_segments = host_run(x[None, None], x[None], lats, N, hop, K, lat_max, detrend, p)
    return arrange(acc[1, 0] / (n_segments * len(band(lats, lat_max)[0])))
