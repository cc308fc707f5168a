"""What the tests of the time quantiles share: the numpy restatement of the definition (written from its text: np.sort of the
valid values per point, the rank rule, numpy's _lerp), the data, the argument structures of the host twins and the bit-for-bit
comparison."""
import ctypes as C

import numpy as np

NAN_KEY = 0xFFFFFFFF
METHODS = ("linear", "lower", "higher")
METHOD_CODE = {"linear": 0, "lower": 1, "higher": 2}
QS = (0.0, 0.125, 0.5, 0.9, 0.99, 1.0)
DYADIC = (0.0, 0.125, 0.5, 1.0)
GRIDS = ((5, 8), (5, 6))                   # 16-byte path, scalar path
MEMBERS = (1, 3)
SAMPLES = 2
TIMES = (1, 2, 3, 37)


# ---- the restatement --------------------------------------------------------------------------------------------------------
def key_of(x):
    """The sortable key of every fp32 value of an array (uint32)."""
    x = np.asarray(x, np.float32)
    u = np.where(x == 0, np.float32(0.0), x).view(np.uint32)              # -0.0 -> +0.0
    k = np.where(u >> 31 == 0, u ^ np.uint32(0x80000000), ~u)
    return np.where(np.isnan(x), np.uint32(NAN_KEY), k).astype(np.uint32)


def value_of(key):
    """The inverse of `key_of` for keys that are not the NaN key (fp32)."""
    key = np.asarray(key, np.uint32)
    u = np.where(key >> 31 != 0, key ^ np.uint32(0x80000000), ~key).astype(np.uint32)
    return u.view(np.float32)


def restate(x, qs, method):
    """x (n, ...) fp32, the values of a group along axis 0 -> (out (Q, ...) float64, n (...) int32 valid values)."""
    x = np.asarray(x, np.float32)
    x = np.where(x == 0, np.float32(0.0), x)                              # the sign of zero is canonical
    s = np.sort(x, axis=0).astype(np.float64)                             # NaNs last: the first n are the valid values
    n = (~np.isnan(x)).sum(axis=0)
    some = n > 0
    nn = np.where(some, n, 1)
    out = np.full((len(qs),) + x.shape[1:], np.nan)
    for i, q in enumerate(qs):
        h = np.float64(q) * (nn - 1).astype(np.float64)
        j = np.minimum(np.floor(h), (nn - 1).astype(np.float64))
        g = h - j
        ji = j.astype(np.int64)
        lo = np.take_along_axis(s, ji[None], axis=0)[0]
        hi = np.take_along_axis(s, np.minimum(ji + 1, nn - 1)[None], axis=0)[0]
        if method == "lower":
            res = lo
        elif method == "higher":
            res = np.where(g > 0, hi, lo)
        else:
            with np.errstate(invalid="ignore"):
                d = hi - lo
                lerp = np.where(g >= 0.5, hi - d * (1.0 - g), lo + d * g)
            res = np.where((g == 0) | (lo == hi), lo, lerp)
        out[i] = np.where(some, res, np.nan)
    return out, n.astype(np.int32)


def same_bits(a, b):
    """float64 arrays equal bit for bit, NaN matching NaN."""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    if a.shape != b.shape:
        return False
    return bool(((a.view(np.int64) == b.view(np.int64)) | (np.isnan(a) & np.isnan(b))).all())


# ---- data -------------------------------------------------------------------------------------------------------------------
def make_data(M, B, n, H, W, seed=0, plain=False):
    """-> (gen (M, B, n, H, W), target (B, n, H, W)) fp32.  Not `plain`: ties (one decimal), NaNs at 20 % of the entries, an
    all-NaN point (0, 1) in every trajectory, +inf at point (1, 2) and -inf at (2, 3) of some times, a -0.0 at (3, 0).  `plain`:
    finite and NaN-free, still with ties."""
    rng = np.random.default_rng(seed + 1000 * M + 10 * n + W)
    x = np.round(rng.standard_normal((M + 1, B, n, H, W)), 1).astype(np.float32)
    if not plain:
        x[rng.random(x.shape) < 0.2] = np.nan
        x[:, :, :, 0, 1] = np.nan
        x[:, :, ::2, 1, 2] = np.inf
        x[:, :, ::3, 2, 3] = -np.inf
        x[:, :, 0, 3, 0] = -0.0
    return x[:M], x[M]


def groupings(M, B):
    """name -> (first, step, count, stride, n_groups), for a series with the generated trajectories."""
    return {"gen": (0, 1, M, B, B), "gen_members": (0, 1, 1, 0, M * B), "target": (M * B, 1, 1, 0, B)}


def group_values(gen, target, which):
    """The restatement's input of a grouping: (values, groups, H, W), group-major as the select writes them."""
    M, B, n, H, W = gen.shape
    if which == "gen":
        return gen.transpose(0, 2, 1, 3, 4).reshape(M * n, B, H, W)
    if which == "gen_members":
        return gen.transpose(2, 0, 1, 3, 4).reshape(n, M * B, H, W)
    return target.transpose(1, 0, 2, 3)


def want(gen, target, which, qs, method):
    """-> (out (groups, Q, H, W), n (groups, H, W)) of the restatement."""
    out, n = restate(group_values(gen, target, which), qs, method)
    return out.transpose(1, 0, 2, 3), n


# ---- the host twins ---------------------------------------------------------------------------------------------------------
def append_args(series, target, gen, t0=0, slot0=0, store_gen=1):
    """One variable: gen (M, B, T, H, W), target (B, T, H, W) fp32 C-contiguous, series (n_traj, capacity, H*W) uint32.
    -> (args, what must stay alive)."""
    from sdy_amd import _lib

    M, B, T, H, W = gen.shape
    a = _lib.SdyTimeQuantileAppendArgs()
    a.nvars, a.gen[0], a.target[0] = 1, gen.ctypes.data, target.ctypes.data
    a.n0, a.n1, a.T, a.gs0, a.gs1, a.ts1 = M, B, T, B * T * H * W, T * H * W, T * H * W
    a.H, a.W, a.t0, a.slot0, a.capacity, a.store_gen = H, W, t0, slot0, series.shape[1], store_gen
    a.series = series.ctypes.data
    return a, (series, target, gen)


def new_series(n_traj, capacity, plane):
    return np.full((n_traj, capacity, plane), NAN_KEY, np.uint32)


def host_series(gen, target, store_gen=1, capacity=None):
    """The series of one window appended by the host twin, every time counted."""
    import sdy_amd

    M, B, T, H, W = gen.shape
    series = new_series(M * B + B if store_gen else B, capacity or T, H * W)
    a, keep = append_args(series, np.ascontiguousarray(target), np.ascontiguousarray(gen), store_gen=store_gen)
    assert sdy_amd.lib.sdy_time_quantile_append_host(C.byref(a)) == 0
    return series


def select_args(series, H, W, group, qs, method, n_slots=None):
    from sdy_amd import _lib

    first, step, count, stride, n_groups = group
    out = np.full((n_groups, len(qs), H, W), -7.0)
    valid = np.full((n_groups, H, W), -7, np.int32)
    a = _lib.SdyTimeQuantileSelectArgs()
    a.series, a.plane, a.n_traj, a.capacity = series.ctypes.data, H * W, series.shape[0], series.shape[1]
    a.n_slots = series.shape[1] if n_slots is None else n_slots
    a.first, a.step, a.count, a.stride, a.n_groups = first, step, count, stride, n_groups
    a.nq, a.method = len(qs), METHOD_CODE[method]
    for i, q in enumerate(qs):
        a.q[i] = q
    a.out, a.valid = out.ctypes.data, valid.ctypes.data
    return a, out, valid, (series,)


def host_select(series, H, W, group, qs, method, n_slots=None):
    import sdy_amd

    a, out, valid, keep = select_args(series, H, W, group, qs, method, n_slots)
    assert sdy_amd.lib.sdy_time_quantile_select_host(C.byref(a)) == 0
    return out, valid
