"""The numpy counterparts of sdy_amd.windows.fill_window and fill_slots, for the _host twins: shared by the *_utils.py of the
aggregators that read a window in place."""
import ctypes as C

import numpy as np


def vp(a):
    return a.ctypes.data_as(C.c_void_p).value


def fill_window(win, target, gen, names):
    """The `sdy_window` of contiguous float32 copies of target[k] (S, T, H, W) and gen[k] (the same, or member-stacked
    (M, S, T, H, W)) for k in names; -> (keep-alive list, (H, W))."""
    keep = []
    win.nvars = len(names)
    for j, k in enumerate(names):
        g, t = np.ascontiguousarray(gen[k], np.float32), np.ascontiguousarray(target[k], np.float32)
        keep += [g, t]
        win.gen[j], win.target[j] = vp(g), vp(t)
    S, T, H, W = t.shape
    win.n0, win.n1, win.T = (g.shape[0] if g.ndim == 5 else 1), S, T
    win.gs0, win.gs1, win.ts1 = (S * T * H * W if g.ndim == 5 else 0), T * H * W, T * H * W
    return keep, (H, W)


def fill_slots(slots, t0, t_start, n_slots, pool):
    """The `sdy_lead_slots` of an argument structure."""
    slots.t0, slots.t_start, slots.n_slots, slots.pool_times = t0, t_start, n_slots, int(pool)
