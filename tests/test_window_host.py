"""The checks every entry point that takes an `sdy_window` shares (csrc/window.h), without a GPU: the three _host twins
refuse a window with one broken field, and the Python side's `WindowLayout`, `runs` and `fill_window`."""
import ctypes as C

import numpy as np
import pytest
import torch

import field_stats_utils as fs
import member_mean_utils as mu

SDY_ERR_ARG = -1
SDY_MAX_VARS = 96


def _call(which):
    """A valid call of one 1 x 1 x 2 x (2 x 4) variable -> (host entry point, args, accumulators, keep-alive)."""
    import sdy_amd

    rng = np.random.default_rng(1)
    target = {"a": rng.standard_normal((1, 2, 2, 4)).astype(np.float32)}
    gen = {"a": rng.standard_normal((1, 1, 2, 2, 4)).astype(np.float32)}
    if which == "video":
        acc = {s: np.full((1, 2, 8), 7.0) for s in fs.VIDEO_STATS}
        a, keep = fs.video_args(target, gen, ["a"], 0, 2, acc)
        return sdy_amd.lib.sdy_video_accumulate_host, a, list(acc.values()), keep
    if which == "zonal":
        acc = [np.full((1, 1, 2, 2), 7.0), np.full((1, 1, 2, 2), 7.0)]
        a, keep = fs.zonal_args(target, gen, ["a"], 0, 2, *acc)
        return sdy_amd.lib.sdy_zonal_accumulate_host, a, acc, keep
    acc = [np.full((1, 1, 1, 2, 4), 7.0), np.full((1, 1, 2, 4), 7.0)]
    a, keep = mu.sum_args(target, gen, ["a"], 0, *acc)
    return sdy_amd.lib.sdy_member_time_sum_host, a, acc, keep


BROKEN = [("nvars", 0), ("nvars", SDY_MAX_VARS + 1), ("gen0", None), ("target0", None), ("gs0", -1), ("gs1", -1), ("ts1", -1),
          ("n0", 0), ("n1", 0), ("T", 0)]


@pytest.mark.parametrize("which", ["video", "zonal", "member_sum"])
def test_host_twins_refuse_a_broken_window(which):
    host, a, acc, keep = _call(which)
    assert (a.win.nvars, a.win.n0, a.win.n1, a.win.T) == (1, 1, 1, 2)
    for field, value in BROKEN:
        host, a, acc, keep = _call(which)
        if field == "gen0":
            a.win.gen[0] = value
        elif field == "target0":
            a.win.target[0] = value
        else:
            setattr(a.win, field, value)
        assert host(C.byref(a)) == SDY_ERR_ARG, (field, value)
        assert all((x == 7.0).all() for x in acc), (field, value)
    host, a, acc, keep = _call(which)                          # the valid call goes through, and writes
    assert host(C.byref(a)) == 0 and all((x != 7.0).any() for x in acc[:2])


def test_window_layout_runs_and_fill_window():
    from sdy_amd._lib import SdyZonalArgs
    from sdy_amd.windows import WindowLayout, fill_window, runs, window_layouts

    shapes = [(4, 8)] * 2 + [(4, 12)] + [(4, 8)] * 3
    target = {f"v{i}": torch.zeros(1, 3, H, W) for i, (H, W) in enumerate(shapes)}
    gen = {f"v{i}": torch.zeros(2, 1, 3, H, W) for i, (H, W) in enumerate(shapes)}
    lay = window_layouts(target, gen)
    assert all(isinstance(l, WindowLayout) for l in lay)
    l = lay[2]
    assert l.extents == (l.n0, l.n1, l.gs0, l.gs1, l.ts1, l.T, l.H, l.W) == (2, 1, 144, 144, 144, 3, 4, 12)
    gv, tv, n0, n1, gs0, gs1, ts1, T, H, W = l                 # tuple unpacking keeps working
    assert gv is l.gen and tv is l.target and (n0, n1, T, H, W) == (2, 1, 3, 4, 12)
    assert list(runs(lay, lambda l: l.extents)) == [(0, 2), (2, 3), (3, 6)]
    assert list(runs(lay, lambda l: l.extents, limit=2)) == [(0, 2), (2, 3), (3, 5), (5, 6)]
    assert list(runs([], lambda l: l)) == []
    a = SdyZonalArgs()
    fill_window(a.win, lay, 3, 6)
    assert (a.win.nvars, a.win.n0, a.win.n1, a.win.T, a.win.gs0, a.win.gs1, a.win.ts1) == (3, 2, 1, 3, 96, 96, 96)
    assert [a.win.gen[j] for j in range(3)] == [lay[3 + j].gen.data_ptr() for j in range(3)]
    assert [a.win.target[j] for j in range(3)] == [lay[3 + j].target.data_ptr() for j in range(3)]
    assert a.win.gen[3] is None and a.nvars == 3               # (the window's fields read as the structure's own)
