"""The InstanceNorm statistics chain of the fused forward, kernel by kernel through the C ABI (include/sdy_amd.h): six
producers that leave (sum, sum of squares) per (image, channel) behind -- the epilogues of conv_h3, mlp_h3 and pair_h3,
sdy_gelu_stats, sdy_affine_copy_stats, sdy_irfft_lon_act with its per-ring partials -- and three consumers that turn them
into the coefficients of xn = a x + d -- sdy_instnorm_from_stats, sdy_instnorm_from_partials, sdy_instnorm_coeffs.
tests/instnorm_utils.py holds the cases, the float64 references and the derived bounds (NOTEBOOK.md 7o).

Producers are held to the float64 sums of their OWN stored output, on planes whose mean is 0, 10, 100 and 1000 standard
deviations, a constant plane and (GELU kernels) a plane of zeros; to "statistics are ADDED"; to leaving rows outside the
launch and the guard bands alone; and, for the row maps and the tile-major handoff, to reproducing the plain launch.

Statistics of two launches are compared bit for bit where one workgroup owns a slot (sdy_gelu_stats, sdy_affine_copy_stats,
the partials).  conv_h3, mlp_h3 and pair_h3 add per-workgroup float64 partials to a slot with atomics, in an order that
differs from launch to launch, so two launches of the same data agree to float64 re-association only: those comparisons
allow ACC64 = 1e-13 of sum |v| (sum v^2), eight orders below what a slot at the wrong row or a missed tile would move."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import torch

import instnorm_utils as iu
from instnorm_utils import Buf, bits_equal

pytestmark = pytest.mark.gpu

E, HID = 256, 512
F64 = torch.float64
SENT = (0.8125, -1.6875)      # what a statistics slot holds before a launch that must ADD to it
PAD = 777.0                   # prefill of tile-major buffers: the padding past HW must keep it and reach no statistic
ROWS5 = (4, 0, 2)             # a permuted, sparse map: 3 launch rows out of 5 batch rows


def env():
    import sdy_amd
    from sdy_amd._lib import current_stream

    return sdy_amd, sdy_amd.lib, current_stream()


@pytest.fixture(autouse=True)
def _clean_status_flags():
    yield
    env()[0].ops.status_flags(reset=True)


def rnd(key, *shape, scale=1.0):
    return torch.from_numpy(iu.gen(*key).standard_normal(shape).astype(np.float32)) * scale


def host_rows(rows):
    arr = (C.c_ubyte * len(rows))(*rows)
    return arr, C.addressof(arr)


def sentinel_stats(rows, Cc, zero_rows=()):
    """(rows, C, 2) float64 Buf holding SENT, zeros in `zero_rows`."""
    st = torch.tensor(SENT, dtype=F64).repeat(rows, Cc, 1)
    for r in zero_rows:
        st[r] = 0.0
    return Buf((rows, Cc, 2), st, F64)


def tiles(HW):
    return (HW + 63) // 64


def cpu_planes(buf, B, Cc, HW):
    return buf.t.detach().cpu().reshape(B, Cc, HW).numpy()


def close_stats(got, want, planes, what, base=0.0):
    """Two launches' statistics of the same stored planes: equal up to float64 re-association (module docstring); `base`: what
    the slots held before the launch, when the sums were added to it and it was subtracted again."""
    v = np.asarray(planes, dtype=np.float64)
    tol = iu.ACC64 * (np.stack([np.abs(v).sum(-1), (v * v).sum(-1)], -1) + base)
    err = np.abs(np.asarray(got) - np.asarray(want))
    assert (err <= tol).all(), f"{what}: statistics differ by up to {float((err / np.maximum(tol, 1e-300)).max()):.3g} x 1e-13 of the sums"


# ---- weights and launch helpers ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def conv_weight(cin, zero_row):
    sdy, _, _ = env()
    w = rnd(("conv w", cin), E, cin, scale=1.0 / math.sqrt(cin))
    w[E - 1] = 0.0
    if zero_row:
        w[E - 2] = 0.0
    return sdy.ops.pack_conv256(w[:, :, None, None], "cuda")


@functools.lru_cache(maxsize=None)
def mlp_weight():
    sdy, _, _ = env()
    w1 = rnd(("mlp w1",), HID, E, scale=1.0 / 16.0)
    w2 = rnd(("mlp w2",), E, HID, scale=1.0 / math.sqrt(HID))
    w2[E - 1] = 0.0
    b1 = rnd(("mlp b1",), HID, scale=0.1).cuda()
    b2 = rnd(("mlp b2",), E, scale=0.1)
    b2[E - 1] = iu.CONST_VALUE
    return sdy.ops.pack_mlp_h3(w1[:, :, None, None], w2[:, :, None, None], "cuda"), b1, b2.cuda()


@functools.lru_cache(maxsize=None)
def pair_weight(cin):
    sdy, _, _ = env()
    w1 = rnd(("pair w1", cin), E, cin, scale=1.0 / math.sqrt(cin))
    w2 = rnd(("pair w2", cin), E, E, scale=1.0 / 16.0)
    w2[E - 1] = 0.0
    return sdy.ops.pack_pair_h3(w1[:, :, None, None], w2[:, :, None, None], "cuda"), rnd(("pair b1", cin), E, scale=0.1).cuda()


def launch_conv(*, x, B, Cin, HW, frag, out, out_bs=None, x_bs=None, bias=None, pa=None, pd=None, add=None, add_bs=0,
                add_mode=0, act=0, stats=None, out_tiled=0, x_rows=None):
    from sdy_amd._lib import SdyConvArgs

    _, lib, stream = env()
    a = SdyConvArgs()
    a.x, a.x_bstride = x.ptr, Cin * HW if x_bs is None else x_bs
    a.ldw = E
    a.out, a.out_bstride = out.ptr, E * HW if out_bs is None else out_bs
    a.B, a.Cin, a.Cout, a.HW = B, Cin, E, HW
    if pa is not None:
        a.pa, a.pd = pa.ptr, pd.ptr
    if bias is not None:
        a.bias = bias.ptr
    if add is not None:
        a.add, a.add_bstride, a.add_mode = add.ptr, add_bs, add_mode
    a.act = act
    a.w_frag, a.w_frag_scale = frag[0].data_ptr(), frag[1]
    if stats is not None:
        a.stats = stats.ptr
    a.out_tiled = out_tiled
    keep = None
    if x_rows is not None:
        keep, a.x_rows = host_rows(x_rows)
    rc = lib.sdy_conv1x1(C.byref(a), stream)
    torch.cuda.synchronize()
    del keep
    return rc


def launch_mlp(*, x, B, HW, out, add, x_bs=None, x_tiled=0, pa=None, pd=None, stats=None, drop=0.0, out_rows=None,
               add_by_launch_row=0, rows_per_call=0, seed=0x1234ABCD5678, call=3):
    from sdy_amd._lib import SdyMlpArgs

    _, lib, stream = env()
    (w, s1, s2), b1, b2 = mlp_weight()
    a = SdyMlpArgs()
    a.x, a.x_bstride, a.x_tiled = x.ptr, E * HW if x_bs is None else x_bs, x_tiled
    if pa is not None:
        a.pa, a.pd = pa.ptr, pd.ptr
    a.w, a.w1_scale, a.w2_scale = w.data_ptr(), s1, s2
    a.b1, a.b2 = b1.data_ptr(), b2.data_ptr()
    a.out, a.out_bstride = out.ptr, E * HW
    a.add, a.add_bstride = add.ptr, E * HW
    a.B, a.E, a.hidden, a.HW = B, E, HID, HW
    a.drop_p, a.seed, a.call, a.stream_fc1, a.stream_fc2, a.batch_offset = drop, seed, call, 4, 5, 7
    a.rows_per_call = rows_per_call
    if stats is not None:
        a.stats = stats.ptr
    keep = None
    if out_rows is not None:
        keep, a.out_rows = host_rows(out_rows)
    a.add_by_launch_row = add_by_launch_row
    rc = lib.sdy_mlp_h3(C.byref(a), stream)
    torch.cuda.synchronize()
    del keep
    return rc


def launch_pair(*, x, B, Cin, HW, out, add, stats):
    from sdy_amd._lib import SdyPairArgs

    _, lib, stream = env()
    (w, s1, s2), b1 = pair_weight(Cin)
    a = SdyPairArgs()
    a.x, a.x_bstride = x.ptr, Cin * HW
    a.w, a.w1_scale, a.w2_scale = w.data_ptr(), s1, s2
    a.b1 = b1.data_ptr()
    a.out, a.out_bstride = out.ptr, E * HW
    a.add, a.add_bstride = add.ptr, 0
    a.B, a.Cin, a.hidden, a.Cout, a.HW = B, Cin, E, E, HW
    a.stats = stats.ptr
    rc = lib.sdy_pair_h3(C.byref(a), stream)
    torch.cuda.synchronize()
    return rc


def fft_plan(nlat):
    from sdy_amd.sht import ShtPlan

    _, lib, _ = env()
    plan = ShtPlan.get(nlat, 360, nlat, nlat, "equiangular", torch.cuda.current_device(), "h3")
    k = (C.c_int * 2)()
    assert lib.sdy_sht_plan_kernels(plan.handle, C.byref(k)) == 0 and k[1] == 1, "the 360-point cases expect fft360.hip"
    return plan


# ---- one producer run ---------------------------------------------------------------------------------------------------------
def offsets_of(case):
    off, const, zero = iu.roles(case.C, case.gelu)
    t = torch.from_numpy(off.astype(np.float32))
    return off, t, const, zero


@functools.lru_cache(maxsize=None)
def producer_inputs(case):
    """Device input buffers of one case (built once; every launch leaves them unchanged)."""
    B, Cc, HW = case.B, case.C, case.HW
    _, t, const, zero = offsets_of(case)
    key = ("in", case.id)
    d = {}
    if case.producer == "conv_h3":
        d["x"] = Buf((B, case.cin, HW), rnd(key + ("x",), B, case.cin, HW))
        if case.form == "skip":     # GELU(W (pa x + pd) + bias + add): the offsets ride on the bias
            bias = t.clone()
            bias[const], bias[zero] = iu.CONST_VALUE, iu.GELU_OFF
            add = rnd(key + ("add",), B, E, HW, scale=0.5)
            add[:, const], add[:, zero] = 0.0, 0.0
            d["bias"], d["add"] = Buf((E,), bias), Buf((B, E, HW), add)
            d["pa"] = Buf((B * E,), 1.0 + rnd(key + ("pa",), B * E, scale=0.2))
            d["pd"] = Buf((B * E,), rnd(key + ("pd",), B * E, scale=0.2))
        else:                       # W x + broadcast addend (the encoder's position embedding): the offsets ride on the addend
            add = rnd(key + ("pos",), 1, E, HW, scale=0.5) + t[None, :, None]
            add[:, const] = iu.CONST_VALUE
            d["add"] = Buf((1, E, HW), add)
    elif case.producer == "mlp_h3":
        d["x"] = Buf((B, E, HW), rnd(key + ("x",), B, E, HW))
        add = rnd(key + ("res",), B, E, HW, scale=0.5) + t[None, :, None]
        add[:, const] = 0.0
        d["add"] = Buf((B, E, HW), add)
        d["pa"] = Buf((B * E,), 1.0 + rnd(key + ("pa",), B * E, scale=0.2))
        d["pd"] = Buf((B * E,), rnd(key + ("pd",), B * E, scale=0.2))
    elif case.producer == "pair_h3":
        d["x"] = Buf((B, case.cin, HW), rnd(key + ("x",), B, case.cin, HW))
        add = rnd(key + ("pos",), 1, E, HW, scale=0.5) + t[None, :, None]
        add[:, const] = iu.CONST_VALUE
        d["add"] = Buf((1, E, HW), add)
    elif case.producer == "gelu_stats":
        y = rnd(key + ("y",), B, Cc, HW) + t[None, :, None]
        y[:, const], y[:, zero] = iu.CONST_VALUE, iu.GELU_OFF
        d["y"] = Buf((B, Cc, HW), y)
    elif case.producer == "affine_copy":
        d["x"] = Buf((B, Cc, HW), rnd(key + ("x",), B, Cc, HW))
        a = 1.0 + rnd(key + ("a",), B, Cc, scale=0.2)
        a[:, const] = 0.0           # fma(x, 0, d) = d: the constant plane
        dd = t[None, :].repeat(B, 1)
        dd[:, const] = iu.CONST_VALUE
        d["a"], d["d"] = Buf((B * Cc,), a), Buf((B * Cc,), dd)
    elif case.producer == "irfft_lon_act":
        K = case.grid[0]
        Yf = rnd(key + ("Yf",), K, K, B, 2, Cc, scale=1.0 / math.sqrt(4.0 * K))     # rings of about unit variance
        Yf[..., const], Yf[..., zero] = 0.0, 0.0
        bias = t.clone()
        bias[const], bias[zero] = iu.CONST_VALUE, iu.GELU_OFF
        d["Yf"], d["bias"] = Buf((K, K, B, 2, Cc), Yf), Buf((Cc,), bias)
    return d


def run_producer(case, sentinel):
    """One launch.  Returns (stored planes (B, C, HW) float32 numpy, statistics (B, C, 2) float64 numpy, `aux`): statistics
    start as zeros (sentinel False) or SENT (True) in the B launch rows and SENT in one row past them."""
    _, lib, stream = env()
    B, Cc, HW = case.B, case.C, case.HW
    d = producer_inputs(case)
    tiled = case.form == "tiled" or case.producer == "irfft_lon_act"
    out = Buf((B, tiles(HW), Cc, 64), PAD) if tiled else Buf((B, Cc, HW))
    st = sentinel_stats(B + 1, Cc, () if sentinel else range(B))
    aux = {}
    if case.producer == "conv_h3":
        frag = conv_weight(case.cin, case.form == "skip")
        if case.form == "skip":
            rc = launch_conv(x=d["x"], B=B, Cin=case.cin, HW=HW, frag=frag, out=out, bias=d["bias"], pa=d["pa"], pd=d["pd"],
                             add=d["add"], add_bs=E * HW, add_mode=1, act=1, stats=st)
        else:
            rc = launch_conv(x=d["x"], B=B, Cin=case.cin, HW=HW, frag=frag, out=out, add=d["add"], add_bs=0, add_mode=2, stats=st)
    elif case.producer == "mlp_h3":
        rc = launch_mlp(x=d["x"], B=B, HW=HW, out=out, add=d["add"], pa=d["pa"], pd=d["pd"], stats=st, drop=case.drop)
    elif case.producer == "pair_h3":
        rc = launch_pair(x=d["x"], B=B, Cin=case.cin, HW=HW, out=out, add=d["add"], stats=st)
    elif case.producer == "gelu_stats":
        rc = lib.sdy_gelu_stats(d["y"].ptr, Cc * HW, out.ptr, out.t[0].numel(), 1 if tiled else 0, st.ptr, B, Cc, HW, stream)
    elif case.producer == "affine_copy":
        keep, rows = host_rows(list(range(B)))
        rc = lib.sdy_affine_copy_stats(d["x"].ptr, Cc * HW, d["a"].ptr, d["d"].ptr, out.ptr, Cc * HW, st.ptr, Cc, HW, rows, B, -1,
                                       stream)
    else:
        K = case.grid[0]
        part = Buf((B, K, Cc, 2), None, F64)
        rc = lib.sdy_irfft_lon_act(fft_plan(K).handle, d["Yf"].ptr, d["bias"].ptr, out.ptr, out.t[0].numel(), part.ptr, B, Cc,
                                   stream)
        aux["part"] = part
    assert rc == 0, (case.id, rc)
    torch.cuda.synchronize()
    assert out.guards_intact() and st.guards_intact(), f"{case.id}: a guard band of out or stats was written"
    for name, b in d.items():
        assert b.unchanged(), f"{case.id}: input {name} was written"
    if tiled:
        planes, pad = iu.untile(out.t.cpu(), Cc, HW)
        assert bool((pad == PAD).all()), f"{case.id}: the padding past HW of the last tile was written"
        planes = planes.contiguous().numpy()
    else:
        planes = cpu_planes(out, B, Cc, HW)
    assert not np.isnan(planes).any(), f"{case.id}: a pixel was not stored"
    if case.producer == "irfft_lon_act":
        part = aux["part"]
        assert part.guards_intact()
        p = part.t.cpu().numpy()
        assert not np.isnan(p).any(), f"{case.id}: a (ring, channel) partial was not written"
        aux["part_np"] = p
        stats = np.zeros((B, Cc, 2))
        for k in range(case.grid[0]):        # the order instnorm_from_partials adds them in
            stats = stats + p[:, k]
        assert bits_equal(st.t, st.before)
    else:
        stats = st.t.cpu().numpy()[:B]
        assert bits_equal(st.t[B], st.before[B]), f"{case.id}: the statistics row past the launch was written"
    aux["out"] = out
    return planes, stats, aux


# ---- producers ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", iu.PRODUCER_CASES, ids=[c.id for c in iu.PRODUCER_CASES])
def test_producer_statistics(case):
    off, _, const, zero = offsets_of(case)
    kind = iu.PRODUCER_ACCUM[case.producer]
    planes, stats, aux = run_producer(case, sentinel=False)
    iu.check_stats(stats, planes, kind, f"GPU {case.id}", off)
    if case.producer in ("gelu_stats", "irfft_lon_act"):
        assert (planes[:, zero] == 0).all() and (stats[:, zero] == 0).all(), "GELU(-30) is not a plane of zeros"
    if case.producer != "mlp_h3" or case.drop == 0.0:
        assert (planes[:, const] == planes[0, const, 0]).all(), "the constant channel is not constant"
    live = np.array([c not in (const, zero) for c in range(case.C)])
    xe = iu.norm_error(stats[:, live], planes[:, live])
    print(f"GPU {case.id}: rel L2 of a x + d" + "".join(f"  [{t:g}: {float(xe[:, off[live] == t].max()):.1e}]" for t in iu.TARGETS))
    if case.producer == "irfft_lon_act":
        # each slot is one ring: its own (sum, sumsq) of the ring's stored pixels, under the same bound
        K, W = case.grid
        rings = planes.reshape(case.B, case.C, K, W).transpose(0, 2, 1, 3)
        iu.check_stats(aux["part_np"], rings, kind, f"GPU {case.id} per ring")
        return
    # statistics are ADDED: a slot that held SENT holds SENT + sums; the stored tensor is the same, bit for bit
    planes2, stats2, _ = run_producer(case, sentinel=True)
    assert np.array_equal(planes.view(np.int32), planes2.view(np.int32)), "two launches stored different tensors"
    sent = np.array(SENT)
    if case.producer in ("gelu_stats", "affine_copy"):
        assert np.array_equal(stats2, sent + stats), "a slot is not SENT + its sums (one float64 add)"
    else:
        close_stats(stats2 - sent, stats, planes, f"{case.id} added to a sentinel", base=np.abs(sent))


# ---- row maps ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid", [(6, 36), (87, 96)])
def test_conv_x_rows(grid):
    """Image z of the launch reads batch row x_rows[z] of x / pa / pd; add, out and stats stay indexed by z."""
    HW = grid[0] * grid[1]
    key = ("xrows", grid)
    frag = conv_weight(E, True)
    x = Buf((5, E, HW), rnd(key + ("x",), 5, E, HW))
    pa, pd = Buf((5 * E,), 1.0 + rnd(key + ("pa",), 5 * E, scale=0.2)), Buf((5 * E,), rnd(key + ("pd",), 5 * E, scale=0.2))
    add = Buf((3, E, HW), rnd(key + ("add",), 3, E, HW, scale=0.5))
    bias = Buf((E,), rnd(key + ("b",), E) * 10.0)
    out, st = Buf((3, E, HW)), sentinel_stats(4, E, range(3))
    assert launch_conv(x=x, B=3, Cin=E, HW=HW, frag=frag, out=out, bias=bias, pa=pa, pd=pd, add=add, add_bs=E * HW, add_mode=1,
                       act=1, stats=st, x_rows=ROWS5) == 0
    assert out.guards_intact() and st.guards_intact() and bits_equal(st.t[3], st.before[3])
    assert x.unchanged() and pa.unchanged() and pd.unchanged() and add.unchanged()
    for z, r in enumerate(ROWS5):
        x1, a1 = Buf((1, E, HW), x.t[r]), Buf((1, E, HW), add.t[z])
        pa1, pd1 = Buf((E,), pa.t[r * E:(r + 1) * E]), Buf((E,), pd.t[r * E:(r + 1) * E])
        o1, s1 = Buf((1, E, HW)), sentinel_stats(1, E, range(1))
        assert launch_conv(x=x1, B=1, Cin=E, HW=HW, frag=frag, out=o1, bias=bias, pa=pa1, pd=pd1, add=a1, add_bs=E * HW,
                           add_mode=1, act=1, stats=s1) == 0
        assert bits_equal(out.t[z], o1.t[0]), f"launch row {z} (batch row {r}) differs from the unmapped launch"
        close_stats(st.t[z].cpu().numpy(), s1.t[0].cpu().numpy(), cpu_planes(o1, 1, E, HW)[0], f"x_rows launch row {z}")
    iu.check_stats(st.t[:3].cpu().numpy(), cpu_planes(out, 3, E, HW), "row64", f"GPU conv_h3 x_rows {grid}")


@pytest.mark.parametrize("by_launch_row", [0, 1])
@pytest.mark.parametrize("grid", [(6, 36), (87, 96)])
def test_mlp_out_rows(grid, by_launch_row):
    """Image z of the launch (x, pa, pd) IS batch row out_rows[z]: out, stats and -- unless add_by_launch_row -- add are taken
    there; batch rows outside the map keep what they held."""
    HW = grid[0] * grid[1]
    key = ("orows", grid)
    x = Buf((3, E, HW), rnd(key + ("x",), 3, E, HW))
    pa, pd = Buf((3 * E,), 1.0 + rnd(key + ("pa",), 3 * E, scale=0.2)), Buf((3 * E,), rnd(key + ("pd",), 3 * E, scale=0.2))
    n_add = 3 if by_launch_row else 5
    add = Buf((n_add, E, HW), rnd(key + ("add", n_add), n_add, E, HW) + 10.0)
    out, st = Buf((5, E, HW), 5.5), sentinel_stats(5, E, ROWS5)
    assert launch_mlp(x=x, B=3, HW=HW, out=out, add=add, pa=pa, pd=pd, stats=st, out_rows=ROWS5, rows_per_call=5,
                      add_by_launch_row=by_launch_row) == 0
    assert out.guards_intact() and st.guards_intact() and x.unchanged() and add.unchanged()
    for r in set(range(5)) - set(ROWS5):
        assert bits_equal(out.t[r], out.before[r]) and bits_equal(st.t[r], st.before[r]), f"batch row {r} is not in the launch"
    for z, r in enumerate(ROWS5):
        x1, a1 = Buf((1, E, HW), x.t[z]), Buf((1, E, HW), add.t[z if by_launch_row else r])
        pa1, pd1 = Buf((E,), pa.t[z * E:(z + 1) * E]), Buf((E,), pd.t[z * E:(z + 1) * E])
        o1, s1 = Buf((1, E, HW)), sentinel_stats(1, E, range(1))
        assert launch_mlp(x=x1, B=1, HW=HW, out=o1, add=a1, pa=pa1, pd=pd1, stats=s1) == 0
        assert bits_equal(out.t[r], o1.t[0]), f"launch row {z} is not at batch row {r}, or differs from the unmapped launch"
        close_stats(st.t[r].cpu().numpy(), s1.t[0].cpu().numpy(), cpu_planes(o1, 1, E, HW)[0], f"out_rows launch row {z}")
    sel = list(ROWS5)
    iu.check_stats(st.t[sel].cpu().numpy(), out.t[sel].cpu().reshape(3, E, HW).numpy(), "quad", f"GPU mlp_h3 out_rows {grid}")


@pytest.mark.parametrize("src_row0", [-1, 1])
@pytest.mark.parametrize("grid", [(6, 36), (87, 96)])
def test_affine_copy_rows(grid, src_row0):
    """Batch row b = rows[i] of out / a / d / stats; its source is x row b, or src_row0 + i."""
    _, lib, stream = env()
    HW, Cc = grid[0] * grid[1], 6
    key = ("arows", grid)
    x = Buf((5, Cc, HW), rnd(key + ("x",), 5, Cc, HW))
    a = Buf((5 * Cc,), 1.0 + rnd(key + ("a",), 5 * Cc, scale=0.2))
    d = Buf((5 * Cc,), rnd(key + ("d",), 5 * Cc) * 30.0)
    out, st = Buf((5, Cc, HW), 5.5), sentinel_stats(5, Cc, ROWS5)
    keep, rows = host_rows(ROWS5)
    assert lib.sdy_affine_copy_stats(x.ptr, Cc * HW, a.ptr, d.ptr, out.ptr, Cc * HW, st.ptr, Cc, HW, rows, 3, src_row0, stream) == 0
    torch.cuda.synchronize()
    assert out.guards_intact() and st.guards_intact() and x.unchanged() and a.unchanged() and d.unchanged()
    for r in set(range(5)) - set(ROWS5):
        assert bits_equal(out.t[r], out.before[r]) and bits_equal(st.t[r], st.before[r]), f"batch row {r} is not in the launch"
    k0, row0 = host_rows([0])
    for i, r in enumerate(ROWS5):
        s = r if src_row0 < 0 else src_row0 + i
        x1, a1, d1 = Buf((1, Cc, HW), x.t[s]), Buf((Cc,), a.t[r * Cc:(r + 1) * Cc]), Buf((Cc,), d.t[r * Cc:(r + 1) * Cc])
        o1, s1 = Buf((1, Cc, HW)), sentinel_stats(1, Cc, range(1))
        assert lib.sdy_affine_copy_stats(x1.ptr, Cc * HW, a1.ptr, d1.ptr, o1.ptr, Cc * HW, s1.ptr, Cc, HW, row0, 1, -1, stream) == 0
        torch.cuda.synchronize()
        assert bits_equal(out.t[r], o1.t[0]) and bits_equal(st.t[r], s1.t[0]), f"rows[{i}] = {r} (source {s})"
        want = torch.addcmul(d1.t.cpu().double().view(Cc, 1), a1.t.cpu().double().view(Cc, 1), x1.t[0].cpu().double())
        assert torch.equal(o1.t[0].cpu(), want.float()), "out is not fma(x, a, d)"
    # a, d NULL: a plain copy, bit for bit, with its statistics
    o2, s2 = Buf((5, Cc, HW), 5.5), sentinel_stats(5, Cc, ROWS5)
    assert lib.sdy_affine_copy_stats(x.ptr, Cc * HW, None, None, o2.ptr, Cc * HW, s2.ptr, Cc, HW, rows, 3, src_row0, stream) == 0
    torch.cuda.synchronize()
    src = [r if src_row0 < 0 else src_row0 + i for i, r in enumerate(ROWS5)]
    assert bits_equal(o2.t[list(ROWS5)], x.t[src])
    iu.check_stats(s2.t[list(ROWS5)].cpu().numpy(), x.t[src].cpu().numpy(), "quad", f"GPU affine copy (plain) {grid}")
    del keep, k0


# ---- tile-major handoff -------------------------------------------------------------------------------------------------------
def _mlp_after(z, z_bs, tiled, B, HW, key):
    add = Buf((B, E, HW), rnd(key + ("res",), B, E, HW) + 10.0)
    pa, pd = Buf((B * E,), 1.0 + rnd(key + ("pa1",), B * E, scale=0.2)), Buf((B * E,), rnd(key + ("pd1",), B * E, scale=0.2))
    out, st = Buf((B, E, HW)), sentinel_stats(B, E, range(B))
    assert launch_mlp(x=z, x_bs=z_bs, x_tiled=tiled, B=B, HW=HW, out=out, add=add, pa=pa, pd=pd, stats=st) == 0
    assert out.guards_intact() and st.guards_intact() and z.unchanged()
    return out, st


@pytest.mark.parametrize("grid", [(6, 36), (87, 96)])
def test_tile_major_handoff_conv_to_mlp(grid):
    """conv_h3 with out_tiled feeding mlp_h3 with x_tiled == the NCHW pair of launches, bit for bit; the padding of the last
    tile keeps its prefill and reaches no statistic."""
    B, HW = 2, grid[0] * grid[1]
    case = iu.Case("conv_h3", grid, B, E, "skip", E)
    d = producer_inputs(case)
    frag = conv_weight(E, True)
    kw = dict(x=d["x"], B=B, Cin=E, HW=HW, frag=frag, bias=d["bias"], pa=d["pa"], pd=d["pd"], add=d["add"], add_bs=E * HW,
              add_mode=1, act=1)
    zn, sn = Buf((B, E, HW)), sentinel_stats(B, E, range(B))
    zt, stt = Buf((B, tiles(HW), E, 64), PAD), sentinel_stats(B, E, range(B))
    assert launch_conv(out=zn, stats=sn, **kw) == 0
    assert launch_conv(out=zt, out_bs=tiles(HW) * E * 64, out_tiled=1, stats=stt, **kw) == 0
    assert zt.guards_intact() and stt.guards_intact()
    planes, pad = iu.untile(zt.t.cpu(), E, HW)
    assert torch.equal(planes.contiguous().view(torch.int32), zn.t.cpu().view(torch.int32)), "tile-major conv output differs"
    assert bool((pad == PAD).all()), "the padding past HW was written"
    close_stats(stt.t.cpu().numpy(), sn.t.cpu().numpy(), cpu_planes(zn, B, E, HW), "conv_h3 tile-major")
    iu.check_stats(stt.t.cpu().numpy(), planes.numpy(), "row64", f"GPU conv_h3 out_tiled {grid}")
    zn.before, zt.before = zn.t.clone(), zt.t.clone()
    on, s_n = _mlp_after(zn, E * HW, 0, B, HW, ("handoff", grid))
    ot, s_t = _mlp_after(zt, tiles(HW) * E * 64, 1, B, HW, ("handoff", grid))
    assert bits_equal(on.t, ot.t), "mlp_h3 on the tile-major tensor differs from the NCHW launch"
    close_stats(s_t.t.cpu().numpy(), s_n.t.cpu().numpy(), cpu_planes(on, B, E, HW), "mlp_h3 x_tiled")
    iu.check_stats(s_t.t.cpu().numpy(), cpu_planes(ot, B, E, HW), "quad", f"GPU mlp_h3 x_tiled {grid}")


def test_tile_major_handoff_gelu_stats_to_mlp():
    """sdy_gelu_stats storing tile-major feeds mlp_h3 like its NCHW form (C = 256, 87 x 96 and 6 x 36)."""
    _, lib, stream = env()
    for grid in ((6, 36), (87, 96)):
        B, HW = 2, grid[0] * grid[1]
        y = Buf((B, E, HW), rnd(("gs handoff", grid), B, E, HW) + 0.5)
        zn, zt = Buf((B, E, HW)), Buf((B, tiles(HW), E, 64), PAD)
        assert lib.sdy_gelu_stats(y.ptr, E * HW, zn.ptr, E * HW, 0, None, B, E, HW, stream) == 0
        assert lib.sdy_gelu_stats(y.ptr, E * HW, zt.ptr, tiles(HW) * E * 64, 1, None, B, E, HW, stream) == 0
        torch.cuda.synchronize()
        planes, pad = iu.untile(zt.t.cpu(), E, HW)
        assert torch.equal(planes.contiguous().view(torch.int32), zn.t.cpu().view(torch.int32)) and bool((pad == PAD).all())
        zn.before, zt.before = zn.t.clone(), zt.t.clone()
        on, s_n = _mlp_after(zn, E * HW, 0, B, HW, ("gs handoff", grid))
        ot, s_t = _mlp_after(zt, tiles(HW) * E * 64, 1, B, HW, ("gs handoff", grid))
        assert bits_equal(on.t, ot.t)
        close_stats(s_t.t.cpu().numpy(), s_n.t.cpu().numpy(), cpu_planes(on, B, E, HW), "mlp_h3 after gelu_stats")


def test_tile_major_handoff_irfft_act_to_mlp_and_partials():
    """sdy_irfft_lon_act's tile-major tensor feeds mlp_h3 like the NCHW tensor of the same values, and
    sdy_irfft_lon_act -> sdy_instnorm_from_partials equals sdy_irfft_lon -> host GELU -> the float64 formula within the
    producer bound (plus gelu_erf's documented error against the exact GELU, instnorm_utils.GELU_ERF_REL)."""
    _, lib, stream = env()
    B, K, Cc = 1, 19, E
    HW = K * 360
    plan = fft_plan(K)
    off, t, const, zero = offsets_of(iu.Case("irfft_lon_act", (K, 360), B, Cc))
    Yf = rnd(("act handoff",), K, K, B, 2, Cc, scale=1.0 / math.sqrt(4.0 * K))
    Yf[..., const], Yf[..., zero] = 0.0, 0.0
    bias = t.clone()
    bias[const], bias[zero] = iu.CONST_VALUE, iu.GELU_OFF
    Yb, bb = Buf((K, K, B, 2, Cc), Yf), Buf((Cc,), bias)
    zt, part, y = Buf((B, tiles(HW), Cc, 64), PAD), Buf((B, K, Cc, 2), None, F64), Buf((B, Cc, HW))
    assert lib.sdy_irfft_lon_act(plan.handle, Yb.ptr, bb.ptr, zt.ptr, tiles(HW) * Cc * 64, part.ptr, B, Cc, stream) == 0
    assert lib.sdy_irfft_lon(plan.handle, Yb.ptr, bb.ptr, y.ptr, B, Cc, stream) == 0
    torch.cuda.synchronize()
    assert zt.guards_intact() and part.guards_intact() and y.guards_intact() and Yb.unchanged() and bb.unchanged()
    planes, pad = iu.untile(zt.t.cpu(), Cc, HW)
    assert bool((pad == PAD).all()) and not bool(torch.isnan(part.t).any())
    # the stored activation against the exact GELU of the ring sdy_irfft_lon stores
    y64 = y.t.cpu().double().numpy()
    g64 = iu.gelu64(y64)
    assert (np.abs(planes.double().numpy() - g64) <= iu.GELU_ERF_REL * np.abs(y64)).all(), "zt is not GELU(ring + bias)"
    # partials -> coefficients against the float64 formula on the host GELU
    gamma, beta = rnd(("act g",), Cc) + 1.0, rnd(("act b",), Cc)
    gb, be = Buf((Cc,), gamma), Buf((Cc,), beta)
    a, d = Buf((B * Cc,)), Buf((B * Cc,))
    part.before = part.t.clone()
    assert lib.sdy_instnorm_from_partials(part.ptr, K, B, Cc, HW, gb.ptr, be.ptr, iu.EPS, a.ptr, d.ptr, stream) == 0
    torch.cuda.synchronize()
    assert part.unchanged() and a.guards_intact() and d.guards_intact()
    ref = iu.plane_sums(g64, "row128")
    dg = iu.GELU_ERF_REL * np.abs(y64)
    dS = ref.dS + dg.sum(-1)
    dS2 = ref.dS2 + (2 * np.abs(g64) * dg + dg * dg).sum(-1)
    S, S2 = iu.exact_sums(g64)
    iu.check_coeffs(a.t.cpu().numpy(), d.t.cpu().numpy(),
                    iu.consumer_ref(S, S2, HW, gamma.numpy(), beta.numpy(), dS=dS, dS2=dS2), "GPU irfft_lon_act -> from_partials")
    # ... and tightly against the float64 sums of what was stored
    pl = planes.contiguous().numpy()
    refp = iu.plane_sums(pl, "row128")
    Sp, S2p = iu.exact_sums(pl)
    iu.check_coeffs(a.t.cpu().numpy(), d.t.cpu().numpy(),
                    iu.consumer_ref(Sp, S2p, HW, gamma.numpy(), beta.numpy(), dS=refp.dS, dS2=refp.dS2),
                    "GPU from_partials vs the stored tensor")
    # the MLP reads the tile-major tensor like an NCHW copy of it
    zn = Buf((B, Cc, HW), planes)
    zt.before = zt.t.clone()
    on, s_n = _mlp_after(zn, E * HW, 0, B, HW, ("act handoff",))
    ot, s_t = _mlp_after(zt, tiles(HW) * E * 64, 1, B, HW, ("act handoff",))
    assert bits_equal(on.t, ot.t)
    close_stats(s_t.t.cpu().numpy(), s_n.t.cpu().numpy(), cpu_planes(on, B, E, HW), "mlp_h3 after irfft_lon_act")


# ---- consumers ----------------------------------------------------------------------------------------------------------------
def consumer_stats(B, Cc, HW, key):
    """Exact double statistics of B x C planes cycling through the offset targets, with a constant plane in slot 0 and, when
    there is a slot 1, a sum of squares just below S^2 / HW there (a variance that comes out negative)."""
    x = rnd(key, B, Cc, HW).numpy() + np.array([iu.TARGETS[i % 4] for i in range(B * Cc)], dtype=np.float32).reshape(B, Cc, 1)
    x.reshape(B * Cc, HW)[0] = iu.CONST_VALUE
    S, S2 = iu.exact_sums(x)
    if B * Cc > 1:
        S2.reshape(-1)[1] = S.reshape(-1)[1] ** 2 / HW * (1 - 1e-15)
    return x, S, S2


def ss_variants(B, Cc, key):
    """(name, device buffer or None, pointer, stride, scale (B, C), shift (B, C))"""
    out = [("none", None, None, 0, None, None)]
    ss = rnd(key + ("ss",), B, 2 * Cc)
    out.append(("2C", Buf((B, 2 * Cc), ss), None, 2 * Cc, ss[:, :Cc].numpy(), ss[:, Cc:].numpy()))
    ss6 = rnd(key + ("ss6",), B, 3, 2 * Cc)          # three layers side by side: this block is layer 1
    out.append(("6C+layer", Buf((B, 6 * Cc), ss6), 2 * Cc, 6 * Cc, ss6[:, 1, :Cc].numpy(), ss6[:, 1, Cc:].numpy()))
    return out


@pytest.mark.parametrize("B,Cc", [(1, 1), (1, 255), (1, 256), (1, 257), (3, 16)])
def test_instnorm_from_stats(B, Cc):
    sdy, lib, stream = env()
    HW = 320
    _, S, S2 = consumer_stats(B, Cc, HW, ("from_stats", B, Cc))
    gamma, beta = rnd(("g", Cc), Cc) + 1.0, rnd(("b", Cc), Cc)
    gb, be = Buf((Cc,), gamma), Buf((Cc,), beta)
    for name, ssb, off, stride, scale, shift in ss_variants(B, Cc, ("from_stats", B, Cc)):
        st = Buf((B, Cc, 2), np.stack([S, S2], -1), F64)
        a, d = Buf((B * Cc,)), Buf((B * Cc,))
        ssp = None if ssb is None else ssb.ptr + 4 * (off or 0)
        sdy.ops.status_flags(reset=True)
        assert lib.sdy_instnorm_from_stats(st.ptr, B, Cc, HW, gb.ptr, be.ptr, ssp, stride, iu.EPS, a.ptr, d.ptr, stream) == 0
        assert sdy.ops.status_flags(reset=True) == 0
        assert st.guards_intact() and a.guards_intact() and d.guards_intact() and (ssb is None or ssb.unchanged())
        assert bool((st.t == 0).all()), "sdy_instnorm_from_stats did not leave its statistics exactly zero"
        ref = iu.consumer_ref(S, S2, HW, gamma.numpy(), beta.numpy(), scale, shift)
        iu.check_coeffs(a.t.cpu().numpy(), d.t.cpu().numpy(), ref, f"GPU from_stats B={B} C={Cc} ss={name}")
        if name == "none" and B * Cc > 1:
            rstd = float(a.t[1]) / float(gamma[1])
            assert abs(rstd * math.sqrt(float(np.float32(iu.EPS))) - 1.0) <= 3 * iu.U, "negative variance: rstd is not 1 / sqrt(eps)"


@pytest.mark.parametrize("K", [1, 19, 20, 21, 41, 181])
def test_instnorm_from_partials(K):
    """Synthetic double partials whose sum depends on the order it is taken in: 2^53 s, then ones times s, then -2^53 s adds
    up to exactly zero in the order of k (each 1 is absorbed) and to (K - 2) s in any grouping that adds the ones first; the
    loop's tail (G = 20: K = 19, 21, 41, 181) holds the last term."""
    sdy, lib, stream = env()
    HW = 320
    rng = iu.gen("partials", K)
    for B, Cc in ((1, 1), (1, 255), (1, 256), (1, 257), (2, 48)):
        part = np.zeros((B, K, Cc, 2))
        part[..., 1] = rng.uniform(0.5, 1.5, size=(B, K, Cc)) * HW / K * 4.0
        s = 2.0 ** rng.integers(-3, 4, size=(B, Cc)) * rng.choice([-1.0, 1.0], size=(B, Cc))
        if K >= 3:
            part[:, :, :, 0] = s[:, None, :]
            part[:, 0, :, 0] = 2.0 ** 53 * s
            part[:, K - 1, :, 0] = -(2.0 ** 53) * s
        else:
            part[..., 0] = rng.standard_normal((B, K, Cc)) * HW
            part[..., 1] += part[..., 0] ** 2 / HW * 2
        S, S2 = np.zeros((B, Cc)), np.zeros((B, Cc))
        for k in range(K):
            S, S2 = S + part[:, k, :, 0], S2 + part[:, k, :, 1]
        if K >= 3:
            assert (S == 0).all()
        pb = Buf((B, K, Cc, 2), part, F64)
        gamma, beta = rnd(("g", Cc), Cc) + 1.0, rnd(("b", Cc), Cc)
        gb, be = Buf((Cc,), gamma), Buf((Cc,), beta)
        a, d = Buf((B * Cc,)), Buf((B * Cc,))
        assert lib.sdy_instnorm_from_partials(pb.ptr, K, B, Cc, HW, gb.ptr, be.ptr, iu.EPS, a.ptr, d.ptr, stream) == 0
        torch.cuda.synchronize()
        assert pb.unchanged() and a.guards_intact() and d.guards_intact()
        ref = iu.consumer_ref(S, S2, HW, gamma.numpy(), beta.numpy())
        iu.check_coeffs(a.t.cpu().numpy(), d.t.cpu().numpy(), ref, f"GPU from_partials K={K} B={B} C={Cc}")
        if K >= 3:      # S = 0 bit for bit: d = beta - 0 * a = beta exactly
            assert bits_equal(d.t.view(B, Cc), be.t.view(1, Cc).expand(B, Cc).contiguous()), "the partials were not added in the order of k"
    sdy.ops.status_flags(reset=True)


@pytest.mark.parametrize("grid", [(8, 40), (87, 96)])
def test_instnorm_coeffs_every_offset(grid):
    """sdy_instnorm_coeffs reads x itself and sums in float64 throughout: the consumer bound at every offset, with only
    float64 accumulation (ACC64) on its inputs."""
    _, lib, stream = env()
    B, Cc, HW = 3, 8, grid[0] * grid[1]
    x, S, S2 = consumer_stats(B, Cc, HW, ("coeffs", grid))
    S2 = iu.exact_sums(x)[1]
    xb = Buf((B, Cc, HW), x)
    gamma, beta = rnd(("g", Cc), Cc) + 1.0, rnd(("b", Cc), Cc)
    gb, be = Buf((Cc,), gamma), Buf((Cc,), beta)
    x64 = x.astype(np.float64)
    dS, dS2 = iu.ACC64 * np.abs(x64).sum(-1), iu.ACC64 * S2
    for name, ssb, off, stride, scale, shift in ss_variants(B, Cc, ("coeffs", grid)):
        a, d = Buf((B * Cc,)), Buf((B * Cc,))
        ssp = None if ssb is None else ssb.ptr + 4 * (off or 0)
        assert lib.sdy_instnorm_coeffs(xb.ptr, B, Cc, HW, gb.ptr, be.ptr, ssp, stride, iu.EPS, a.ptr, d.ptr, stream) == 0
        torch.cuda.synchronize()
        assert xb.unchanged() and a.guards_intact() and d.guards_intact()
        ref = iu.consumer_ref(S, S2, HW, gamma.numpy(), beta.numpy(), scale, shift, dS=dS, dS2=dS2)
        iu.check_coeffs(a.t.cpu().numpy(), d.t.cpu().numpy(), ref, f"GPU instnorm_coeffs {grid} ss={name}")


def test_nonfinite_flag():
    """SDY_FLAG_NONFINITE for a NaN or infinite statistic, not for a large finite one (both flat consumers)."""
    sdy, lib, stream = env()
    Cc, HW, K = 4, 320, 3
    gb, be = Buf((Cc,), torch.ones(Cc)), Buf((Cc,), torch.zeros(Cc))
    for bad, want in ((float("nan"), iu.FLAG_NONFINITE), (float("inf"), iu.FLAG_NONFINITE), (-float("inf"), iu.FLAG_NONFINITE),
                      (1e300, 0)):
        for slot in (0, 1):
            st = np.tile(np.array([3.0, 400.0]), (1, Cc, 1))
            st[0, 2, slot] = abs(bad) if slot == 1 else bad
            a, d = Buf((Cc,)), Buf((Cc,))
            sdy.ops.status_flags(reset=True)
            sb = Buf((1, Cc, 2), st, F64)
            assert lib.sdy_instnorm_from_stats(sb.ptr, 1, Cc, HW, gb.ptr, be.ptr, None, 0, iu.EPS, a.ptr, d.ptr, stream) == 0
            assert sdy.ops.status_flags(reset=True) & iu.FLAG_NONFINITE == want, ("from_stats", bad, slot)
            part = np.zeros((1, K, Cc, 2))
            part[0, 0], part[0, K - 1] = st[0] / 2, st[0] / 2
            if not math.isfinite(bad):
                part[0, 0, 2, slot], part[0, K - 1, 2, slot] = 1.0, st[0, 2, slot]
            pb = Buf((1, K, Cc, 2), part, F64)
            assert lib.sdy_instnorm_from_partials(pb.ptr, K, 1, Cc, HW, gb.ptr, be.ptr, iu.EPS, a.ptr, d.ptr, stream) == 0
            assert sdy.ops.status_flags(reset=True) & iu.FLAG_NONFINITE == want, ("from_partials", bad, slot)


# ---- refusals: by status code, nothing launched ---------------------------------------------------------------------------------
def test_refusals():
    _, lib, stream = env()
    A, U_, L = iu.SDY_ERR_ARG, iu.SDY_ERR_UNSUPPORTED, iu.SDY_ERR_ALIGN
    B, Cc, HW, K = 2, 16, 360 * 18, 18
    T = tiles(HW) * Cc * 64
    x, xo = Buf((B, Cc, HW), torch.ones(B, Cc, HW)), Buf((B, Cc, HW), torch.ones(B, Cc, HW), offset=1)
    out, outo = Buf((B, Cc, HW), 5.5), Buf((B, Cc, HW), 5.5, offset=1)
    zt, zto = Buf((B, T), 5.5), Buf((B, T), 5.5, offset=1)
    st, sto = sentinel_stats(B, Cc), Buf((B, Cc, 2), 1.5, F64, offset=1)
    part, parto = Buf((B, K, Cc, 2), 1.5, F64), Buf((B, K, Cc, 2), 1.5, F64, offset=1)
    v, a, d = Buf((B * Cc,), 1.0), Buf((B * Cc,), 5.5), Buf((B * Cc,), 5.5)
    Yf, Yfo = Buf((K, K, B, 2, Cc), 0.5), Buf((K, K, B, 2, Cc), 0.5, offset=1)
    keep, rows = host_rows([0, 1])
    keep2, rows129 = host_rows([0] * 129)
    plan = fft_plan(K)
    from sdy_amd.sht import ShtPlan

    plan64 = ShtPlan.get(16, 64, 16, 16, "equiangular", torch.cuda.current_device(), "h3")      # not a 360-point plan
    S = stream
    calls = [
        # sdy_gelu_stats
        (A, lambda: lib.sdy_gelu_stats(None, Cc * HW, out.ptr, Cc * HW, 0, st.ptr, B, Cc, HW, S)),
        (A, lambda: lib.sdy_gelu_stats(x.ptr, Cc * HW, None, Cc * HW, 0, st.ptr, B, Cc, HW, S)),
        (A, lambda: lib.sdy_gelu_stats(x.ptr, Cc * HW, out.ptr, Cc * HW, 0, st.ptr, 0, Cc, HW, S)),
        (A, lambda: lib.sdy_gelu_stats(x.ptr, Cc * HW, zt.ptr, T - 64, 1, st.ptr, B, Cc, HW, S)),            # tile-major stride too small
        (L, lambda: lib.sdy_gelu_stats(x.ptr, Cc * (HW - 2), out.ptr, Cc * (HW - 2), 0, st.ptr, B, Cc, HW - 2, S)),
        (L, lambda: lib.sdy_gelu_stats(x.ptr, Cc * HW + 2, out.ptr, Cc * HW, 0, st.ptr, B, Cc, HW, S)),
        (L, lambda: lib.sdy_gelu_stats(x.ptr, Cc * HW, out.ptr, Cc * HW + 2, 0, st.ptr, B, Cc, HW, S)),
        (L, lambda: lib.sdy_gelu_stats(xo.ptr, Cc * HW, out.ptr, Cc * HW, 0, st.ptr, B, Cc, HW, S)),
        (L, lambda: lib.sdy_gelu_stats(x.ptr, Cc * HW, outo.ptr, Cc * HW, 0, st.ptr, B, Cc, HW, S)),
        (L, lambda: lib.sdy_gelu_stats(x.ptr, Cc * HW, out.ptr, Cc * HW, 0, sto.ptr, B, Cc, HW, S)),
        # sdy_affine_copy_stats
        (A, lambda: lib.sdy_affine_copy_stats(None, Cc * HW, v.ptr, v.ptr, out.ptr, Cc * HW, st.ptr, Cc, HW, rows, 2, -1, S)),
        (A, lambda: lib.sdy_affine_copy_stats(x.ptr, Cc * HW, v.ptr, v.ptr, None, Cc * HW, st.ptr, Cc, HW, rows, 2, -1, S)),
        (A, lambda: lib.sdy_affine_copy_stats(x.ptr, Cc * HW, v.ptr, v.ptr, out.ptr, Cc * HW, st.ptr, Cc, HW, None, 2, -1, S)),
        (A, lambda: lib.sdy_affine_copy_stats(x.ptr, Cc * HW, v.ptr, None, out.ptr, Cc * HW, st.ptr, Cc, HW, rows, 2, -1, S)),
        (A, lambda: lib.sdy_affine_copy_stats(x.ptr, Cc * HW, v.ptr, v.ptr, out.ptr, Cc * HW, st.ptr, Cc, HW, rows129, 129, -1, S)),
        (A, lambda: lib.sdy_affine_copy_stats(x.ptr, Cc * HW, v.ptr, v.ptr, out.ptr, Cc * HW, st.ptr, Cc, HW, rows, 0, -1, S)),
        (L, lambda: lib.sdy_affine_copy_stats(x.ptr, Cc * (HW - 2), v.ptr, v.ptr, out.ptr, Cc * (HW - 2), st.ptr, Cc, HW - 2, rows, 2, -1, S)),
        (L, lambda: lib.sdy_affine_copy_stats(x.ptr, Cc * HW + 1, v.ptr, v.ptr, out.ptr, Cc * HW, st.ptr, Cc, HW, rows, 2, -1, S)),
        (L, lambda: lib.sdy_affine_copy_stats(x.ptr, Cc * HW, v.ptr, v.ptr, out.ptr, Cc * HW + 1, st.ptr, Cc, HW, rows, 2, -1, S)),
        (L, lambda: lib.sdy_affine_copy_stats(xo.ptr, Cc * HW, v.ptr, v.ptr, out.ptr, Cc * HW, st.ptr, Cc, HW, rows, 2, -1, S)),
        (L, lambda: lib.sdy_affine_copy_stats(x.ptr, Cc * HW, v.ptr, v.ptr, outo.ptr, Cc * HW, st.ptr, Cc, HW, rows, 2, -1, S)),
        (L, lambda: lib.sdy_affine_copy_stats(x.ptr, Cc * HW, v.ptr, v.ptr, out.ptr, Cc * HW, sto.ptr, Cc, HW, rows, 2, -1, S)),
        # sdy_instnorm_from_partials
        (A, lambda: lib.sdy_instnorm_from_partials(None, K, B, Cc, HW, v.ptr, v.ptr, iu.EPS, a.ptr, d.ptr, S)),
        (A, lambda: lib.sdy_instnorm_from_partials(part.ptr, K, B, Cc, HW, None, v.ptr, iu.EPS, a.ptr, d.ptr, S)),
        (A, lambda: lib.sdy_instnorm_from_partials(part.ptr, K, B, Cc, HW, v.ptr, v.ptr, iu.EPS, a.ptr, None, S)),
        (A, lambda: lib.sdy_instnorm_from_partials(part.ptr, 0, B, Cc, HW, v.ptr, v.ptr, iu.EPS, a.ptr, d.ptr, S)),
        (L, lambda: lib.sdy_instnorm_from_partials(part.ptr, K, B, Cc, HW - 2, v.ptr, v.ptr, iu.EPS, a.ptr, d.ptr, S)),
        (L, lambda: lib.sdy_instnorm_from_partials(parto.ptr, K, B, Cc, HW, v.ptr, v.ptr, iu.EPS, a.ptr, d.ptr, S)),
        # sdy_irfft_lon_act
        (A, lambda: lib.sdy_irfft_lon_act(None, Yf.ptr, None, zt.ptr, T, part.ptr, B, Cc, S)),
        (A, lambda: lib.sdy_irfft_lon_act(plan.handle, None, None, zt.ptr, T, part.ptr, B, Cc, S)),
        (A, lambda: lib.sdy_irfft_lon_act(plan.handle, Yf.ptr, None, None, T, part.ptr, B, Cc, S)),
        (A, lambda: lib.sdy_irfft_lon_act(plan.handle, Yf.ptr, None, zt.ptr, T, None, B, Cc, S)),
        (A, lambda: lib.sdy_irfft_lon_act(plan.handle, Yf.ptr, None, zt.ptr, T - 64, part.ptr, B, Cc, S)),
        (L, lambda: lib.sdy_irfft_lon_act(plan.handle, Yf.ptr, None, zt.ptr, T + 2, part.ptr, B, Cc, S)),
        (L, lambda: lib.sdy_irfft_lon_act(plan.handle, Yfo.ptr, None, zt.ptr, T, part.ptr, B, Cc, S)),
        (L, lambda: lib.sdy_irfft_lon_act(plan.handle, Yf.ptr, None, zto.ptr, T, part.ptr, B, Cc, S)),
        (L, lambda: lib.sdy_irfft_lon_act(plan.handle, Yf.ptr, None, zt.ptr, T, parto.ptr, B, Cc, S)),
        (L, lambda: lib.sdy_irfft_lon_act(plan.handle, Yf.ptr, None, zt.ptr, T, part.ptr, B, 6, S)),
        (U_, lambda: lib.sdy_irfft_lon_act(plan.handle, Yf.ptr, None, zt.ptr, T, part.ptr, B, 8, S)),           # C % 16
        (U_, lambda: lib.sdy_irfft_lon_act(plan64.handle, Yf.ptr, None, zt.ptr, T, part.ptr, B, Cc, S)),        # not 360 points
    ]
    for i, (want, call) in enumerate(calls):
        assert call() == want, i
    torch.cuda.synchronize()
    for b in (x, xo, out, outo, zt, zto, st, sto, part, parto, v, a, d, Yf, Yfo):
        assert b.unchanged(), "a refused call wrote something"
    del keep, keep2
