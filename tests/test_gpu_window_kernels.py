"""The stepper and aggregator kernels of csrc/pointwise.hip one by one, through the C entry points, against plain torch float64
restatements written from include/sdy_amd.h (tests/window_kernels_utils.py holds the reductions' restatements and tolerances).

Shapes (window_kernels_utils.SHAPES): 5 x 12 (HW4 = 15: one partial workgroup), 9 x 116 (HW4 = 261: one full workgroup plus
five threads), 67 x 248 (16616 pixels: 17 workgroups against lp_terms_kernel's cap of 16, 65 against the ensemble kernels' cap
of 64, so a second grid-stride pass of 58 float4 / 232 pixels; a non-full last span in the gradient kernel).  B = 3, T1 = 4.

Element-wise kernels: every element is compared.  Copies and selections are bit for bit; arithmetic is held to a bound summed
along the operation chain in float64, each fp32 operation contributing at most U = 2^-24 times the magnitude of its float64
result (its inputs' errors carried through), with no margin on top.  Every buffer a kernel sees sits inside a larger allocation
with a guard band of 64 elements on both sides; outputs start as NaN.  A test asserts that no NaN is left where the kernel
writes, that everything else still is NaN, and that every guard band is untouched."""
import contextlib
import ctypes as C
import math

import numpy as np
import pytest
import torch

import window_kernels_utils as wk

pytestmark = pytest.mark.gpu

U, B, T1 = wk.U, wk.B, wk.T1
GUARD, GUARD_VALUE, NAN = 64, -777.25, float("nan")


class Buf:
    """A device tensor `t` of `shape` inside a larger allocation: GUARD elements of GUARD_VALUE on both sides (`offset` more in
    front, so that `offset = 1` gives a float view 4 bytes off a 16-byte boundary that is still in bounds).  `fill`: a value, or
    a CPU tensor to copy."""

    def __init__(self, shape, fill=NAN, dtype=torch.float32, offset=0):
        n = math.prod(shape)
        self.raw = torch.full((n + 2 * GUARD + offset,), GUARD_VALUE, dtype=dtype, device="cuda")
        self.lo, self.hi = GUARD + offset, GUARD + offset + n
        self.t = self.raw[self.lo:self.hi].view(shape)
        if isinstance(fill, torch.Tensor):
            self.t.copy_(fill.reshape(shape).to(dtype))
        else:
            self.t.fill_(fill)
        assert self.t.data_ptr() % 16 == (offset * self.raw.element_size()) % 16
        self.before = self.t.clone()

    @property
    def ptr(self):
        return self.t.data_ptr()

    def guards_intact(self):
        return bool((self.raw[:self.lo] == GUARD_VALUE).all()) and bool((self.raw[self.hi:] == GUARD_VALUE).all())

    def unchanged(self):
        return self.guards_intact() and bits_equal(self.t, self.before)


def bits_equal(a, b):
    view = torch.int32 if a.dtype == torch.float32 else torch.int64
    return a.shape == b.shape and torch.equal(a.contiguous().view(view).cpu(), b.contiguous().view(view).cpu())


def lib_and_stream():
    import sdy_amd
    from sdy_amd._lib import current_stream

    return sdy_amd.lib, current_stream()


def within(got, ref, bound, what):
    """Element by element |got - ref| <= bound (float64 CPU tensors), no NaN in got; prints the worst ratio."""
    assert not bool(torch.isnan(got).any()), f"{what}: sentinel left in the output"
    err = (got - ref).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max())
    print(f"{what}: worst |err| / bound = {ratio:.3f}, worst |err| = {float(err.max()):.3e}")
    assert bool((err <= bound).all()), f"{what}: |err| / bound up to {ratio:.3f}"


def var_data(nvars, HW, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return [(0.3 + 1.7 * torch.randn(B, T1, HW, generator=g)) * wk.STDS[v] + wk.MEANS[v] for v in range(nvars)]


def table(bufs):
    from sdy_amd._lib import SdyVarTable

    t = SdyVarTable()
    t.nvars = len(bufs)
    for v, b in enumerate(bufs):
        t.data[v], t.mean[v], t.std[v] = b.ptr, wk.MEANS[v], wk.STDS[v]
    return t


def norm64(x, v):
    """float64 (x - mean) / std of variable v and its bound: two operations, U |x - mean| / |std| + U |result| = 2 U
    |result|."""
    m, s = wk.f32(wk.MEANS[v]), wk.f32(wk.STDS[v])
    a = x.double() - m
    y = a / s
    return y, U * a.abs() / s.abs() + U * y.abs()


def denorm64(y, mean, std):
    """float64 y * std + mean from the fp32 y the device stored, and its bound: U |y std| + U |result| (one term less if the
    compiler contracts the two into an FMA)."""
    m, s = wk.f32(mean), wk.f32(std)
    p = y.double() * s
    return p + m, U * p.abs() + U * (p + m).abs()


# ---- normalise + pack -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", wk.SHAPES)
def test_norm_pack(H, W):
    """norm_pack_kernel: the partial last workgroup (`i >= HW4`) at 5 x 12 (HW4 = 15) and 9 x 116 (HW4 = 261), 17 workgroups
    with a partial last one at 67 x 248 (HW4 = 4154); t = 0 and t = T1 - 1; the stepper's (B * T1, 1) flattening of one
    variable.  Bound: 2 U |result|."""
    lib, stream = lib_and_stream()
    HW, nv = H * W, 5
    data = var_data(nv, HW, 11)
    bufs = [Buf((B, T1, HW), x) for x in data]
    tab = table(bufs)
    for t in (0, T1 - 1):
        out = Buf((B, nv, HW))
        assert lib.sdy_norm_pack(C.byref(tab), t, T1, B, HW, out.ptr, stream) == 0
        got = out.t.cpu().double()
        for v in range(nv):
            y, bound = norm64(data[v][:, t], v)
            within(got[:, v], y, bound, f"norm_pack {H}x{W} t={t} v={v}")
        assert out.guards_intact() and all(b.unchanged() for b in bufs)
    from sdy_amd._lib import SdyVarTable

    for v in (0, 2):
        one = SdyVarTable()
        one.nvars, one.data[0], one.mean[0], one.std[0] = 1, bufs[v].ptr, wk.MEANS[v], wk.STDS[v]
        out = Buf((B * T1, 1, HW))
        assert lib.sdy_norm_pack(C.byref(one), 0, 1, B * T1, HW, out.ptr, stream) == 0
        y, bound = norm64(data[v].reshape(B * T1, HW), v)
        within(out.t.cpu().double()[:, 0], y, bound, f"norm_pack {H}x{W} flattened v={v}")
        assert out.guards_intact() and bufs[v].unchanged()


@pytest.mark.parametrize("H,W", wk.SHAPES)
def test_init_timeline(H, W):
    """init_timeline_kernel: the partial last workgroup at 5 x 12 and 9 x 116, 17 workgroups (the last partial) at 67 x 248.
    Slot 0 of the normalised timeline within 2 U |result|, of the denormalised one within U |y std| + U |result| of the float64
    value of the stored y; slots 1 .. T1 - 1 of both stay as they were."""
    lib, stream = lib_and_stream()
    HW, nv = H * W, 4
    data = var_data(nv, HW, 12)
    bufs = [Buf((B, T1, HW), x) for x in data]
    tln, tld = [Buf((B, T1, HW)) for _ in range(nv)], [Buf((B, T1, HW)) for _ in range(nv)]
    pn, pd = (C.c_void_p * nv)(*[b.ptr for b in tln]), (C.c_void_p * nv)(*[b.ptr for b in tld])
    assert lib.sdy_init_timeline(C.byref(table(bufs)), T1, B, HW, pn, pd, stream) == 0
    for v in range(nv):
        gn, gd = tln[v].t.cpu(), tld[v].t.cpu()
        y, bound = norm64(data[v][:, 0], v)
        within(gn[:, 0].double(), y, bound, f"init_timeline {H}x{W} norm v={v}")
        d, bound = denorm64(gn[:, 0], wk.MEANS[v], wk.STDS[v])
        within(gd[:, 0].double(), d, bound, f"init_timeline {H}x{W} denorm v={v}")
        assert bool(torch.isnan(gn[:, 1:]).all()) and bool(torch.isnan(gd[:, 1:]).all())
        assert tln[v].guards_intact() and tld[v].guards_intact() and bufs[v].unchanged()


# ---- step finish --------------------------------------------------------------------------------------------------------------
# entry: (out_idx, in_idx).  In-and-out entries in different orders in the two packers, an input-only entry that is NOT the
# first input (carried over from prev_in), an output-only (diagnostic) entry; entry 2 is the prescribed one.
ENTRIES = ((2, 1), (-1, 2), (0, 0), (1, -1), (3, 3))
PRESC = 2
MASK_SET = (-0.5, 0.0, 0.5, 1.0, 1.5, 2.5)


@pytest.mark.parametrize("mode,use_ar,t", [
    ("none", False, 1), ("none", True, T1 - 1),
    ("interp", False, 1), ("interp", True, T1 - 1),
    ("mask0", False, T1 - 1), ("mask0", True, 1),
    ("mask1", False, 1), ("mask1", True, T1 - 1)])
def test_step_finish(mode, use_ar, t):
    """step_finish_kernel at 9 x 116 (HW4 = 261: the partial last workgroup), t = 1 and t = T1 - 1, ar_init set and unset.
    Entries: in-and-out in different packer orders, output-only (in_idx < 0), input-only carried over from prev_in at in_idx 2
    (not HGTsfc at index 0).  Prescriber: off; interpolating with a fractional mask (four operations on top of the two of the
    normalised target); not interpolating with mask_value 0 and 1 and masks from {-0.5, 0, 0.5, 1, 1.5, 2.5}, where rintf (half
    to even) must agree with torch.round -- bit for bit, the normalised target being the two IEEE operations (x - mean) / std.
    With ar_init the timeline receives the prescribed PREDICTION and next_in the prescribed ar_init.  Timeline slot t is
    checked, every other slot must be untouched, next_in is checked in full."""
    from sdy_amd._lib import SdyStepFinishArgs

    lib, stream = lib_and_stream()
    H, W = wk.SHAPES[1]
    HW, n_out, n_in = H * W, 4, 4
    g = torch.Generator(device="cpu").manual_seed(100 + t + 10 * use_ar + 97 * len(mode))
    gen = 0.3 + 1.7 * torch.randn(B, n_out, HW, generator=g)
    ar = 0.3 + 1.7 * torch.randn(B, n_out, HW, generator=g)
    prev = torch.randn(B, n_in, HW, generator=g)
    target = (0.3 + 1.7 * torch.randn(B, T1, HW, generator=g)) * wk.STDS[PRESC] + wk.MEANS[PRESC]
    if mode == "interp":
        mask = torch.rand(B, T1, HW, generator=g)
    else:
        mask = torch.tensor(MASK_SET)[torch.randint(0, len(MASK_SET), (B, T1, HW), generator=g)]
    b_gen, b_ar, b_prev, b_target, b_mask = (Buf(x.shape, x) for x in (gen, ar, prev, target, mask))
    b_next = Buf((B, n_in, HW))
    tln = {e: Buf((B, T1, HW)) for e, (oi, _) in enumerate(ENTRIES) if oi >= 0}
    tld = {e: Buf((B, T1, HW)) for e in tln}

    a = SdyStepFinishArgs()
    a.B, a.HW, a.T1, a.t = B, HW, T1, t
    a.gen, a.n_out, a.prev_in, a.next_in, a.n_in, a.n_entries = b_gen.ptr, n_out, b_prev.ptr, b_next.ptr, n_in, len(ENTRIES)
    for e, (oi, ii) in enumerate(ENTRIES):
        a.out_idx[e], a.in_idx[e], a.mean[e], a.std[e] = oi, ii, wk.MEANS[e], wk.STDS[e]
        if oi >= 0:
            a.gen_norm_tl[e], a.gen_tl[e] = tln[e].ptr, tld[e].ptr
    a.presc_entry = -1
    if mode != "none":
        a.presc_entry, a.presc_target, a.presc_mask = PRESC, b_target.ptr, b_mask.ptr
        a.interpolate, a.mask_value = (1, 1) if mode == "interp" else (0, int(mode[-1]))
    a.ar_init = b_ar.ptr if use_ar else None
    assert lib.sdy_step_finish(C.byref(a), stream) == 0

    got_next = b_next.t.cpu()
    assert not bool(torch.isnan(got_next).any())
    m32, s32 = torch.tensor(wk.MEANS[PRESC], dtype=torch.float32), torch.tensor(wk.STDS[PRESC], dtype=torch.float32)
    for e, (oi, ii) in enumerate(ENTRIES):
        what = f"step_finish {mode} ar={use_ar} t={t} entry {e}"
        if oi < 0:
            assert bits_equal(got_next[:, ii], prev[:, ii]), f"{what}: carried over"
            continue
        gn, gd = tln[e].t.cpu(), tld[e].t.cpu()
        pred, fb = gen[:, oi], (ar if use_ar else gen)[:, oi]
        if e != PRESC or mode == "none":
            assert bits_equal(gn[:, t], pred), f"{what}: normalised timeline"
            if ii >= 0:
                assert bits_equal(got_next[:, ii], fb), f"{what}: next_in"
        elif mode == "interp":
            tn, tn_err = norm64(target[:, t], PRESC)
            mk = mask[:, t].double()
            q = 1.0 - mk
            for got, x, label in ((gn[:, t], pred, "normalised timeline"), (got_next[:, ii], fb, "next_in")):
                p1, p2 = mk * tn, q * x.double()
                # mk * tn: mk times tn's error + U |mk tn|;  q = 1 - mk: U |q|, times |x|;  q * x: U |q x|;  the sum: U |result|
                bound = mk.abs() * tn_err + U * p1.abs() + 2 * U * p2.abs() + U * (p1 + p2).abs()
                within(got.double(), p1 + p2, bound, f"{what}: {label}")
        else:
            on = torch.round(mask[:, t]) == float(mode[-1])
            assert 0.1 < float(on.float().mean()) < 0.9
            tn = (target[:, t] - m32) / s32
            assert bits_equal(gn[:, t], torch.where(on, tn, pred)), f"{what}: normalised timeline"
            assert bits_equal(got_next[:, ii], torch.where(on, tn, fb)), f"{what}: next_in"
        d, bound = denorm64(gn[:, t], wk.MEANS[e], wk.STDS[e])
        within(gd[:, t].double(), d, bound, f"{what}: denormalised timeline")
        other = [s for s in range(T1) if s != t]
        assert bool(torch.isnan(gn[:, other]).all()) and bool(torch.isnan(gd[:, other]).all()), f"{what}: another slot written"
        assert tln[e].guards_intact() and tld[e].guards_intact()
    assert b_next.guards_intact() and all(b.unchanged() for b in (b_gen, b_ar, b_prev, b_target, b_mask))


# ---- concat, cold update, noise fill --------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", wk.SHAPES)
def test_concat_channels(H, W):
    """concat_kernel: the partial last workgroup at 5 x 12 and 9 x 116, 17 workgroups (the last partial) at 67 x 248; two,
    three and four sources of unequal widths; bit for bit torch.cat."""
    lib, stream = lib_and_stream()
    HW = H * W
    g = torch.Generator(device="cpu").manual_seed(13)
    for chans in ((2, 1), (2, 1, 3), (1, 3, 1, 2)):
        srcs = [torch.randn(B, c, HW, generator=g) for c in chans]
        bufs = [Buf(x.shape, x) for x in srcs]
        out = Buf((B, sum(chans), HW))
        ps, cs = (C.c_void_p * len(chans))(*[b.ptr for b in bufs]), (C.c_int * len(chans))(*chans)
        assert lib.sdy_concat_channels(ps, cs, len(chans), out.ptr, B, HW, stream) == 0
        assert bits_equal(out.t, torch.cat(srcs, dim=1))
        assert out.guards_intact() and all(b.unchanged() for b in bufs)


@pytest.mark.parametrize("n", [1, 3, 6483, 2_098_355])
@pytest.mark.parametrize("with_ip_s", [True, False])
@pytest.mark.parametrize("offset", [0, 1])
def test_cold_update(n, with_ip_s, offset):
    """cold_update_kernel bit for bit against torch fp32 a + (b - c): n = 1 and 3 (scalar tail only), 6483 (tail of 3 after 1620
    float4), 2 098 355 = 2 097 152 + 1203 (the grid of 2048 workgroups takes a second stride pass, then a tail of 3); with
    x_ip_s and without (c = a).  offset = 1: x_ip_next starts 4 bytes off a 16-byte boundary and the scalar loop takes the whole
    range (for the largest n in several stride passes)."""
    lib, stream = lib_and_stream()
    g = torch.Generator(device="cpu").manual_seed(n)
    a, b, c = (torch.randn(n, generator=g) for _ in range(3))
    ba, bb, bc = Buf((n,), a), Buf((n,), b, offset=offset), Buf((n,), c)
    out = Buf((n,))
    assert lib.sdy_cold_update(ba.ptr, bb.ptr, bc.ptr if with_ip_s else None, out.ptr, n, stream) == 0
    assert bits_equal(out.t, a + (b - (c if with_ip_s else a)))
    assert out.guards_intact() and ba.unchanged() and bb.unchanged() and bc.unchanged()


@pytest.mark.parametrize("H,W", wk.SHAPES)
def test_cond_noise_fill(H, W):
    """cond_noise_kernel: the partial last workgroup at 5 x 12 (HW4 = 15), 9 x 116 (HW4 = 261) and 67 x 248 (HW4 = 4154 = 16
    x 256 + 58).  Every float4 is compared at the two small shapes; at 67 x 248 (37 386 host calls otherwise) the first 8, every
    61st and all of the last workgroup's 58 float4 of every plane -- and no NaN anywhere.  The words come from the
    library's host evaluation of its generator (sdy_dropout_stream_words) at the counters include/sdy_amd.h gives; Box-Muller in
    float64; 1e-5 absolute as tests/test_gpu_fcond.py derives it (log, sqrt, sincospi in fp32 on |eps| <= 5.77)."""
    lib, stream = lib_and_stream()
    HW, Cc, seed, call, boff, rpc = H * W, 3, 0x0123456789ABCDEF, 7, 5, 0
    out = Buf((B, Cc, HW))
    assert lib.sdy_cond_noise_fill(seed, call, boff, rpc, B, Cc, HW, out.ptr, stream) == 0
    HW4 = HW // 4
    qs = list(range(HW4)) if HW4 < 1000 else sorted(set(range(8)) | set(range(0, HW4, 61)) | set(range(HW4 - 58, HW4)))
    words = np.zeros((B, Cc, len(qs), 4), dtype=np.uint64)
    w4 = (C.c_uint32 * 4)()
    for b in range(B):
        for c in range(Cc):
            for j, q in enumerate(qs):
                ctr = (q, (b + boff) * Cc + c, 0x2000, call)
                assert lib.sdy_dropout_stream_words(*ctr, seed & 0xFFFFFFFF, seed >> 32, w4) == 0
                words[b, c, j] = list(w4)
    u = ((words >> np.uint64(8)) + np.uint64(1)).astype(np.float64) * 2.0 ** -24
    r0, r1 = np.sqrt(-2 * np.log(u[..., 0])), np.sqrt(-2 * np.log(u[..., 2]))
    want = np.stack([r0 * np.cos(2 * np.pi * u[..., 1]), r0 * np.sin(2 * np.pi * u[..., 1]),
                     r1 * np.cos(2 * np.pi * u[..., 3]), r1 * np.sin(2 * np.pi * u[..., 3])], axis=-1)
    got = out.t.cpu().double().numpy()
    assert not np.isnan(got).any()
    got = got.reshape(B, Cc, HW4, 4)[:, :, qs]
    err = np.abs(got - want).max()
    print(f"cond_noise_fill {H}x{W}: max |err| {err:.3e}")
    assert err < 1e-5 and out.guards_intact()


# ---- LpLoss terms --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", wk.SHAPES)
@pytest.mark.parametrize("t", [0, T1 - 1])
@pytest.mark.parametrize("preloaded", [False, True])
def test_lp_rel_terms(H, W, t, preloaded):
    """lp_terms_kernel: 67 x 248 gives 17 workgroups of float4 against the cap of 16, so the first workgroup takes a second
    grid-stride pass (58 float4); 5 x 12 and 9 x 116 the partial workgroup.  t = 0 and T1 - 1; accumulation into zeros and into
    known non-zero terms; the row after the last b must not be disturbed.  Tolerance: 4 x the float32 restatement's measured
    error, relative to the float64 sum of the terms (all non-negative) -- window_kernels_utils.YARD."""
    lib, stream = lib_and_stream()
    HW = H * W
    gen, data = wk.lp_case(H, W)
    want = wk.lp_sums(wk.lp_terms(gen, data, t, torch.float64))
    b_gen, bufs = Buf(gen.shape, gen), [Buf(x.shape, x) for x in data]
    pre = (1000.5 + 3.25 * torch.arange(2.0 * (B + 1), dtype=torch.float64).reshape(B + 1, 2)) if preloaded \
        else torch.zeros(B + 1, 2, dtype=torch.float64)
    terms = Buf((B + 1, 2), pre, dtype=torch.float64)
    assert lib.sdy_lp_rel_terms(b_gen.ptr, C.byref(table(bufs)), t, T1, B, HW, terms.ptr, stream) == 0
    got = terms.t.cpu()
    tol = wk.KERNEL_FACTOR * wk.YARD[("lp", 0)]
    rel = ((got[:B] - pre[:B]) - want).abs() / want
    print(f"lp_rel_terms {H}x{W} t={t} preloaded={preloaded}: worst error / sum|terms| {float(rel.max()):.3e} "
          f"(allowed {tol:.1e})")
    assert bool((rel <= tol).all())
    assert bits_equal(got[B], pre[B]) and terms.guards_intact() and b_gen.unchanged() and all(b.unchanged() for b in bufs)


# ---- ensemble diagnostics -----------------------------------------------------------------------------------------------
def ensemble_call(kernel, M, H, W, layout, claim_M=None):
    """One call (or, for sdy_ensemble_metrics on the transposed layout, one call per sample) into an `out` preloaded with known
    values.  layout "contiguous": pred stored (M, n_sample, T, HW); "transposed": stored (n_sample, M, T, HW) as the window
    driver keeps its batch, handed over through the strides of the transposed view, with truth a slice of a (n_sample, T + 1, HW)
    buffer.  Returns (return code, out after, out before, buffers)."""
    lib, stream = lib_and_stream()
    pred, truth, w = wk.ens_case(M, H, W)
    S, T, HW, nq = wk.N_SAMPLE, wk.T_ENS, H * W, wk.N_SUMS[kernel]
    pred, truth = pred.reshape(M, S, T, HW), truth.reshape(S, T, HW)
    if layout == "contiguous":
        b_pred, ms, ss = Buf(pred.shape, pred), S * T * HW, T * HW
        b_truth, truth_ptr, ts = Buf(truth.shape, truth), None, T * HW
        truth_ptr = b_truth.ptr
    else:
        stored = pred.transpose(0, 1).contiguous()
        b_pred, ms, ss = Buf(stored.shape, stored), T * HW, M * T * HW
        padded = torch.zeros(S, T + 1, HW)
        padded[:, 1:] = truth
        b_truth, ts = Buf(padded.shape, padded), (T + 1) * HW
        truth_ptr = b_truth.ptr + 4 * HW
    b_w = Buf((HW,), w)
    pre = 1000.5 + 3.25 * torch.arange(float(S * T * nq), dtype=torch.float64).reshape(S, T, nq)
    out = Buf((S, T, nq), pre, dtype=torch.float64)
    Mc = claim_M or M
    if kernel == "metrics" and layout == "contiguous":
        rc = lib.sdy_ensemble_metrics(b_pred.ptr, truth_ptr, b_w.ptr, Mc, ms, S * T, HW, out.ptr, stream)
    elif kernel == "metrics":
        rc = 0
        for s in range(S):
            rc = rc or lib.sdy_ensemble_metrics(b_pred.ptr + 4 * s * ss, truth_ptr + 4 * s * ts, b_w.ptr, Mc, ms, T, HW,
                                                out.ptr + 8 * s * T * nq, stream)
    elif kernel == "series":
        rc = lib.sdy_ensemble_series(b_pred.ptr, Mc, ms, ss, truth_ptr, ts, b_w.ptr, S, T, HW, out.ptr, stream)
    else:
        rc = lib.sdy_ensemble_series_grad(b_pred.ptr, Mc, ms, ss, truth_ptr, ts, b_w.ptr, S, T, H, W, out.ptr, stream)
    return rc, out.t.cpu(), pre, (out, b_pred, b_truth, b_w)


@pytest.mark.parametrize("layout", ["contiguous", "transposed"])
@pytest.mark.parametrize("H,W", wk.ENS_SHAPES)
@pytest.mark.parametrize("M", wk.ENS_M)
@pytest.mark.parametrize("kernel", ["metrics", "series", "grad"])
def test_ensemble_sums(kernel, M, H, W, layout):
    """ens_metrics_kernel, ens_series_pass<false> and <true> (sdy_ensemble_metrics / _series / _series_grad): M = 1 (the `crps =
    skill`, `var = 0` branch), 2, 25 and 64 = ENS_MAX; 9 x 116 (one full workgroup and a partial one) and 67 x 248 (65
    workgroups of pixels against the cap of 64: the second grid-stride pass of 232 pixels; for the gradient kernel span = 512
    with a last span of 488); n_sample = 2, T = 3, non-uniform weights; the strides of a contiguous tensor and of the
    window driver's transposed view; atomicAdd into a preloaded `out`.  Each sum within 4 x the float32 restatement's measured
    error (window_kernels_utils.YARD[(kernel, M)]) of the float64 sum, relative to the float64 sum of its absolute terms."""
    rc, got, pre, bufs = ensemble_call(kernel, M, H, W, layout)
    assert rc == 0
    nq = wk.N_SUMS[kernel]
    want, scale = (v[..., :nq] for v in wk.ens_reference(M, H, W))
    tol = wk.KERNEL_FACTOR * wk.YARD[(kernel, M)]
    err = ((got - pre) - want).abs()
    rel = err / scale.clamp_min(1e-300)
    print(f"{kernel} M={M} {H}x{W} {layout}: worst error / sum|terms| per sum "
          f"{[f'{float(v):.1e}' for v in rel.amax(dim=(0, 1))]} (allowed {tol:.1e})")
    assert bool((err <= tol * scale).all())
    if M == 1:
        pred, truth, w = wk.ens_case(M, H, W)
        mae = (w.double() * (pred[0].double() - truth.double()).abs()).sum(dim=(2, 3))
        assert bits_equal(got[..., 1], pre[..., 1]), "var of a single member must be exactly 0"
        assert bool((((got - pre)[..., 2] - mae).abs() <= tol * mae).all()), "CRPS of a single member is its weighted |x - t|"
    assert all(b.guards_intact() for b in bufs) and all(b.unchanged() for b in bufs[1:])


@pytest.mark.parametrize("kernel", ["metrics", "series", "grad"])
def test_ensemble_refuses_65_members(kernel):
    """M = 65 > ENS_MAX: SDY_ERR_UNSUPPORTED from all three entry points, `out` untouched."""
    rc, got, pre, bufs = ensemble_call(kernel, 2, *wk.ENS_SHAPES[0], "contiguous", claim_M=65)
    assert rc == -2 and bits_equal(got, pre) and all(b.unchanged() for b in bufs)


# ---- time mean ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", wk.SHAPES)
@pytest.mark.parametrize("n0,n1", [(1, 3), (4, 2)])
@pytest.mark.parametrize("t0", [0, 1])
def test_time_mean_accumulate(H, W, n0, n1, t0):
    """time_mean_kernel: the partial last workgroup at 5 x 12 and 9 x 116, 17 workgroups at 67 x 248; (members, samples) =
    (1, 3) and (4, 2) read through the strides of a transposed (samples, members, ...) buffer; t0 = 0 and 1; into a non-zero `acc`.
    Per pixel |got - float64| <= (n + 1) U (scale sum|x| + |acc|) with n = n0 n1 (T - t0) summed values: n - 1 additions, the
    product with scale and the addition to acc, each at most U times a magnitude that sum bounds."""
    lib, stream = lib_and_stream()
    HW, T = H * W, T1
    g = torch.Generator(device="cpu").manual_seed(17 * n0 + t0)
    x = 0.3 + 1.7 * torch.randn(n1, n0, T, HW, generator=g)          # stored sample-major: member stride T HW, sample stride n0 T HW
    acc0 = torch.randn(HW, generator=g)
    bx, acc = Buf(x.shape, x), Buf((HW,), acc0)
    n = n0 * n1 * (T - t0)
    scale = 1.0 / n
    assert lib.sdy_time_mean_accumulate(bx.ptr, n0, T * HW, n1, n0 * T * HW, t0, T, HW, scale, acc.ptr, stream) == 0
    s64 = wk.f32(scale)
    xs = x[:, :, t0:].double()
    want = acc0.double() + s64 * xs.sum(dim=(0, 1, 2))
    bound = (n + 1) * U * (s64 * xs.abs().sum(dim=(0, 1, 2)) + acc0.double().abs())
    within(acc.t.cpu().double(), want, bound, f"time_mean {H}x{W} n0={n0} n1={n1} t0={t0}")
    assert acc.guards_intact() and bx.unchanged()


# ---- alignment ----------------------------------------------------------------------------------------------------------------
def test_entry_points_refuse_a_buffer_offset_by_one_float():
    """Real device buffers that start 4 bytes off a 16-byte boundary (allocated with slack: in bounds), in turn as an input and
    as an output of every float4 entry point: SDY_ERR_ALIGN, and nothing is written (the check precedes the launch)."""
    from sdy_amd._lib import SdyStepFinishArgs

    lib, stream = lib_and_stream()
    H, W = wk.SHAPES[0]
    HW, nv = H * W, 2
    data = var_data(nv, HW, 19)
    good = [Buf((B, T1, HW), x) for x in data]
    bad = [good[0], Buf((B, T1, HW), data[1], offset=1)]
    out, out_off = Buf((B, nv, HW)), Buf((B, nv, HW), offset=1)
    assert lib.sdy_norm_pack(C.byref(table(bad)), 0, T1, B, HW, out.ptr, stream) == -3
    assert lib.sdy_norm_pack(C.byref(table(good)), 0, T1, B, HW, out_off.ptr, stream) == -3
    assert lib.sdy_lp_rel_terms(out_off.ptr, C.byref(table(good)), 0, T1, B, HW, Buf((B, 2), 0.0, torch.float64).ptr, stream) == -3
    terms = Buf((B, 2), 0.0, torch.float64)
    missing = table(good)
    missing.data[1] = None
    assert lib.sdy_lp_rel_terms(out.ptr, C.byref(missing), 0, T1, B, HW, terms.ptr, stream) == -1        # a NULL variable
    assert lib.sdy_lp_rel_terms(Buf((B, nv, HW), 1.0).ptr, C.byref(table(bad)), 0, T1, B, HW, terms.ptr, stream) == -3
    tl = [Buf((B, T1, HW)) for _ in range(4)]
    tl_off = Buf((B, T1, HW), offset=1)
    ptrs = lambda *b: (C.c_void_p * len(b))(*[x.ptr for x in b])      # noqa: E731
    assert lib.sdy_init_timeline(C.byref(table(bad)), T1, B, HW, ptrs(tl[0], tl[1]), ptrs(tl[2], tl[3]), stream) == -3
    assert lib.sdy_init_timeline(C.byref(table(good)), T1, B, HW, ptrs(tl[0], tl_off), ptrs(tl[2], tl[3]), stream) == -3
    assert lib.sdy_init_timeline(C.byref(table(good)), T1, B, HW, ptrs(tl[0], tl[1]), ptrs(tl_off, tl[3]), stream) == -3
    acc, acc_off = Buf((HW,), 0.5), Buf((HW,), 0.5, offset=1)
    assert lib.sdy_time_mean_accumulate(bad[1].ptr, 1, 0, B, T1 * HW, 0, T1, HW, 1.0, acc.ptr, stream) == -3
    assert lib.sdy_time_mean_accumulate(good[1].ptr, 1, 0, B, T1 * HW, 0, T1, HW, 1.0, acc_off.ptr, stream) == -3
    cat, cat_off = Buf((B, 2 * T1, HW)), Buf((B, 2 * T1, HW), offset=1)
    ch = (C.c_int * 2)(T1, T1)
    assert lib.sdy_concat_channels(ptrs(*bad), ch, 2, cat.ptr, B, HW, stream) == -3
    assert lib.sdy_concat_channels(ptrs(*good), ch, 2, cat_off.ptr, B, HW, stream) == -3
    noise_off = Buf((B, 2, HW), offset=1)
    assert lib.sdy_cond_noise_fill(1, 0, 0, 0, B, 2, HW, noise_off.ptr, stream) == -3

    # two entries: in-and-out (prescribed), and input-only, carried over from prev_in
    gen, gen_off = Buf((B, 1, HW), 1.0), Buf((B, 1, HW), 1.0, offset=1)
    nxt, nxt_off = Buf((B, 2, HW)), Buf((B, 2, HW), offset=1)
    prev, prev_off = Buf((B, 2, HW), 2.0), Buf((B, 2, HW), 2.0, offset=1)
    for wrong in ("gen", "next_in", "prev_in", "ar_init", "presc_target", "presc_mask", "gen_norm_tl", "gen_tl"):
        a = SdyStepFinishArgs()
        a.B, a.HW, a.T1, a.t, a.n_out, a.n_in, a.n_entries = B, HW, T1, 1, 1, 2, 2
        a.out_idx[0], a.in_idx[0], a.mean[0], a.std[0] = 0, 1, 0.0, 1.0
        a.out_idx[1], a.in_idx[1], a.mean[1], a.std[1] = -1, 0, 0.0, 1.0
        a.presc_entry, a.mask_value, a.interpolate = 0, 1, 0
        a.gen = (gen_off if wrong == "gen" else gen).ptr
        a.next_in = (nxt_off if wrong == "next_in" else nxt).ptr
        a.prev_in = (prev_off if wrong == "prev_in" else prev).ptr
        a.ar_init = (gen_off if wrong == "ar_init" else gen).ptr
        a.presc_target = (bad if wrong == "presc_target" else good)[1].ptr
        a.presc_mask = (bad if wrong == "presc_mask" else good)[1].ptr
        a.gen_norm_tl[0] = (tl_off if wrong == "gen_norm_tl" else tl[0]).ptr
        a.gen_tl[0] = (tl_off if wrong == "gen_tl" else tl[1]).ptr
        assert lib.sdy_step_finish(C.byref(a), stream) == -3, wrong
    torch.cuda.synchronize()
    everything = good + bad + tl + [out, out_off, terms, tl_off, acc, acc_off, cat, cat_off, noise_off, gen, gen_off, nxt, nxt_off,
                                   prev, prev_off]
    assert all(b.unchanged() for b in everything)


def shifted(x):
    """A contiguous view with x's values that starts 4 bytes off a 16-byte boundary (`.contiguous()` returns it as it is)."""
    buf = torch.zeros(x.numel() + 1, dtype=x.dtype, device=x.device)
    buf[1:] = x.reshape(-1)
    out = buf[1:].view(x.shape)
    assert out.data_ptr() % 16 == 4 and out.is_contiguous()
    return out


def test_python_callers_copy_a_misaligned_view():
    """TimeMeanAggregator.record_batch (flat and member-stacked), ops.cold_update and ops.concat_channels fed one-float-offset
    views of larger tensors give, bit for bit, what they give on aligned copies."""
    import sdy_amd

    H, W = wk.SHAPES[0]
    g = torch.Generator(device="cpu").manual_seed(23)
    w = (0.2 + torch.rand(H, W, generator=g)).cuda()
    tgt = {"x": torch.randn(2, T1, H, W, generator=g).cuda()}
    gen = {"x": torch.randn(3, 2, T1, H, W, generator=g).cuda()}
    maps = []
    for f in (lambda v: v, shifted):
        agg = sdy_amd.metrics.TimeMeanAggregator(w, is_ensemble=True)
        for i0 in (0, T1):
            agg.record_batch(0.0, {k: f(v) for k, v in tgt.items()}, {k: f(v) for k, v in gen.items()}, None, None, i_time_start=i0)
        maps.append(agg.time_mean_maps())
    for kind in ("gen", "target"):
        assert bits_equal(maps[0][kind]["x"], maps[1][kind]["x"])
    a, b, c = (torch.randn(B, 2, H, W, generator=g).cuda() for _ in range(3))
    assert bits_equal(sdy_amd.ops.cold_update(shifted(a), b, shifted(c)), a + (b - c))
    assert bits_equal(sdy_amd.ops.concat_channels([a, shifted(b), c]), torch.cat([a, b, c], dim=1))


def test_network_copies_a_misaligned_input():
    """sdy_sfno_forward concatenates its inputs with the float4 concat kernel and so refuses a misaligned one; the network's
    forward copies such a view.  The smallest network of the suite (32 x 64, embed_dim 16, two blocks, no dropout): inputs and
    condition as one-float-offset views give the output on aligned tensors -- to 1e-6 relative L2, not bit for bit: the
    InstanceNorm statistics are float64 atomics whose order changes from launch to launch, which can move an fp32 coefficient
    by an ulp (6e-8)."""
    from helpers import make_pair
    from oracle.sfno import SFNOConfig

    cfg = SFNOConfig(in_chans=5, out_chans=3, nlat=32, nlon=64, embed_dim=16, num_layers=2, with_time_emb=True, min_time=0.0,
                     max_time=5.0)
    net, _, _ = make_pair(cfg, 3, 2, seed=11)
    g = torch.Generator(device="cpu").manual_seed(37)
    x, cond = torch.randn(2, 3, 32, 64, generator=g).cuda(), torch.randn(2, 2, 32, 64, generator=g).cuda()
    time = torch.tensor([1.0, 3.0]).cuda()
    want = net(x, time=time, condition=cond).clone()
    got = net(shifted(x), time=time, condition=shifted(cond))
    err = float((got.double() - want.double()).norm() / want.double().norm())
    assert not bool(torch.isnan(got).any()) and err < 1e-6, err


class FakeModule:
    """The smallest module the stepper accepts: one step per window, the prediction an affine function of the state, handed back
    (like the autoregressive initial state) as a view 4 bytes off a 16-byte boundary."""
    true_horizon, model = 1, None
    ema_scope = inference_dropout_scope = staticmethod(contextlib.nullcontext)

    def get_preds_at_t_for_batch(self, batch, horizon, **kw):
        x = batch["dynamics"]
        return {f"t{horizon}_preds_normed": shifted(0.5 * x + 0.25), "preds_autoregressive_init_normed": shifted(0.25 * x - 1.0)}


def run_stepper(data):
    import sdy_amd

    names = ["a", "b", "c"]
    means, stds = {n: wk.MEANS[i] for i, n in enumerate(names)}, {n: wk.STDS[i] for i, n in enumerate(names)}
    stepper = sdy_amd.MultiStepStepper(FakeModule(), names, names, [], means, stds, sdy_amd.Prescriber("b", "frac", 1, True))
    return stepper.run_on_batch(data, None, n_forward_steps=1)


def test_stepper_copies_a_misaligned_view():
    """MultiStepStepper's `_table` path (sdy_init_timeline, sdy_norm_pack, sdy_lp_rel_terms, sdy_step_finish with an
    interpolating prescriber and ar_init): every variable of the window, the module's prediction and its autoregressive initial
    state arrive as one-float-offset views; one step at 9 x 116.  Bit for bit the timelines of the run on aligned copies (the
    loss terms sum their workgroups' float64 partial sums in any order: 1e-12 relative on the terms, one float32 ulp on the
    float32 losses made of them)."""
    H, W = wk.SHAPES[1]
    g = torch.Generator(device="cpu").manual_seed(29)
    data = {n: ((0.3 + 1.7 * torch.randn(B, 2, H, W, generator=g)) * wk.STDS[i] + wk.MEANS[i]).cuda()
            for i, n in enumerate(["a", "b", "c"])}
    data["frac"] = torch.rand(B, 2, H, W, generator=g).cuda()
    want, got = run_stepper(data), run_stepper({k: shifted(v) for k, v in data.items()})
    for n in ("a", "b", "c"):
        assert not bool(torch.isnan(got.gen_data[n]).any())
        assert bits_equal(got.gen_data[n], want.gen_data[n]) and bits_equal(got.gen_data_norm[n], want.gen_data_norm[n])
        assert bits_equal(got.target_data_norm[n], want.target_data_norm[n])
    # (float32 of a float64 that differs by the order of a few double additions: one float32 ulp at the most, and only if the
    #  float64 values straddle a rounding boundary; the float64 terms themselves are compared through the per-step losses)
    for k in ("loss", "loss_step_0"):
        assert abs(float(got.metrics[k]) - float(want.metrics[k])) <= 2.0 ** -23 * float(want.metrics[k]), k
    tg, tw = got.metrics._terms.double(), want.metrics._terms.double()
    assert bool(((tg - tw).abs() <= 1e-12 * tw).all())


def test_grids_that_are_no_multiple_of_four():
    """7 x 10 (HW = 70): the stepper and TimeMeanAggregator still raise SdyError (the float4 kernels refuse HW % 4 != 0),
    MeanAggregator still works (its kernels read scalars): weighted_rmse against float64."""
    import sdy_amd

    H, W, S, T = 7, 10, 2, 3
    g = torch.Generator(device="cpu").manual_seed(31)
    data = {n: torch.randn(B, 2, H, W, generator=g).cuda() for n in ("a", "b", "c", "frac")}
    with pytest.raises(sdy_amd.SdyError):
        run_stepper(data)
    w = 0.2 + torch.rand(H, W, generator=g)
    tgt, gen = torch.randn(S, T, H, W, generator=g), torch.randn(3, S, T, H, W, generator=g)
    with pytest.raises(sdy_amd.SdyError):
        sdy_amd.metrics.TimeMeanAggregator(w.cuda(), is_ensemble=True).record_batch(0.0, {"x": tgt.cuda()}, {"x": gen.cuda()},
                                                                                     None, None)
    agg = sdy_amd.metrics.MeanAggregator(w.cuda(), n_timesteps=T, is_ensemble=True)
    agg.record_batch(0.0, {"x": tgt.cuda()}, {"x": gen.cuda()}, None, None, i_time_start=0)
    sums, _ = wk.ens_sums(wk.ens_terms(gen, tgt, w, torch.float64))
    want = (sums[..., 0] / w.double().sum()).sqrt().mean(dim=0)
    got = agg.get_series()["weighted_rmse/x"].cpu()
    assert torch.allclose(got, want, rtol=1e-6, atol=0.0), (got, want)
