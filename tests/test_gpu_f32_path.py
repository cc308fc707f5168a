"""The fp32 fallback network (gemm_mode="f32", SDY_GEMM_MODE=f32) against the reference and float64 at production sizes.

`gemm_mode="f32"` is the documented way out when the split-fp16 path cannot represent a field (the SdyError raised on
SDY_FLAG_F16_RANGE names it).  At E = 256 it is a separate implementation at nearly every stage: encoder
and decoder as two fp32 GEMM launches each (no pair_h3), the MLP as fc1 -> GELU -> dropout -> fc2 -> dropout -> drop-path
scale -> residual with the hidden activation in HBM and the Philox masks drawn in the GEMM epilogue (gemm_epilogue.h), no
drop-path skip (dropped rows are multiplied by 0), a real inner-skip convolution in every block, the dhconv as a triangular
fp32 GEMM over the expanded complex weight (SDY_TRI_DHCONV), the Legendre transforms as triangular fp32 GEMMs, and 32-bit
lane offsets that cap one native call at sdy_sfno_max_batch = 60 rows at 180 x 360 (not 128).

Every network case here proves it ran that path: `net.gemm_mode == "f32"` and, by the stage timer, the unfused stages once
per block / native call and none of the fused ones (f32_path below) -- a silent fall-through to the default kernels fails.
Bounds: the single-forward (2e-5), single-op (2e-6) and chain (1e-4) bounds of the default path's tests for the global
relative L2; every worst-slice bound about 3x what the MI355X measures (docstrings, NOTEBOOK.md).
"""
import contextlib
import gc

import numpy as np
import pytest
import torch

import golden_utils as gu
import test_gpu_golden as tg
from conftest import rel_l2
from helpers import PhiloxMasks, SliceErrors, make_pair, oracle_sampling_chain
from oracle.sfno import OracleSFNO, SFNOConfig
from test_gpu_production_batches import _chunk, _gen_cuda, _mm, _need, _tie_to_cpu

pytestmark = pytest.mark.gpu

MODE = "f32"
TOL_OP = 2e-6            # single-op bound (tests/test_gpu_ops.py, test_gpu_production_batches.py)
TOL_TIGHT = 2e-5         # single network forward (tests/test_gpu_golden.py, test_gpu_sfno.py)
TOL_NET = 1e-4           # north_star bound: per output channel at full size, every lead time of a sampling pass
NLAT, NLON, E, HID = 180, 360, 256, 512
HW = NLAT * NLON

# Worst-slice / worst-channel bounds: about 3x the worst value measured on the MI355X (docstrings).
# A tile of the wrong dropout row group, a degree missing from the dhconv or an unwritten column tile moves its slice by 1e-2
# or more.
CHAN_FULL_REF = 8e-6     # fx_sfno_full, worst output channel (measured 2.66e-6)
CHAN_B1 = 7e-6           # B = 1 production forward vs the CPU oracle, worst output channel (2.23e-6 / 2.32e-6)
SLICE_NET = 4.5e-6       # production batches vs float64, worst (row, channel) (1.46e-6)
SLICE_CONV = {"fc1": 1.5e-6, "fc2": 1.2e-6, "skip": 9e-7, "enc65": 7e-7, "enc128": 9e-7, "dec0": 1.4e-6, "dec2": 9e-7}
SLICE_DH = 1.4e-6        # (4.65e-7)
SLICE_SHT = 9e-7         # (3.09e-7)
SLICE_ISHT = 7e-7        # (2.42e-7)


@pytest.fixture(autouse=True)
def _free_device_memory():
    yield
    gc.collect()
    torch.cuda.empty_cache()


# ---- the path proof -----------------------------------------------------------------------------------------------------
def check_f32_stages(stages, calls, exact_encoder=True):
    """Stage counts of the forwards issued under sdy_amd.ops.stage_timer (`stages`: {name: (launches, ms)}) for native
    calls of `calls` blocks each: every block launches fc1, fc2, the inner-skip convolution and the fp32 dhconv; every call
    the two-launch encoder (unless a later forward reused the stored encoder output) and decoder; nothing fused."""
    n = {k: v[0] for k, v in stages.items()}
    fused = sorted(k for k in n if k.startswith("mlp fused") or k.endswith("(fused pair)") or
                   k in ("inner skip folded (gelu)", "drop-path copy"))
    assert not fused, f"fused / default-path stages in an f32 forward: {fused} ({n})"
    blocks = sum(calls)
    for st in ("mlp fc1", "mlp fc2", "inner-skip conv", "dhconv"):
        assert n.get(st) == blocks, f"{st}: {n.get(st)} launches, expected one per block ({blocks}): {n}"
    assert n.get("decoder.0 conv") == n.get("decoder.2 conv") == len(calls), n
    enc = n.get("encoder.0 conv", 0)
    assert n.get("encoder.2 conv", 0) == enc, n
    if exact_encoder:
        assert enc == len(calls), n
    else:
        assert 1 <= enc <= len(calls), n


@contextlib.contextmanager
def f32_path(*nets, exact_encoder=True):
    """Around forwards of `nets`: assert they are f32 networks, record the blocks of every native call they issue and
    check the launched stages afterwards (check_f32_stages).  Yields the list of native calls (blocks per call)."""
    import sdy_amd

    for net in nets:     # (at E = 16 both modes launch the same stages: there this is the whole proof)
        assert net.gemm_mode == "f32", f"network built with gemm_mode {net.gemm_mode!r}"
    calls = []
    for net in nets:
        def wrapped(*a, _orig=net._native_call, _blocks=net.num_layers, **k):
            calls.append(_blocks)
            return _orig(*a, **k)
        net._native_call = wrapped
    try:
        with sdy_amd.ops.stage_timer() as t:
            yield calls
    finally:
        for net in nets:
            del net._native_call
    assert calls, "no native forward was issued"
    check_f32_stages(t.stages, calls, exact_encoder)


def _sampler_probe(*nets):
    return f32_path(*nets, exact_encoder=False)     # (the sampler's interpolator pairs may reuse the encoder output)


# ---- 1a: the reference's own vectors (tests/golden) ---------------------------------------------------------------------
@pytest.mark.parametrize("name", ["fx_block_c1", "fx_sfno_tiny", "fx_sfno_tiny_lg"])
def test_reference_goldens_in_f32(name):
    """test_gpu_golden.py::test_network_vs_reference on the f32 network (and its recorded-dropout case for fx_sfno_tiny).
    Measured on the MI355X: 2.35e-7 (fx_block_c1), 5.39e-7 (fx_sfno_tiny; 5.65e-7 with the recorded masks), 3.58e-7
    (fx_sfno_tiny_lg)."""
    z = gu.load(name)
    cfg, n_in, n_cond = gu.cfg_from(z)
    net = tg._net(cfg, n_in, n_cond, gu.state_dict(z), gemm_mode=MODE)
    with f32_path(net):
        y = net(tg._cu(tg._t(z, "x")), time=tg._cu(tg._t(z, "time")), condition=tg._cu(tg._t(z, "cond")))
    err = rel_l2(y, tg._t(z, "y"))
    print(f"[f32 golden] {name}: rel L2 {err:.3e}")
    assert err < TOL_TIGHT, f"{name}: rel L2 {err:.3e}"
    if "t_repr" in z.files:
        trep, _ = net.time_embedding(tg._cu(tg._t(z, "time")))
        assert rel_l2(trep, tg._t(z, "t_repr")) < 2e-6
    if name == "fx_sfno_tiny":
        net.mask_injector = tg._injector(gu.masks_per_forward(gu.recorded_masks(z), cfg), cfg, first_call=net._call)
        net.enable_inference_dropout()
        with f32_path(net):
            yd = net(tg._cu(tg._t(z, "x")), time=tg._cu(tg._t(z, "time")), condition=tg._cu(tg._t(z, "cond")))
        err = rel_l2(yd, tg._t(z, "y_dropout"))
        print(f"[f32 golden] {name} recorded dropout: rel L2 {err:.3e}")
        assert err < TOL_TIGHT, f"{name} with the recorded masks: rel L2 {err:.3e}"


def test_full_size_reference_golden_in_f32():
    """The reference network's own 180 x 360, 8-block output (fx_sfno_full) from the f32 network, with the per-channel check
    of test_gpu_golden.py::test_full_size_network_vs_reference.
    Measured on the MI355X: 2.30e-6, worst output channel 2.66e-6."""
    z = gu.load("fx_sfno_full")
    cfg, n_in, n_cond, sd, x, cond, t = gu.seeded_case(z)
    net = tg._net(cfg, n_in, n_cond, sd, gemm_mode=MODE)
    with f32_path(net):
        y = net(x.cuda(), time=t.cuda(), condition=cond.cuda())
    assert torch.isfinite(y).all()
    ref = tg._t(z, "y")
    err = rel_l2(y, ref)
    worst = max(rel_l2(y[:, c], ref[:, c]) for c in range(ref.shape[1]))
    print(f"[f32 golden] fx_sfno_full: rel L2 {err:.3e}, worst output channel {worst:.3e}")
    assert err < TOL_TIGHT, f"full size vs reference: rel L2 {err:.3e}"
    assert worst < CHAN_FULL_REF, f"worst output channel rel L2 {worst:.3e}"


def test_wide_reference_golden_with_recorded_masks_in_f32():
    """fx_sfno_wide_masks (E = 256, hidden 512) on the f32 network: without dropout, then with the reference's recorded
    dropout and drop-path masks injected -- here they drive the fp32 GEMM epilogue's keep_mask and the drop-path scale.
    Measured on the MI355X: 1.07e-6 without dropout, 1.11e-6 with the recorded masks."""
    z = gu.load("fx_sfno_wide_masks")
    cfg, n_in, n_cond, sd, x, cond, t = gu.seeded_case(z)
    net = tg._net(cfg, n_in, n_cond, sd, gemm_mode=MODE)
    with f32_path(net):
        y = net(x.cuda(), time=t.cuda(), condition=cond.cuda())
    e0 = rel_l2(y, tg._t(z, "y"))
    net.mask_injector = tg._injector(gu.masks_per_forward(gu.recorded_masks(z), cfg), cfg, first_call=net._call)
    net.enable_inference_dropout()
    with f32_path(net):
        yd = net(x.cuda(), time=t.cuda(), condition=cond.cuda())
    e1 = rel_l2(yd, tg._t(z, "y_dropout"))
    print(f"[f32 golden] fx_sfno_wide_masks: rel L2 {e0:.3e} (no dropout), {e1:.3e} (recorded masks)")
    assert e0 < TOL_TIGHT and e1 < TOL_TIGHT, (e0, e1)


@pytest.mark.parametrize("name", ["fx_sample_tiny", "fx_sample_tiny_masks"])
def test_reference_sampler_goldens_in_f32(name):
    """test_gpu_golden.py::test_sampler_vs_reference with both networks in f32 (TOL_TIGHT at every lead time).
    Measured on the MI355X, worst lead time: 2.28e-6 (fx_sample_tiny), 1.42e-6 (fx_sample_tiny_masks)."""
    tg.sampler_vs_reference(name, gemm_mode=MODE, probe=_sampler_probe)


def test_reference_stepper_golden_in_f32():
    """test_gpu_golden.py::test_stepper_vs_reference with both networks in f32.
    Measured on the MI355X, worst variable: 1.28e-6 (normalised), 6.48e-7 (physical units)."""
    tg.stepper_vs_reference(gemm_mode=MODE, probe=_sampler_probe)


# ---- 1b: the production forward, B = 1, full depth, against the CPU oracle ----------------------------------------------
def _interp_cfg(layers, data_grid="equiangular"):
    return SFNOConfig(in_chans=70, out_chans=34, nlat=NLAT, nlon=NLON, embed_dim=E, num_layers=layers, with_time_emb=True,
                      dropout_mlp=0.1, drop_path_rate=0.1, min_time=1.0, max_time=5.0, data_grid=data_grid)


@pytest.mark.parametrize("data_grid", ["equiangular", "legendre-gauss"])
def test_production_forward_b1_vs_oracle(data_grid):
    """The interpolator (68 + 2 -> 34, 180 x 360, E = 256, 8 blocks, time embedding, dropout 0.1, drop path 0.1) in f32 at
    B = 1 against the CPU oracle replaying the Philox stream, on both data grids.  The dropout seed is picked as in
    test_gpu_sfno.py::test_c2_full_size_interpolator_forward_with_dropout: an inner block is dropped whole (f32 multiplies its
    branch by 0 and feeds the residual to the next InstanceNorm) and at least five are kept (seed 5000: blocks 3 and 7
    dropped).  Measured on the MI355X: 2.00e-6 / 2.11e-6 (equiangular / Legendre-Gauss), worst output channel 2.23e-6 /
    2.32e-6."""
    from oracle.philox import drop_path_keep

    cfg = _interp_cfg(8, data_grid)
    rates = cfg.drop_path_rates

    def kept(seed):
        return [bool(drop_path_keep(seed, 0, layer, rates[layer], 1)[0]) for layer in range(8)]

    seed = next(sd for sd in range(5000, 5400) if not all(kept(sd)[1:7]) and sum(kept(sd)) >= 5)
    net, ora, _ = make_pair(cfg, 68, 2, net_seed=seed, gemm_mode=MODE)
    g = torch.Generator(device="cpu").manual_seed(1234)
    x = torch.randn(1, 68, NLAT, NLON, generator=g)
    cond = torch.randn(1, 2, NLAT, NLON, generator=g)
    t = torch.tensor([3.0])
    masks = PhiloxMasks(cfg, seed=seed)
    masks.device = "cuda"
    masks.call = 0
    ref = ora(x, time=t, condition=cond, mask_fn=masks)
    net.enable_inference_dropout()
    with f32_path(net):
        got = net(x.cuda(), time=t.cuda(), condition=cond.cuda())
    assert torch.isfinite(got).all()
    err = rel_l2(got, ref)
    worst = max(rel_l2(got[:, c], ref[:, c]) for c in range(ref.shape[1]))
    print(f"[f32 B=1 {data_grid}] seed {seed} kept {kept(seed)}: rel L2 {err:.3e}, worst output channel {worst:.3e}")
    assert err < TOL_TIGHT, f"f32 full-size forward ({data_grid}): rel L2 {err:.3e}"
    assert worst < CHAN_B1, f"f32 full-size forward ({data_grid}): worst output channel {worst:.3e}"
    again = net(x.cuda(), time=t.cuda(), condition=cond.cuda())       # the masks matter
    assert rel_l2(again, ref) > 1e-3


# ---- 1c: production batches against float64 on the device ---------------------------------------------------------------
def test_production_batches_vs_float64():
    """The interpolator in f32 (3 blocks: both grid changes and one Gauss-grid block; dropout and drop path on) at B = 25, at
    the batch limit of one f32 native call (sdy_sfno_max_batch, read from the library: 60 at 180 x 360, where the Legendre
    synthesis' 32-bit lane offsets reach 99 % of 2^32) and one row beyond it (two native calls), against the oracle's op
    sequence in float64 on the device, every row replaying its own dropout stream (PhiloxMasks.rows).  Global relative L2 and
    the worst (row, channel) slice.  Rows 0, middle and last of the max-batch call against the same trajectory run alone
    (batch_offset = b).
    Measured on the MI355X: max_batch 60; 12 (row, block) pairs dropped whole; global 1.17e-6 (B = 25), 1.16e-6 (B = 60
    and 61), worst slice 1.46e-6 (row 23, channel 16) at every B; the split call's rows equal the one-call rows bit for bit,
    and rows 0, 30, 59 are bit-identical to the lone trajectories."""
    import sdy_amd

    cfg = _interp_cfg(3)
    net_seed = 2024
    net, _, sd = make_pair(cfg, 68, 2, net_seed=net_seed, gemm_mode=MODE)
    h = net._get_native(torch.device("cuda", 0))
    max_b = int(sdy_amd.lib.sdy_sfno_max_batch(h))
    assert 1 < max_b < 128, f"f32 max batch {max_b}: the non-tiled limit is below the drop-path map's 128"
    B = max_b + 1
    _need(int(sdy_amd.lib.sdy_sfno_workspace_floats(h, max_b)) * 4 + 3 * B * (70 + 34) * HW * 4 + (4 << 30))
    gc_ = _gen_cuda(61)
    x = torch.randn(B, 68, NLAT, NLON, device="cuda", generator=gc_)
    cond = torch.randn(B, 2, NLAT, NLON, device="cuda", generator=gc_)
    t = 1.0 + 4.0 * torch.rand(B, device="cuda", generator=gc_)
    net.enable_inference_dropout()
    outs = {}
    for n_rows, n_calls in ((25, 1), (max_b, 1), (B, 2)):
        net.batch_offset, net._call = 0, 0
        with f32_path(net) as calls:
            outs[n_rows] = net(x[:n_rows], time=t[:n_rows], condition=cond[:n_rows])
        assert len(calls) == n_calls, f"B={n_rows}: {len(calls)} native calls"
        assert torch.isfinite(outs[n_rows]).all()
    # the reference: float64 on the device, chunks of rows that keep their trajectory index
    ora = OracleSFNO(cfg, sd, dtype=torch.float64, device="cuda")
    masks = PhiloxMasks(cfg, seed=net_seed)
    masks.device = "cuda"
    masks.call = 0
    errs = {n: SliceErrors() for n in outs}
    ck = _chunk((70 + 6 * E + 2 * HID) * HW * 8)
    dropped = 0
    for r0 in range(0, B, ck):
        r1 = min(B, r0 + ck)
        masks.rows = list(range(r0, r1))
        ref = ora(x[r0:r1], time=t[r0:r1], condition=cond[r0:r1], mask_fn=masks)
        for n, y in outs.items():
            if r0 < n:
                errs[n].add(y[r0:min(r1, n)], ref[:min(r1, n) - r0], rows=range(r0, min(r1, n)))
        del ref
    from oracle.philox import drop_path_keep
    for layer in range(cfg.num_layers):
        dropped += int((drop_path_keep(net_seed, 0, layer, cfg.drop_path_rates[layer], B) == 0).sum())
    assert dropped > 0, "no trajectory lost a block to drop path"
    res = {n: errs[n].result() for n in outs}
    print(f"[f32 batches] max_batch {max_b}, {dropped} dropped (row, block) pairs; " +
          ", ".join(f"B={n}: global {g_:.3e} worst slice {w:.3e} at {i}" for n, (g_, w, i) in res.items()))
    alone = {}
    for b in (0, max_b // 2, max_b - 1):
        net.batch_offset, net._call = b, 0
        y1 = net(x[b:b + 1], time=t[b:b + 1], condition=cond[b:b + 1])[0]
        alone[b] = (torch.equal(y1, outs[max_b][b]), rel_l2(outs[max_b][b], y1))
    print(f"[f32 batches] rows of the max-batch call vs the lone trajectories (bitwise, rel L2): {alone}")
    for n in outs:
        errs[n].check(f"f32 interpolator B={n}", TOL_TIGHT, SLICE_NET)
    assert torch.equal(outs[max_b], outs[B][:max_b]), "the split into two native calls changed rows"
    for b, (same, e) in alone.items():
        assert same, f"row {b}: batch row differs from the lone trajectory (rel L2 {e:.3e})"


# ---- 1d: the f32 kernels alone at production batch, against torch float64 on the device ---------------------------------
BATCHES = [1, 25, 100]
# name: (Cin, Cout, bias, gelu, pre_affine, add_mode, dropout kind or None, batch_scale)
CONV_CASES = {
    "fc1": (E, HID, True, True, True, 0, 0, False),          # MLP fc1: norm1 affine, bias, GELU, dropout (stream 2 l)
    "fc2": (HID, E, True, False, False, 2, 1, True),         # MLP fc2: bias, dropout (stream 2 l + 1), drop-path scale, residual
    "skip": (E, E, True, True, False, 1, None, False),       # inner skip: GELU(conv + bias + filter output)
    "enc65": (65, E, True, True, False, 0, None, False),     # encoder.0 of the forecaster (63 + 2 inputs)
    "enc128": (128, E, True, True, False, 0, None, False),   # encoder.0 of the interpolator (126 + 2 inputs)
    "dec0": (E + 128, E, True, True, False, 0, None, False),  # decoder.0: [block output | inputs] -> 256
    "dec2": (E, 63, False, False, False, 0, None, False),    # decoder.2: 256 -> 63 state channels
}


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("case", list(CONV_CASES))
def test_conv1x1_f32_production_batches(case, B):
    """ops.conv1x1 on its default fp32 GEMM (no packed weights) at 180 x 360 in every form the f32 network issues, against
    a float64 dgemm on the device.  With dropout the Philox stream runs at call 5, layer 3, batch_offset 70 (trajectories at
    and above 64): the output's zeros are exactly the zeros of oracle.philox.element_keep_mask_torch (fc1), and the reference
    applies those masks (both).  fc2's drop-path scale holds zeros: those rows are exactly the residual.
    Measured on the MI355X over B = 1 / 25 / 100: global 1.8e-7 (enc65) .. 3.9e-7 (dec0); worst slice 4.86e-7 (fc1),
    3.89e-7 (fc2), 2.90e-7 (skip), 2.32e-7 (enc65), 2.93e-7 (enc128), 4.78e-7 (dec0), 3.08e-7 (dec2).  Besides the dropped
    elements, one or two kept elements per 1e9 come out exactly 0 (fp32 bias and accumulator cancel; float64 |value| < 1e-7)."""
    import sdy_amd
    from oracle.philox import element_keep_mask_torch

    F = torch.nn.functional
    Cin, Cout, has_bias, gelu, affine, add_mode, kind, scaled = CONV_CASES[case]
    _need(B * (Cin + 3 * Cout) * HW * 4 + 4 * (2 << 30))
    g = torch.Generator(device="cpu").manual_seed(300 + Cin + Cout)
    w = torch.randn(Cout, Cin, generator=g) / np.sqrt(Cin)
    b = 0.1 * torch.randn(Cout, generator=g) if has_bias else None
    gc_ = _gen_cuda(400 + B)
    x = torch.randn(B, Cin, NLAT, NLON, device="cuda", generator=gc_) * 1.3 + 0.1
    pa = (1 + 0.2 * torch.randn(B, Cin, device="cuda", generator=gc_)) if affine else None
    pd = (0.2 * torch.randn(B, Cin, device="cuda", generator=gc_)) if affine else None
    add = torch.randn(B, Cout, NLAT, NLON, device="cuda", generator=gc_) if add_mode else None
    bs = None
    if scaled:
        bs = 1 + 0.25 * torch.randn(B, device="cuda", generator=gc_)
        bs[1::3] = 0.0                                  # rows whose MLP branch drop path removed
    p, seed, call, layer, boff = 0.1, 0x0123456789ABCDEF, 5, 3, 70
    kw = dict(pre_affine=None if pa is None else (pa, pd), add=add, add_mode=add_mode, gelu=gelu, batch_scale=bs,
              kernel_tag={"fc1": 1, "fc2": 2, "skip": 3}.get(case, 0))
    if kind is not None:
        kw.update(drop_p=p, seed=seed, call=call, stream_id=2 * layer + kind, batch_offset=boff)
    out = sdy_amd.ops.conv1x1(x, w[:, :, None, None], b, **kw)
    wd = w.double().cuda()
    bd = None if b is None else b.double().cuda()

    def ref(r0, r1, keep=None, dev="cuda"):
        f64 = dict(device=dev, dtype=torch.float64)
        xa = x[r0:r1].to(**f64)
        if affine:
            xa = xa * pa[r0:r1, :, None, None].to(**f64) + pd[r0:r1, :, None, None].to(**f64)
        y = F.conv2d(xa, w.double()[:, :, None, None]) if dev == "cpu" else _mm(wd, xa)
        if b is not None:
            y = y + b.double().to(dev)[None, :, None, None]
        if add_mode == 1:
            y = y + add[r0:r1].to(**f64)
        if gelu:
            y = F.gelu(y)
        if keep is not None:
            y = y * keep.to(**f64) / (1.0 - p)
        if bs is not None:
            y = y * bs[r0:r1, None, None, None].to(**f64)
        if add_mode == 2:
            y = y + add[r0:r1].to(**f64)
        return y

    def keep_of(r0, r1):
        if kind is None:
            return None
        return element_keep_mask_torch(seed, call, layer, kind, p, r1 - r0, Cout, NLAT, NLON, batch_offset=boff + r0,
                                       device="cuda").cuda()

    se = SliceErrors()
    ck = _chunk((Cin + 4 * Cout) * HW * 8)
    for r0 in range(0, B, ck):
        r1 = min(B, r0 + ck)
        keep = keep_of(r0, r1)
        want = ref(r0, r1, keep)
        se.add(out[r0:r1], want)
        if kind is not None and add_mode == 0:
            # Every dropped element is 0, and every other 0 is a kept element whose pre-activation is 0 to fp32 rounding
            # (|GELU| < 1e-6 in float64: bias + accumulator cancel exactly now and then, a few per 1e9 elements)
            o = out[r0:r1]
            extra = (o == 0) & (keep != 0) & (want.abs() >= 1e-6 / (1.0 - p))     # kept, not tiny, but zero
            missing = (o != 0) & (keep == 0)                                      # dropped but not zero
            if extra.any() or missing.any():
                pre = ref(r0, r1)                   # the undropped float64 output at those elements
                raise AssertionError(
                    f"{case} B={B} rows {r0}..{r1}: the zeros of the output are not the dropped elements of the Philox "
                    f"oracle: {int(extra.sum())} kept elements are 0 (float64 values {pre[extra][:8].tolist()} at "
                    f"{extra.nonzero()[:4].tolist()}), {int(missing.sum())} dropped elements are not (values "
                    f"{o[missing][:8].tolist()} at {missing.nonzero()[:4].tolist()})")
        del keep, want
    se.check(f"conv1x1 f32 {case} B={B}", TOL_OP, SLICE_CONV[case])
    if bs is not None and B > 1:
        z = (bs == 0).nonzero().reshape(-1)
        assert len(z) and torch.equal(out[z], add[z]), f"{case}: rows with drop-path scale 0 are not the residual"
    k = keep_of(B - 1, B)
    _tie_to_cpu(ref(B - 1, B, k), ref(B - 1, B, None if k is None else k.cpu(), dev="cpu"), f"conv1x1 f32 {case}")


@pytest.mark.parametrize("B", BATCHES)
def test_contract_dhconv_f32_full_degree_range(B):
    """contract_dhconv(gemm_mode="f32") -- the triangular fp32 GEMM over the expanded complex weight (SDY_TRI_DHCONV, rows
    (m, b) with m <= l) -- at L = 180, M = 181, E = 256, against a complex128 contraction on the device; errors per
    (row, degree).  Measured on the MI355X: global 4.05e-7 at every B; worst slice 4.65e-7 (B = 100, degree 0)."""
    import sdy_amd

    L, M = NLAT, NLON // 2 + 1
    g = torch.Generator(device="cpu").manual_seed(5)
    w = torch.randn(E, E, L, 2, generator=g) / np.sqrt(E)
    x = torch.randn(B, E, L, M, dtype=torch.complex64, device="cuda", generator=_gen_cuda(105))
    x = x * (torch.arange(M, device="cuda")[None, :] <= torch.arange(L, device="cuda")[:, None])
    got = sdy_amd.ops.contract_dhconv(x, w.cuda(), gemm_mode=MODE)
    wc = torch.view_as_complex(w.double().contiguous()).cuda()
    se = SliceErrors(keep=(0, 2), what="(row, degree)")
    ck = _chunk(3 * E * L * M * 16)
    for r0 in range(0, B, ck):
        se.add(got[r0:r0 + ck], torch.einsum("bixy,iox->boxy", x[r0:r0 + ck].to(torch.complex128), wc))
    se.check(f"dhconv f32 B={B}", TOL_OP, SLICE_DH)
    cpu = torch.einsum("bixy,iox->boxy", x[-1:].cpu().to(torch.complex128), torch.view_as_complex(w.double().contiguous()))
    _tie_to_cpu(torch.einsum("bixy,iox->boxy", x[-1:].to(torch.complex128), wc), cpu, "dhconv f32")


@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("grid", ["legendre-gauss", "equiangular"])
def test_sht_f32_both_directions_network_width(grid, B):
    """RealSHT / InverseRealSHT(gemm_mode="f32") -- rfft + the triangular fp32 Legendre GEMMs (SDY_TRI_LEG_FWD / _INV) --
    at C = 256 against the oracle's transforms in float64 on the device; forward errors per (row, degree), inverse per
    (row, channel).  Measured on the MI355X, both grids: global 2.34e-7 (forward), 2.23e-7 .. 2.25e-7 (inverse); worst
    slice 3.09e-7 (forward, equiangular, B = 100), 2.42e-7 (inverse, equiangular, B = 100)."""
    import sdy_amd
    from oracle.sht import InverseRealSHT as OInv, RealSHT as OFwd

    L, M = NLAT, NLON // 2 + 1
    fwd_ref = OFwd(NLAT, NLON, lmax=L, mmax=M, grid=grid).cuda()
    x = torch.randn(B, E, NLAT, NLON, device="cuda", generator=_gen_cuda(171))
    fwd = sdy_amd.RealSHT(NLAT, NLON, lmax=L, mmax=M, grid=grid, gemm_mode=MODE)
    assert fwd._plan(x.device) is sdy_amd.sht.ShtPlan.get(NLAT, NLON, L, M, grid, 0, MODE)
    got = fwd(x)
    se = SliceErrors(keep=(0, 2), what="(row, degree)")
    ck = _chunk(6 * E * HW * 8)
    for r0 in range(0, B, ck):
        se.add(got[r0:r0 + ck], fwd_ref(x[r0:r0 + ck].double()))
    se.check(f"RealSHT f32 {grid} B={B}", TOL_OP, SLICE_SHT)
    _tie_to_cpu(fwd_ref(x[-1:].double()), OFwd(NLAT, NLON, lmax=L, mmax=M, grid=grid)(x[-1:].cpu().double()),
                "RealSHT")
    del x, got
    inv_ref = OInv(NLAT, NLON, lmax=L, mmax=M, grid=grid).cuda()
    c = torch.randn(B, E, L, M, dtype=torch.complex64, device="cuda", generator=_gen_cuda(172))
    goti = sdy_amd.InverseRealSHT(NLAT, NLON, lmax=L, mmax=M, grid=grid, gemm_mode=MODE)(c)
    se = SliceErrors()
    for r0 in range(0, B, ck):
        se.add(goti[r0:r0 + ck], inv_ref(c[r0:r0 + ck].to(torch.complex128)))
    se.check(f"InverseRealSHT f32 {grid} B={B}", TOL_OP, SLICE_ISHT)
    _tie_to_cpu(inv_ref(c[-1:].to(torch.complex128)),
                OInv(NLAT, NLON, lmax=L, mmax=M, grid=grid)(c[-1:].cpu().to(torch.complex128)), "InverseRealSHT")


# ---- 1e: a full sampling pass in f32 against the float64 chain ----------------------------------------------------------
def test_sampling_pass_f32_vs_float64_chain():
    """One horizon-6 DYffusion sampling pass at production width and depth (180 x 360, E = 256, 8 blocks, interpolator
    dropout and drop path on) with both networks in f32, against the oracle's op sequence in float64 on the device
    (test_gpu_fullsize.py::test_c3_chain_error_against_a_float64_yardstick's chain, one weight draw): 1e-4 at every lead time.
    Measured on the MI355X: 3.1e-6, 6.1e-6, 1.2e-5, 1.7e-5, 3.0e-5, 5.3e-5 at t1 .. t6 (the chain's amplification of one
    forward's rounding, as on the default path)."""
    import sdy_amd

    C_STATE, C_FORC, HZ = 63, 2, 6
    sf, si = 4321, 4322
    fcfg = SFNOConfig(in_chans=C_STATE + C_FORC, out_chans=C_STATE, nlat=NLAT, nlon=NLON, embed_dim=E, num_layers=8,
                      with_time_emb=True, min_time=0.0, max_time=HZ - 1.0)
    icfg = SFNOConfig(in_chans=2 * C_STATE + C_FORC, out_chans=C_STATE, nlat=NLAT, nlon=NLON, embed_dim=E, num_layers=8,
                      with_time_emb=True, dropout_mlp=0.1, drop_path_rate=0.1, min_time=1.0, max_time=HZ - 1.0)
    fnet, _, fsd = make_pair(fcfg, C_STATE, C_FORC, seed=sf, gemm_mode=MODE)
    inet, _, isd = make_pair(icfg, 2 * C_STATE, C_FORC, seed=si, net_seed=1000 + sf, gemm_mode=MODE)
    exp = sdy_amd.MultiHorizonForecastingDYffusion(fnet, sdy_amd.InterpolationExperiment(inet, horizon=HZ), horizon=HZ)
    g = torch.Generator(device="cpu").manual_seed(sf)
    x0 = torch.randn(1, C_STATE, NLAT, NLON, generator=g)
    forc = torch.randn(1, C_FORC, NLAT, NLON, generator=g)
    with _sampler_probe(fnet, inet):
        got = {k: v.cpu() for k, v in exp.model.sample(x0.cuda(), static_condition=forc.cuda()).items()}
    assert (fnet._call, inet._call) == (6, 10)
    ref64 = oracle_sampling_chain(fcfg, fsd, icfg, isd, 1000 + sf, x0, forc, torch.float64, HZ)
    keys = [f"t{k}_preds" for k in range(1, HZ + 1)]
    assert sorted(got) == sorted(ref64) == sorted(keys)
    err = {k: rel_l2(got[k], ref64[k]) for k in keys}
    print("[f32 chain] rel L2 vs the float64 chain:", {k: f"{v:.2e}" for k, v in err.items()})
    for k in keys:
        assert torch.isfinite(got[k]).all()
        assert err[k] < TOL_NET, f"{k}: f32 path {err[k]:.3e} from the float64 chain (bound 1e-4)"
