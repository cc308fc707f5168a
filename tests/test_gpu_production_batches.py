"""The fused kernels alone at the production grid and batch sizes, against float64.

tests/test_gpu_ops.py holds every kernel to fp64 at grids up to 87 x 96 and B <= 3, where a persistent workgroup walks at
most a few 64-pixel tiles.  The benchmark runs them at 180 x 360 (1013 tiles per image, the last one half full: 64800 =
1012.5 x 64) and B = 25 .. 128, where each workgroup walks a contiguous range of t_per = ceil(B * 1013 / workgroups) tiles
and crosses image boundaries inside it (mlp_h3.hip, conv_h3.hip, pair_h3.hip: per-image coefficients reloaded, statistics
flushed).  Here every kernel runs at those sizes against torch float64 on the device (rocBLAS dgemm, torch.fft: no project
kernel), which is itself tied to the CPU float64 oracle on one row, and every case bounds both the global relative L2
(TOL_OP, the single-op bound) and the worst (row, channel) or (row, degree) slice: one wrong row out of B moves the global
number by only ~1 / sqrt(B).  The per-slice bounds are set from what the MI355X measures (in each docstring).

The network part runs the interpolator at the native batch limit (one call of 128 rows) and through the Python split of a
larger batch into near-equal native calls.
"""
import gc

import numpy as np
import pytest
import torch

from conftest import rel_l2
from helpers import PhiloxMasks, SliceErrors, make_pair
from oracle.sfno import SFNOConfig

pytestmark = pytest.mark.gpu

TOL_OP = 2e-6            # single-op bound of tests/test_gpu_ops.py
TOL_NET_TIGHT = 2e-5     # full-size single forward vs the oracle (tests/test_gpu_sfno.py)
NLAT, NLON, E, HID = 180, 360, 256, 512
HW = NLAT * NLON
TN = 64                                # pixels per tile of mlp_h3 / conv_h3 / pair_h3
TPI = -(-HW // TN)                     # 1013 tiles per image (a prime: see _batch)
REF_BYTES = 2 << 30                    # float64 working set of one reference chunk
BATCHES = ["1", "25", "100", "edge", "straddle"]

# Worst-slice bounds: about 3x the worst slice measured on the MI355X over every batch size of the case (docstrings).
# A tile computed with the wrong image's coefficients, or a dropped half tile, moves its (row, channel) slice by ~1e-2.
SLICE_CONV256 = 6e-7
SLICE_CONV_CIN = 8e-7
SLICE_MLP = 1e-6
SLICE_PAIR = 1.2e-6
SLICE_DH = 9e-7
SLICE_SHT = 5e-7
SLICE_ISHT = 5e-7


@pytest.fixture(scope="module")
def sdy():
    import sdy_amd

    return sdy_amd


@pytest.fixture(autouse=True)
def _free_device_memory():
    yield
    gc.collect()
    torch.cuda.empty_cache()


def _workgroups(kernel, cin=E):
    """Workgroups of the persistent launch: mlp_h3 / pair_h3 one per CU; conv_h3 two per CU in its 4-wave form
    (Cin <= 256) and one in its 8-wave form (Cin > 256) -- ConvCfg::WGS in conv_h3.hip."""
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    if kernel == "conv":
        return n_cu * (2 if cin <= 256 else 1)
    return n_cu


def _ranges(B, G):
    """[t_begin, t_end) of every workgroup, as the kernels split B * TPI tiles over min(tiles, G) workgroups."""
    nt = B * TPI
    g = min(nt, G)
    t_per = -(-nt // g)
    return [(w * t_per, min(nt, (w + 1) * t_per)) for w in range(g) if w * t_per < nt]


def _batch(which, G):
    """The batch sizes of the parametrisation.  'edge': t_per = ceil(B * 1013 / G) is a multiple of 1013 only when B is a
    multiple of G (1013 is prime and larger than G), so B = G is the smallest batch at which workgroup ranges end exactly on
    image boundaries -- there, every range is one whole image.  'straddle': B = G / 2 + 1 gives ranges of a little more
    than half an image (511 tiles at G = 256), so ranges begin and end inside images and cross image boundaries mid-range,
    the half-filled last tile of the image included."""
    if which == "edge":
        B = G
        assert all(e % TPI == 0 for _, e in _ranges(B, G))
    elif which == "straddle":
        B = G // 2 + 1
        r = _ranges(B, G)
        assert all(e % TPI != 0 for _, e in r[:-1])
        assert sum(1 for s, e in r if s // TPI != (e - 1) // TPI) >= G // 4   # ranges holding an image boundary
    else:
        B = int(which)
    return B


def _crossing_rows(B, G, n=3):
    """Batch rows on both sides of the first image boundaries that fall inside a workgroup's range."""
    rows = []
    for s, e in _ranges(B, G):
        if s // TPI != (e - 1) // TPI:
            rows += [s // TPI, (e - 1) // TPI]
        if len(rows) >= 2 * n:
            break
    return rows


def _need(nbytes):
    free, _ = torch.cuda.mem_get_info()
    if free < nbytes:
        pytest.skip(f"needs {nbytes / 2**30:.1f} GiB of free device memory, {free / 2**30:.1f} GiB free")


def _chunk(row_bytes):
    return max(1, int(REF_BYTES // row_bytes))


def _gen_cuda(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _mm(w, x):
    """float64 1x1 convolution on the device: (Cout, Cin) @ (b, Cin, H, W) by dgemm."""
    b, cin, h, wd = x.shape
    return torch.matmul(w, x.to(torch.float64).reshape(b, cin, h * wd)).reshape(b, w.shape[0], h, wd)


def _check_stats(st, out, name, rows_per_chunk=8):
    """(sum, sumsq) per (row, channel) from the epilogue == float64 sums of the kernel's own output (rtol 1e-5 as
    test_gpu_ops.py)."""
    B = out.shape[0]
    for r0 in range(0, B, rows_per_chunk):
        od = out[r0:r0 + rows_per_chunk].double()
        want = torch.stack([od.sum((2, 3)), (od * od).sum((2, 3))], -1)
        got = st[r0:r0 + rows_per_chunk]
        bad = ~torch.isclose(got, want, rtol=1e-5, atol=1e-6 * HW)
        if bad.any():
            b, c, k = (int(v) for v in bad.nonzero()[0])
            raise AssertionError(f"{name}: statistics of row {r0 + b}, channel {c} ({'sum' if k == 0 else 'sumsq'}): "
                                 f"{float(got[b, c, k]):.9e} vs float64 {float(want[b, c, k]):.9e}")


def _tie_to_cpu(dev_ref_row, cpu_ref_row, name):
    """The device float64 reference of one row == the CPU float64 one (ties the dgemm / torch.fft path to the oracle)."""
    e = rel_l2(dev_ref_row, cpu_ref_row)
    assert e < 1e-12, f"{name}: device float64 reference vs CPU float64: {e:.3e}"


# ---- conv_h3: the 256 -> 256 persistent convolution ------------------------------------------------------------------
@pytest.mark.parametrize("which", BATCHES)
def test_conv256_inner_skip_and_encoder_forms(sdy, which):
    """conv_h3 at 180 x 360, 256 -> 256: the inner-skip form GELU(conv(pa * x + pd) + bias + add) with statistics, and
    the encoder form conv(x) + broadcast addend with statistics.
    Measured on the MI355X over B = 1 / 25 / 100 / 512 (edge) / 257 (straddle): global 1.69e-7 .. 1.71e-7 (inner skip),
    1.57e-7 (encoder form); worst slice 2.06e-7 (inner skip, B = 257), 1.71e-7 (encoder form)."""
    F = torch.nn.functional
    G = _workgroups("conv", E)
    B = _batch(which, G)
    _need(3 * B * E * HW * 4 + 4 * REF_BYTES)
    g = torch.Generator(device="cpu").manual_seed(31)
    w = torch.randn(E, E, generator=g) / np.sqrt(E)
    b = 0.1 * torch.randn(E, generator=g)
    pe = torch.randn(1, E, NLAT, NLON, generator=g)
    gc_ = _gen_cuda(131)
    x = torch.randn(B, E, NLAT, NLON, device="cuda", generator=gc_) * 1.4 + 0.1
    add = torch.randn(B, E, NLAT, NLON, device="cuda", generator=gc_)
    pa = 1 + 0.2 * torch.randn(B, E, device="cuda", generator=gc_)
    pd = 0.2 * torch.randn(B, E, device="cuda", generator=gc_)
    frag = sdy.ops.pack_conv256(w[:, :, None, None], "cuda")
    wd, bd, ped = w.double().cuda(), b.double().cuda(), pe.double().cuda()

    st = torch.zeros(B, E, 2, dtype=torch.float64, device="cuda")
    out = sdy.ops.conv1x1(x, w[:, :, None, None], b, pre_affine=(pa, pd), add=add, add_mode=1, gelu=True,
                          frag_prepared=frag, stats=st)

    def ref_skip(r0, r1, dev="cuda"):
        xa = x[r0:r1].to(dev, torch.float64) * pa[r0:r1, :, None, None].to(dev, torch.float64) \
            + pd[r0:r1, :, None, None].to(dev, torch.float64)
        if dev == "cpu":
            y = F.conv2d(xa, w.double()[:, :, None, None], b.double())
        else:
            y = _mm(wd, xa) + bd[None, :, None, None]
        return F.gelu(y + add[r0:r1].to(dev, torch.float64))

    se = SliceErrors()
    ck = _chunk(4 * E * HW * 8)
    for r0 in range(0, B, ck):
        se.add(out[r0:r0 + ck], ref_skip(r0, min(B, r0 + ck)))
    se.check(f"conv_h3 inner skip B={B}", TOL_OP, SLICE_CONV256)
    _tie_to_cpu(ref_skip(B - 1, B), ref_skip(B - 1, B, "cpu"), "conv_h3 inner skip")
    _check_stats(st, out, f"conv_h3 inner skip B={B}")
    del add, out, st

    st = torch.zeros(B, E, 2, dtype=torch.float64, device="cuda")
    out = sdy.ops.conv1x1(x, w[:, :, None, None], None, add=pe.cuda(), add_mode=2, frag_prepared=frag, stats=st)
    se = SliceErrors()
    for r0 in range(0, B, ck):
        se.add(out[r0:r0 + ck], _mm(wd, x[r0:r0 + ck]) + ped)
    se.check(f"conv_h3 encoder form B={B}", TOL_OP, SLICE_CONV256)
    _check_stats(st, out, f"conv_h3 encoder form B={B}")


@pytest.mark.parametrize("which", BATCHES)
@pytest.mark.parametrize("Cin", [65, 128, 321, 384])
def test_conv_cin_to_256_persistent(sdy, Cin, which):
    """The Cin -> 256 persistent convolution (the encoders' first layers 65 / 128, the decoder's 321 / 384 in the 8-wave
    form) at 180 x 360: bias + GELU, and without bias with statistics.
    Measured on the MI355X over B = 1 / 25 / 100 / edge / straddle: global 1.2e-7 (Cin = 65) .. 2.5e-7 (Cin = 384);
    worst slice 1.65e-7 (65), 1.88e-7 (128), 2.79e-7 (321), 2.84e-7 (384, bias + GELU, B = 25)."""
    F = torch.nn.functional
    G = _workgroups("conv", Cin)
    B = _batch(which, G)
    _need(B * (Cin + 2 * E) * HW * 4 + 4 * REF_BYTES)
    g = torch.Generator(device="cpu").manual_seed(47)
    w = torch.randn(E, Cin, generator=g) / np.sqrt(Cin)
    b = 0.1 * torch.randn(E, generator=g)
    x = torch.randn(B, Cin, NLAT, NLON, device="cuda", generator=_gen_cuda(147)) * 1.3 - 0.2
    frag = sdy.ops.pack_conv256(w[:, :, None, None], "cuda")
    wd, bd = w.double().cuda(), b.double().cuda()
    out = sdy.ops.conv1x1(x, w[:, :, None, None], b, gelu=True, frag_prepared=frag)
    se = SliceErrors()
    ck = _chunk((Cin + 3 * E) * HW * 8)
    for r0 in range(0, B, ck):
        se.add(out[r0:r0 + ck], F.gelu(_mm(wd, x[r0:r0 + ck]) + bd[None, :, None, None]))
    se.check(f"conv Cin={Cin} bias+gelu B={B}", TOL_OP, SLICE_CONV_CIN)
    cpu = F.gelu(F.conv2d(x[-1:].cpu().double(), w.double()[:, :, None, None], b.double()))
    _tie_to_cpu(F.gelu(_mm(wd, x[-1:]) + bd[None, :, None, None]), cpu, f"conv Cin={Cin}")
    del out
    st = torch.zeros(B, E, 2, dtype=torch.float64, device="cuda")
    out = sdy.ops.conv1x1(x, w[:, :, None, None], None, frag_prepared=frag, stats=st)
    se = SliceErrors()
    for r0 in range(0, B, ck):
        se.add(out[r0:r0 + ck], _mm(wd, x[r0:r0 + ck]))
    se.check(f"conv Cin={Cin} plain B={B}", TOL_OP, SLICE_CONV_CIN)
    _check_stats(st, out, f"conv Cin={Cin} B={B}")


# ---- mlp_h3: the fused MLP --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", BATCHES)
@pytest.mark.parametrize("drop", [0.0, 0.1])
def test_mlp_fused_production_batches(sdy, drop, which):
    """mlp_fused at 180 x 360, E = 256, hidden 512: norm affine per row, both dropouts (Philox stream, batch_offset),
    a per-row batch_scale with zeros (drop path), the residual add and the statistics of the output.  With dropout the
    reference is built for the first and last row and the rows at tile-range crossings (CPU masks of the Philox oracle,
    B = 1 with batch_offset = boff + b, as test_gpu_ops.py's test_mlp_fused_matches_fp64_and_unfused).
    Measured on the MI355X over B = 1 / 25 / 100 / 256 (edge) / 129 (straddle): global 1.9e-7 .. 2.6e-7; worst slice
    3.54e-7 (dropout 0, B = 256), 3.43e-7 (dropout 0.1, B = 100)."""
    from oracle.philox import element_keep_mask

    F = torch.nn.functional
    G = _workgroups("mlp")
    B = _batch(which, G)
    _need(3 * B * E * HW * 4 + 4 * REF_BYTES)
    g = torch.Generator(device="cpu").manual_seed(21)
    w1 = torch.randn(HID, E, generator=g) / np.sqrt(E)
    b1 = 0.1 * torch.randn(HID, generator=g)
    w2 = torch.randn(E, HID, generator=g) / np.sqrt(HID)
    b2 = 0.1 * torch.randn(E, generator=g)
    gc_ = _gen_cuda(121)
    x = torch.randn(B, E, NLAT, NLON, device="cuda", generator=gc_) * 1.3 + 0.2
    res = torch.randn(B, E, NLAT, NLON, device="cuda", generator=gc_)
    pa = 1 + 0.2 * torch.randn(B, E, device="cuda", generator=gc_)
    pd = 0.2 * torch.randn(B, E, device="cuda", generator=gc_)
    bs = 1 + 0.25 * torch.randn(B, device="cuda", generator=gc_)
    bs[2::5] = 0.0                                  # rows whose MLP branch drop path removed
    seed, call, layer, boff = 0xABCDEF0123456789, 3, 5, 7
    st = torch.zeros(B, E, 2, dtype=torch.float64, device="cuda")
    prep = sdy.ops.pack_mlp_h3(w1[:, :, None, None], w2[:, :, None, None], "cuda")
    out = sdy.ops.mlp_fused(x, w1, b1, w2, b2, pre_affine=(pa, pd), add=res, drop_p=drop, seed=seed, call=call,
                            stream_fc1=2 * layer, stream_fc2=2 * layer + 1, batch_offset=boff, batch_scale=bs, stats=st,
                            prepared=prep)
    w1d, b1d, w2d, b2d = w1.double().cuda(), b1.double().cuda(), w2.double().cuda(), b2.double().cuda()

    def ref(r0, r1, k1=None, k2=None, dev="cuda"):
        f64 = dict(device=dev, dtype=torch.float64)
        xa = x[r0:r1].to(**f64) * pa[r0:r1, :, None, None].to(**f64) + pd[r0:r1, :, None, None].to(**f64)
        if dev == "cpu":
            hid = F.gelu(F.conv2d(xa, w1.double()[:, :, None, None], b1.double()))
        else:
            hid = F.gelu(_mm(w1d, xa) + b1d[None, :, None, None])
        if k1 is not None:
            hid = hid * k1.to(**f64) / (1.0 - drop)
        if dev == "cpu":
            o = F.conv2d(hid, w2.double()[:, :, None, None], b2.double())
        else:
            o = _mm(w2d, hid) + b2d[None, :, None, None]
        if k2 is not None:
            o = o * k2.to(**f64) / (1.0 - drop)
        return o * bs[r0:r1, None, None, None].to(**f64) + res[r0:r1].to(**f64)

    se = SliceErrors()
    if drop == 0.0:
        ck = _chunk((3 * E + 2 * HID) * HW * 8)
        for r0 in range(0, B, ck):
            se.add(out[r0:r0 + ck], ref(r0, min(B, r0 + ck)))
        rows = [B - 1]
        masks = {B - 1: (None, None)}
    else:
        rows = sorted({0, B - 1, *_crossing_rows(B, G)})
        masks = {}
        for b in rows:
            k1 = torch.from_numpy(element_keep_mask(seed, call, layer, 0, drop, 1, HID, NLAT, NLON, batch_offset=boff + b))
            k2 = torch.from_numpy(element_keep_mask(seed, call, layer, 1, drop, 1, E, NLAT, NLON, batch_offset=boff + b))
            masks[b] = (k1, k2)
            se.add(out[b:b + 1], ref(b, b + 1, k1.cuda(), k2.cuda()), rows=[b])
    se.check(f"mlp_fused drop={drop} B={B} rows={rows if drop else 'all'}", TOL_OP, SLICE_MLP)
    b = rows[-1]
    _tie_to_cpu(ref(b, b + 1, *(None if k is None else k.cuda() for k in masks[b])), ref(b, b + 1, *masks[b], dev="cpu"),
                "mlp_fused")
    _check_stats(st, out, f"mlp_fused drop={drop} B={B}")


# ---- pair_h3: the fused encoder / decoder -----------------------------------------------------------------------------
# test_gpu_fullsize._build: forecaster 63 + 2 = 65 inputs, interpolator 126 + 2 = 128; the decoders read
# [block output (256) | inputs] and write the 63 state channels
PAIR_SHAPES = [(65, 256), (128, 256), (321, 63), (384, 63)]


@pytest.mark.parametrize("which", BATCHES)
@pytest.mark.parametrize("Cin,Cout", PAIR_SHAPES)
def test_conv_pair_production_batches(sdy, Cin, Cout, which):
    """conv_pair (Cin -> 256 -> GELU -> Cout in one launch) at the encoder and decoder shapes of the production networks:
    encoders with the broadcast position embedding and statistics, decoders plain.
    Measured on the MI355X over B = 1 / 25 / 100 / 256 (edge) / 129 (straddle): global 2.2e-7 (65 -> 256) .. 3.3e-7
    (384 -> 63); worst slice 2.68e-7 (65), 2.66e-7 (128), 3.66e-7 (321), 3.90e-7 (384, B = 256)."""
    F = torch.nn.functional
    G = _workgroups("pair")
    B = _batch(which, G)
    _need(B * (Cin + Cout) * HW * 4 + 4 * REF_BYTES)
    g = torch.Generator(device="cpu").manual_seed(77)
    w1 = torch.randn(256, Cin, generator=g) / np.sqrt(Cin)
    b1 = 0.1 * torch.randn(256, generator=g)
    w2 = torch.randn(Cout, 256, generator=g) / 16.0
    pos = 0.5 * torch.randn(1, Cout, NLAT, NLON, generator=g)
    x = torch.randn(B, Cin, NLAT, NLON, device="cuda", generator=_gen_cuda(177)) * 1.3 + 0.2
    enc = Cout == 256
    st = torch.zeros(B, Cout, 2, dtype=torch.float64, device="cuda") if enc else None
    out = sdy.ops.conv_pair(x, w1, b1, w2, add=pos.cuda() if enc else None, stats=st)
    w1d, b1d, w2d, posd = w1.double().cuda(), b1.double().cuda(), w2.double().cuda(), pos.double().cuda()

    def ref(r0, r1):
        y = _mm(w2d, F.gelu(_mm(w1d, x[r0:r1]) + b1d[None, :, None, None]))
        return y + posd if enc else y

    se = SliceErrors()
    ck = _chunk((Cin + 256 + 2 * Cout) * HW * 8)
    for r0 in range(0, B, ck):
        se.add(out[r0:r0 + ck], ref(r0, min(B, r0 + ck)))
    se.check(f"conv_pair {Cin}->256->{Cout} B={B}", TOL_OP, SLICE_PAIR)
    xc = x[-1:].cpu().double()
    cpu = F.conv2d(F.gelu(F.conv2d(xc, w1.double()[:, :, None, None], b1.double())), w2.double()[:, :, None, None])
    _tie_to_cpu(ref(B - 1, B), cpu + pos.double() if enc else cpu, f"conv_pair {Cin}->{Cout}")
    if enc:
        _check_stats(st, out, f"conv_pair {Cin}->256->256 B={B}")


# ---- dh_h3: the spectral contraction ----------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 25, 100])
def test_contract_dhconv_h3_full_degree_range(sdy, B):
    """contract_dhconv in split-fp16 mode at L = 180, M = 181, E = 256 (the fragment-stream kernel of the network),
    against a complex128 contraction on the device; errors per (row, degree).
    Measured on the MI355X: global 2.58e-7 at every B; worst slice 2.91e-7 (B = 25, degree 0)."""
    L, M = NLAT, NLON // 2 + 1
    g = torch.Generator(device="cpu").manual_seed(4)
    w = torch.randn(E, E, L, 2, generator=g) / np.sqrt(E)
    x = torch.randn(B, E, L, M, dtype=torch.complex64, device="cuda", generator=_gen_cuda(104))
    x = x * (torch.arange(M, device="cuda")[None, :] <= torch.arange(L, device="cuda")[:, None])
    got = sdy.ops.contract_dhconv(x, w.cuda(), gemm_mode="h3")
    wc = torch.view_as_complex(w.double().contiguous()).cuda()
    se = SliceErrors(keep=(0, 2), what="(row, degree)")
    ck = _chunk(3 * E * L * M * 16)
    for r0 in range(0, B, ck):
        se.add(got[r0:r0 + ck], torch.einsum("bixy,iox->boxy", x[r0:r0 + ck].to(torch.complex128), wc))
    se.check(f"dhconv h3 B={B}", TOL_OP, SLICE_DH)
    cpu = torch.einsum("bixy,iox->boxy", x[-1:].cpu().to(torch.complex128), torch.view_as_complex(w.double().contiguous()))
    _tie_to_cpu(torch.einsum("bixy,iox->boxy", x[-1:].to(torch.complex128), wc), cpu, "dhconv")


# ---- fft360 / leg_par: the transforms at network width ----------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 25, 100])
@pytest.mark.parametrize("grid", ["legendre-gauss", "equiangular"])
def test_sht_both_directions_network_width(sdy, grid, B):
    """RealSHT / InverseRealSHT at C = 256 (many 16-channel blocks of fft360, the folded Legendre kernels) against the
    oracle's transforms run in float64 on the device; forward errors per (row, degree), inverse per (row, channel).
    B = 100 is 25600 fields: more than one native inverse call addresses (sht.py splits them; it raised SdyError before).
    Measured on the MI355X, both grids: global 1.58e-7 (forward), 1.59e-7 .. 1.63e-7 (inverse); worst slice 1.75e-7
    (forward, Legendre-Gauss, B = 100), 1.67e-7 (inverse, equiangular, B = 100)."""
    from oracle.sht import InverseRealSHT as OInv, RealSHT as OFwd

    L, M = NLAT, NLON // 2 + 1
    fwd_ref = OFwd(NLAT, NLON, lmax=L, mmax=M, grid=grid).cuda()
    x = torch.randn(B, E, NLAT, NLON, device="cuda", generator=_gen_cuda(161))
    got = sdy.RealSHT(NLAT, NLON, lmax=L, mmax=M, grid=grid, gemm_mode="h3")(x)
    se = SliceErrors(keep=(0, 2), what="(row, degree)")
    ck = _chunk(6 * E * HW * 8)
    for r0 in range(0, B, ck):
        se.add(got[r0:r0 + ck], fwd_ref(x[r0:r0 + ck].double()))
    se.check(f"RealSHT {grid} B={B}", TOL_OP, SLICE_SHT)
    _tie_to_cpu(fwd_ref(x[-1:].double()), OFwd(NLAT, NLON, lmax=L, mmax=M, grid=grid)(x[-1:].cpu().double()),
                "RealSHT")
    del x, got
    inv_ref = OInv(NLAT, NLON, lmax=L, mmax=M, grid=grid).cuda()
    c = torch.randn(B, E, L, M, dtype=torch.complex64, device="cuda", generator=_gen_cuda(162))
    goti = sdy.InverseRealSHT(NLAT, NLON, lmax=L, mmax=M, grid=grid, gemm_mode="h3")(c)
    se = SliceErrors()
    for r0 in range(0, B, ck):
        se.add(goti[r0:r0 + ck], inv_ref(c[r0:r0 + ck].to(torch.complex128)))
    se.check(f"InverseRealSHT {grid} B={B}", TOL_OP, SLICE_ISHT)
    _tie_to_cpu(inv_ref(c[-1:].to(torch.complex128)),
                OInv(NLAT, NLON, lmax=L, mmax=M, grid=grid)(c[-1:].cpu().to(torch.complex128)), "InverseRealSHT")


# ---- the network at its batch limits ----------------------------------------------------------------------------------
def _count_native_calls(net):
    """Record (rows, batch_offset, call number) of every native forward the network issues."""
    calls = []
    orig = net._native_call

    def wrapped(h, dev, pieces, tt, out, call, batch_offset, *a, **k):
        calls.append((out.shape[0], batch_offset, call))
        return orig(h, dev, pieces, tt, out, call, batch_offset, *a, **k)

    net._native_call = wrapped
    return calls


def test_interpolator_forward_at_the_native_batch_limit_and_beyond(sdy):
    """The 2-block full-width interpolator (tests/variant_forward.py: 68 + 2 -> 34 channels, dropout and drop path on) at
    the batch limit of one native call (128 rows: drop-path row maps, dh_h3's 32-bit element offsets) and one row beyond it
    (129 rows: two native calls of 65 + 64 rows).  Rows at both ends of each call equal the lone trajectory with
    batch_offset = b (2e-6 as test_b25), and row 127 equals the oracle replaying its dropout stream.
    Measured on the MI355X: rows 0, 64, 65, 127, 128 bit-identical to the lone trajectories; row 127 vs the oracle
    1.21e-6."""
    cfg = SFNOConfig(in_chans=70, out_chans=34, nlat=NLAT, nlon=NLON, embed_dim=E, num_layers=2, with_time_emb=True,
                     dropout_mlp=0.1, drop_path_rate=0.1, min_time=1.0, max_time=5.0)
    net_seed = 777
    net, ora, _ = make_pair(cfg, 68, 2, net_seed=net_seed)
    dev = torch.device("cuda", 0)
    h = net._get_native(dev)
    assert sdy.lib.sdy_sfno_max_batch(h) == 128
    B = 129
    need = int(sdy.lib.sdy_sfno_workspace_floats(h, 128)) * 4 + B * (70 + 2 * 34) * HW * 4 + (2 << 30)
    _need(need)
    gc_ = _gen_cuda(55)
    x = torch.randn(B, 68, NLAT, NLON, device="cuda", generator=gc_)
    cond = torch.randn(B, 2, NLAT, NLON, device="cuda", generator=gc_)
    t = 1.0 + 4.0 * torch.rand(B, device="cuda", generator=gc_)
    net.enable_inference_dropout()
    calls = _count_native_calls(net)
    net.batch_offset, net._call = 0, 0
    y128 = net(x[:128], time=t[:128], condition=cond[:128])
    assert calls == [(128, 0, 0)] and net._call == 1
    calls.clear()
    net._call = 0
    y129 = net(x, time=t, condition=cond)
    assert calls == [(65, 0, 0), (64, 65, 0)] and net._call == 1
    assert torch.isfinite(y128).all() and torch.isfinite(y129).all()
    assert torch.equal(y128, y129[:128])
    for b in (0, 64, 65, 127, 128):
        net.batch_offset, net._call = b, 0
        alone = net(x[b:b + 1], time=t[b:b + 1], condition=cond[b:b + 1])[0]
        e = rel_l2(y129[b], alone)
        print(f"[network] B=129 row {b} vs lone trajectory: rel L2 {e:.3e} (bitwise: {torch.equal(y129[b], alone)})")
        assert e < 2e-6, f"row {b}: batch row vs lone trajectory rel L2 {e:.3e} (bitwise: {torch.equal(y129[b], alone)})"
    assert float((y129[0] - y129[1]).abs().max()) > 1e-3
    masks = PhiloxMasks(cfg, seed=net_seed, batch_offset=127)
    masks.call = 0
    ref = ora(x[127:128].cpu(), time=t[127:128].cpu(), condition=cond[127:128].cpu(), mask_fn=masks)
    err = rel_l2(y129[127], ref[0])
    print(f"[network] B=129 row 127 vs oracle: rel L2 {err:.3e}")
    assert err < TOL_NET_TIGHT, f"row 127 vs oracle with its dropout stream: rel L2 {err:.3e}"


def test_chunked_forward_small_grid_every_row_vs_oracle(sdy):
    """The Python split of a larger batch, cheaply: 32 x 64, E = 16, B = 300 = three native calls of 100 rows, dropout and
    drop path on, batch_offset 11, call number 3: every row equals the oracle on the whole batch, and the call counter
    advances by exactly one.  Measured on the MI355X: worst row 5.6e-7 vs the oracle."""
    cfg = SFNOConfig(in_chans=8, out_chans=6, nlat=32, nlon=64, embed_dim=16, num_layers=2, with_time_emb=True,
                     dropout_mlp=0.1, drop_path_rate=0.1, min_time=1.0, max_time=5.0)
    net, ora, _ = make_pair(cfg, 6, 2, net_seed=31337)
    h = net._get_native(torch.device("cuda", 0))
    assert sdy.lib.sdy_sfno_max_batch(h) == 128
    B, boff, call = 300, 11, 3
    g = torch.Generator(device="cpu").manual_seed(9)
    x = torch.randn(B, 6, 32, 64, generator=g)
    cond = torch.randn(B, 2, 32, 64, generator=g)
    t = 1.0 + 4.0 * torch.rand(B, generator=g)
    net.enable_inference_dropout()
    calls = _count_native_calls(net)
    net.batch_offset, net._call = boff, call
    got = net(x.cuda(), time=t.cuda(), condition=cond.cuda())
    assert calls == [(100, boff, call), (100, boff + 100, call), (100, boff + 200, call)]
    assert net._call == call + 1
    masks = PhiloxMasks(cfg, seed=31337, batch_offset=boff)
    masks.call = call
    ref = ora(x, time=t, condition=cond, mask_fn=masks)
    per_row = [rel_l2(got[b], ref[b]) for b in range(B)]
    worst = int(np.argmax(per_row))
    print(f"[network] 32x64 B=300: worst row {worst} vs oracle: rel L2 {per_row[worst]:.3e}")
    assert per_row[worst] < TOL_NET_TIGHT, f"row {worst}: rel L2 {per_row[worst]:.3e} vs the oracle"
