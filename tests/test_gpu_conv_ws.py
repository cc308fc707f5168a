"""The weight-stationary inner-skip convolution (conv_h3_kernel<4, 8, true>: the 256 x 256 weight held in registers) against
float64 and against the ring kernel it replaces (SDY_NO_CONV_WS=1, in a child process: the switches are read once).

Tolerances are those of test_conv256_persistent_kernel_and_statistics (tests/test_gpu_ops.py): output rel L2 < TOL_OP,
statistics rtol 1e-5 / atol 1e-6 HW against the float64 sums of the stored output, and rel L2 < 5e-6 between the two kernels.
Whether the two kernels agree bit for bit is printed, not asserted."""
import functools
import os
import subprocess
import sys

import pytest
import torch

import conv_ws_cases as cc
from conftest import rel_l2

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL_OP = 2e-6            # single-op bound of tests/test_gpu_ops.py
TOL_KERNELS = 5e-6


@pytest.fixture(scope="module")
def sdy():
    assert "SDY_NO_CONV_WS" not in os.environ, "this module tests the default kernel selection"
    import sdy_amd

    return sdy_amd


@pytest.fixture(scope="module")
def ring(tmp_path_factory):
    """Every case on the ring kernel: one child process for the module."""
    out = tmp_path_factory.mktemp("conv_ws") / "ring.pt"
    env = dict(os.environ)
    env["SDY_NO_CONV_WS"] = "1"
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "conv_ws_cases.py"), str(out)], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return torch.load(out)


@functools.lru_cache(maxsize=None)
def reference(name):
    """float64 GELU(conv(pa x + pd) + b + add), computed once per case."""
    _, _, _, _, rows = cc.CASES[name]
    t = cc.inputs(name)
    xd = t["x"].double()
    if t["pa"] is not None:
        xd = xd * t["pa"].double()[:, :, None, None] + t["pd"].double()[:, :, None, None]
    if rows is not None:
        xd = xd[rows]
    F = torch.nn.functional
    return F.gelu(F.conv2d(xd, t["w"].double(), t["b"].double()) + t["add"].double())


@pytest.mark.parametrize("name", list(cc.CASES))
def test_conv_ws_matches_float64_and_the_ring_kernel(sdy, ring, name):
    (B, H, W), _, stats, _, _ = cc.CASES[name]
    out, st = cc.run(sdy, name)
    err = rel_l2(out, reference(name))
    old_out, old_st = ring[name]
    err_old, err_k = rel_l2(old_out, reference(name)), rel_l2(out, old_out)
    print(f"[conv_ws] {name} {B}x{H}x{W}: rel L2 vs float64 {err:.3e} (ring kernel {err_old:.3e}), between the kernels "
          f"{err_k:.3e}, bitwise equal: {torch.equal(out, old_out)}")
    assert torch.isfinite(out).all()
    assert err < TOL_OP
    assert err_k < TOL_KERNELS
    assert (st is None) == (not stats)
    if stats:
        od = out.double()
        want = torch.stack([od.sum((2, 3)), (od * od).sum((2, 3))], -1)
        assert torch.allclose(st, want, rtol=1e-5, atol=1e-6 * H * W)
        assert torch.allclose(st, old_st, rtol=1e-5, atol=1e-6 * H * W)
        print(f"[conv_ws] {name}: statistics bitwise equal to the ring kernel's: {torch.equal(st, old_st)}")


def test_conv_ws_raises_the_fp16_range_flag(sdy, ring):
    """A staged value beyond the fp16 range sets the same sticky flag as in the ring kernel, and a clean launch sets none."""
    sdy.ops.status_flags(reset=True)
    cc.run(sdy, "shape1")
    assert sdy.ops.status_flags(reset=True) == 0
    cc.run(sdy, "shape1", cc.overflow_x())
    flags = sdy.ops.status_flags(reset=True)
    assert flags & sdy.ops.FLAG_F16_RANGE
    assert flags == ring["overflow_flags"]
