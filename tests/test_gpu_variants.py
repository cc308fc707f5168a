"""The kernel-selection switches (fallback paths kept for A/B measurements) must all compute the same network.

Every variant runs the same seeded forward (E = 256, 180 x 360, dropout and drop path ON, so the Philox streams of the
fused and the unfused kernels are compared too) in its own process and is held to the default path's output.
Tolerance: 2e-5 relative L2 (both sides are fp32-class; the bound of the path is 1e-4)."""
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (retired with their questions settled, round 6: SDY_NO_CONV_FRAG, SDY_NO_FUSED_STATS, SDY_NO_POLAR_SKIP, SDY_NO_PAIR -- the paths
#  they selected remain what other shapes take and are held to the oracle there, tests/test_gpu_sfno.py, test_gpu_golden.py)
# SDY_NO_SKIP_FOLD: the first / last block's inner skip as the reference computes it (a convolution of the residual) instead of
# folded into the dhconv weights -- the two agree to rounding, which this test holds them to
# SDY_GEMM_MODE=f32: the fp32-MFMA network (the escape hatch from SDY_FLAG_F16_RANGE) -- every stage on
# the fp32 GEMM, none of the split-fp16 kernels; tests/test_gpu_f32_path.py holds it to float64 in detail
VARIANTS = {"SDY_NO_DH_FRAG": "1", "SDY_NO_FFT360": "1", "SDY_NO_FUSED_MLP": "1", "SDY_NO_LEG_FRAG": "1", "SDY_NO_LEG_PAR": "1",
            "SDY_NO_SKIP_FOLD": "1", "SDY_GEMM_MODE": "f32"}
TOL = 2e-5


def _run(tmp_path, tag, env_extra):
    out = tmp_path / f"{tag}.pt"
    env = dict(os.environ)
    env.update(env_extra)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "variant_forward.py"), str(out)], env=env, cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, f"{tag}: {r.stderr[-2000:]}"
    return torch.load(out)


@pytest.mark.gpu
def test_kernel_selection_switches_agree(tmp_path):
    ref = _run(tmp_path, "default", {})
    assert torch.isfinite(ref).all()
    for v, val in VARIANTS.items():
        got = _run(tmp_path, v, {v: val})
        err = (torch.linalg.vector_norm(got.double() - ref.double()) / torch.linalg.vector_norm(ref.double())).item()
        print(f"[variants] {v}={val}: rel L2 {err:.3e} vs the default path")
        assert err < TOL, f"{v}={val} differs from the default path: rel L2 {err:.3e}"


@pytest.mark.gpu
def test_drop_path_skip_is_bit_identical(tmp_path):
    """The drop-path skip (capi.hip: a block runs on the trajectories its DropPath draw keeps, the dropped ones' output is the
    residual a x + d) against SDY_NO_DROP_SKIP=1, which computes every branch and multiplies the dropped ones by 0
    (src/models/modules/drop_path.py:15-22, sfnonet.py:330-337): the same bits, for a batch, for stacked calls, for single
    trajectories whose blocks are dropped whole, on both data grids (with the Legendre-Gauss grid the last block skips too)."""
    def run(tag, env_extra):
        out = tmp_path / f"{tag}.pt"
        env = dict(os.environ)
        env.update(env_extra)
        env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "drop_skip_forward.py"), str(out)], env=env, cwd=ROOT,
                           capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, f"{tag}: {r.stderr[-2000:]}"
        return torch.load(out)

    skip, full = run("skip", {}), run("full", {"SDY_NO_DROP_SKIP": "1"})
    assert skip.keys() == full.keys()
    bad = {k: (skip[k] - full[k]).abs().max().item() for k in skip if not torch.equal(skip[k], full[k])}
    assert all(torch.isfinite(v).all() for v in skip.values())
    assert not bad, f"outputs differ (max |diff| per case): {bad}"
    # the stacked forward is the two calls of three trajectories: its rows differ from the one-call batch (other call numbers)
    assert not torch.equal(skip["equiangular/b6"][3:], skip["equiangular/b6_stacked"][3:])
