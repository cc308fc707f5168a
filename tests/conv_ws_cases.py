"""Cases of test_gpu_conv_ws.py: the block's inner-skip convolution GELU(conv(pa x + pd) + b + add) through ops.conv1x1.

Imported by the test (weight-stationary kernel, the default) and run as a script in a child process with SDY_NO_CONV_WS=1
(the ring kernel): the kernel-selection switches are read once per process.  Both sides build their inputs from the same seeds."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

E = 256
# (B, H, W): 5 full tiles (fewer tiles than workgroups) | 5 full tiles + a 40-pixel ragged tile per image, an image boundary |
# 202 tiles per image, the last ragged: 606 tiles over 256 workgroups, several tiles per workgroup, images crossed mid-range
SHAPES = [(1, 8, 40), (2, 10, 36), (3, 20, 644)]
ROWS = [2, 0]              # permuted 2-of-3 row map of the second shape
# name -> (shape, pre-affine, statistics, tile-major output, row map)
CASES = {f"shape{i}": (s, True, True, False, None) for i, s in enumerate(SHAPES)}
CASES.update({
    "tiled": (SHAPES[1], True, True, True, None),
    "no_affine": (SHAPES[1], False, True, False, None),
    "x_rows": (SHAPES[1], True, True, False, ROWS),
    "no_stats": (SHAPES[1], True, False, False, None),
    "tiled_x_rows": (SHAPES[1], True, True, True, ROWS),
})


def inputs(name):
    """CPU float32 inputs of a case: x and pa / pd have the batch rows of the tensor the launch reads (3 with a row map)."""
    (B, H, W), affine, _, _, rows = CASES[name]
    g = torch.Generator(device="cpu").manual_seed(1000 + sorted(CASES).index(name))
    Bx = 3 if rows is not None else B
    x = torch.randn(Bx, E, H, W, generator=g) * 1.4 + 0.1
    w = torch.randn(E, E, 1, 1, generator=g) / np.sqrt(E)
    b = 0.1 * torch.randn(E, generator=g)
    add = torch.randn(B, E, H, W, generator=g)
    pa = 1 + 0.2 * torch.randn(Bx, E, generator=g)
    pd = 0.2 * torch.randn(Bx, E, generator=g)
    return dict(x=x, w=w, b=b, add=add, pa=pa if affine else None, pd=pd if affine else None)


def run(sdy, name, x=None):
    """One launch of a case on the GPU -> (output as (B, E, H, W) on the CPU, statistics (B, E, 2) float64 or None)."""
    (B, H, W), affine, stats, tiled, rows = CASES[name]
    t = inputs(name)
    if x is not None:
        t["x"] = x
    st = torch.zeros(B, E, 2, dtype=torch.float64, device="cuda") if stats else None
    out = sdy.ops.conv1x1(t["x"].cuda(), t["w"], t["b"], pre_affine=(t["pa"].cuda(), t["pd"].cuda()) if affine else None,
                          add=t["add"].cuda(), add_mode=1, gelu=True, frag_prepared=sdy.ops.pack_conv256(t["w"], "cuda"),
                          stats=st, x_rows=rows, out_tiled=tiled)
    torch.cuda.synchronize()
    out = out.cpu()
    if tiled:   # (B, tiles, E, 64) -> (B, E, H, W); the padding of the last tile is not part of the result
        out = out.permute(0, 2, 1, 3).reshape(B, E, -1)[:, :, :H * W].reshape(B, E, H, W).contiguous()
    return out, None if st is None else st.cpu()


def overflow_x():
    """x of case `shape1` with one value whose scaled split input leaves the fp16 range (16 pa x >= 65504)."""
    x = inputs("shape1")["x"].clone()
    x[1, 5, 3, 7] = 3.0e4
    return x


def main(out_path):
    import sdy_amd

    res = {}
    for name in CASES:
        res[name] = run(sdy_amd, name)
    sdy_amd.ops.status_flags(reset=True)
    run(sdy_amd, "shape1", overflow_x())
    res["overflow_flags"] = sdy_amd.ops.status_flags(reset=True)
    torch.save(res, out_path)


if __name__ == "__main__":
    main(sys.argv[1])
