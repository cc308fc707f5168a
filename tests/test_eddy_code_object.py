"""The eddy-covariance kernels keep nothing in private memory (no GPU needed): the group size K, the points per work item and the
times in flight of the accumulate kernel are template arguments, so every per-variable and per-pair array is indexed at compile
time and stays in registers, and the registers leave at least two waves per SIMD.  Read from the gfx950 code objects embedded in
the built library, as tests/test_spacetime_code_object.py does: kernel metadata only."""
import os

import pytest

import sdy_amd.eddies  # noqa: F401  (the feature under test)
from test_code_objects import LIB, _code_objects, _kernels


# the accumulate kernel: K = 2, 3, 4, each with 16-byte and with scalar loads; the stats kernel: K = 2, 3, 4
@pytest.mark.parametrize("kernel,count", [("time_covariance_kernel", 6), ("time_covariance_maps_kernel", 1),
                                          ("time_covariance_stats_kernel", 3)])
def test_eddy_kernels_have_no_private_segment_and_no_spills(kernel, count):
    if not os.path.exists(LIB):
        pytest.skip("libsdy_amd.so is not built (python -c 'import __graft_entry__ as g; g.build()')")
    blob = open(LIB, "rb").read()
    found = {k[".name"]: k for co in _code_objects(blob) for k in _kernels(co) if kernel in k[".name"]}
    assert len(found) == count, sorted(found)
    for name, k in found.items():
        assert k[".private_segment_fixed_size"] == 0, (name, k[".private_segment_fixed_size"])
        assert k.get(".vgpr_spill_count", 0) == 0 and k.get(".sgpr_spill_count", 0) == 0, name
        # two waves per SIMD: 512 vector registers per lane, accumulation registers included
        assert k[".vgpr_count"] + k.get(".agpr_count", 0) <= 256, (name, k[".vgpr_count"], k.get(".agpr_count", 0))
        assert k[".group_segment_fixed_size"] <= 64 * 1024, (name, k[".group_segment_fixed_size"])


def test_accumulate_instantiations_are_the_expected_ones():
    """time_covariance_kernel<K, W, times in flight>: (2, 4, 6), (3, 4, 4), (4, 4, 2) with 16-byte loads and their scalar twins."""
    if not os.path.exists(LIB):
        pytest.skip("libsdy_amd.so is not built (python -c 'import __graft_entry__ as g; g.build()')")
    blob = open(LIB, "rb").read()
    names = sorted(k[".name"] for co in _code_objects(blob) for k in _kernels(co) if "time_covariance_kernel" in k[".name"])
    want = sorted(f"ILi{K}ELi{W}ELi{t}EE" for K, t in ((2, 6), (3, 4), (4, 2)) for W in (4, 1))
    assert len(names) == len(want) and all(any(w in n for n in names) for w in want), names
