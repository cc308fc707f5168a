"""The Helmholtz coefficient kernel is element-wise and bound by memory (no GPU needed): it keeps nothing in private memory,
spills nothing, uses no LDS, and its registers leave at least two waves per SIMD.  Read from the gfx950 code objects embedded in
the built library, as tests/test_eddy_code_object.py does: kernel metadata only."""
import os

import pytest

import sdy_amd.helmholtz  # noqa: F401  (the feature under test)
from test_code_objects import LIB, _code_objects, _kernels


def test_helmholtz_kernel_has_no_private_segment_no_spills_and_no_lds():
    if not os.path.exists(LIB):
        pytest.skip("libsdy_amd.so is not built (python -c 'import __graft_entry__ as g; g.build()')")
    blob = open(LIB, "rb").read()
    found = {k[".name"]: k for co in _code_objects(blob) for k in _kernels(co) if "helmholtz_kernel" in k[".name"]}
    assert len(found) == 1, sorted(found)
    for name, k in found.items():
        print(f"{name}: {k['.vgpr_count']} VGPR + {k.get('.agpr_count', 0)} AGPR, {k['.sgpr_count']} SGPR")
        assert k[".private_segment_fixed_size"] == 0, (name, k[".private_segment_fixed_size"])
        assert k.get(".vgpr_spill_count", 0) == 0 and k.get(".sgpr_spill_count", 0) == 0, name
        # two waves per SIMD: 512 vector registers per lane, accumulation registers included
        assert k[".vgpr_count"] + k.get(".agpr_count", 0) <= 256, (name, k[".vgpr_count"], k.get(".agpr_count", 0))
        assert k[".group_segment_fixed_size"] == 0, (name, k[".group_segment_fixed_size"])
