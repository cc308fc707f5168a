"""The wavenumber-frequency kernels keep nothing in private memory (no GPU needed): the load width of the store kernel is a
template argument, and the power kernel carries a fixed group of four complex sums through a walk over the times, indexed at
compile time only, so nothing is indexed at run time and everything stays in registers.  Read from the gfx950 code objects
embedded in the built library, as tests/test_fss_code_object.py does: kernel metadata only."""
import os

import pytest

import sdy_amd.spacetime  # noqa: F401  (the feature under test)
from test_code_objects import LIB, _code_objects, _kernels


# the store kernel: 16-byte and scalar loads
@pytest.mark.parametrize("kernel,count", [("spacetime_store_kernel", 2), ("spacetime_power_kernel", 1), ("spacetime_sum_kernel", 1)])
def test_spacetime_kernels_have_no_private_segment_and_no_spills(kernel, count):
    if not os.path.exists(LIB):
        pytest.skip("libsdy_amd.so is not built (python -c 'import __graft_entry__ as g; g.build()')")
    blob = open(LIB, "rb").read()
    found = {k[".name"]: k for co in _code_objects(blob) for k in _kernels(co) if kernel in k[".name"]}
    assert len(found) == count, sorted(found)
    for name, k in found.items():
        assert k[".private_segment_fixed_size"] == 0, (name, k[".private_segment_fixed_size"])
        assert k.get(".vgpr_spill_count", 0) == 0 and k.get(".sgpr_spill_count", 0) == 0, name
        assert k[".group_segment_fixed_size"] <= 64 * 1024, (name, k[".group_segment_fixed_size"])
