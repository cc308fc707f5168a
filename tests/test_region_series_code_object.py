"""The region-series kernels keep nothing in private memory (no GPU needed): a run-time-indexed per-thread member array, or
8 x n_regions accumulators per thread, would land in scratch and cost the launch its bandwidth.  Read from the gfx950 code
objects embedded in the built library, as tests/test_code_objects.py does."""
import os

import pytest

from test_code_objects import LIB, _code_objects, _kernels


def test_region_series_kernels_have_no_private_segment():
    if not os.path.exists(LIB):
        pytest.skip("libsdy_amd.so is not built (python -c 'import __graft_entry__ as g; g.build()')")
    blob = open(LIB, "rb").read()
    found = {k[".name"]: k for co in _code_objects(blob) for k in _kernels(co) if "region_series" in k[".name"]}
    # the 16-byte and the scalar instantiation of the series kernel
    assert len(found) >= 2, sorted(found)
    for name, k in found.items():
        assert k[".private_segment_fixed_size"] == 0, (name, k[".private_segment_fixed_size"])
        assert k.get(".vgpr_spill_count", 0) == 0 and k.get(".sgpr_spill_count", 0) == 0, name
