"""The neighbourhood-verification kernels keep nothing in private memory (no GPU needed): the event count is a template argument
of the encode kernel, so its per-thread threshold and counter arrays are indexed at compile time and stay in registers; the sum
kernel picks its radius without a run-time index into its arguments.  Read from the gfx950 code objects embedded in the built
library, as tests/test_event_verif_code_object.py does: kernel metadata only."""
import os

import pytest

from test_code_objects import LIB, _code_objects, _kernels


@pytest.mark.parametrize("kernel,count", [("fss_encode_kernel", 16), ("fss_sum_kernel", 1)])
def test_fss_kernels_have_no_private_segment(kernel, count):
    if not os.path.exists(LIB):
        pytest.skip("libsdy_amd.so is not built (python -c 'import __graft_entry__ as g; g.build()')")
    blob = open(LIB, "rb").read()
    found = {k[".name"]: k for co in _code_objects(blob) for k in _kernels(co) if kernel in k[".name"]}
    # the encode kernel: event counts 1 .. 8, each with 16-byte and with scalar loads
    assert len(found) == count, sorted(found)
    for name, k in found.items():
        assert k[".private_segment_fixed_size"] == 0, (name, k[".private_segment_fixed_size"])
        assert k.get(".vgpr_spill_count", 0) == 0 and k.get(".sgpr_spill_count", 0) == 0, name
