"""The event-verification kernels keep nothing in private memory (no GPU needed): the event count is a template argument, so
the per-thread threshold and counter arrays are indexed at compile time and stay in registers; an event count that became a
run-time index would put them in scratch and cost the launch its bandwidth.  Read from the gfx950 code objects embedded in
the built library, as tests/test_code_objects.py does: kernel metadata only."""
import os

import pytest

from test_code_objects import LIB, _code_objects, _kernels


@pytest.mark.parametrize("kernel", ["event_table_kernel", "event_frequency_kernel"])
def test_event_kernels_have_no_private_segment(kernel):
    if not os.path.exists(LIB):
        pytest.skip("libsdy_amd.so is not built (python -c 'import __graft_entry__ as g; g.build()')")
    blob = open(LIB, "rb").read()
    found = {k[".name"]: k for co in _code_objects(blob) for k in _kernels(co) if kernel in k[".name"]}
    # event counts 1 .. 8, each with 16-byte and with scalar loads
    assert len(found) == 16, sorted(found)
    for name, k in found.items():
        assert k[".private_segment_fixed_size"] == 0, (name, k[".private_segment_fixed_size"])
        assert k.get(".vgpr_spill_count", 0) == 0 and k.get(".sgpr_spill_count", 0) == 0, name
