"""The spell kernel keeps nothing in private memory (no GPU needed): the event count and the load width are template
arguments, so the per-thread state and threshold arrays are indexed at compile time and stay in registers -- at 8 events with
16-byte loads the state alone would be 128 registers, which is why more than 4 events are taken in two passes.  Read from the
gfx950 code objects embedded in the built library, as tests/test_code_objects.py does: kernel metadata only."""
import os

import pytest

from test_code_objects import LIB, _code_objects, _kernels


def test_spell_kernels_have_no_private_segment_and_no_spills():
    if not os.path.exists(LIB):
        pytest.skip("libsdy_amd.so is not built (python -c 'import __graft_entry__ as g; g.build()')")
    blob = open(LIB, "rb").read()
    found = {k[".name"]: k for co in _code_objects(blob) for k in _kernels(co) if "spell_kernel" in k[".name"]}
    # event counts 1 .. 8, each with 16-byte and with scalar loads; the two passes of 5 .. 8 events are inside one kernel
    assert len(found) == 16, sorted(found)
    for name, k in found.items():
        assert k[".private_segment_fixed_size"] == 0, (name, k[".private_segment_fixed_size"])
        assert k.get(".vgpr_spill_count", 0) == 0 and k.get(".sgpr_spill_count", 0) == 0, name
        assert k[".vgpr_count"] <= 256, (name, k[".vgpr_count"])          # at least two waves per SIMD
