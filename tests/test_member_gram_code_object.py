"""The Gram kernel keeps nothing in private memory (no GPU needed): the number of 16-row blocks is a template argument, so the
upper tiles' float64 accumulators and the operand arrays are indexed at compile time and stay in registers; a block count that
became a run-time index would put 120 registers of accumulators in scratch.  Read from the gfx950 code objects embedded in the
built library, as tests/test_code_objects.py does: kernel metadata only."""
import os

import pytest

from test_code_objects import LIB, _code_objects, _kernels


def test_gram_kernels_have_no_private_segment():
    if not os.path.exists(LIB):
        pytest.skip("libsdy_amd.so is not built (python -c 'import __graft_entry__ as g; g.build()')")
    blob = open(LIB, "rb").read()
    found = {k[".name"]: k for co in _code_objects(blob) for k in _kernels(co) if "member_gram_kernel" in k[".name"]}
    # 1 .. 5 blocks of 16 rows, each with 16-byte and with scalar loads
    assert len(found) == 10, sorted(found)
    for name, k in found.items():
        assert k[".private_segment_fixed_size"] == 0, (name, k[".private_segment_fixed_size"])
        assert k.get(".vgpr_spill_count", 0) == 0 and k.get(".sgpr_spill_count", 0) == 0, name
