"""The time-quantile kernels keep nothing in private memory (no GPU needed): the rank count and the load width are template
arguments, so the per-thread rank state -- prefix, remaining rank and three digit counters per (rank, point) -- is indexed at
compile time and stays in registers; at 4 ranks x 4 points it is 80 registers, which is why more than 4 quantiles are taken in
two launches.  Read from the gfx950 code objects embedded in the built library, as tests/test_code_objects.py does: kernel
metadata only."""
import os

import pytest

import sdy_amd.quantiles  # noqa: F401  (the feature under test)
from test_code_objects import LIB, _code_objects, _kernels


def test_quantile_kernels_have_no_private_segment_and_no_spills():
    if not os.path.exists(LIB):
        pytest.skip("libsdy_amd.so is not built (python -c 'import __graft_entry__ as g; g.build()')")
    blob = open(LIB, "rb").read()
    kernels = [k for co in _code_objects(blob) for k in _kernels(co)]
    append = {k[".name"]: k for k in kernels if "append_kernel" in k[".name"]}
    select = {k[".name"]: k for k in kernels if "select_kernel" in k[".name"]}
    # append: 16-byte and scalar accesses; select: 1 .. 4 ranks per launch, each with 16-byte and with scalar loads
    assert len(append) == 2 and len(select) == 8, (sorted(append), sorted(select))
    for name, k in {**append, **select}.items():
        assert k[".private_segment_fixed_size"] == 0, (name, k[".private_segment_fixed_size"])
        assert k.get(".vgpr_spill_count", 0) == 0 and k.get(".sgpr_spill_count", 0) == 0, name
        assert k[".vgpr_count"] <= 256, (name, k[".vgpr_count"])
