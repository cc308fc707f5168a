"""The binned time-sum kernel keeps nothing in private memory (no GPU needed): the points per work item, the pooling of members
and the extremes are template arguments, so the loads in flight, the sums and the extremes of a work item are arrays indexed at
compile time and stay in registers, and the registers leave at least two waves per SIMD.  Read from the gfx950 code objects
embedded in the built library, as tests/test_eddy_code_object.py does: kernel metadata only."""
import os

import pytest

import sdy_amd.time_bins  # noqa: F401  (the feature under test)
from test_code_objects import LIB, _code_objects, _kernels


def _found():
    if not os.path.exists(LIB):
        pytest.skip("libsdy_amd.so is not built (python -c 'import __graft_entry__ as g; g.build()')")
    blob = open(LIB, "rb").read()
    return {k[".name"]: k for co in _code_objects(blob) for k in _kernels(co) if "binned_sum_kernel" in k[".name"]}


def test_binned_sum_kernels_have_no_private_segment_and_no_spills():
    found = _found()
    assert len(found) == 8, sorted(found)
    for name, k in found.items():
        assert k[".private_segment_fixed_size"] == 0, (name, k[".private_segment_fixed_size"])
        assert k.get(".vgpr_spill_count", 0) == 0 and k.get(".sgpr_spill_count", 0) == 0, name
        # two waves per SIMD: 512 vector registers per lane, accumulation registers included
        assert k[".vgpr_count"] + k.get(".agpr_count", 0) <= 256, (name, k[".vgpr_count"], k.get(".agpr_count", 0))
        assert k[".group_segment_fixed_size"] == 0, (name, k[".group_segment_fixed_size"])      # no LDS
        # the groups travel by value: the whole structure and the item count inside the 4 KB of kernel arguments
        assert k[".kernarg_segment_size"] <= 4096, (name, k[".kernarg_segment_size"])


def test_instantiations_are_the_expected_ones():
    """binned_sum_kernel<W, POOL, EXT>: 16-byte and scalar loads, members apart or pooled, with and without the extremes."""
    names = sorted(_found())
    want = sorted(f"ILi{W}ELb{pool}ELb{ext}EE" for W in (4, 1) for pool in (0, 1) for ext in (0, 1))
    assert len(names) == len(want) and all(any(w in n for n in names) for w in want), names
