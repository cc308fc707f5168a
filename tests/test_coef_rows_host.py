"""The checks the two entry points that embed an `sdy_coef_rows` share (csrc/coef_rows.h), without a GPU: both _host twins and
both device entry points (NULL stream: a refusal comes before anything is launched) refuse a call with a broken field of the
descriptor with one and the same code and leave the accumulators alone; the layout of the embedding structures; and the
Python side's `_fill_rows`.  What is an entry point's own -- pointers, struct_size, v offsets, "both error accumulators or
neither" -- is in tests/test_spectrum_host.py and tests/test_vector_spectrum_host.py.

Every case: `Layout(7, 5, 2, 3, 2, 3, 0)` (two variables or pairs, 3 members x 2 samples, 3 times, lmax 7, mtr 5, groups on
multiples of four), accumulators of 6 times prefilled with 7."""
import ctypes as C

import numpy as np
import pytest

import spectrum_utils as su
import vector_spectrum_utils as vu

WHICH = ["scalar-host", "scalar-device", "vector-host", "vector-device"]


def _call(which):
    """A valid call -> (entry point taking the structure alone, args, accumulators, keep-alive)."""
    import sdy_amd

    addr = lambda x: x.ctypes.data      # noqa: E731
    kind, where = which.split("-")
    if kind == "scalar":
        lay = su.Layout(7, 5, 2, 3, 2, 3, 0)
        bufs = su.random_case(lay, 0)[:2]
        acc = [np.full((2, 6, 7), 7.0) for _ in range(3)]
        a = su.fill_args(lay, addr(bufs[0]), addr(bufs[1]), None, None, 0, 6, tuple(addr(x) for x in acc))
        host, dev = sdy_amd.lib.sdy_degree_power_host, sdy_amd.lib.sdy_degree_power
    else:
        lay = vu.Layout(7, 5, 2, 3, 2, 3, 0)
        bufs = vu.random_case(lay, 0)[:4]
        acc = [np.full((2, 6, 7), 7.0) for _ in vu.ACCS]
        a = vu.fill_args(lay, *[addr(b) for b in bufs], None, None, 0, 6, tuple(addr(x) for x in acc))
        host, dev = sdy_amd.lib.sdy_vector_degree_power_host, sdy_amd.lib.sdy_vector_degree_power
    fn = host if where == "host" else (lambda p: dev(p, None))
    return fn, a, acc, bufs


def _untouched(acc):
    return all((x == 7.0).all() for x in acc)


def _break(rows, fields):
    for field, value in fields.items():
        setattr(rows, field, value(rows) if callable(value) else value)


# one broken field (or two that belong together) of the descriptor: SDY_ERR_ARG
BROKEN_ROWS = [{k: v} for k in ("lmax", "mtr", "gen_fields", "target_fields", "nvars", "n0", "n1", "T", "n_timesteps")
               for v in (0, -1)]
BROKEN_ROWS += [dict(mtr=8), dict(t_start=-1), dict(t_start=4), dict(t_start=2 ** 31 - 2), dict(n_timesteps=2)]
BROKEN_ROWS += [{k: -4} for k in ("gen_var_stride", "gen_time_stride", "target_var_stride", "target_time_stride")]
# a buffer that ends before the last row of the last time of the last variable (in the vector structure: before its v field)
BROKEN_ROWS += [dict(gen_fields=lambda r: r.gen_fields - 4), dict(target_fields=lambda r: r.target_fields - 4), dict(n0=5),
                dict(T=4, n_timesteps=8), dict(nvars=3)]

# extents outside the supported range: SDY_ERR_UNSUPPORTED
BIG = 2 ** 31 - 1
UNSUPPORTED_ROWS = [dict(n0=2 ** 16, n1=2 ** 15, gen_fields=BIG, target_fields=BIG),
                    dict(T=65536, n_timesteps=65536, gen_fields=BIG, target_fields=BIG, gen_time_stride=8, target_time_stride=4),
                    dict(nvars=65536, gen_fields=BIG, target_fields=BIG),
                    dict(lmax=2 ** 15, mtr=2 ** 15, gen_fields=1024, target_fields=1024),
                    dict(n_timesteps=2 ** 31 - 1, nvars=65535, lmax=64, mtr=5)]


@pytest.mark.parametrize("which", WHICH)
@pytest.mark.parametrize("cases,code", [(BROKEN_ROWS, su.SDY_ERR_ARG), (UNSUPPORTED_ROWS, su.SDY_ERR_UNSUPPORTED)],
                         ids=["broken", "unsupported"])
def test_entry_points_refuse_a_broken_descriptor(which, cases, code):
    for fields in cases:
        fn, a, acc, keep = _call(which)
        _break(a.rows, fields)
        assert fn(C.byref(a)) == code, fields
        assert _untouched(acc), fields


@pytest.mark.parametrize("which", ["scalar-host", "vector-host"])
def test_the_valid_call_goes_through(which):
    fn, a, acc, keep = _call(which)
    r = a.rows
    assert (r.lmax, r.mtr, r.nvars, r.n0, r.n1, r.T, r.t_start, r.n_timesteps) == (7, 5, 2, 3, 2, 3, 0, 6)
    assert fn(C.byref(a)) == 0 and not _untouched(acc)


def test_layout():
    from sdy_amd import _lib

    S, V, R = _lib.SdySpectrumArgs, _lib.SdyVectorSpectrumArgs, _lib.SdyCoefRows
    assert (C.sizeof(R), C.sizeof(S), C.sizeof(V)) == (72, 112, 168)
    assert (S.rows.offset, V.rows.offset) == (16, 40)
    assert dict(S._fields_)["rows"] is R and dict(V._fields_)["rows"] is R
    # every field of sdy_spectrum_args where it was before the descriptor
    want = dict(gen=0, target=8, gen_scale=16, target_scale=24, lmax=32, mtr=36, gen_fields=40, target_fields=44,
                gen_var_stride=48, gen_time_stride=52, target_var_stride=56, target_time_stride=60, nvars=64, n0=68, n1=72,
                T=76, t_start=80, n_timesteps=84, gen_power=88, target_power=96, err_power=104)
    assert {k: getattr(S, k).offset for k in want} == want
    # sdy_vector_spectrum_args: the v offsets behind the descriptor
    want = dict(struct_size=0, gen_d=8, gen_m=16, target_d=24, target_m=32, gen_scale=40, target_scale=48, lmax=56,
                n_timesteps=108, gen_v_offset=112, target_v_offset=116, gen_rot=120, gen_div=128, target_rot=136,
                target_div=144, err_rot=152, err_div=160)
    assert {k: getattr(V, k).offset for k in want} == want
    assert S in _lib.ABI_STRUCTS and V not in _lib.ABI_STRUCTS and R not in _lib.ABI_STRUCTS
    assert len(_lib.ABI_STRUCTS) == 25                         # like SdyWindow, the descriptor is no argument structure


def test_fill_rows():
    from types import SimpleNamespace

    from sdy_amd._lib import SdyCoefRows, SdySpectrumArgs, SdyVectorSpectrumArgs
    from sdy_amd.spectrum import _fill_rows

    hand = SdyCoefRows()
    hand.gen_scale, hand.target_scale = 0x1000, 0x2000
    hand.lmax, hand.mtr = 12, 9
    hand.gen_fields, hand.target_fields = 336, 56
    hand.gen_var_stride, hand.gen_time_stride = 84, 28
    hand.target_var_stride, hand.target_time_stride = 12, 4
    hand.nvars, hand.n0, hand.n1, hand.T = 2, 25, 1, 3
    hand.t_start, hand.n_timesteps = 4, 11
    plan = SimpleNamespace(lmax=12, mtr=9)
    for a in (SdySpectrumArgs(), SdyVectorSpectrumArgs()):
        _fill_rows(a.rows, plan, 0x1000, 0x2000, (336, 84, 28), (56, 12, 4), 2, 25, 1, 3, 4, 11)
        assert bytes(a.rows) == bytes(hand)
        # the descriptor's fields as the structure's own
        assert (a.lmax, a.mtr, a.gen_fields, a.target_time_stride, a.n0, a.t_start, a.n_timesteps) == (12, 9, 336, 4, 25, 4, 11)
        assert (a.gen_scale, a.target_scale) == (0x1000, 0x2000)
    _fill_rows(a.rows, plan, None, None, (336, 84, 28), (56, 12, 4), 2, 25, 1, 3, 4, 11)
    assert a.rows.gen_scale is None and a.rows.target_scale is None
