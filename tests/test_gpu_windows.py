"""The plumbing the field aggregators share (sdy_amd/windows.py: `runs`, `fill_window`, the accumulators' offsets) on the
device, where it can go wrong: a window whose variables split into several launches -- by shape, by the SDY_MAX_VARS limit,
with a run on the scalar path -- must leave in every accumulator the bits that each variable leaves when it is fed alone."""
import pytest
import torch

pytestmark = pytest.mark.gpu

M, S, T, N_TIMESTEPS, T_START = 2, 1, 3, 5, 1


def _window(shapes, offset_var=None):
    g = torch.Generator(device="cuda").manual_seed(len(shapes))
    target, gen = {}, {}
    for i, (H, W) in enumerate(shapes):
        target[f"v{i:02d}"] = torch.randn(S, T, H, W, device="cuda", generator=g)
        x = torch.randn(M, S, T, H, W, device="cuda", generator=g)
        if i == offset_var:      # a view that starts one element into its buffer: 4 bytes off a 16-byte boundary
            buf = torch.zeros(x.numel() + 1, device="cuda")
            buf[1:] = x.reshape(-1)
            x = buf[1:].view(x.shape)
            assert x.data_ptr() % 16 == 4
        gen[f"v{i:02d}"] = x
    return target, gen


def _aggregators():
    import sdy_amd

    return {"video": sdy_amd.VideoAggregator(N_TIMESTEPS, True), "zonal": sdy_amd.ZonalMeanAggregator(N_TIMESTEPS),
            "member": sdy_amd.EnsembleTimeMeanAggregator(torch.ones(1, 1, device="cuda"))}


def _record(aggs, target, gen):
    for agg in aggs.values():
        agg.record_batch(0.0, target, gen, target, gen, i_time_start=T_START)
    return aggs


def _check_together_against_alone(shapes, want_runs, offset_var=None):
    from sdy_amd.windows import runs, window_layouts

    target, gen = _window(shapes, offset_var)
    lay = window_layouts(target, gen)
    assert [last - first for first, last in runs(lay, lambda l: l.extents)] == want_runs
    if offset_var is not None:
        assert lay[offset_var].gen.data_ptr() % 16 == 4
    together = _record(_aggregators(), target, gen)
    alone = [_record(_aggregators(), {k: target[k]}, {k: gen[k]}) for k in gen]
    for which, agg in together.items():
        assert set(agg._acc) == set(alone[0][which]._acc) and len(agg._acc) == {"video": 7, "zonal": 2, "member": 2}[which]
        for stat, buf in agg._acc.items():
            want = torch.cat([a[which]._acc[stat] for a in alone])
            assert torch.equal(buf, want), f"{which} {stat}"        # NaN-free: err_var of two rows is finite
            assert not torch.isnan(buf).any() and bool((buf != 0).any())
    assert together["member"]._gen_sum is together["member"]._acc["gen_sum"]
    assert together["video"]._n_batches == [0, 1, 1, 1, 0] and together["member"]._n_times == T


def test_runs_by_shape_with_a_scalar_run():
    """98 variables, variable 40 on another grid: launches of 40, 1 and 57 variables; the gen of variable 70 is a
    storage-offset view, so the third launch takes the 4-byte loads."""
    shapes = [(4, 8)] * 98
    shapes[40] = (4, 12)
    _check_together_against_alone(shapes, [40, 1, 57], offset_var=70)


def test_run_split_at_max_vars():
    """97 variables of one shape: SDY_MAX_VARS = 96 in the first launch, 1 in the second."""
    _check_together_against_alone([(4, 8)] * 97, [96, 1])
