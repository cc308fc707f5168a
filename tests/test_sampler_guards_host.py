"""Host-side refusals of the sampler and of its two pointwise ops: every check here comes before a device pointer is taken or a
kernel is launched, so the tests run without a GPU (CPU tensors; a call that passed the check would fail with "GPU only")."""
import pytest
import torch


@pytest.fixture(scope="module")
def sdy():
    import sdy_amd

    return sdy_amd


def test_cold_update_refuses_operands_that_differ(sdy):
    """`sdy_cold_update` walks all operands with x_s's element count: a 6-channel forecast beside a 7-channel state (what the
    sampler once handed it under hack_for_imprecise_interpolation with a cold AR init) would be read B * H * W floats past its
    end.  ops.cold_update raises ValueError for any operand of another shape, dtype or device."""
    s7, s6 = torch.zeros(2, 7, 4, 8), torch.zeros(2, 6, 4, 8)
    with pytest.raises(ValueError, match="one shape"):
        sdy.ops.cold_update(s7, s6, s7)
    with pytest.raises(ValueError, match="one shape"):
        sdy.ops.cold_update(s7, s7, s6)
    with pytest.raises(ValueError, match="one shape"):
        sdy.ops.cold_update(s6, s7, None)
    with pytest.raises(ValueError, match="one shape"):
        sdy.ops.cold_update(s7, s7.reshape(2, 7, 8, 4), None)          # the same element count is not enough
    with pytest.raises(ValueError, match="one shape"):
        sdy.ops.cold_update(s7, s7, s7.to("meta"))                      # another device
    for bad in (torch.float64, torch.float16, torch.int32):
        with pytest.raises(ValueError, match="float32"):
            sdy.ops.cold_update(s7, s7.to(bad), s7)
        with pytest.raises(ValueError, match="float32"):
            sdy.ops.cold_update(s7.to(bad), s7, None)
    with pytest.raises(RuntimeError, match="GPU only"):                 # operands that agree pass the check
        sdy.ops.cold_update(s7, s7, s7)


def test_concat_channels_refuses_inputs_that_disagree_in_batch_or_grid(sdy):
    """`sdy_concat_channels` takes B, H and W from the first input only."""
    a = torch.zeros(2, 3, 4, 8)
    for other in (torch.zeros(3, 3, 4, 8), torch.zeros(2, 3, 5, 8), torch.zeros(2, 3, 4, 12), torch.zeros(2, 3, 8, 4),
                  torch.zeros(2, 3, 32), torch.zeros(2, 1, 4, 8, device="meta")):
        for order in ([a, other], [other, a], [a, a[:, :1], other]):
            with pytest.raises(ValueError, match="one B, H and W"):
                sdy.ops.concat_channels(order)
    with pytest.raises(ValueError, match="1 to 4"):
        sdy.ops.concat_channels([a] * 5)
    with pytest.raises(ValueError, match="1 to 4"):
        sdy.ops.concat_channels([])
    with pytest.raises(RuntimeError, match="GPU only"):                 # inputs that agree (channel counts may differ) pass
        sdy.ops.concat_channels([a, a[:, :1], a[:, :2]])


class _FakeIpol:
    window, true_horizon = 1, 6


class _Refuse:
    """A network that must not be reached."""

    def predict_forward(self, *a, **k):
        raise AssertionError("the forecaster was called")


def test_sampler_refuses_carried_channel_with_cold_ar_init_before_any_network_call(sdy):
    """hack_for_imprecise_interpolation (7-channel state) with use_cold_sampling_for_last_step=False and
    use_cold_sampling_for_init_of_ar_step=True: the reference fails at its last step on x_s + xhat - x_interpolated_s
    (src/diffusion/dyffusion.py:508; 7 channels against 6) after a whole pass; here sample_loop raises before its first network
    call and names the three options.  The two neighbouring combinations stay allowed (they reach the forecaster)."""
    x0 = torch.zeros(1, 7, 4, 8)
    bad = sdy.DYffusion(model=_Refuse(), interpolator=_FakeIpol(), timesteps=6, hack_for_imprecise_interpolation=True,
                        use_cold_sampling_for_last_step=False, use_cold_sampling_for_init_of_ar_step=True)
    with pytest.raises(RuntimeError) as e:
        bad.sample(x0)
    for option in ("hack_for_imprecise_interpolation", "use_cold_sampling_for_last_step", "use_cold_sampling_for_init_of_ar_step"):
        assert option in str(e.value)
    # init_of_ar_step defaults to last_step: False, False is the reference's working "plain forecast at the end" setting
    for kw in (dict(hack_for_imprecise_interpolation=True, use_cold_sampling_for_last_step=False),
               dict(hack_for_imprecise_interpolation=False, use_cold_sampling_for_last_step=False,
                    use_cold_sampling_for_init_of_ar_step=True)):
        ok = sdy.DYffusion(model=_Refuse(), interpolator=_FakeIpol(), timesteps=6, **kw)
        with pytest.raises(AssertionError, match="the forecaster was called"):
            ok.sample(x0)


def test_time_encoding_continuous_is_refused_at_construction(sdy):
    """The reference accepts time_encoding="continuous" (t / num_timesteps, src/diffusion/dyffusion.py:289-290); this sampler
    does not implement it and says so when it is built, not with wrong times later.  A known divergence."""
    with pytest.raises(ValueError, match="time_encoding"):
        sdy.DYffusion(model=None, interpolator=_FakeIpol(), timesteps=6, time_encoding="continuous")
    for ok in ("dynamics", "discrete"):
        assert sdy.DYffusion(model=None, interpolator=_FakeIpol(), timesteps=6, time_encoding=ok).hparams.time_encoding == ok
