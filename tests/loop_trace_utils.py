"""A stepper that launches no project kernel, for tracing `sdy_amd.run_inference` itself: what it hands to writer and
aggregator, in which order, from which dropout call numbers.  Every value is an integer-valued float32 (exact through a
chain of windows), so traces compare with `torch.equal`."""
import types

import torch

NLAT, NLON, STEPS = 4, 8, 2                  # grid, forecast steps per window
OUT_NAMES, FORCING = ["a", "b"], "f"         # two generated variables, one forcing-only
CALLS_PER_BATCH = (2, 3)                     # what one run_on_batch moves the (forecaster, interpolator) call counters by
LOSS_UNIT = 42.0                             # per-row losses are multiples of 42: means over 1, 2, 3, 6, 7 rows stay integers


def series(n_ics, n_windows, seed=0):
    """name -> (n_ics, n_windows x STEPS + 1, NLAT, NLON).  The forcing is 16 x (time step) + a pattern below 16 that
    differs per initial condition and vanishes at pixel (0, 0): a batch's window can be read off its forcing."""
    g = torch.Generator().manual_seed(seed)
    n_t = n_windows * STEPS + 1
    out = {k: torch.randint(0, 50, (n_ics, n_t, NLAT, NLON), generator=g).float() for k in OUT_NAMES}
    pattern = (torch.arange(NLAT * NLON).view(1, 1, NLAT, NLON) % 5) * (torch.arange(n_ics).view(-1, 1, 1, 1) + 1)
    out[FORCING] = (16 * torch.arange(n_t).view(1, -1, 1, 1) + pattern).float()
    return out


def windows(data, n_windows, ics=slice(None)):
    return [{k: v[ics, i * STEPS:(i + 1) * STEPS + 1].clone() for k, v in data.items()} for i in range(n_windows)]


def loader(wins):
    return [types.SimpleNamespace(data=w, times=None) for w in wins]


def step_rows(data, rows, calls):
    """The fake network.  `data`: name -> (n, STEPS + 1, H, W); `rows`: (n,) global trajectory indices; `calls`: the call
    numbers the batch starts from.  gen[k][r, t] = state at time 0 + t x (1 + trajectory + 5 x variable) + calls[1] + 2 x
    calls[0] + the forcing's pattern at time t (t >= 1; slot 0 is the initial condition, as in the stepper's timelines).
    Returns (gen_data, gen_data_norm, per-row loss (float64))."""
    rows = rows.to(data[FORCING].device, torch.float32).view(-1, 1, 1, 1)
    t = torch.arange(STEPS + 1, device=rows.device, dtype=torch.float32).view(1, -1, 1, 1)
    moved = (t > 0).float() * (float(calls[1] + 2 * calls[0]) + torch.remainder(data[FORCING], 16.0))
    gen = {k: data[k][:, :1] + t * (1.0 + rows + 5.0 * j) + moved for j, k in enumerate(OUT_NAMES)}
    loss = LOSS_UNIT * (1.0 + rows.double().view(-1) + calls[1] + 3 * calls[0])
    return gen, {k: 2.0 * v - 3.0 for k, v in gen.items()}, loss


class Loss:
    """A window's loss as the stepper defers it: a device scalar read at `float()`, which raises for a flagged window."""

    def __init__(self, value, flagged):
        self.value, self.flagged = value, flagged

    def __float__(self):
        if self.flagged:
            from sdy_amd import SdyError

            raise SdyError("the fake stepper flagged this window")
        return float(self.value)

    def __mul__(self, w):
        return Loss(self.value * w, self.flagged)

    def __add__(self, other):
        other = other if isinstance(other, Loss) else Loss(other, False)
        return Loss(self.value + other.value, self.flagged or other.flagged)

    __radd__ = __add__


class FakeModule:
    def __init__(self):
        self.offset, self.calls = 0, (0, 0)

    def set_batch_offset(self, offset):
        self.offset = int(offset)

    def set_dropout_calls(self, calls):
        self.calls = tuple(int(c) for c in calls)

    def dropout_calls(self):
        return self.calls


class FakeStepper:
    """`module`, `out_names`, `run_on_batch` as `run_inference` uses them.  `log`: (batch offset, rows, call numbers at the
    batch's start, the batch's forcing at time slot 1, pixel (0, 0): 16 x its global time step) of every device batch."""

    out_names = OUT_NAMES

    def __init__(self, flag_window=None):
        self.module, self.log, self.flag_window = FakeModule(), [], flag_window

    def run_on_batch(self, data, optimization, n_forward_steps, defer_metrics=False):
        assert optimization is None and n_forward_steps == STEPS and defer_metrics
        m = self.module
        n = data[FORCING].shape[0]
        self.log.append((m.offset, n, m.calls, data[FORCING][0, 1, 0, 0].clone()))
        gen, gen_norm, loss = step_rows(data, m.offset + torch.arange(n), m.calls)
        flagged = self.flag_window is not None and m.calls[1] == self.flag_window * CALLS_PER_BATCH[1]
        m.calls = (m.calls[0] + CALLS_PER_BATCH[0], m.calls[1] + CALLS_PER_BATCH[1])
        from sdy_amd.stepper import SteppedData

        return SteppedData(metrics={"loss": Loss(loss.mean(), flagged)}, gen_data=gen, target_data=data,
                           gen_data_norm=gen_norm, target_data_norm={k: 2.0 * v - 3.0 for k, v in data.items()})

    def windows_of_log(self):
        """[(offset, rows, calls, window)] of the batches logged so far; clears the log."""
        out = [(o, n, c, (int(f) // 16 - 1) // STEPS) for o, n, c, f in self.log]
        self.log.clear()
        return out
