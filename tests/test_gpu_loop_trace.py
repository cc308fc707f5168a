"""`sdy_amd.run_inference` traced with a stepper that launches no project kernel (tests/loop_trace_utils.py): every call the
writer and the aggregator receive, under every combination of the driver's options, for the unsharded job, its shares
(`unit_range`, `trajectory_offset`) and a relayed remainder trajectory.  All values are exact integers: traces compare with
`torch.equal`.  Goes through the public call only."""
import itertools
import threading

import pytest
import torch

import loop_trace_utils as lt
from relay_utils import MailboxComm

pytestmark = pytest.mark.gpu

N_ICS, MEMBERS, N_WINDOWS = 2, 3, 4
RELAY_MEMBERS, RELAY_WORLD, RELAY_WINDOWS = 7, 3, 6
COMBOS = [dict(prefetch=p, max_batch=b, host_outputs=h, derive=d)
          for p, b, h, d in itertools.product((2, 0), (None, 1), (False, True), (False, True))]
BASE_TIMERS = {"data_loading", "run_on_batch_host", "writer_and_aggregator", "run_on_batch", "wall", "trajectory_steps",
               "forecast_steps_per_second", "forecast_steps_per_second_run_on_batch"}


def _combo_id(c):
    return "prefetch{prefetch}-max_batch{max_batch}-host{host_outputs:d}-derive{derive:d}".format(**c)


def _derive(d):
    return {**d, "d": d["a"] + d["b"]}


class Writer:
    """Every (trajectory, time step) -> the generated fields, and the calls as they came."""

    def __init__(self, members, first_ic=0, derived=False, device="cuda"):
        self.members, self.first_ic, self.derived, self.device = members, first_ic, derived, device
        self.fields, self.calls = {}, []

    def append_batch(self, target, prediction, start_timestep, start_sample, batch_times=None):
        assert {v.device.type for d in (target, prediction) for v in d.values()} == {self.device}
        assert list(prediction) == lt.OUT_NAMES + (["d"] if self.derived else [])
        assert list(target) == lt.OUT_NAMES + [lt.FORCING] + (["d"] if self.derived else [])
        if self.derived:
            assert torch.equal(prediction["d"], prediction["a"] + prediction["b"])
            assert torch.equal(target["d"], target["a"] + target["b"])
        pred = {k: prediction[k].detach().cpu().clone() for k in lt.OUT_NAMES}
        self.calls.append((start_timestep, start_sample, {k: tuple(v.shape) for k, v in pred.items()},
                           {k: tuple(v.shape) for k, v in target.items() if k != "d"}, pred))
        v = torch.stack([pred[k] for k in lt.OUT_NAMES], dim=-3)         # (..., time, variable, H, W)
        if v.dim() == 6:          # (members, n_sample, time, ...): the reference's presentation of a rectangular share
            assert start_sample == 0
            rows = {(self.first_ic + s) * self.members + m: v[m, s] for m in range(v.shape[0]) for s in range(v.shape[1])}
        else:                     # flat rows from global trajectory start_sample on
            rows = {start_sample + r: v[r] for r in range(v.shape[0])}
        for u, traj in rows.items():
            for t in range(traj.shape[0]):
                assert (u, start_timestep + t) not in self.fields, f"trajectory {u}, time step {start_timestep + t} written twice"
                self.fields[(u, start_timestep + t)] = traj[t]


class Aggregator:
    accepts_sample_weights = True

    def __init__(self, derived=False):
        self.derived, self.calls = derived, []

    def record_batch(self, loss, target_data, gen_data, target_data_norm, gen_data_norm, i_time_start=0, sample_weights=None):
        assert isinstance(loss, float)
        assert {v.device.type for d in (target_data, gen_data, target_data_norm, gen_data_norm) for v in d.values()} == {"cuda"}
        assert list(gen_data) == lt.OUT_NAMES + (["d"] if self.derived else []) and list(gen_data_norm) == lt.OUT_NAMES
        assert all(torch.equal(gen_data_norm[k], 2.0 * gen_data[k] - 3.0) for k in lt.OUT_NAMES)
        assert all(torch.equal(target_data_norm[k], 2.0 * target_data[k] - 3.0) for k in (lt.FORCING,))
        shapes = {name: {k: tuple(v.shape) for k, v in d.items() if k != "d"}
                  for name, d in (("target", target_data), ("gen", gen_data), ("target_norm", target_data_norm))}
        self.calls.append((i_time_start, sample_weights, shapes, loss,
                           {k: gen_data[k].detach().cpu().clone() for k in lt.OUT_NAMES}))


def _same(a, b):
    """Nested tuples / lists / dicts of plain values and tensors, compared exactly."""
    if isinstance(a, torch.Tensor):
        return isinstance(b, torch.Tensor) and torch.equal(a, b)
    if isinstance(a, dict):
        return isinstance(b, dict) and list(a) == list(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return type(a) is type(b) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return a == b


def _run(wins, n_windows, members, combo, first_ic=0, stepper=None, **kw):
    """One `run_inference` from call numbers (0, 0); returns (writer, aggregator, timers, [(offset, rows, calls, window)])."""
    import sdy_amd

    stepper = stepper if stepper is not None else lt.FakeStepper()
    stepper.module.set_dropout_calls((0, 0))
    derived = combo["derive"]
    wr = Writer(members, first_ic, derived, "cpu" if combo["host_outputs"] else "cuda")
    agg = Aggregator(derived)
    timers = sdy_amd.run_inference(agg, stepper, lt.loader(wins), n_windows * lt.STEPS, lt.STEPS, n_ensemble_members=members,
                                   writer=wr, derive=_derive if derived else None, host_outputs=combo["host_outputs"],
                                   prefetch=combo["prefetch"], max_batch=combo["max_batch"], trajectory_offset=first_ic, **kw)
    assert not [t for t in threading.enumerate() if t.name == "sdy-window-prefetch"]
    log = stepper.windows_of_log()
    # every device batch of window w starts from the call numbers of window w, whatever ran in between
    assert all(c == (w * lt.CALLS_PER_BATCH[0], w * lt.CALLS_PER_BATCH[1]) for _, _, c, w in log), log
    if combo["max_batch"] == 1:
        assert all(n == 1 for _, n, _, _ in log)
    assert timers["trajectory_steps"] == sum(n for _, n, _, _ in log) * lt.STEPS
    assert set(timers) - {"relay_host", "relay_recv_wait"} == BASE_TIMERS
    return wr, agg, timers, log


PLAIN = dict(prefetch=2, max_batch=None, host_outputs=False, derive=False)


@pytest.fixture(scope="module")
def job():
    data = lt.series(N_ICS, N_WINDOWS, seed=3)
    wins = lt.windows(data, N_WINDOWS)
    wr, agg, _, _ = _run(wins, N_WINDOWS, MEMBERS, PLAIN)
    assert sorted(wr.fields) == [(u, t) for u in range(N_ICS * MEMBERS) for t in range(N_WINDOWS * lt.STEPS + 1)]
    return data, wins, wr, agg


@pytest.fixture(scope="module")
def relay_job():
    data = lt.series(1, RELAY_WINDOWS, seed=4)
    wins = lt.windows(data, RELAY_WINDOWS)
    wr, _, _, _ = _run(wins, RELAY_WINDOWS, RELAY_MEMBERS, PLAIN)
    assert sorted(wr.fields) == [(u, t) for u in range(RELAY_MEMBERS) for t in range(RELAY_WINDOWS * lt.STEPS + 1)]
    return wins, wr


def test_unsharded_job_equals_the_serial_oracle(job):
    """Writer calls (start_timestep, prediction) and aggregator calls (loss, i_time_start) of the batched driver == the
    restated reference loop driving the same fake member by member."""
    from oracle.loop import run_inference as oracle_run

    _, wins, wr, agg = job
    seen = {"n": 0}

    def run_on_batch(data, m):
        w = seen["n"] // MEMBERS
        seen["n"] += 1
        rows = torch.tensor([s * MEMBERS + m for s in range(N_ICS)])
        gen, gen_norm, loss = lt.step_rows(data, rows, (w * lt.CALLS_PER_BATCH[0], w * lt.CALLS_PER_BATCH[1]))
        return {"loss": float(loss.mean())}, gen, gen_norm

    wref, aref = oracle_run(wins, run_on_batch, N_WINDOWS * lt.STEPS, lt.STEPS, MEMBERS)
    assert [(c[0], c[1]) for c in wr.calls] == [(t, 0) for t, _ in wref]
    for (_, pref), call in zip(wref, wr.calls):
        assert _same(call[4], {k: pref[k] for k in lt.OUT_NAMES})
        assert call[4]["a"].shape[:2] == (MEMBERS, N_ICS)
    assert [(c[3], c[0]) for c in agg.calls] == aref
    assert [c[1] for c in agg.calls] == [None] * N_WINDOWS
    v = wr.calls[0][4]["a"]
    assert not torch.equal(v[0], v[1])          # members differ


@pytest.mark.parametrize("combo", COMBOS, ids=_combo_id)
def test_unsharded_job_traces_do_not_depend_on_the_options(job, combo):
    _, wins, wr0, agg0 = job
    wr, agg, _, log = _run(wins, N_WINDOWS, MEMBERS, combo)
    assert _same(wr.calls, wr0.calls) and _same(agg.calls, agg0.calls)
    chunks = N_ICS * MEMBERS if combo["max_batch"] == 1 else 1
    assert [w for _, _, _, w in log] == [w for w in range(N_WINDOWS) for _ in range(chunks)]


# (world, [(start, count)], sample_weights of each share: the fraction of every touched initial condition's members in it)
SHARES = [(2, [(0, 3), (3, 3)], [[1.0], [1.0]]),
          (4, [(0, 2), (2, 2), (4, 1), (5, 1)], [[2 / 3], [1 / 3, 1 / 3], [1 / 3], [1 / 3]])]


@pytest.mark.parametrize("combo", COMBOS, ids=_combo_id)
def test_unit_range_shares_write_every_trajectory_once(job, combo):
    from sdy_amd import ensemble

    _, wins, wr0, _ = job
    for world, shares, weights in SHARES:
        assert [ensemble.shard(N_ICS, MEMBERS, r, world)[:2] for r in range(world)] == shares
        seen = {}
        for (start, count), wts in zip(shares, weights):
            wr, agg, timers, _ = _run(wins, N_WINDOWS, MEMBERS, combo, unit_range=(start, count))
            assert timers["trajectory_steps"] == count * N_WINDOWS * lt.STEPS
            assert not set(wr.fields) & set(seen)
            seen.update(wr.fields)
            n_ic = len(wts)
            for w, (wc, ac) in enumerate(zip(wr.calls, agg.calls)):
                n_t = lt.STEPS + (1 if w == 0 else 0)
                assert wc[:2] == (w * lt.STEPS + (1 if w else 0), start)
                assert wc[2] == {k: (count, n_t, lt.NLAT, lt.NLON) for k in lt.OUT_NAMES}          # flat rows
                assert wc[3] == {k: (n_ic, n_t, lt.NLAT, lt.NLON) for k in lt.OUT_NAMES + [lt.FORCING]}
                assert ac[0] == wc[0] and ac[1] == wts
                assert ac[2]["target_norm"] == wc[3] and ac[2]["gen"] == wc[2]
            assert len(wr.calls) == len(agg.calls) == N_WINDOWS
        assert sorted(seen) == sorted(wr0.fields) and all(torch.equal(v, wr0.fields[k]) for k, v in seen.items())


@pytest.mark.parametrize("combo", COMBOS, ids=_combo_id)
def test_trajectory_offset_shares_write_every_trajectory_once(job, combo):
    data, _, wr0, _ = job
    seen = {}
    for ic in range(N_ICS):
        wr, agg, _, _ = _run(lt.windows(data, N_WINDOWS, slice(ic, ic + 1)), N_WINDOWS, MEMBERS, combo, first_ic=ic)
        assert all(c[2]["a"][:2] == (MEMBERS, 1) and c[1] == 0 for c in wr.calls) and all(c[1] is None for c in agg.calls)
        assert not set(wr.fields) & set(seen)
        seen.update(wr.fields)
    assert sorted(seen) == sorted(wr0.fields) and all(torch.equal(v, wr0.fields[k]) for k, v in seen.items())


@pytest.mark.parametrize("combo", COMBOS, ids=_combo_id)
def test_relayed_trajectory_is_written_once_from_whichever_rank_hosts_it(relay_job, combo):
    from sdy_amd import ensemble

    wins, wr0 = relay_job
    unit = RELAY_MEMBERS - 1
    box, seen = {}, {}
    for rank in range(RELAY_WORLD):
        plan = ensemble.relay_plan(RELAY_MEMBERS, RELAY_WORLD, RELAY_WINDOWS, rank)
        assert plan.count == 2 and [t.unit for t in plan.tasks] == [unit]
        task = plan.tasks[0]
        wr, agg, timers, log = _run(wins, RELAY_WINDOWS, RELAY_MEMBERS, combo, relay=plan, relay_comm=MailboxComm(box))
        assert {"relay_host", "relay_recv_wait"} <= set(timers)
        assert timers["trajectory_steps"] == (2 * RELAY_WINDOWS + (task.w_end - task.w_begin)) * lt.STEPS
        assert not set(wr.fields) & set(seen)
        seen.update(wr.fields)
        # relay rows: one-row flat batches keyed by the trajectory's own index, for this rank's slice of the windows
        relayed = [c for c in wr.calls if c[1] == unit]
        assert [c[0] for c in relayed] == [w * lt.STEPS + (1 if w else 0) for w in range(task.w_begin, task.w_end)]
        assert all(c[2]["a"][0] == 1 and len(c[2]["a"]) == 4 for c in relayed)
        assert {c[1] for c in wr.calls} == {plan.start, unit}
        assert sorted(w for o, _, _, w in log if o == unit) == list(range(task.w_begin, task.w_end))
        assert all(n == 1 for o, n, _, _ in log if o == unit)
        assert sorted(w for o, _, _, w in log if o == plan.start) == list(range(RELAY_WINDOWS))
        assert [c[1] for c in agg.calls if c[2]["gen"]["a"][0] == 1] == [[1 / RELAY_MEMBERS]] * (task.w_end - task.w_begin)
    assert not box
    assert sorted(seen) == sorted(wr0.fields) and all(torch.equal(v, wr0.fields[k]) for k, v in seen.items())


@pytest.mark.parametrize("prefetch", [2, 0])
def test_flagged_window_raises_before_it_is_written(job, prefetch):
    import sdy_amd

    _, wins, _, _ = job
    stepper = lt.FakeStepper(flag_window=2)
    wr, agg = Writer(MEMBERS), Aggregator()
    with pytest.raises(sdy_amd.SdyError):
        sdy_amd.run_inference(agg, stepper, lt.loader(wins), N_WINDOWS * lt.STEPS, lt.STEPS, n_ensemble_members=MEMBERS,
                              writer=wr, prefetch=prefetch)
    assert [c[0] for c in wr.calls] == [0, lt.STEPS + 1] and [c[0] for c in agg.calls] == [0, lt.STEPS + 1]
    assert max(t for _, t in wr.fields) == 2 * lt.STEPS         # nothing from window 2 onward
    assert not [t for t in threading.enumerate() if t.name == "sdy-window-prefetch"]
