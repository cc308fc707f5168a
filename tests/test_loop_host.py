"""The pieces of the window driver (`sdy_amd.loop`) on the host: the presenter, the chunk runner, the dropout call numbering,
the hand-over queue and the stitcher's export / resume.  CPU tensors, integer-valued float32 on a 2 x 4 grid: every comparison
is `torch.equal`."""
import pytest
import torch

H, W = 2, 4


@pytest.fixture(scope="module")
def loop():
    from sdy_amd import loop

    return loop


def _ints(*shape, base=0.0):
    n = 1
    for s in shape:
        n *= s
    return torch.arange(n, dtype=torch.float32).view(*shape) + base


def _stepped(loop, rows, t1):
    return loop.SteppedData(metrics={"loss": torch.tensor(1.0)}, gen_data={"a": _ints(rows, t1, H, W)}, target_data={},
                            gen_data_norm={"a": _ints(rows, t1, H, W, base=10000.0)},
                            target_data_norm={"a": _ints(rows, t1, H, W, base=20000.0),
                                              "f": _ints(rows, t1, H, W, base=30000.0)})


def _window(n_sample, t1):
    return {"a": _ints(n_sample, t1, H, W, base=40000.0), "f": _ints(n_sample, t1, H, W, base=50000.0)}


class _Times:
    def __init__(self):
        self.sliced = []

    def isel(self, time):
        self.sliced.append(time)
        return ("sliced", time)


def test_present_rectangular_share_is_a_member_stacked_view(loop):
    from sdy_amd.ensemble import plan_rows

    n_sample, members, t1 = 3, 2, 3
    win, stepped = _window(n_sample, t1), _stepped(loop, n_sample * members, t1)
    plan = plan_rows(n_sample, members, 0, None)
    times = _Times()
    out, i_time_agg, weights, t_out, start_sample, last = loop._present(win, stepped, plan, members, None, 0, times)
    assert (i_time_agg, weights, start_sample) == (0, None, 0) and t_out is times and times.sliced == []
    assert out.metrics is stepped.metrics
    for got, src in ((out.gen_data, stepped.gen_data), (out.gen_data_norm, stepped.gen_data_norm)):
        assert got["a"].shape == (members, n_sample, t1, H, W)
        assert got["a"].untyped_storage().data_ptr() == src["a"].untyped_storage().data_ptr()
        for m in range(members):
            for s in range(n_sample):
                assert torch.equal(got["a"][m, s], src["a"][s * members + m])
    assert all(torch.equal(out.target_data[k], win[k]) for k in win) and list(out.target_data) == list(win)
    for k, v in stepped.target_data_norm.items():
        assert torch.equal(out.target_data_norm[k], v[0::members])
    assert torch.equal(last["a"], stepped.gen_data["a"][:, -1]) and last["a"].shape == (n_sample * members, H, W)

    # a later window: the first time is dropped everywhere, the aggregator's index moves on by one, times are sliced once
    out2, i_time_agg, weights, t_out, start_sample, last2 = loop._present(win, stepped, plan, members, None, 2, times)
    assert (i_time_agg, weights, start_sample) == (3, None, 0)
    assert times.sliced == [slice(1, None)] and t_out == ("sliced", slice(1, None))
    assert torch.equal(out2.gen_data["a"], out.gen_data["a"][:, :, 1:])
    assert torch.equal(out2.gen_data_norm["a"], out.gen_data_norm["a"][:, :, 1:])
    assert out2.gen_data["a"].untyped_storage().data_ptr() == stepped.gen_data["a"].untyped_storage().data_ptr()
    for k in win:
        assert torch.equal(out2.target_data[k], win[k][:, 1:])
        assert torch.equal(out2.target_data_norm[k], stepped.target_data_norm[k][0::members, 1:])
    assert torch.equal(last2["a"], last["a"])


def test_present_without_members_hands_the_stepped_tensors_on(loop):
    from sdy_amd.ensemble import plan_rows

    win, stepped = _window(3, 3), _stepped(loop, 3, 3)
    out, i_time_agg, weights, _, start_sample, _ = loop._present(win, stepped, plan_rows(3, 1, 0, None), 1, None, 0, None)
    assert out.gen_data["a"] is stepped.gen_data["a"] and out.gen_data_norm["a"] is stepped.gen_data_norm["a"]
    assert (i_time_agg, weights, start_sample) == (0, None, 0)
    assert all(torch.equal(out.target_data_norm[k], v) for k, v in stepped.target_data_norm.items())
    out, i_time_agg, _, t_out, _, _ = loop._present(win, stepped, plan_rows(3, 1, 0, None), 1, None, 2, None)
    assert i_time_agg == 3 and t_out is None and torch.equal(out.gen_data["a"], stepped.gen_data["a"][:, 1:])


@pytest.mark.parametrize("unit_range,ics,first,weights", [((2, 5), [0, 1, 1, 1, 2], [0, 1, 4], [1 / 3, 1.0, 1 / 3]),
                                                         ((1, 4), [0, 0, 1, 1], [0, 2], [2 / 3, 2 / 3])])
def test_present_ragged_share_stays_flat(loop, unit_range, ics, first, weights):
    from sdy_amd.ensemble import plan_rows

    n_sample, members, t1 = 3, 3, 3
    plan = plan_rows(n_sample, members, 0, unit_range)
    assert plan[2] == ics and not plan[4]
    win, stepped = _window(n_sample, t1), _stepped(loop, unit_range[1], t1)
    out, i_time_agg, got_w, _, start_sample, last = loop._present(win, stepped, plan, members, None, 0, None)
    assert start_sample == unit_range[0] and i_time_agg == 0 and got_w == weights
    assert out.gen_data["a"] is stepped.gen_data["a"] and out.gen_data["a"].shape[0] == unit_range[1]
    assert out.gen_data_norm["a"] is stepped.gen_data_norm["a"]
    for k in win:       # the targets of the initial conditions touched, normalised ones from the first row of each
        assert torch.equal(out.target_data[k], win[k][ics[0]:ics[-1] + 1])
        assert torch.equal(out.target_data_norm[k], stepped.target_data_norm[k][first])
    assert torch.equal(last["a"], stepped.gen_data["a"][:, -1])
    out2, i_time_agg, got_w, _, start_sample, _ = loop._present(win, stepped, plan, members, None, 2, None)
    assert (i_time_agg, got_w, start_sample) == (3, weights, unit_range[0])
    assert torch.equal(out2.gen_data["a"], stepped.gen_data["a"][:, 1:])
    assert torch.equal(out2.target_data_norm["f"], stepped.target_data_norm["f"][first][:, 1:])


def test_present_derives_before_the_first_time_is_dropped(loop):
    from sdy_amd.ensemble import plan_rows

    n_sample, members, t1 = 3, 2, 3
    win, stepped = _window(n_sample, t1), _stepped(loop, n_sample * members, t1)
    seen = []

    def derive(d):
        seen.append(d["a"].shape[-3])
        return {**d, "d": d["a"] * 2.0}

    out, _, _, _, _, _ = loop._present(win, stepped, plan_rows(n_sample, members, 0, None), members, derive, 2, None)
    assert seen == [t1, t1]                                     # targets, then predictions: both with all T + 1 times
    assert torch.equal(out.target_data["d"], win["a"][:, 1:] * 2.0)
    plain, _, _, _, _, _ = loop._present(win, stepped, plan_rows(n_sample, members, 0, None), members, None, 2, None)
    assert torch.equal(out.gen_data["d"], plain.gen_data["a"] * 2.0) and torch.equal(out.gen_data["a"], plain.gen_data["a"])
    assert list(out.gen_data_norm) == ["a"] and list(out.target_data_norm) == ["a", "f"]


class _Module:
    def __init__(self, calls=(0, 0)):
        self.offset, self.calls = None, tuple(calls)

    def set_batch_offset(self, offset):
        self.offset = offset

    def set_dropout_calls(self, calls):
        self.calls = tuple(calls)

    def dropout_calls(self):
        return self.calls


class _Stepper:
    """gen_data[r, t] = the row's time-0 state + 1000 x its global index + 10 x forecaster calls + interpolator calls + t."""

    def __init__(self, loop, losses):
        self.loop, self.module, self.log, self.losses, self.last = loop, _Module(), [], list(losses), None

    def run_on_batch(self, data, optimization, n_forward_steps, defer_metrics):
        assert optimization is None and defer_metrics is True
        m, rows = self.module, data["a"].shape[0]
        self.log.append((m.offset, rows, m.calls))
        key = ((m.offset + torch.arange(rows)) * 1000.0 + 10.0 * m.calls[0] + m.calls[1]).view(rows, 1, 1, 1)
        gen = data["a"][:, :1] + key + torch.arange(n_forward_steps + 1.0).view(1, -1, 1, 1)
        m.calls = (m.calls[0] + 6, m.calls[1] + 10)
        self.last = self.loop.SteppedData(metrics={"loss": self.losses.pop(0)}, gen_data={"a": gen}, target_data=data,
                                          gen_data_norm={"a": gen * 2.0}, target_data_norm={k: v * 3.0 for k, v in data.items()})
        return self.last


def test_run_chunks_equals_the_unchunked_window(loop):
    start, n_steps, calls0 = 7, 2, (12, 20)
    batch = _window(3, n_steps + 1)
    l0, l1 = torch.tensor(0.3), torch.tensor(0.7)
    whole = _Stepper(loop, [torch.tensor(0.5)])
    ref = loop._run_chunks(whole, batch, start, n_steps, None, calls0)
    assert ref is whole.last and whole.log == [(start, 3, calls0)]              # one chunk: the stepper's own object
    for max_batch, losses, rows in ((1, [l0, l1, l0], [1, 1, 1]), (2, [l0, l1], [2, 1]), (3, [l0], [3]), (5, [l0], [3])):
        st = _Stepper(loop, losses)
        got = loop._run_chunks(st, batch, start, n_steps, max_batch, calls0)
        offsets = [start + sum(rows[:i]) for i in range(len(rows))]
        assert st.log == [(o, r, calls0) for o, r in zip(offsets, rows)]      # own offset, the window's call numbers again
        assert (got is st.last) == (len(rows) == 1)
        for name in ("gen_data", "gen_data_norm", "target_data_norm"):
            a, b = getattr(got, name), getattr(ref, name)
            assert list(a) == list(b) and all(torch.equal(a[k], b[k]) for k in b), (max_batch, name)
        assert all(torch.equal(got.target_data[k], batch[k]) for k in batch)
        if max_batch == 2:
            want = sum(m * (r / 3.0) for r, m in ((2, l0), (1, l1)))
            assert torch.equal(got.metrics["loss"], want) and list(got.metrics) == ["loss"] and len(got.metrics) == 1
    # without call numbers the module's counters are left to run on
    st = _Stepper(loop, [l0, l1])
    loop._run_chunks(st, batch, start, n_steps, 2, None)
    assert st.log == [(start, 2, (0, 0)), (start + 2, 1, (6, 10))]


def test_dropout_calls_number_the_windows_from_the_origin(loop):
    m = _Module((5, 7))
    calls = loop._DropoutCalls(m)
    assert calls.at(0) == (5, 7)
    m.calls = (11, 17)
    assert calls.at(0) == (5, 7)
    calls.learn((5, 7))
    m.calls = (99, 99)                          # (relay work in between: the numbering no longer looks at the counters)
    calls.learn((5, 7))                         # learned once, from the first resident batch
    assert calls.at(3) == (23, 37) and calls.at(1) == (11, 17) and calls.at(0) == (5, 7)
    # no relay hosted: a window starts from wherever the counters stand
    free = loop._DropoutCalls(m, replay=False)
    m.calls = (3, 4)
    assert free.at(0) == (3, 4) and free.at(5) == (3, 4)
    # a module without counters
    none = loop._DropoutCalls(object())
    assert none.at(0) is None
    none.learn(None)
    assert none.at(3) is None


class _Flagged(RuntimeError):
    pass


class _Loss:
    def __init__(self, value, flagged=False):
        self.value, self.flagged = value, flagged

    def __float__(self):
        if self.flagged:
            raise _Flagged("window flagged")
        return self.value


def _entry(loop, k, log, weights=None, flagged=False):
    out = loop.SteppedData(metrics={"loss": _Loss(float(k), flagged)}, gen_data={"k": k}, target_data={}, gen_data_norm={},
                           target_data_norm={})
    return out, 10 * k, weights, lambda: log.append(("write", k))


class _Agg:
    def __init__(self, log):
        self.log = log

    def record_batch(self, loss, target_data, gen_data, target_data_norm, gen_data_norm, i_time_start=0):
        self.log.append(("agg", gen_data["k"], loss, i_time_start))


class _WeightedAgg:
    accepts_sample_weights = True

    def __init__(self, log):
        self.log = log

    def record_batch(self, loss, target_data, gen_data, target_data_norm, gen_data_norm, i_time_start=0, **kw):
        self.log.append(("agg", gen_data["k"], kw))


def test_handover_flushes_behind_the_loss(loop):
    def done(k):
        return [("write", k), ("agg", k, float(k), 10 * k)]

    log = []
    h = loop._Handover(_Agg(log), depth=1)
    h.add(_entry(loop, 0, log))
    assert log == []
    h.add(_entry(loop, 1, log))
    assert log == done(0)
    h.drain()
    assert log == done(0) + done(1)
    h.drain()
    assert log == done(0) + done(1)

    log = []
    h = loop._Handover(_Agg(log), depth=0)
    for k in range(2):
        h.add(_entry(loop, k, log))
        assert log == sum((done(j) for j in range(k + 1)), [])

    # a flagged entry raises out of the hand-over: neither its write nor the aggregator ran, earlier ones went out in order
    log = []
    h = loop._Handover(_Agg(log), depth=1)
    h.add(_entry(loop, 0, log))
    h.add(_entry(loop, 1, log))
    h.add(_entry(loop, 2, log, flagged=True))
    with pytest.raises(_Flagged):
        h.add(_entry(loop, 3, log))
    assert log == done(0) + done(1)
    log = []
    h = loop._Handover(_Agg(log), depth=0)
    with pytest.raises(_Flagged):
        h.add(_entry(loop, 0, log, flagged=True))
    assert log == []


def test_handover_passes_sample_weights_only_where_declared(loop):
    log = []
    h = loop._Handover(_WeightedAgg(log), depth=0)
    h.add(_entry(loop, 0, log, weights=[0.5, 1.0]))
    h.add(_entry(loop, 1, log))
    assert log == [("write", 0), ("agg", 0, {"sample_weights": [0.5, 1.0]}), ("write", 1), ("agg", 1, {})]
    log = []
    h = loop._Handover(_Agg(log), depth=0)          # (its record_batch would refuse the keyword)
    h.add(_entry(loop, 0, log, weights=[0.5, 1.0]))
    assert log == [("write", 0), ("agg", 0, 0.0, 0)]


def test_window_stitcher_exports_and_resumes_its_carried_state(loop):
    steps, n_windows = 2, 3
    calls = []

    class Writer:
        def __init__(self, tag):
            self.tag = tag

        def append_batch(self, target, prediction, start_timestep, start_sample, batch_times=None):
            calls.append((self.tag, start_timestep, start_sample))

    def window(w):
        return {k: _ints(1, steps + 1, H, W, base=1000.0 * (w + 1) + 100.0 * j) for j, k in enumerate(("a", "b", "f"))}

    def gen(w):
        return {k: _ints(1, steps + 1, H, W, base=7000.0 * (w + 1) + 100.0 * j) for j, k in enumerate(("a", "b"))}

    st = loop.WindowStitcher(steps * n_windows, Writer("whole"), is_ensemble=True)
    st.append(window(0), gen(0), None, last_state={k: v[:, -1] for k, v in gen(0).items()}, start_sample=4)
    st.append({k: v[:, 1:] for k, v in window(1).items()}, {k: v[:, 1:] for k, v in gen(1).items()}, None,
              last_state={k: v[:, -1] for k, v in gen(1).items()}, start_sample=4)
    state = st.carried_state(["b", "a"])
    assert state.shape == (2, H, W)
    assert torch.equal(state[0], gen(1)["b"][0, -1]) and torch.equal(state[1], gen(1)["a"][0, -1])

    fresh = loop.WindowStitcher(steps * n_windows, Writer("resumed"), is_ensemble=True)
    fresh.resume(2 * steps + 1, ["b", "a"], state, {k: v[:, -1] for k, v in window(1).items()})
    assert fresh.i_time == st.i_time == 2 * steps + 1
    batches = [{k: v.clone() for k, v in window(2).items()} for _ in range(2)]
    st.apply_initial_condition(batches[0])
    fresh.apply_initial_condition(batches[1])
    for k in ("a", "b", "f"):
        assert torch.equal(batches[0][k], batches[1][k])
        assert torch.equal(batches[0][k][:, 1:], window(2)[k][:, 1:])
    assert torch.equal(batches[1]["a"][:, 0], gen(1)["a"][:, -1]) and torch.equal(batches[1]["f"][:, 0], window(1)["f"][:, -1])
    calls.clear()
    for s in (st, fresh):
        s.append({k: v[:, 1:] for k, v in window(2).items()}, {k: v[:, 1:] for k, v in gen(2).items()}, None, start_sample=4)
    assert calls == [("whole", 2 * steps + 1, 4), ("resumed", 2 * steps + 1, 4)]


def test_run_inference_keeps_its_shape(loop):
    """The driver's body is a sequence of named pieces: no nested function, no `nonlocal`, no lambda bound to a name; and the
    stitcher's carried state is touched by the stitcher alone."""
    import ast
    import inspect

    src = inspect.getsource(loop)
    tree = ast.parse(src)
    fn = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "run_inference")
    assert not [n for n in ast.walk(fn) if n is not fn and isinstance(n, (ast.FunctionDef, ast.Nonlocal))]
    assert not [n for n in ast.walk(fn) if isinstance(n, ast.Assign) and isinstance(n.value, ast.Lambda)]
    assert "noqa: E731" not in src
    cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "WindowStitcher")
    inside = {id(n) for n in ast.walk(cls)}
    for n in ast.walk(tree):
        if isinstance(n, ast.Attribute) and id(n) not in inside:
            assert n.attr not in ("_carry_gen", "_carry_target"), n.lineno
            assert not (n.attr == "i_time" and isinstance(n.ctx, ast.Store)), n.lineno
