"""The relay's peer transport (`ensemble.RelayComm(transport="peer")`) on gloo process groups of 2, 3 and 4 ranks, with a
host-memory copy engine injected in place of the GPU one (`HostEngine`: the same create / open / copy / query surface, shared
memory standing in for the exported device pool, copies that land a fixed latency after they are enqueued).  The schedule is
the product's (`relay_plan`, `RelayRunner` via `run_relay`), the windows are the deterministic stand-in of
tests/test_distributed_cpu.py, and every group runs under a time limit."""
import multiprocessing as mp
import os
import socket
import sys
import time
import uuid

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LATENCY_S = 0.1        # a copy lands this long after it was enqueued (or when the "compute stream" waits for it)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _advance(x, unit, w):
    return x * 1.0001 + torch.sin(torch.arange(4, dtype=torch.float64) + 7.0 * unit + 0.37 * w) * (1.0 + x.abs().sum())


def _serial(n_units, n_windows):
    out = {}
    for u in range(n_units):
        x = torch.full((4,), float(u), dtype=torch.float64)
        for w in range(n_windows):
            x = _advance(x, u, w)
        out[u] = x
    return out


class HostEngine:
    """Host-memory copy engine.  Pools are POSIX shared memory (the handle names the segment and its owner); a copy is
    performed lazily, when `query` finds its latency elapsed or when a consumer `wait`s / `sync`s on it.  Instrumented:
    waiting on a SEND copy outside warm-up is an error (the sender must never block on its copies), and the registry shared
    by all ranks counts the open mappings of every pool, so that freeing a mapped pool fails."""

    def __init__(self, rank, registry, log):
        self.rank, self.registry, self.log = rank, registry, log
        self.shm, self.views, self.in_warm_up = {}, {}, True

    def _addr(self, seg):
        import ctypes as C

        view = C.c_char.from_buffer(seg.buf)
        self.views[seg.name] = view
        return C.addressof(view)

    def create(self, slot_bytes, n_slots):
        from multiprocessing import shared_memory

        seg = shared_memory.SharedMemory(create=True, size=slot_bytes * n_slots, name=f"sdyrelay_{uuid.uuid4().hex[:16]}")
        self.shm[seg.name] = seg
        self.registry[seg.name] = 0
        base = self._addr(seg)
        return base, f"{self.rank}:{seg.name}".encode().ljust(64, b"\0")

    def destroy(self, base):
        name = self._name_at(base)
        if self.registry[name] != 0:
            raise AssertionError(f"rank {self.rank} frees its pool while {self.registry[name]} mapping(s) are open")
        self.log.append(("destroy", name, self.rank, time.monotonic()))
        del self.views[name]
        seg = self.shm.pop(name)
        seg.close()
        seg.unlink()

    def _name_at(self, ptr):
        import ctypes as C

        names = [n for n, v in self.views.items() if C.addressof(v) == ptr]
        assert len(names) == 1, ptr
        return names[0]

    def open(self, handle):
        from multiprocessing import shared_memory

        owner, name = handle.rstrip(b"\0").decode().split(":")
        seg = shared_memory.SharedMemory(name=name)
        self.shm[name] = seg
        self.registry[name] = self.registry[name] + 1
        self.log.append(("open", name, self.rank, time.monotonic()))
        return self._addr(seg)

    def close(self, ptr):
        name = self._name_at(ptr)
        del self.views[name]
        self.shm.pop(name).close()
        time.sleep(0.05)                      # a slow opener: the owner has to wait for it
        self.registry[name] = self.registry[name] - 1
        self.log.append(("close", name, self.rank, time.monotonic()))

    def copy(self, dst, src, nbytes, after_compute):
        return {"dst": dst, "src": src, "n": nbytes, "t": time.monotonic(), "done": False, "send": after_compute,
                "warm": self.in_warm_up}

    def _land(self, tok):
        import ctypes as C

        if not tok["done"]:
            C.memmove(tok["dst"], tok["src"], tok["n"])
            tok["done"] = True

    def query(self, tok):
        if time.monotonic() - tok["t"] >= LATENCY_S:
            self._land(tok)
        return tok["done"]

    def elapsed_ms(self, tok):
        return LATENCY_S * 1e3

    def wait(self, tok):
        assert not (tok["send"] and not tok["warm"]), "the sender waited for its own copy"
        self._land(tok)

    def sync(self, tok):
        if tok is not None:
            self.wait(tok)
        else:
            self.in_warm_up = False


def _init(rank, world, port):
    import torch.distributed as dist

    store = dist.TCPStore("127.0.0.1", port, world, rank == 0)
    dist.init_process_group("gloo", store=store, rank=rank, world_size=world)
    sys.path.insert(0, ROOT)
    return dist, store


def _timed(obj, name, durations):
    fn = getattr(obj, name)

    def wrapped(*a, **k):
        t0 = time.monotonic()
        try:
            return fn(*a, **k)
        finally:
            durations.append((name, time.monotonic() - t0))

    setattr(obj, name, wrapped)


def _job(rank, world, store, registry, log, n_units, n_windows, delays, durations=None, jobs=1):
    """`jobs` consecutive relayed jobs on this rank; returns [(job id, plan, {unit: final}, log of advanced windows)]."""
    from sdy_amd import ensemble

    out = []
    for _ in range(jobs):
        plan = ensemble.relay_plan(n_units, world, n_windows, rank)
        like = torch.empty(4, dtype=torch.float64)
        comm = ensemble.RelayComm(transport="peer", store=store, plan=plan, like=like, engine=HostEngine(rank, registry, log),
                                  timeout_s=60.0)
        assert isinstance(comm, ensemble.PeerRelayComm) and comm.transport == "peer"
        comm.warm_up()
        if durations is not None:
            for name in ("send", "ready", "poll"):
                _timed(comm, name, durations)
        res = {u: torch.full((4,), float(u), dtype=torch.float64) for u in range(plan.start, plan.start + plan.count)}
        steps = []

        def resident_step(w):
            for u in res:
                res[u] = _advance(res[u], u, w)
            if delays:
                time.sleep(delays[rank])

        def relay_step(task, w, x):
            steps.append((task.unit, w))
            return _advance(x, task.unit, w)

        finals = ensemble.run_relay(plan, n_windows, resident_step, relay_step,
                                    lambda u: torch.full((4,), float(u), dtype=torch.float64), comm,
                                    like=lambda task: like)
        comm.close()
        res.update({u: v.clone() for u, v in finals.items()})
        out.append((comm.job, plan, res, steps, list(comm.handover_ms)))
    return out


def _worker(rank, world, port, n_units, n_windows, delays, jobs, registry, log, ret):
    dist, store = _init(rank, world, port)
    durations = []
    ret[rank] = (_job(rank, world, store, registry, log, n_units, n_windows, delays, durations, jobs), durations)
    dist.barrier()
    dist.destroy_process_group()


def _launch(target, world, args, timeout=120.0):
    ctx = mp.get_context("spawn")
    mgr = ctx.Manager()
    registry, log, ret = mgr.dict(), mgr.list(), mgr.dict()
    port = _free_port()
    procs = [ctx.Process(target=target, args=(r, world, port) + tuple(args) + (registry, log, ret)) for r in range(world)]
    for p in procs:
        p.start()
    deadline = time.monotonic() + timeout
    for p in procs:
        p.join(max(0.0, deadline - time.monotonic()))
    hung = [r for r, p in enumerate(procs) if p.is_alive()]
    for p in procs:
        if p.is_alive():
            p.terminate()
            p.join(5)
    assert not hung, f"ranks {hung} did not finish within {timeout} s"
    assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
    return dict(ret), list(log)


def _check(world, n_units, n_windows, ret, log, jobs=1):
    want = _serial(n_units, n_windows)
    for j in range(jobs):
        got, seen = {}, []
        ids = {ret[r][0][j][0] for r in range(world)}
        assert len(ids) == 1, f"job {j}: ranks disagree on the job id: {ids}"
        for r in range(world):
            _, plan, res, steps, _ = ret[r][0][j]
            got.update(res)
            seen += steps
        assert sorted(got) == list(range(n_units))
        for u in range(n_units):
            assert torch.equal(got[u], want[u]), (world, n_units, j, u)
        relayed = list(range(world * (n_units // world), n_units))
        assert sorted(seen) == [(u, w) for u in relayed for w in range(n_windows)]
    if jobs > 1:
        assert len({ret[0][0][j][0] for j in range(jobs)}) == jobs, "consecutive jobs share an id"
    # teardown: every pool opened by another rank is freed, after the last of its openers closed it
    opened = {e[1] for e in log if e[0] == "open"}
    freed = {e[1]: e[3] for e in log if e[0] == "destroy"}
    assert opened and opened <= set(freed)
    for name, t_free in freed.items():
        closes = [c[3] for c in log if c[0] == "close" and c[1] == name]
        assert len(closes) == sum(o[0] == "open" and o[1] == name for o in log), name
        assert all(t < t_free for t in closes), (name, closes, t_free)


@pytest.mark.parametrize("world,n_units,n_windows,delays", [
    (2, 5, 6, None),
    (3, 7, 7, (0.0, 0.02, 0.0)),
    (3, 8, 5, (0.02, 0.0, 0.01)),       # two relay trajectories; the second one's chain wraps around the ring
    (4, 9, 8, (0.0, 0.01, 0.02, 0.0)),
])
def test_peer_transport_relays_bit_identically_to_the_serial_run(world, n_units, n_windows, delays):
    ret, log = _launch(_worker, world, (n_units, n_windows, delays, 1))
    _check(world, n_units, n_windows, ret, log)
    tasks = [t for r in range(world) for t in ret[r][0][0][1].tasks]
    if (world, n_units) == (3, 8):
        assert any(t.src is not None and t.dst is not None and t.src > t.dst for t in tasks)      # 2 -> 0 -> 1: wraps
    n_hops = sum(t.src is not None for t in tasks)
    assert sum(len(ret[r][0][0][4]) for r in range(world)) == n_hops        # a hand-over time for every hand-over


def test_no_sender_call_blocks():
    """The copies take LATENCY_S; send / ready / poll return long before that (HostEngine also asserts that nobody waits on a
    send copy), with a receiver that runs four times slower than the sender."""
    ret, log = _launch(_worker, 2, (5, 8, (0.01, 0.04), 1))
    _check(2, 5, 8, ret, log)
    assert any(n == "send" for n, _ in ret[0][1])
    for r in range(2):
        slow = [(n, d) for n, d in ret[r][1] if d > LATENCY_S / 2]
        assert not slow, (r, slow)


def _only_sender_worker(rank, world, port, registry, log, ret):
    """Rank 0 hosts the relay trajectory's first slice and only sends; rank 1 is slow.  Records whether rank 0's hand-over
    was announced before rank 0 entered drain()."""
    dist, store = _init(rank, world, port)
    from sdy_amd import ensemble

    n_windows = 6
    plan = ensemble.relay_plan(5, 2, n_windows, rank)
    like = torch.empty(4, dtype=torch.float64)
    comm = ensemble.RelayComm(transport="peer", store=store, plan=plan, like=like, engine=HostEngine(rank, registry, log),
                              timeout_s=60.0)
    comm.warm_up()
    runner = ensemble.RelayRunner(plan, comm, lambda t, w, x: _advance(x, t.unit, w),
                                  lambda t: torch.full((4,), float(t.unit), dtype=torch.float64), lambda t: like)
    announced_before_drain = None
    key = None
    for w in range(n_windows):
        time.sleep(0.25 if rank == 0 else 0.6)           # a window of the resident batch
        runner.after_window(w)
        if rank == 0 and plan.tasks and plan.tasks[0].w_end == w + 1:
            key = comm._key("ready", plan.tasks[0].unit, plan.tasks[0].w_end)
    if rank == 0:
        announced_before_drain = store.check([key])
    finals = runner.drain(n_windows - 1)
    comm.close()
    ret[rank] = (plan, announced_before_drain, {u: v.clone() for u, v in finals.items()})
    dist.barrier()
    dist.destroy_process_group()


def test_a_rank_that_only_sends_announces_at_its_next_window_boundary():
    ret, _ = _launch(_only_sender_worker, 2, ())
    plan0 = ret[0][0]
    assert all(t.src is None and t.dst == 1 for t in plan0.tasks) and plan0.tasks
    assert ret[0][1] is True, "the sender announced its state only at drain()"
    assert torch.equal(ret[1][2][4], _serial(5, 6)[4])


def test_chains_crossing_one_pair_in_opposite_directions_complete():
    """world = 4, r = 2, two windows: trajectory 4 hops 1 -> 3 and trajectory 5 hops 3 -> 1 after window 0."""
    from sdy_amd import ensemble

    hops = {(t.unit, t.src, r) for r in range(4) for t in ensemble.relay_plan(6, 4, 2, r).tasks if t.src is not None}
    assert hops == {(4, 1, 3), (5, 3, 1)}
    ret, log = _launch(_worker, 4, (6, 2, (0.0, 0.03, 0.0, 0.01), 1), timeout=90.0)
    _check(4, 6, 2, ret, log)


def test_consecutive_jobs_agree_on_their_ids_when_some_ranks_host_no_slice():
    """25-over-8 in miniature with fewer windows than ranks: ranks 0 and 2 host no slice (and race ahead into the second job);
    every rank still builds the comm for every job, and the job ids come from the store, not from a per-process count."""
    from sdy_amd import ensemble

    assert [bool(ensemble.relay_plan(5, 4, 2, r).tasks) for r in range(4)] == [False, True, False, True]
    ret, log = _launch(_worker, 4, (5, 2, (0.0, 0.02, 0.0, 0.02), 2), timeout=90.0)
    _check(4, 5, 2, ret, log, jobs=2)


def test_unknown_transport_raises():
    from sdy_amd import ensemble

    with pytest.raises(ValueError, match="unknown relay transport"):
        ensemble.RelayComm(transport="rdma")
    with pytest.raises(ValueError, match="unknown relay transport"):
        ensemble.RelayComm(transport="default")
