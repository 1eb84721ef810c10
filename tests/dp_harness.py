"""Two data-parallel ranks for the GPU tests (tests/test_gpu_dp.py, tests/test_gpu_dp_options.py): ``launch`` starts ``world``
fresh processes (the ``spawn`` context), hands each one picklable case description and collects one result dictionary per rank.

Transport: gloo, both processes on device 0 (two RCCL ranks cannot share a device).  Where this PyTorch build's gloo cannot move
device tensors, the worker installs ``HostStagedExchange`` in place of ``dp.GradExchange`` -- the package itself is untouched --
and every result says which of the two ran (``result["transport"]``: "gloo-device" or "gloo-host-staged").

Time limits.  The world-2 test of tests/test_gpu_dp.py as it stood before this harness -- one launch: two ranks, the
interpreter and library start-up, ONE ngf 16 ResNet cycle model per rank, two steps -- took 3.8 s (eager) and 2.9 s (replayed)
on an MI355X, its own single-process comparison step included: MEASURED_LAUNCH_S.  A launch gets three times that,
LAUNCH_LIMIT_S = 11.4 s, for every model a worker builds and steps (``models``: the tests of tests/test_gpu_dp_options.py build
three or four per launch -- the probe that finds the clip bound, the eager model, the graph=True model, a lockstep twin), plus
``oracle_s`` for the float64 oracle a worker runs after its last collective (5-15 s of CPU per rank and step; the tests state
theirs).  Every wait is bounded by what is left of that limit; a worker still alive at the limit is terminated.  A worker that ended by a signal or at its limit may have left the device in a bad state: the harness records it, and
every later launch of the same pytest session fails at once without starting anything on the GPU.  Nothing is retried."""
import os
import queue as _queue
import socket
import sys
import time
import traceback

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_WORKERS = 2
MEASURED_LAUNCH_S = 3.8
LAUNCH_LIMIT_S = 3 * MEASURED_LAUNCH_S

_POISONED = None            # why no further launch may start (a worker was killed by a signal or ran into its limit)


def free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _host_staged_exchange():
    from sggan_amd.dp import GradExchange
    import torch
    import torch.distributed as dist

    class _Done:
        def wait(self):
            return True

    class HostStagedExchange(GradExchange):
        """dp.GradExchange for a gloo that only moves host tensors: the stream is synchronised, the bucket copied to pinned host
        memory, reduced there and copied back -- complete when the call returns, so the handle's wait() has nothing to do."""

        def _staged(self, t, collective):
            torch.cuda.current_stream(t.device).synchronize()
            host = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
            host.copy_(t)
            collective(host)
            t.copy_(host)
            torch.cuda.current_stream(t.device).synchronize()

        def broadcast_(self, flat_params, src_rank_in_group=0):
            src = dist.get_global_rank(self.group, src_rank_in_group)
            self._staged(flat_params, lambda h: dist.broadcast(h, src=src, group=self.group))

        def allreduce_async(self, flat_grad):
            self._staged(flat_grad, lambda h: dist.all_reduce(h, op=dist.ReduceOp.SUM, group=self.group))
            return _Done()

    return HostStagedExchange


def _install_transport():
    """"gloo-device" if this build's gloo sums a device tensor (both ranks probe with the same collective, so both take the same
    branch), else the host-staged subclass is put in dp.GradExchange's place and "gloo-host-staged" is returned."""
    import torch
    import torch.distributed as dist
    import sggan_amd.dp as dp
    try:
        probe = torch.ones(4, dtype=torch.float32, device="cuda")
        dist.all_reduce(probe)
        ok = bool((probe.cpu() == dist.get_world_size()).all())
    except (RuntimeError, NotImplementedError):
        ok = False
    if ok:
        return "gloo-device"
    dp.GradExchange = _host_staged_exchange()
    return "gloo-host-staged"


def _entry(rank, world, port, limit, worker, case, out):
    try:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
        if ROOT not in sys.path:
            sys.path.insert(0, ROOT)
        import datetime
        import torch
        import torch.distributed as dist
        torch.cuda.set_device(0)
        dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=limit))
        transport = _install_transport()
        res = dict(worker(rank, world, case))
        res.update(rank=rank, transport=transport, error=None)
        torch.cuda.synchronize()
        out.put(res)
        dist.destroy_process_group()
    except BaseException:                           # surfaced by the parent, which fails with it
        out.put({"rank": rank, "error": traceback.format_exc()})


def launch(worker, cases, models=1, oracle_s=0.0):
    """Run ``worker(rank, world, cases[rank]) -> dict`` in ``len(cases)`` fresh processes; the list of their results by rank, each
    with "rank" and "transport" added.  ``worker`` must be importable by name (a module-level function).  Fails -- with the
    worker's traceback where there is one -- if any rank raised, died or ran into the limit."""
    global _POISONED
    import torch.multiprocessing as mp
    world = len(cases)
    assert 1 <= world <= MAX_WORKERS, f"at most {MAX_WORKERS} workers at a time, got {world}"
    if _POISONED is not None:
        raise AssertionError(f"no launch after a worker was lost earlier in this session ({_POISONED}): nothing was started")
    limit = LAUNCH_LIMIT_S * max(int(models), 1) + float(oracle_s)
    deadline = time.monotonic() + limit
    left = lambda: max(deadline - time.monotonic(), 0.0)
    ctx = mp.get_context("spawn")
    out = ctx.Queue()
    port = free_port()
    procs = [ctx.Process(target=_entry, args=(r, world, port, limit, worker, cases[r], out)) for r in range(world)]
    for p in procs:
        p.start()
    results, lost = {}, None

    def collect(wait):
        try:
            r = out.get(timeout=max(wait, 0.001))
        except _queue.Empty:
            return False
        results[r["rank"]] = r
        return True

    try:
        while len(results) < world and lost is None:
            if collect(min(left(), 1.0)):
                continue
            gone = [p.exitcode for rank, p in enumerate(procs) if rank not in results and not p.is_alive()]
            if gone and not collect(0.5):           # (ended, and nothing of its in the queue)
                lost = f"a worker ended with exit code {gone[0]} and no result"
            elif left() <= 0:
                lost = f"no result within the launch limit of {limit:.0f} s"
            elif any(r["error"] is not None for r in results.values()):
                # a rank raised: gloo fails its peer's pending collective once the process is gone, and the peer reports that;
                # it gets a short while to do so, not the whole limit
                deadline = min(deadline, time.monotonic() + 30.0)
    finally:
        for p in procs:                             # results are in (or given up on): the workers only have to exit
            p.join(timeout=min(left(), 30.0) if len(results) == world else 5.0)
        for p in procs:
            if p.is_alive():
                lost = lost or "a worker was still alive at its limit and was terminated"
                p.terminate()
                p.join(timeout=10)
                if p.is_alive():
                    p.kill()
                    p.join(timeout=10)
        signalled = [p.exitcode for p in procs if p.exitcode is not None and p.exitcode < 0]
        if signalled and lost is None:
            lost = f"a worker was ended by signal {-signalled[0]}"
        if lost is not None:
            _POISONED = lost
    errors = [r["error"] for r in results.values() if r["error"] is not None]
    if errors:
        raise AssertionError("a data-parallel worker raised:\n" + "\n".join(errors) + (f"\n({lost})" if lost else ""))
    if lost is not None:
        raise AssertionError("data-parallel launch lost a worker: " + lost)
    return [results[r] for r in range(world)]
