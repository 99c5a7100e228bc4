"""Rank processes for the multi-process tests: ONE set per world size, reused by every test that needs that many ranks.

Up to round 4 every parametrisation spawned its own ranks (118 python processes in the GPU suite, each importing torch, creating
a HIP context and joining a fresh gloo group): ~40 % of the suite's wall time on the GPU box (VERDICT r04 "weak" 1).  Here a pool
of `world` processes joins ONE gloo group when it is first asked for and then serves jobs

    run_ranks(world, "test_distributed", "_native_body", spec, out_dir, ...)   ->   module.fn(rank, world, *args) on every rank

A job runs with a fresh engine context (the engine reads its MI_* switches when a context is created, so per-job os.environ
changes take effect; the pool restores the environment afterwards) and closes what it created before the next one.  ONE pool is
alive at a time; tests/conftest.py groups the multi-process tests by world size, plain-transport jobs before window jobs.
A rank that raises, or a job that exceeds its time limit, costs that pool its life (its processes are killed -- by PID -- and the
next job for that world size starts new ones), so one failing test cannot poison the ones after it.  That is MI_TEST_POOL=1; the
DEFAULT is fresh processes per call (same code path, pool closed after its one job): see run_ranks.
"""
import atexit
import importlib
import multiprocessing
import os
import socket
import sys
import tempfile
import time
import traceback

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
_POOLS = {}


def free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _rank_main(rank, world, store, conn, persistent):
    for p in (ROOT, HERE):
        if p not in sys.path:
            sys.path.insert(0, p)
    os.environ["MASTER_ADDR"] = "127.0.0.1"       # (no MASTER_PORT: the group meets through a file, below; a job body that opens a TCPStore or an
    os.environ.pop("MASTER_PORT", None)           #  nccl group of its own picks its port when it needs it -- test_distributed.py / test_gpu_configs.py do)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    try:
        import torch.distributed as dist
        # rendezvous through a FileStore: no port that is found free here and bound by rank 0 seconds later (EADDRINUSE in 2 of 58 pools
        # of one GPU-suite run of round 5); gloo's own pair sockets bind port 0 themselves
        dist.init_process_group("gloo", init_method=f"file://{store}", rank=rank, world_size=world)
        conn.send(("ready", None))
    except BaseException:
        conn.send(("error", traceback.format_exc()))
        return
    while True:
        try:
            job = conn.recv()
        except EOFError:
            break
        if job is None:
            break
        module, fn, args = job
        saved = dict(os.environ)
        try:
            getattr(importlib.import_module(module), fn)(rank, world, *args)
            _collect()
            conn.send(("ok", None))
        except BaseException:
            conn.send(("error", traceback.format_exc()))
        finally:
            for k in [k for k in os.environ if k not in saved]:
                del os.environ[k]
            for k, v in saved.items():
                if os.environ.get(k) != v:
                    os.environ[k] = v
        if not persistent:
            break
    try:
        dist.destroy_process_group()
    except Exception:
        pass


def _collect():
    import gc
    gc.collect()
    import torch
    if torch.cuda.is_available() and torch.cuda.is_initialized():
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


class RankPool:
    def __init__(self, world, persistent=True, caller_rank0=False, timeout=600.0):
        # The ranks meet through a FileStore (no rendezvous port that is found free here and bound a moment later -- round 5's
        # EADDRINUSE, 2 of 58 pools).  gloo's own pair sockets can still fail to bind on a busy box: start again instead of failing the test.
        # caller_rank0: rank 0 is THIS process (one process fewer with the GPU open), ranks 1 .. world-1 are started; its collectives
        # give up after `timeout` seconds, so a rank that dies cannot hold the caller forever.
        self.caller_rank0, self.timeout = caller_rank0, timeout
        for attempt in range(4):
            try:
                self._start(world, persistent)
                return
            except AssertionError as e:
                if attempt == 3 or "address already in use" not in str(e).lower():
                    raise

    def _start(self, world, persistent):
        ctx = multiprocessing.get_context("spawn")
        fd, store = tempfile.mkstemp(prefix="mi_rank_pool_", suffix=".store")
        os.close(fd); os.unlink(store)                 # (the FileStore creates it; the name only has to be unique)
        self.store = store
        self.world, self.procs, self.conns = world, [], []
        self.ranks = list(range(1 if self.caller_rank0 else 0, world))     # the ranks of the started processes, in procs / conns order
        self.joined = False
        for r in self.ranks:
            a, b = ctx.Pipe()
            p = ctx.Process(target=_rank_main, args=(r, world, store, b, persistent), daemon=True)
            p.start()
            b.close()
            self.procs.append(p); self.conns.append(a)
        try:
            if self.caller_rank0:
                self._join_caller()
            self._gather(180.0, "ready")
        except BaseException:
            self.kill()           # (kill() ran inside _gather; a rank that died before it could be killed leaves the file)
            raise

    def _join_caller(self):
        import datetime
        import torch.distributed as dist
        dist.init_process_group("gloo", init_method=f"file://{self.store}", rank=0, world_size=self.world,
                                timeout=datetime.timedelta(seconds=self.timeout))
        self.joined = True

    def _run_caller(self, module, fn, args):
        """the job's rank 0 in this process, with the environment of a rank process (restored afterwards); its traceback or None"""
        saved = dict(os.environ)
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ.pop("MASTER_PORT", None)
        try:
            for p in (ROOT, HERE):
                if p not in sys.path:
                    sys.path.insert(0, p)
            getattr(importlib.import_module(module), fn)(0, self.world, *args)
            _collect()
            return None
        except BaseException:
            return traceback.format_exc()
        finally:
            for k in [k for k in os.environ if k not in saved]:
                del os.environ[k]
            for k, v in saved.items():
                if os.environ.get(k) != v:
                    os.environ[k] = v

    def _gather(self, timeout, want, errors=None):
        deadline = time.monotonic() + timeout
        errors, pending = list(errors or []), set(range(len(self.conns)))
        if errors:
            deadline = time.monotonic() + 15.0
        while pending:
            for i in sorted(pending):
                r, c = self.ranks[i], self.conns[i]
                try:
                    if c.poll(0.05):
                        kind, payload = c.recv()
                        pending.discard(i)
                        if kind != want:
                            errors.append(f"--- rank {r} ---\n{payload}")
                            deadline = min(deadline, time.monotonic() + 15.0)    # the others may be waiting for this rank: do not wait long
                except (EOFError, OSError):
                    pending.discard(i)
                    errors.append(f"--- rank {r} ---\nprocess died (exit code {self.procs[i].exitcode})")
                    deadline = min(deadline, time.monotonic() + 15.0)
            if pending and time.monotonic() > deadline:
                if not errors:
                    errors.append(f"ranks {[self.ranks[i] for i in sorted(pending)]} did not answer within {timeout:.0f} s")
                break
        if errors:
            self.kill()
            raise AssertionError("rank job failed:\n" + "\n".join(errors))

    def run(self, module, fn, *args, timeout=600.0):
        for c in self.conns:
            c.send((module, fn, args))
        err = self._run_caller(module, fn, args) if self.caller_rank0 else None
        self._gather(timeout, "ok", [f"--- rank 0 (this process) ---\n{err}"] if err else None)

    def alive(self):
        return bool(self.procs) and all(p.is_alive() for p in self.procs)

    def close(self):
        for c in self.conns:
            try:
                c.send(None)
            except Exception:
                pass
        for p in self.procs:
            p.join(timeout=20)
        self.kill()

    def kill(self):
        for p in self.procs:          # exactly the processes this pool started
            if p.is_alive():
                p.kill()
        for p in self.procs:
            p.join(timeout=5)
        for c in self.conns:
            c.close()
        self.procs, self.conns = [], []
        if getattr(self, "joined", False):
            import torch.distributed as dist
            try:
                dist.destroy_process_group()
            except Exception:
                pass
            self.joined = False
        self._unlink_store()

    def _unlink_store(self):
        try:
            os.unlink(getattr(self, "store", ""))
        except OSError:
            pass


# GPU machines that are shared between users may cap the processes that have a device open at the same time: MAX_GPU_PROCESSES
# (default 6; MI_TEST_MAX_GPU_PROCESSES where the cap differs).  The test process has the GPU open as well, so a job of exactly that
# many ranks runs its rank 0 in the test process (run_ranks); a test with more ranks than the cap skips before it starts any.
MAX_GPU_PROCESSES = int(os.environ.get("MI_TEST_MAX_GPU_PROCESSES", "6"))


def skip_unless_gpu_processes(world):
    """pytest.skip unless `world` ranks fit under MAX_GPU_PROCESSES (the test process counts as rank 0 where it has to)"""
    import pytest
    if world > MAX_GPU_PROCESSES:
        pytest.skip(f"needs {world} rank processes with the GPU open at once, at most {MAX_GPU_PROCESSES} allowed here")


def run_ranks(world, module, fn, *args, timeout=600.0, fresh=False):
    """module.fn(rank, world, *args) on `world` ranks that share one gloo group; raises AssertionError with the ranks' tracebacks.
    fresh: do not reuse rank processes of earlier jobs (a process whose kernels have once waited on another process's windows
    stays slow -- 60 x on the plain transport, profiles/r05_c_native_solve_timings.tsv; the large plain-transport jobs ask for new ones)"""
    if fresh:
        for w in list(_POOLS):
            _POOLS.pop(w).close()
    # Default: fresh processes per call.  Re-used processes (MI_TEST_POOL=1) save ~3 s of start-up per test, but jobs that talk through
    # the host transport (a hipMemcpy per callback) get slower and slower in a process that has served jobs before -- measured on the
    # GPU box: a 4-rank cyclicAMI case 127 s re-used against ~12 s fresh, a 2-rank one 79 s against 3.3 s
    # (profiles/r05_c_multiprocess_test_timing.md); the cause was not found within the round's GPU time.
    caller = world + 1 > MAX_GPU_PROCESSES          # the test process + world ranks would exceed the cap: rank 0 runs here
    if caller:
        close_all()
    if os.environ.get("MI_TEST_POOL", "0") != "1" or caller:
        pool = RankPool(world, persistent=False, caller_rank0=caller, timeout=timeout)
        try:
            pool.run(module, fn, *args, timeout=timeout)
        finally:
            pool.close()
        return
    pool = _POOLS.get(world)
    if pool is None or not pool.alive():
        if pool is not None:
            pool.kill()
        # ONE pool at a time: every process with a HIP context takes one of the device's few process slots, and beyond them the
        # hardware scheduler swaps whole processes in and out -- ranks that wait for each other INSIDE kernels (windows, persistent
        # grids) then pay a scheduling quantum per exchange.  tests/conftest.py orders the multi-process tests by world size, so
        # the suite starts 2 + 3 + 4 + 8 rank processes in all.
        for w in list(_POOLS):
            _POOLS.pop(w).close()
        pool = _POOLS[world] = RankPool(world)
    try:
        pool.run(module, fn, *args, timeout=timeout)
    except BaseException:
        _POOLS.pop(world, None)
        raise


def close_all():
    for w in list(_POOLS):
        _POOLS.pop(w).close()


atexit.register(close_all)
