"""The one way a test starts other processes: run_ranks (the spawned ranks of a world) and run_child (a fresh `python -c` child
under another environment).  Both fail fast -- a rank or child that dies, raises or overruns its limit fails the caller at once,
with exit codes, signal names and the traceback or stderr tail in the message -- both leave no process behind, and neither retries.

A launch marked gpu=True also keeps the rule of a shared device: once a process that may have had the GPU open died by a signal or
was killed at its time limit, nothing more is started on the card by this pytest process (the latch, below).

A plain helper, not a conftest; torch is imported only inside a rank that asked for a process group, so a spawned child that
re-imports this module, and the launcher's own tests (test_ranks_cpu.py), start fast."""
import multiprocessing
import os
import queue
import signal
import subprocess
import sys
import tempfile
import time
import traceback

TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)
POLL = 1.0                        # seconds between two looks at the ranks' exit codes
STDERR_TAIL = 3000                # characters of a failed child's stderr quoted in the failure
PRELUDE = 'import os, sys\nsys.path[:0] = [os.environ["OV_ROOT"], os.path.join(os.environ["OV_ROOT"], "tests")]\n'


class LaunchError(AssertionError):
    """A rank or child died, raised, overran its limit, or was not started because of the latch."""


# ---- the latch: the first gpu=True process to die by a signal or at its time limit; every later gpu=True launch quotes it and refuses
_gpu_death = None


def reset():
    """Forget the latched death.  For the latch's own test, whose 'GPU' children never touch a device."""
    global _gpu_death
    _gpu_death = None


def _obey_latch(gpu):
    if gpu and _gpu_death is not None:
        raise LaunchError("not started: an earlier GPU process of this session died, and nothing more runs on the card after that.  "
                          f"It was:\n{_gpu_death}")


def _fail(message, latch=False):
    global _gpu_death
    if latch and _gpu_death is None:
        _gpu_death = message
    raise LaunchError(message)


def _exit_name(code):
    if code is None:
        return "still running"
    try:
        return f"{code} ({signal.Signals(-code).name})"          # a negative exit code is the signal that ended the process
    except ValueError:
        return str(code)


def _rank_main(target, rank, world_size, args, backend, store, q):
    """(In the spawned rank.)  The frame every worker shares: paths, the process group, the result or the traceback on the queue."""
    sys.path[:0] = [ROOT, TESTS]
    try:
        if backend is not None:
            import torch
            import torch.distributed as dist
            kw = {}
            if backend == "nccl":
                torch.cuda.set_device(0)
                kw["device_id"] = torch.device("cuda:0")
            dist.init_process_group(backend, init_method=f"file://{store}", rank=rank, world_size=world_size, **kw)
        q.put((rank, target(rank, world_size, *args), None))
        if backend is not None:
            dist.barrier()
            dist.destroy_process_group()
    except Exception:
        q.put((rank, None, traceback.format_exc()))
        raise


def run_ranks(target, world_size, *args, timeout, backend=None, gpu=False):
    """Runs the module-level target(rank, world_size, *args) in world_size spawned processes and returns what they returned
    (picklable), in rank order.  With a backend ("gloo" / "nccl") each rank stands inside an initialised process group (file store
    in a temporary directory; nccl: device 0) and leaves it through barrier + destroy_process_group after delivering its result.
    Fails (LaunchError) as soon as a rank raised, exited without a result, or `timeout` seconds have passed; after the last result
    the ranks have 60 s (nccl: 120 s) to exit, and must exit 0.  No rank outlives the call."""
    _obey_latch(gpu)
    ctx = multiprocessing.get_context("spawn")
    grace = 120 if backend == "nccl" else 60
    codes_of = lambda ps: "exit codes by rank " + ", ".join(_exit_name(p.exitcode) for p in ps)
    res, t0 = {}, time.monotonic()
    with tempfile.TemporaryDirectory() as d:
        q = ctx.Queue()
        ps = [ctx.Process(target=_rank_main, args=(target, r, world_size, args, backend, os.path.join(d, "store"), q))
              for r in range(world_size)]
        try:
            [p.start() for p in ps]
            while len(res) < world_size:
                try:
                    rank, out, err = q.get(timeout=POLL)
                except queue.Empty:
                    codes = [p.exitcode for p in ps]
                    if not q.empty():                 # a rank flushes its queue before it exits: what a rank seen dead in `codes`
                        continue                      # had put since the poll is there now, and is read first
                    if any(codes):
                        _fail(f"a rank died: {codes_of(ps)}", latch=gpu and any(c is not None and c < 0 for c in codes))
                    silent = [r for r, c in enumerate(codes) if c == 0 and r not in res]
                    if silent:
                        _fail(f"rank(s) {silent} exited 0 without delivering a result: {codes_of(ps)}")
                    if time.monotonic() - t0 >= timeout:
                        _fail(f"the ranks did not answer in {timeout} s (killed): {codes_of(ps)}", latch=gpu)
                    continue
                if err is not None:
                    _fail(f"rank {rank} raised:\n{err}")
                res[rank] = out
            deadline = time.monotonic() + grace
            [p.join(max(0.0, deadline - time.monotonic())) for p in ps]
            codes = [p.exitcode for p in ps]
            if None in codes:
                _fail(f"a rank was still running {grace} s after the last result (killed): {codes_of(ps)}", latch=gpu)
            if any(codes):
                late = []
                while not q.empty():
                    late.append(q.get()[2])
                _fail(f"a rank failed after delivering its result: {codes_of(ps)}\n" + "\n".join(e for e in late if e),
                      latch=gpu and any(c < 0 for c in codes))
        finally:
            for p in ps:
                if p.is_alive():
                    p.kill()
                if p.pid is not None:
                    p.join()
    return [res[r] for r in range(world_size)]


def run_child(code, *argv, env=None, timeout, gpu=False):
    """One fresh `python -c` child: PRELUDE (os, sys, the repository root and tests/ on sys.path) in front of `code`, `argv` as its
    sys.argv[1:], under os.environ plus `env` (a value of None removes the variable) with OV_ROOT set.  Returns the
    CompletedProcess, output captured as text (and passed on to this process's streams); a non-zero exit fails (LaunchError) with
    the tail of the child's stderr, and so does `timeout`, at which the child is killed."""
    _obey_latch(gpu)
    full = dict(os.environ, OV_ROOT=ROOT)
    for k, v in (env or {}).items():
        if v is None:
            full.pop(k, None)
        else:
            full[k] = v
    try:
        p = subprocess.run([sys.executable, "-c", PRELUDE + code, *argv], env=full, capture_output=True, text=True, timeout=timeout)
    except subprocess.TimeoutExpired as e:
        err = e.stderr.decode(errors="replace") if isinstance(e.stderr, bytes) else e.stderr or ""
        _fail(f"the child was killed at its limit of {timeout} s; its stderr ended:\n{err[-STDERR_TAIL:]}", latch=gpu)
    sys.stdout.write(p.stdout)
    sys.stderr.write(p.stderr)
    if p.returncode != 0:
        _fail(f"the child exited {_exit_name(p.returncode)}; its stderr ended:\n{p.stderr[-STDERR_TAIL:]}", latch=gpu and p.returncode < 0)
    return p
