"""CPU: the tests' process launcher (tests/ranks.py) on children that import no torch and touch no device -- results in rank order,
every way a rank can die noticed long before the time limit and named in the failure, nothing left running, the `python -c` child,
and the latch that stops GPU launches after a GPU process died by a signal."""
import multiprocessing
import os
import signal
import time

import pytest

import ranks

LIMIT = 120           # the death cases pass this time limit ...
NOTICED = 10          # ... and must fail within this many seconds: the death was noticed, not the limit waited for


def _square(rank, world_size, base):
    return (rank, world_size, (base + rank) ** 2)


def _exit_7(rank, world_size):
    if rank == 1:
        os._exit(7)
    time.sleep(60)


def _kill_self(rank, world_size):
    if rank == 0:
        os.kill(os.getpid(), signal.SIGKILL)
    time.sleep(60)


def _raise(rank, world_size):
    if rank == 1:
        raise ValueError("the payload of rank one went wrong")
    time.sleep(60)


def _exit_0_silently(rank, world_size):
    if rank == 1:
        os._exit(0)
    time.sleep(60)


def _sleep(rank, world_size):
    time.sleep(60)


def _touch(rank, world_size, path):
    open(path, "w").close()
    return rank


def fails(target, *args, timeout=LIMIT, within=NOTICED, **kw):
    """The LaunchError's text of a call that must fail within `within` seconds and leave no child of this process alive."""
    t0 = time.monotonic()
    with pytest.raises(ranks.LaunchError) as e:
        ranks.run_ranks(target, 2, *args, timeout=timeout, **kw)
    took = time.monotonic() - t0
    print(f"{target.__name__}: failed after {took:.2f} s: {str(e.value).splitlines()[0]}")
    assert took < within, took
    assert multiprocessing.active_children() == []
    return str(e.value)


def test_clean_world_returns_results_in_rank_order():
    assert ranks.run_ranks(_square, 2, 3, timeout=LIMIT) == [(0, 2, 9), (1, 2, 16)]
    assert multiprocessing.active_children() == []


def test_exit_code_of_a_dead_rank_is_named():
    text = fails(_exit_7)
    assert "a rank died" in text and "still running, 7" in text


def test_signal_of_a_killed_rank_is_named():
    text = fails(_kill_self)
    assert "-9 (SIGKILL), still running" in text


def test_traceback_of_a_raising_rank_is_in_the_message():
    text = fails(_raise)
    assert "rank 1 raised" in text and "Traceback (most recent call last)" in text
    assert 'raise ValueError("the payload of rank one went wrong")' in text and "in _raise" in text


def test_rank_that_exits_0_without_a_result_fails():
    text = fails(_exit_0_silently)
    assert "rank(s) [1] exited 0 without delivering a result" in text


def test_time_limit_fails_and_says_so():
    text = fails(_sleep, timeout=3)
    assert "did not answer in 3 s" in text and "still running, still running" in text


def test_child_gets_argv_and_environment_and_returns_its_output():
    p = ranks.run_child("print(sys.argv[1:], os.environ['OV_RANKS_TEST'], 'HOME' in os.environ, os.environ['OV_ROOT'])",
                        "a", "b c", env={"OV_RANKS_TEST": "seen", "HOME": None}, timeout=LIMIT)
    assert p.returncode == 0 and p.stdout.split("\n")[0] == f"['a', 'b c'] seen False {ranks.ROOT}"
    p = ranks.run_child("print(sys.path[:2])", timeout=LIMIT)                                   # the shared prelude's two paths
    assert p.stdout.strip() == str([ranks.ROOT, ranks.TESTS])


def test_failing_child_fails_with_its_stderr():
    with pytest.raises(ranks.LaunchError) as e:
        ranks.run_child("print('the reason, on stderr', file=sys.stderr); sys.exit(3)", timeout=LIMIT)
    assert "exited 3" in str(e.value) and "the reason, on stderr" in str(e.value)
    with pytest.raises(ranks.LaunchError) as e:
        ranks.run_child("import time; print('started', file=sys.stderr, flush=True); time.sleep(60)", timeout=2)
    assert "killed at its limit of 2 s" in str(e.value) and "started" in str(e.value)


def test_latch_refuses_gpu_launches_after_a_signal_death(tmp_path):
    """The children touch no device; gpu=True only marks them.  A non-zero exit does not latch, a signal or a time limit does:
    then a gpu=True launch of either kind is refused before a process exists, a gpu=False one still runs, and reset() lifts it."""
    marker = str(tmp_path / "started")
    die = "os.kill(os.getpid(), 9)"
    try:
        with pytest.raises(ranks.LaunchError):
            ranks.run_child("sys.exit(3)", timeout=LIMIT, gpu=True)                                    # no signal: does not latch
        with pytest.raises(ranks.LaunchError, match="SIGKILL"):
            ranks.run_child(die, timeout=LIMIT)                                                        # gpu=False does not set it
        assert ranks.run_ranks(_touch, 1, marker, timeout=LIMIT, gpu=True) == [0] and os.path.exists(marker)
        os.remove(marker)
        fails(_kill_self, gpu=True)
        for launch in (lambda: ranks.run_ranks(_touch, 1, marker, timeout=LIMIT, gpu=True),
                       lambda: ranks.run_child("open(sys.argv[1], 'w').close()", marker, timeout=LIMIT, gpu=True)):
            t0 = time.monotonic()
            with pytest.raises(ranks.LaunchError) as e:
                launch()
            assert "not started" in str(e.value) and "-9 (SIGKILL)" in str(e.value)                    # quotes the earlier death
            assert time.monotonic() - t0 < 0.1 and not os.path.exists(marker)
        assert ranks.run_ranks(_square, 2, 0, timeout=LIMIT) == [(0, 2, 0), (1, 2, 1)]                # gpu=False does not obey it
        ranks.reset()
        with pytest.raises(ranks.LaunchError, match="SIGKILL"):
            ranks.run_child(die, timeout=LIMIT, gpu=True)                                              # a child latches too
        with pytest.raises(ranks.LaunchError, match="not started"):
            ranks.run_ranks(_touch, 1, marker, timeout=LIMIT, gpu=True)
        ranks.reset()
        with pytest.raises(ranks.LaunchError, match="did not answer in 1 s"):
            ranks.run_ranks(_sleep, 1, timeout=1, gpu=True)                                            # and so does a time limit
        with pytest.raises(ranks.LaunchError, match="not started"):
            ranks.run_child("open(sys.argv[1], 'w').close()", marker, timeout=LIMIT, gpu=True)
        ranks.reset()
        assert ranks.run_ranks(_touch, 1, marker, timeout=LIMIT, gpu=True) == [0] and os.path.exists(marker)
    finally:
        ranks.reset()
