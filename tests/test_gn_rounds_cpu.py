"""The pipelined rounds of the four-kernel chain (bpvo_amd/csrc/gn_rounds.h) without a GPU: tests/cpp/gn_rounds_harness.cc includes only that
header, is compiled by the host's C++ compiler — which proves the header free of HIP — and runs the real run_rounds against a fake device that
"finishes" workspace i after a given number of iterations.  An off-by-one in this loop hangs nothing: it costs a round per level, or ends a
level a round early — so the order of the calls, the slots and the counts are asserted here, call by call."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUEUE_ITERATIONS, QUEUE_FLAGS, WAIT, READ = range(4)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("gn_rounds") / "libgn_rounds.so")
    cmd = [os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-fPIC", "-shared",
           "-I", os.path.join(ROOT, "bpvo_amd", "csrc"), "-o", out, os.path.join(ROOT, "tests", "cpp", "gn_rounds_harness.cc")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return C.CDLL(out)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def run_cameras(lib, max_iterations, finish, freeze=None, l2_moot=0, fused_path=1, fail_at=-1):
    finish = np.ascontiguousarray(finish, np.int32)
    freeze = np.ascontiguousarray(finish if freeze is None else freeze, np.int32)
    done = np.zeros(len(finish), np.int32)
    log = np.zeros((4096, 5), np.int32)
    n_log = C.c_int()
    rc = lib.gr_run_cameras(max_iterations, len(finish), _p(finish), _p(freeze), l2_moot, fused_path, fail_at, _p(done), _p(log), log.size, C.byref(n_log))
    assert n_log.value <= len(log)
    return rc, done.tolist(), [tuple(int(v) for v in row) for row in log[:n_log.value]]


def run_rigs(lib, max_iterations, finish):
    finish = np.ascontiguousarray(finish, np.int32)
    done = np.zeros(len(finish), np.int32)
    log = np.zeros((4096, 5), np.int32)
    n_log = C.c_int()
    rc = lib.gr_run_rigs(max_iterations, len(finish), _p(finish), _p(done), _p(log), log.size, C.byref(n_log))
    return rc, done.tolist(), [tuple(int(v) for v in row) for row in log[:n_log.value]]


def check_protocol(lib, log, max_iterations):
    """What holds for every run: rounds 0, 1, 2, ... queued in order, each followed by its flags into slot round % 3; from round 1 on a wait for and a
    read of slot (round - 1) % 3, after the round was queued; no slot marked again before it was read, none waited for unmarked; the round after the
    one whose flags first read zero is the last; never more than max_rounds.  Returns {round: (dispatched, warp, median)}, {round: (count, moving)}."""
    queued, read = {}, {}
    at = 0
    for rnd in range(10 ** 6):
        if at == len(log):
            break
        kind, a, b, c, d = log[at]
        assert (kind, a) == (QUEUE_ITERATIONS, rnd), (at, log[at])
        queued[rnd] = (b, c, d)
        assert log[at + 1][:3] == (QUEUE_FLAGS, rnd % 3, 0), (at, log[at + 1])      # (0: the slot's last flags had been read)
        at += 2
        if rnd == 0:
            continue
        assert log[at][:3] == (WAIT, (rnd - 1) % 3, 1), (at, log[at])
        assert log[at + 1][:2] == (READ, (rnd - 1) % 3), (at, log[at + 1])
        read[rnd - 1] = log[at + 1][2:4]
        at += 2
        if read[rnd - 1][0] == 0:
            assert at == len(log), "the round queued before the zero was read is the last"
    rounds = len(queued)
    assert rounds <= lib.gr_max_rounds(max_iterations)
    zero = [r for r, (count, _) in read.items() if count == 0]
    if zero:
        assert zero == [rounds - 2], "one empty round: the one queued while the first zero was on its way"
    return queued, read


def test_limits(harness):
    """min(max(maxIterations, 0) + 2, maxFuncEvals) linearisations per level, in rounds of kItersPerSync, plus two"""
    lib = harness
    K, cap = lib.gr_iters_per_sync(), lib.gr_max_fun_evals()
    assert (K, cap) == (4, 1200)
    assert [lib.gr_max_linearizations(v) for v in (0, -3, 1, 50, cap - 2, cap - 1, 5000)] == [2, 2, 3, 52, cap, cap, cap]
    assert [lib.gr_max_rounds(v) for v in (0, -3, 2, 3, 50, 5000)] == [3, 3, 3, 4, 15, 302]
    # a workspace that would never finish gets exactly that many linearisations — the device's limit — and the host stops queueing behind it
    for max_it, lin in ((0, 2), (-7, 2), (5, 7), (50, 52), (5000, cap)):
        rc, done, log = run_cameras(lib, max_it, [10 ** 9])
        assert rc == 0 and done == [lin]
        queued, read = check_protocol(lib, log, max_it)
        assert len(queued) == (lin + K - 1) // K + 1 <= lib.gr_max_rounds(max_it)


@pytest.mark.parametrize("finish", [[1], [4], [5], [8], [9, 3, 17], [16, 16], [1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13], [40, 1, 1, 39]])
def test_camera_rounds(harness, finish):
    lib = harness
    rc, done, log = run_cameras(lib, 50, finish)
    assert rc == 0 and done == finish, "every workspace ran until it had finished: no level ended a round early"
    queued, read = check_protocol(lib, log, 50)
    K = lib.gr_iters_per_sync()
    first_zero = (max(finish) + K - 1) // K - 1      # the round in which the last workspace finishes
    assert len(queued) == first_zero + 2 and read[first_zero][0] == 0, "no round beyond the empty one"
    # what a round dispatches: everything in rounds 0 and 1, then the count that came out of the round before the last
    n = len(finish)
    for rnd, (dispatched, _, _) in queued.items():
        assert dispatched == (n if rnd < 2 else read[rnd - 2][0]), (rnd, dispatched)
    for rnd, (count, _) in read.items():
        assert count == sum(f > K * (rnd + 1) for f in finish), (rnd, count)


def test_none_moving_latches(harness):
    """Once no active workspace estimates its scale any more the median is dropped from the rounds queued after that was read, and with the fused
    path warp_residual too — for the rest of the level."""
    lib = harness
    finish, freeze = [30, 22, 9], [6, 11, 2]
    for fused in (1, 0):
        rc, done, log = run_cameras(lib, 50, finish, freeze, fused_path=fused)
        assert rc == 0 and done == finish
        queued, read = check_protocol(lib, log, 50)
        assert [m for _, m in read.values()][:4] == [2, 1, 0, 0]      # after 4, 8, 12, 16 iterations
        # read of round 2 says "none moving": rounds 0 .. 3 were queued with both launches (round 3 before that read), 4 .. without
        for rnd, (_, warp, median) in queued.items():
            assert median == (1 if rnd <= 3 else 0), (rnd, median)
            assert warp == (1 if rnd <= 3 or not fused else 0), (rnd, warp, fused)
    # kL2 with the fused path: moot from the first linearisation
    rc, done, log = run_cameras(lib, 50, finish, freeze, l2_moot=1)
    queued, _ = check_protocol(lib, log, 50)
    assert all(q[1:] == (0, 0) for q in queued.values())


def test_an_error_ends_the_level(harness):
    rc, done, log = run_cameras(harness, 50, [100], fail_at=2)
    assert rc == 7 and log[-1][:2] == (QUEUE_FLAGS, 2) and sum(r[0] == QUEUE_ITERATIONS for r in log) == 3


@pytest.mark.parametrize("finish", [[6], [3, 14], [14, 3], [1, 1, 30], [8, 8, 8]])
def test_rig_rounds(harness, finish):
    """any body still active keeps every rig going (a finished rig idles); the level ends one empty round after all have finished"""
    lib = harness
    rc, done, log = run_rigs(lib, 50, finish)
    assert rc == 0 and done == finish
    queued, read = check_protocol(lib, log, 50)
    K = lib.gr_iters_per_sync()
    assert all(q == (len(finish), 1, 1) for q in queued.values())
    assert len(queued) == (max(finish) + K - 1) // K + 1
    for rnd, (left, _) in read.items():
        assert left == sum(f > K * (rnd + 1) for f in finish), (rnd, left)
