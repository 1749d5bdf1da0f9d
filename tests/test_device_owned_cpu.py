"""The owners of device buffers, pinned buffers, streams and events (bpvo_amd/csrc/device_owned.h) without a GPU:
tests/cpp/device_owned_harness.cc includes only that header, is compiled by the host's C++ compiler — which proves the header free of HIP — and
runs the owners over a fake runtime that hands out malloc blocks, counts what is live per kind, logs every call and fails the k-th acquisition on
request.  Every case runs once plain and once under -fsanitize=address,undefined, where a double release, a use after release or a leak ends the
program: the harness is run directly, nothing is preloaded."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]

# scope          alloc / create, use through the implicit conversions, scope exit; reset twice
# reserve_keeps  reserve of at most size(): same pointer, no call into the runtime
# reserve_grows  reserve of more: the old block is released BEFORE the new one is acquired (the fake's call log)
# reserve_fails  a failed reserve leaves size() == 0 and a null pointer, the next reserve succeeds; failed alloc / create leave the owner empty
# zero           n == 0 succeeds, leaves the buffer empty and calls nothing
# moves          move construction, move assignment onto a full owner, self-move-assignment, for buffers, streams and events
# vector         a std::vector of a struct of one owner of each kind, grown from 1 to 100 elements, then erased from the front
# build_fails    a function acquiring one owner of each kind in turn, the k-th acquisition failing, for every k: nothing live after it
CASES = ["scope", "reserve_keeps", "reserve_grows", "reserve_fails", "zero", "moves", "vector", "build_fails"]


@pytest.fixture(scope="module", params=["plain", "sanitizers"])
def harness(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("device_owned") / "device_owned_harness")
    cmd = [os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-Wall", "-Werror", *(SANITIZE if request.param == "sanitizers" else []),
           "-I", os.path.join(ROOT, "bpvo_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "cpp", "device_owned_harness.cc")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def run(case):
        out = subprocess.run([exe, case], capture_output=True, text=True)
        assert out.returncode == 0 and not out.stderr, (case, out.returncode, out.stderr)
        return out.stdout
    return run


def test_cases_listed(harness):
    assert harness("list").split() == CASES


@pytest.mark.parametrize("case", CASES)
def test_case(harness, case):
    assert harness(case) == f"ok {case}\n"
