"""The frame stage's decisions (bpvo_amd/csrc/frame_plan.h) without a GPU: tests/cpp/frame_plan_harness.cc includes only that header and the C API, is
compiled by the host's C++ compiler — which proves the header free of HIP — and prints the plans for the inputs of its command line.  The
expectations are written out here, as the frame stage stood before its decisions moved into the header: which descriptor kernels the parameters
ask for, which levels share a launch, and — what no GPU test can see — on which stream each normalisation launch runs, which events become
nrm_pending / nrm_pending_finest and which one the stage joins.  The same queries run once more under -fsanitize=address,undefined."""
import os
import subprocess

import pytest

from bpvo_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


@pytest.fixture(scope="module", params=["plain", "sanitizers"])
def plan(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("frame_plan") / "frame_plan_harness")
    cmd = [os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-Wall", "-Werror", *(SANITIZE if request.param == "sanitizers" else []),
           "-I", os.path.join(ROOT, "bpvo_amd", "csrc"), "-I", os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tests", "cpp", "frame_plan_harness.cc")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def run(queries):
        args = []
        for q in queries:
            args += [str(v) for v in q] + [","]
        out = subprocess.run([exe, *args], capture_output=True, text=True)
        assert out.returncode == 0 and not out.stderr, (out.returncode, out.stderr)
        lines = [l.strip() for l in out.stdout.splitlines()]
        assert len(lines) == len(queries)
        return lines
    return run


# the descriptors that are told apart by name or channel count alone, with the channel counts each can have
BY_NAME = [
    (capi.DESC_INTENSITY, (1,), "intensity"),
    (capi.DESC_LAPLACIAN, (1,), "laplacian"),
    (capi.DESC_GRADIENT, (3,), "gradient"),
    (capi.DESC_FIELDS1, (5,), "fields_1st"),
    (capi.DESC_FIELDS2, (10,), "fields_2nd"),
    (capi.DESC_CENTRAL_DIFFERENCE, (8, 24, 48, 80, 120, 168, 224, 288, 360), "central_difference"),
    (capi.DESC_LATCH, (8, 16, 32, 64, 128, 256, 512), "latch"),
]
# bit-planes: (sigmaPriorToCensusTransform, sigmaBitPlanes) -> the census fused into the blur unless it is taken of the smoothed image or the planes stay unsmoothed
BITPLANES = {
    (-1.0, -1.0): "bitplanes_unsmoothed", (0.0, -1.0): "bitplanes_unsmoothed", (0.75, -1.0): "bitplanes_unsmoothed",
    (-1.0, 0.0): "bitplanes_unsmoothed", (0.0, 0.0): "bitplanes_unsmoothed", (0.75, 0.0): "bitplanes_unsmoothed",
    (-1.0, 1.6): "bitplanes_fused", (0.0, 1.6): "bitplanes_fused", (0.75, 1.6): "bitplanes_smoothed_census",
}
FORMS = ["bitplanes_fused", "bitplanes_smoothed_census", "bitplanes_unsmoothed", "intensity", "laplacian", "gradient", "fields_1st", "fields_2nd",
         "central_difference", "latch"]


def test_descriptor_form(plan):
    queries, want = [], []
    for sigmas, form in BITPLANES.items():
        queries.append(("form", capi.DESC_BITPLANES, *sigmas, 8))
        want.append(form)
        for desc, channels, name in BY_NAME:
            for C in channels:
                queries.append(("form", desc, *sigmas, C))
                want.append(name)
    assert plan(queries) == want


def test_spans(plan):
    assert plan([("spans", 3, 0, 1), ("spans", 3, 0, 0), ("spans", 4, 1, 1), ("spans", 4, 1, 0), ("spans", 1, 0, 1), ("spans", 1, 0, 0)]) == \
        ["0:3", "2:1 1:1 0:1", "1:3", "3:1 2:1 1:1", "0:1", "0:1"]
    queries, want = [], []
    for L in range(1, 6):
        for lo in range(L):
            queries += [("spans", L, lo, 1), ("spans", L, lo, 0)]
            want += [f"{lo}:{L - lo}", " ".join(f"{l}:1" for l in range(L - 1, lo - 1, -1))]      # one span, or singles with the coarsest first
    assert plan(queries) == want


def test_merge_predicates(plan):
    """descriptor: the two blurred bit-planes forms and intensity only; selection: only if every level is tiled; template build: always — each for
    at most levels_in_one_launch_max_frames frames and more than one tested level"""
    queries, want = [], []
    for count in (1, 8, 9):
        for max_frames in (0, 8):
            for tested in (1, 2, 4):
                few = count <= max_frames and tested > 1
                for form in FORMS:
                    for tiled in (0, 1):
                        queries.append(("merge", count, max_frames, tested, form, tiled))
                        descriptor = few and form in ("bitplanes_fused", "bitplanes_smoothed_census", "intensity")
                        want.append(f"{int(descriptor)} {int(few and tiled == 1)} {int(few)}")
    got = plan(queries)
    assert got == want
    # ... and row by row: (count, max_frames, tested levels, form, every level tiled) -> descriptor, selection, template build in one launch
    rows = [
        ((1, 8, 3, "bitplanes_fused", 1), "1 1 1"), ((1, 8, 3, "bitplanes_fused", 0), "1 0 1"), ((8, 8, 3, "bitplanes_fused", 1), "1 1 1"),
        ((9, 8, 3, "bitplanes_fused", 1), "0 0 0"), ((1, 0, 3, "bitplanes_fused", 1), "0 0 0"), ((1, 8, 1, "bitplanes_fused", 1), "0 0 0"),
        ((4, 8, 2, "bitplanes_smoothed_census", 1), "1 1 1"), ((4, 8, 2, "bitplanes_smoothed_census", 0), "1 0 1"), ((9, 8, 2, "bitplanes_smoothed_census", 1), "0 0 0"),
        ((1, 8, 3, "intensity", 1), "1 1 1"), ((8, 8, 3, "intensity", 0), "1 0 1"), ((9, 8, 3, "intensity", 1), "0 0 0"), ((1, 0, 3, "intensity", 1), "0 0 0"),
        ((1, 8, 1, "intensity", 1), "0 0 0"),
        ((2, 8, 2, "bitplanes_unsmoothed", 1), "0 1 1"), ((2, 8, 2, "bitplanes_unsmoothed", 0), "0 0 1"), ((2, 8, 2, "laplacian", 1), "0 1 1"),
        ((2, 8, 2, "gradient", 1), "0 1 1"), ((2, 8, 2, "fields_1st", 1), "0 1 1"), ((2, 8, 2, "fields_2nd", 0), "0 0 1"),
        ((2, 8, 2, "central_difference", 1), "0 1 1"), ((2, 8, 2, "latch", 1), "0 1 1"), ((2, 8, 2, "latch", 0), "0 0 1"),
        ((9, 8, 4, "latch", 1), "0 0 0"), ((8, 8, 1, "gradient", 1), "0 0 0"), ((12, 0, 3, "central_difference", 0), "0 0 0"),
    ]
    assert plan([("merge", *q) for q, _ in rows]) == [w for _, w in rows]


# (side, defer, dense) -> the plan at maxTestLevel 0 by the number of tested levels: launches `first-end:stream:event` in order, then the events
INLINE = {T: f"0-{T}:inline:-1 | join -1 pending -1 finest -1 behind 1" for T in (1, 2, 3, 4)}
JOINED = {T: f"0-{T}:side:1 | join 1 pending -1 finest -1 behind 0" for T in (1, 2, 3, 4)}
NRM = {
    (0, 0, 0): INLINE, (0, 0, 1): INLINE, (0, 1, 0): INLINE, (0, 1, 1): INLINE,
    (1, 0, 0): JOINED, (1, 0, 1): JOINED,
    (1, 1, 0): {1: JOINED[1],
                2: "1-2:side:1 0-1:side:2 | join 1 pending 2 finest -1 behind 0",
                3: "2-3:side:1 0-2:side:2 | join 1 pending 2 finest -1 behind 0",
                4: "3-4:side:1 0-3:side:2 | join 1 pending 2 finest -1 behind 0"},
    (1, 1, 1): {1: JOINED[1],
                2: "0-1:side2:3 1-2:side:1 | join 1 pending -1 finest 3 behind 0",
                3: "0-1:side2:3 2-3:side:1 1-2:side:2 | join 1 pending 2 finest 3 behind 0",
                4: "0-1:side2:3 3-4:side:1 1-3:side:2 | join 1 pending 2 finest 3 behind 0"},
}


def test_normalization_plan(plan):
    queries, want = [], []
    for (side, defer, dense), by_levels in NRM.items():
        for tested, line in by_levels.items():
            queries.append(("nrm", tested, 0, side, defer, dense))
            want.append(line)
    assert plan(queries) == want
    # ... and above a maxTestLevel of 1 the same plans, a level up
    assert plan([("nrm", 4, 1, 0, 1, 1), ("nrm", 4, 1, 1, 0, 0), ("nrm", 4, 1, 1, 1, 0), ("nrm", 4, 1, 1, 1, 1), ("nrm", 3, 1, 1, 1, 1), ("nrm", 2, 1, 1, 1, 1)]) == [
        "1-4:inline:-1 | join -1 pending -1 finest -1 behind 1",
        "1-4:side:1 | join 1 pending -1 finest -1 behind 0",
        "3-4:side:1 1-3:side:2 | join 1 pending 2 finest -1 behind 0",
        "1-2:side2:3 3-4:side:1 2-3:side:2 | join 1 pending 2 finest 3 behind 0",
        "1-2:side2:3 2-3:side:1 | join 1 pending -1 finest 3 behind 0",
        "1-2:side:1 | join 1 pending -1 finest -1 behind 0"]
