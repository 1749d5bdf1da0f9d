"""The scratch layouts of the semi-global matchers without a GPU.  Each matcher carves its scratch in one function (kernels_sgm.hip sgm_layout,
kernels_sgbm.hip sgbm_layout) and sgm_scratch_bytes / sgbm_scratch_bytes are that function on a null base; SGM's multi-frame launches advance every
pointer by that count, so a wrong total is a silent overlap of two frames' slices.  tests/cpp/sg_layout_harness.cc links the product library (the two
functions are host code) and prints the sizes; the expectations are the hand-summed formulas the two functions were before the layouts, restated here."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def up(v):
    return (v + 255) // 256 * 256


def sgm_bytes(rows, cols, D):
    npix, pitch = rows * cols, cols + 15 - (cols - 1) % 16
    return 2 * up(pitch * rows) + 2 * up(npix * 4) + up(npix * D) + 2 * up(npix * D * 2) + up(8 * npix * D * 2) + 2 * up(npix * 2) + 2 * up(npix * 4)


def sgbm_bytes(rows, cols, min_disp, D):
    npix = rows * cols
    nvol = rows * max(cols - (min_disp + D), 1) * D
    return 2 * up(2 * npix) + up(nvol) + up(nvol * 2) + up(5 * nvol * 2) + 2 * up(npix * 2) + up(npix * 2) + 2 * up(npix * 4)


@pytest.fixture(scope="module")
def sizes(tmp_path_factory):
    import __graft_entry__ as ge
    lib = ge.HIP_LIB if os.path.exists(ge.HIP_LIB) else ge.build_hip()
    exe = str(tmp_path_factory.mktemp("sg_layout") / "sg_layout_harness")
    cmd = [os.environ.get("CXX", "g++"), "-O1", "-std=c++17", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "cpp", "sg_layout_harness.cc"),
           lib, "-Wl,-rpath," + os.path.dirname(lib), "-Wl,-rpath," + os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def run(queries):
        out = subprocess.run([exe, *[str(v) for q in queries for v in q]], capture_output=True, text=True)
        assert out.returncode == 0 and not out.stderr, (out.returncode, out.stderr)
        return [int(l) for l in out.stdout.split()]
    return run


ROWS = (8, 15, 33, 121, 376, 480)
COLS = (8, 17, 32, 33, 40, 160, 161, 640, 1241)      # (cols - 1) % 16: 7, 0, 15, 0, 7, 15, 0, 15, 8
DISPS = (16, 32, 48, 64, 128, 144, 256)


def test_sgm_scratch_bytes_are_the_hand_summed_formula(sizes):
    assert {(c - 1) % 16 for c in COLS} >= {0, 15}
    grid = [(r, c, D) for r in ROWS for c in COLS for D in DISPS]
    got = sizes([("sgm", *q) for q in grid])
    want = [sgm_bytes(*q) for q in grid]
    assert got == want, [(q, g, w) for q, g, w in zip(grid, got, want) if g != w][:8]
    assert all(g % 256 == 0 for g in got)


def test_sgbm_scratch_bytes_are_the_hand_summed_formula(sizes):
    grid = [(r, c, m, D) for r in ROWS for c in COLS for m in (0, 3, 16) for D in DISPS]
    assert any(c - (m + D) <= 0 for _, c, m, D in grid) and any(c - (m + D) == 1 for _, c, m, D in grid)      # no cost column at all; exactly one
    got = sizes([("sgbm", *q) for q in grid])
    want = [sgbm_bytes(*q) for q in grid]
    assert got == want, [(q, g, w) for q, g, w in zip(grid, got, want) if g != w][:8]
    assert all(g % 256 == 0 for g in got)
