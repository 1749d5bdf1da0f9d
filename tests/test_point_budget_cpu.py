"""Point budget, without a GPU: the numpy statement of the rule (tests/point_budget_ref.py) against brute force and — with no budget — against
the oracle's selection, which pins its candidate rule before the GPU tests rely on it; the C ABI's and the facade's surface."""
import os
import re
import subprocess

import numpy as np
import pytest

import bpvo_amd
import point_budget_ref as pb
from util import setup_pair

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_FUNCTIONS = ["bpvo_hip_set_point_budget", "bpvo_hip_get_point_budget", "bpvo_hip_seq_set_point_budget", "bpvo_hip_seq_get_point_budget",
                 "bpvo_hip_get_selection_info"]


def _check(s, K):
    pos, t, quota, bound = pb.select(s, K)
    assert list(pos) == pb.brute_force(s, K), (K, list(s))
    n = len(s)
    assert bound == (0 < K < n)
    if bound:
        s = np.asarray(s, np.float32)
        assert len(pos) == K and np.all(np.diff(pos) > 0)
        assert t == np.sort(s)[::-1][K - 1] and quota == K - int((s > t).sum())
        assert np.all(s[pos] >= t) and np.all(np.delete(s, pos) <= t)
    else:
        assert len(pos) == n and t is None and quota == 0


def test_rule_against_brute_force_on_random_inputs():
    rng = np.random.default_rng(7)
    for trial in range(200):
        n = int(rng.integers(1, 120))
        # few distinct values: ties everywhere; many: hardly any
        s = rng.integers(0, int(rng.choice([2, 4, 1000])), n).astype(np.float32) * np.float32(0.125)
        for K in {0, 1, 16, 17, n - 1, n, n + 1, int(rng.integers(1, n + 1))}:
            if K >= 0:
                _check(s, K)


def test_rule_on_hand_made_inputs():
    s = np.array([3, 1, 2, 2, 5, 2, 2, 4], np.float32)
    _check(s, 8)                                              # K >= n: nothing changes
    _check(s, 9)
    _check(s, 7)                                              # K == n - 1: the smallest leaves
    assert list(pb.select(s, 7)[0]) == [0, 2, 3, 4, 5, 6, 7]
    pos, t, quota, _ = pb.select(s, 5)                        # ties straddle the cut: 5, 4, 3 and the FIRST two of the four 2s
    assert list(pos) == [0, 2, 3, 4, 7] and t == 2 and quota == 2
    pos, t, quota, _ = pb.select(s, 3)                        # a clean cut: #{S >= t} == K
    assert list(pos) == [0, 4, 7] and t == 3 and quota == 1
    same = np.full(40, 0.75, np.float32)                      # all saliencies equal: the first K in raster order
    pos, t, quota, _ = pb.select(same, 17)                    # (K no multiple of 16)
    assert list(pos) == list(range(17)) and t == np.float32(0.75) and quota == 17
    _check(same, 17)
    assert list(pb.select(s, 0)[0]) == list(range(8))         # no budget


def test_kept_indices_cut_to_a_multiple_of_16_and_the_capacity():
    S = np.zeros((40, 40), np.float32)
    rng = np.random.default_rng(3)
    S[4:36, 4:36] = rng.integers(1, 5, (32, 32)).astype(np.float32)
    disp = np.ones((40, 40), np.float32)
    r = pb.kept_indices(S, disp, 0, -1, 0.5, 0.001, 512.0, 100)
    assert r["bound"] and len(r["kept"]) == 96 and np.all(np.diff(r["kept"]) > 0)
    full = pb.select(S.reshape(-1)[r["cand"]], 100)[0]
    assert np.array_equal(r["kept"], r["cand"][full][:96])     # the LAST N mod 16 leave
    assert len(pb.kept_indices(S, disp, 0, -1, 0.5, 0.001, 512.0, 100, cap=64)["kept"]) == 64


@pytest.mark.parametrize("descriptor", ["intensity", "bitplanes"])
@pytest.mark.parametrize("rows,cols", [(96, 128), (100, 150)])
def test_without_a_budget_the_rule_is_the_oracles_selection(orc, rows, cols, descriptor):
    """Level 0 with non-maximum suppression, level 1 without (minNumPixelsForNonMaximaSuppression = the level-0 size)."""
    ctx, d, p = setup_pair(orc, rows, cols, descriptor=descriptor, levels=2, minNumPixelsForNonMaximaSuppression=rows * cols)
    for l in range(2):
        S = ctx.get_saliency(0, l)
        r = pb.kept_indices(S, d["dispA"], l, 1 if l == 0 else -1, p.minSaliency, p.minValidDisparity, p.maxValidDisparity, 0,
                            nms_param_radius=p.nonMaxSuppRadius)
        inds = ctx.get_point_indices(0, l)
        assert len(inds) > 0 and np.array_equal(r["kept"], inds), (l, len(r["kept"]), len(inds))
    ctx.close()


def test_without_a_budget_the_rule_is_the_oracles_selection_at_radius_2(orc):
    """nonMaxSuppRadius 2 (the flag path of the device selection): a strict maximum over the 5 x 5 window, at both levels"""
    rows, cols = 100, 150
    ctx, d, p = setup_pair(orc, rows, cols, descriptor="intensity", levels=2, nonMaxSuppRadius=2, minNumPixelsForNonMaximaSuppression=1)
    for l in range(2):
        r = pb.kept_indices(ctx.get_saliency(0, l), d["dispA"], l, 2, p.minSaliency, p.minValidDisparity, p.maxValidDisparity, 0)
        inds = ctx.get_point_indices(0, l)
        assert len(inds) > 0 and np.array_equal(r["kept"], inds), (l, len(r["kept"]), len(inds))
    ctx.close()


def test_header_declares_and_library_exports_the_new_functions():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "bpvo_hip", "c_api.h")).read(), flags=re.S)
    lib = bpvo_amd.load()
    for name in NEW_FUNCTIONS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), f"{name} is not declared in c_api.h"
        assert hasattr(lib.lib, name), f"{name} is not exported"
    # every one of them says it is an extension with no reference member
    doc = open(os.path.join(ROOT, "include", "bpvo_hip", "c_api.h")).read()
    for name in NEW_FUNCTIONS:
        assert re.search(name + r" \(an extension, no reference member", doc), name


def test_facade_point_budget_compiles():
    src = os.path.join(ROOT, "tests", "cpp", "point_budget_compile.cc")
    out = subprocess.run(["g++", "-std=c++11", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"), src], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
