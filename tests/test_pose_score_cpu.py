"""Pose scoring without a GPU: the finish (bpvo_amd/csrc/pose_score_math.h) compiled with a plain C++ compiler against the numpy statement
of the score, the record's layout in the header and in the ctypes mirror, and — on the CPU oracle — the scenes the feature exists for: the
identity start ends metres from the truth, the start chosen by the score among six candidates ends at it."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import pose_score_ref as ref
from bpvo_amd import capi
from util import make_params, pose_error

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pose_score") / "pose_score_harness")
    r = subprocess.run(["g++", "-std=c++11", "-O2", "-ffp-contract=off", "-Wall", "-Werror", os.path.join(ROOT, "tests", "cpp", "pose_score_harness.cc"), "-o", exe],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def run(*args):
        out = subprocess.run([exe, *[a if isinstance(a, str) else repr(a) for a in args]], capture_output=True, text=True)
        assert out.returncode == 0, out.stderr
        return out.stdout.strip()
    return run


def test_score_formula_on_the_host(harness):
    """pose_score_value against the numpy statement, every bit: ordinary sums, nothing valid (every point charged tau), everything valid, an
    empty template (score = tau whatever the sums), and a tau that is no f64-exact decimal (it enters as the f32 it is passed as)."""
    cases = [  # cost_sum, n_valid, N, C, tau
        (1234.56789, 700, 1024, 8, 0.5),
        (0.0, 0, 1024, 8, 0.5),
        (0.0, 0, 16, 1, 30.0),
        (3071.999, 1024, 1024, 3, 1.0),
        (0.0, 0, 0, 8, 0.5),
        (5.0, 3, 0, 8, 0.7),
        (98765.4321, 3000, 3856, 1, 0.1),
        (1e-3, 1, 300000, 48, 0.3),
    ]
    for cost, nv, N, Cn, tau in cases:
        got = float.fromhex(harness("score", float(cost).hex(), str(nv), str(N), str(Cn), repr(float(np.float32(tau)))))
        want = ref.score_from_formula(cost, nv, N, Cn, tau)
        assert got == want and np.float64(got).tobytes() == np.float64(want).tobytes(), (cost, nv, N, Cn, tau, got, want)
    assert float.fromhex(harness("score", "0.0", "0", "0", "8", "0.5")) == 0.5                       # N = 0: tau
    assert float.fromhex(harness("score", "0.0", "0", "64", "8", "0.5")) == 0.5                      # nothing valid: every term charged tau
    assert float.fromhex(harness("score", "0.0", "64", "64", "8", "0.5")) == 0.0


def test_argmin_ties_and_nans(harness):
    assert harness("argmin", "0.3", "0.2", "0.25") == "1"
    assert harness("argmin", "0.2", "0.3", "0.2", "0.2") == "0"          # ties: the lowest index
    assert harness("argmin", "0.5", "0.2", "0.2") == "1"
    assert harness("argmin", "nan", "0.4", "0.3") == "2"                 # a NaN never wins ...
    assert harness("argmin", "0.4", "nan", "0.5") == "0"
    assert harness("argmin", "nan", "nan", "7.0") == "2"
    assert harness("argmin", "nan", "nan") == "0"                        # ... unless there is nothing else: the first
    assert harness("argmin", "inf", "1e300") == "1"
    assert harness("argmin", "0.1") == "0"


def test_record_layout_in_header_and_ctypes():
    src = open(os.path.join(ROOT, "include", "bpvo_hip", "c_api.h")).read()
    body = re.search(r"typedef struct bpvo_hip_pose_score \{(.*?)\} bpvo_hip_pose_score;", src, re.S).group(1)
    fields = re.findall(r"\b(double|int)\s+(\w+);", body)
    assert fields == [("double", "cost_sum"), ("double", "score"), ("int", "n_valid"), ("int", "n_below")]
    assert [f[0] for f in capi.PoseScore._fields_] == [n for _, n in fields]
    assert C.sizeof(capi.PoseScore) == 24 and capi.POSE_SCORE.itemsize == 24 and ref.POSE_SCORE == capi.POSE_SCORE
    assert [capi.POSE_SCORE.fields[n][1] for n in ("cost_sum", "score", "n_valid", "n_below")] == [0, 8, 16, 20]
    assert [getattr(capi.PoseScore, n).offset for n in ("cost_sum", "score", "n_valid", "n_below")] == [0, 8, 16, 20]


def test_numpy_reference_on_a_hand_made_case():
    r = np.array([[0.1, -0.7, 0.5, 9.0], [-0.2, 0.3, -0.5, 9.0]], np.float32)      # [C = 2][N = 4]; point 3 invalid
    rec = ref.score_ref(r.reshape(-1), [1, 1, 1, 0], 2, 0.5)
    terms = [np.float32(v) for v in (0.1, 0.5, 0.5, 0.2, 0.3, 0.5)]
    assert rec["n_valid"] == 3 and rec["n_below"] == 3      # 0.1, 0.2, 0.3: |r| = tau is not below
    assert rec["cost_sum"] == float(sum(np.float64(t) for t in terms))
    assert rec["score"] == (rec["cost_sum"] + 0.5 * 2) / 8
    empty = ref.score_ref(np.zeros(0, np.float32), np.zeros(0), 8, 0.5)
    assert (empty["cost_sum"], empty["score"], empty["n_valid"], empty["n_below"]) == (0.0, 0.5, 0, 0)


@pytest.mark.parametrize("descriptor,rows,cols,index,max_trans", ref.FIXTURES)
def test_the_score_picks_the_start_that_rescues_the_estimate(orc, descriptor, rows, cols, index, max_trans):
    """Conditions on the INPUTS of the GPU test, on the oracle: among twist_to_matrix(s * twist), s in SCALES, scored at level 2 the winner is
    s = 0.9; the oracle's estimate from identity ends more than 0.5 m from the truth (measured: 2.2 - 12.4 m), from the winner within 0.05 m
    (measured: 0.0003 - 0.029 m)."""
    d = ref.fixture_pair(rows, cols, index, max_trans)
    p = make_params(orc, descriptor=descriptor, levels=3)
    ctx = orc.create(d["K"], d["b"], rows, cols, p, n_frames=2, n_pairs=1)
    ctx.frame_set_data(0, d["imgA"], d["dispA"])
    ctx.frame_set_template(0)
    ctx.frame_set_data(1, d["imgB"], d["dispB"])
    cands = ref.candidates(d)
    scores = [float(ref.score_by_linearize(ctx, 0, 1, ref.SCORE_LEVEL, T, ref.TAU[descriptor])["score"]) for T in cands]
    order = np.argsort(scores, kind="stable")
    print(descriptor, rows, cols, index, max_trans, "scores", [round(s, 4) for s in scores])
    assert order[0] == ref.WINNER, scores
    T_id, _ = ctx.estimate_pose(0, 0, 1, np.eye(4, dtype=np.float32))
    T_win, _ = ctx.estimate_pose(0, 0, 1, cands[ref.WINNER])
    e_id, e_win = pose_error(T_id, d["T_gt"]), pose_error(T_win, d["T_gt"])
    print("identity start", e_id, "winner start", e_win)
    assert e_id[1] > 0.5, e_id
    assert e_win[1] < 0.05, e_win
    ctx.close()
