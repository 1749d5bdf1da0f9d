"""The pose-scoring surface of the C++ facade (include/bpvo_hip/vo.hpp: VisualOdometryPoseEstimator::scorePoses / estimatePoseFromBest) on the
GPU: tests/cpp/pose_score_facade.cc, compiled against the library and run on one of the fixture pairs, must give what the ctypes binding gets
through the same C ABI, bit for bit."""
import os
import subprocess

import numpy as np
import pytest

import pose_score_ref as ref
from bpvo_amd import capi
from util import bits_equal, make_params

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_score_poses_and_estimate_from_best_through_the_facade(hip, tmp_path):
    descriptor, rows, cols, index, max_trans = ref.FIXTURES[0]
    d = ref.fixture_pair(rows, cols, index, max_trans)
    cands = ref.candidates(d)
    for name in ("imgA", "dispA", "imgB", "dispB"):
        np.ascontiguousarray(d[name], np.uint8 if name.startswith("img") else np.float32).tofile(tmp_path / (name + (".u8" if name.startswith("img") else ".f32")))
    cands.tofile(tmp_path / "candidates.f32")
    exe = str(tmp_path / "pose_score_facade")
    csrc = os.path.join(ROOT, "bpvo_amd", "csrc")
    r = subprocess.run(["g++", "-std=c++11", "-O2", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "pose_score_facade.cc"),
                        "-o", exe, "-L", csrc, "-lbpvo_hip", f"-Wl,-rpath,{csrc}"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    K = d["K"]
    tau = ref.TAU[descriptor]
    r = subprocess.run([exe, str(tmp_path), str(rows), str(cols), repr(float(K[0, 0])), repr(float(K[1, 1])), repr(float(K[0, 2])), repr(float(K[1, 2])),
                        repr(float(d["b"])), str(len(cands)), repr(tau), str(ref.SCORE_LEVEL), descriptor], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    scores_cpp = np.fromfile(tmp_path / "scores.bin", capi.POSE_SCORE)
    best = np.fromfile(tmp_path / "best.bin", np.uint8)
    chosen_cpp = int(best[:4].view(np.float32)[0])
    T_cpp = best[4:68].view(np.float32).reshape(4, 4)
    again = best[68:].view(np.float64).reshape(-1, 4)

    p = make_params(hip, descriptor=descriptor, levels=3)
    ctx = hip.create(K, d["b"], rows, cols, p, n_frames=2, n_pairs=1)
    ctx.frame_set_data(0, d["imgA"], d["dispA"])
    ctx.frame_set_template(0)
    ctx.frame_set_data(1, d["imgB"], d["dispB"])
    scores = ctx.score_poses(0, 1, ref.SCORE_LEVEL, cands, tau)
    T, stats, chosen, _ = ctx.estimate_pose_best_start(0, 0, 1, cands, tau, score_level=ref.SCORE_LEVEL)
    assert scores_cpp.shape == scores.shape and scores_cpp.tobytes() == scores.tobytes()
    assert chosen_cpp == chosen == ref.WINNER
    assert bits_equal(T_cpp, T)
    assert np.array_equal(again[:, 0], scores["cost_sum"]) and np.array_equal(again[:, 1], scores["score"])
    assert np.array_equal(again[:, 2], scores["n_valid"]) and np.array_equal(again[:, 3], scores["n_below"])
    assert r.stdout.split() == ["iterations"] + [str(s["numIterations"]) for s in stats]
    ctx.close()
