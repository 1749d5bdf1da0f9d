"""The pose score (include/bpvo_hip/c_api.h, bpvo_hip_score_poses) restated in numpy from residuals and valid flags, and the scenes on which
a start chosen by it rescues the estimate (measured on the CPU oracle: plane scene, 3 pyramid levels, Tukey, score at level 2).

  n_valid  = #{i : valid_i}
  n_below  = #{(i, c) : valid_i and |r[i][c]| < tau}
  cost_sum = sum over valid i and all c of min(|r[i][c]|, tau): every term an f32 converted to f64, summed exactly (math.fsum)
  score    = (cost_sum + tau C (N - n_valid)) / (C N);  N = 0: tau

Used by tests/test_pose_score_cpu.py (the fixtures on the oracle) and tests/test_gpu_pose_score.py (the device against this)."""
import math

import numpy as np

from bpvo_amd import synth

POSE_SCORE = np.dtype([("cost_sum", np.float64), ("score", np.float64), ("n_valid", np.int32), ("n_below", np.int32)])

# tau in descriptor units
TAU = {"bitplanes": 0.5, "intensity": 30.0}
# the candidate starts: twist_to_matrix(s * twist) of the pair's true twist
SCALES = (0.0, 0.5, 0.9, -1.0, 1.5, 2.0)
WINNER = SCALES.index(0.9)
SCORE_LEVEL = 2
# (descriptor, rows, cols, index, max_trans): the identity start ends 2.2 - 12.4 m from the truth, the start at the winner within 0.03 m
FIXTURES = [
    ("bitplanes", 120, 160, 1, 1.0),
    ("bitplanes", 120, 160, 0, 2.0),
    ("bitplanes", 120, 160, 3, 2.0),
    ("bitplanes", 120, 160, 1, 2.0),
    ("intensity", 120, 160, 1, 2.0),
    ("intensity", 240, 320, 0, 2.0),
    ("intensity", 240, 320, 1, 1.0),
    ("intensity", 240, 320, 3, 2.0),
]


def score_from_formula(cost_sum, n_valid, N, C, tau):
    """The score from the sums: tau as the f32 it is passed as, the two integer products exact, then one product, one sum, one quotient in f64."""
    tau = float(np.float32(tau))
    if N <= 0:
        return tau
    return (float(cost_sum) + tau * float(C * (N - int(n_valid)))) / float(C * N)


def score_ref(r, valid, C, tau):
    """One POSE_SCORE record from get_residuals' [C * N] f32 (channel-major) and get_valid's [N]."""
    tau32 = np.float32(tau)
    valid = np.asarray(valid).astype(bool)
    N = valid.shape[0]
    out = np.zeros((), POSE_SCORE)
    if N == 0:
        out["score"] = float(tau32)
        return out
    a = np.abs(np.asarray(r, np.float32).reshape(C, N)[:, valid])
    terms = np.minimum(a, tau32).astype(np.float64)
    out["cost_sum"] = math.fsum(terms.ravel().tolist())
    out["n_valid"] = int(valid.sum())
    out["n_below"] = int(np.count_nonzero(a < tau32))
    out["score"] = score_from_formula(out["cost_sum"], out["n_valid"], N, C, tau32)
    return out


def score_by_linearize(ctx, ref, cur, level, T, tau, ws=0):
    """The record from a context's OWN linearisation at T (any binding: the oracle, or the library's bpvo_hip_linearize): what the score is
    defined by."""
    ctx.linearize(ws, ref, cur, level, T, reset_scale=True)
    return score_ref(ctx.get_residuals(ws), ctx.get_valid(ws), ctx.Cn, tau)


def cost_sum_bound(rec, C):
    """|cost_sum - exact| allowed: n_terms * 2^-52 relative — an f64 sum of n non-negative terms in ANY order is within (n - 1) * 2^-53 of the
    exact sum, relative; a factor 2 of slack."""
    return int(rec["n_valid"]) * C * 2.0 ** -52 * float(rec["cost_sum"])


def candidates(d):
    return np.stack([synth.twist_to_matrix(s * d["twist"]).astype(np.float32) for s in SCALES])


def fixture_pair(rows, cols, index, max_trans):
    return synth.make_pair(rows, cols, index, max_rot=0.03, max_trans=max_trans)
