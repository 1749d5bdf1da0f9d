"""The start policy (include/bpvo_hip/c_api.h, bpvo_amd/csrc/vo_state.h: "where an estimate starts") restated in numpy, and the scenarios its
tests run on.

The rule.  A call of an addFrame driver makes up to two estimates: which = 0 against the key frame the call began with, base B = T_kf; which = 1
against the new key frame, base B = Identity.  M is the pose of the body's last Result.  A candidate c starts the estimate at m44_mul(c, B) — the
host's f32 product with index-order sums —; for which = 1 it is c itself, and the candidate Identity is B itself.
  mode 0: Identity;  mode 1: the first pending hint, else M;  mode 2: Identity (kind 0), M (kind 1), m44_mul(M, M) (kind 2), the hints (kind 3),
  the lowest score wins, ties go to the first, a NaN never wins.
A rig scores member p at rig_member_pose(X_p, candidate) and pools (sum cost_sum_p + tau sum C (N_p - n_valid_p)) / sum C N_p in f64, member order.

Scenario S: the plane scene, 120x160, under a camera that accelerates sideways — translation steps 0.3 .. 2.2 m along DIRECTION plus the rotation
step ROT every frame, 8 frames, default key-framing.  Every frame becomes a key frame (the steps exceed minTranslationMagToKeyFrame) and none has
a previous frame that was none, so no re-estimate runs: the one estimate of frame k (which = 0) is against frame k - 1 with T_kf = Identity.
Scenario Q: the same with steps of 0.05 m, 6 frames, key-framing switched off (both motion thresholds 1e3, maxFractionOfGoodPointsToKeyFrame 0), so
that T_kf accumulates.

Scenario R: steps 0.04, 0.04, 0.9, 0.04, 1.3 m under default key-framing — two frames that are no key frames, a key frame with a previous frame
(the re-estimate, which = 1, runs), a key frame behind it whose T_kf is not the Identity, and one more: every branch of the state machine.

Used by tests/test_start_policy_cpu.py (the rule against vo_state.h; the scenarios' conditions on the oracle) and tests/test_gpu_start_policy.py."""
import functools

import numpy as np

from bpvo_amd import synth

ROWS, COLS, LEVELS = 120, 160, 3
DIRECTION = np.array([0.9, 0.3, 0.3]) / np.linalg.norm([0.9, 0.3, 0.3])
ROT = (0.004, -0.006, 0.003)
S_STEPS = (0.3, 0.7, 1.1, 1.5, 1.9, 2.2, 2.2)
Q_STEPS = (0.05,) * 5
R_STEPS = (0.04, 0.04, 0.9, 0.04, 1.3)
Q_PARAMS = dict(minTranslationMagToKeyFrame=1e3, minRotationMagToKeyFrame=1e3, maxFractionOfGoodPointsToKeyFrame=0.0)
# the frames of S on which the reference's start fails (the oracle: 5.8 - 9.3 m off) and a start at the last motion does not (<= 0.034 m)
S_HARD = (4, 5, 6, 7)
TAU = {"bitplanes": 0.5, "intensity": 30.0}
SCORE_LEVEL = 2
MODE_KEYFRAME_POSE, MODE_CONSTANT_VELOCITY, MODE_SCORED = 0, 1, 2
KIND_IDENTITY, KIND_LAST_MOTION, KIND_LAST_MOTION_TWICE, KIND_HINT = 0, 1, 2, 3
MAX_HINTS = 13


@functools.lru_cache(maxsize=None)
def scenario_S(index=0):
    return synth.make_sequence_steps(ROWS, COLS, S_STEPS, DIRECTION, ROT, index)


@functools.lru_cache(maxsize=None)
def scenario_Q(index=0):
    return synth.make_sequence_steps(ROWS, COLS, Q_STEPS, DIRECTION, ROT, index)


@functools.lru_cache(maxsize=None)
def scenario_R(index=0):
    return synth.make_sequence_steps(ROWS, COLS, R_STEPS, DIRECTION, ROT, index)


@functools.lru_cache(maxsize=None)
def scenario_S_rig(extrinsics_key):
    X = [np.array(x, np.float64).reshape(4, 4) for x in extrinsics_key]
    return synth.make_sequence_steps(ROWS, COLS, S_STEPS, DIRECTION, ROT, 0, extrinsics=X)


def true_motion(seq, k):
    """The frame-to-frame motion of frame k in Result.pose's convention: X_k = pose X_{k-1}."""
    return seq["poses"][k] @ np.linalg.inv(seq["poses"][k - 1])


def translation_error(T, T_true):
    return float(np.linalg.norm(np.asarray(T, np.float64)[:3, 3] - np.asarray(T_true, np.float64)[:3, 3]))


def m44_mul(a, b):
    """device_math.h m44_mul: f32, ((a0 b0 + a1 b1) + a2 b2) + a3 b3 per entry."""
    a = np.asarray(a, np.float32).reshape(4, 4)
    b = np.asarray(b, np.float32).reshape(4, 4)
    r = np.empty((4, 4), np.float32)
    for i in range(4):
        for j in range(4):
            s = np.float32(a[i, 0] * b[0, j])
            s = np.float32(s + np.float32(a[i, 1] * b[1, j]))
            s = np.float32(s + np.float32(a[i, 2] * b[2, j]))
            s = np.float32(s + np.float32(a[i, 3] * b[3, j]))
            r[i, j] = s
    return r


def candidates(mode, which, T_kf, M, hints=()):
    """(poses f32 [n, 4, 4], kinds [n]) of estimate `which` of a body with T_kf, last motion M and the pending hints."""
    I = np.eye(4, dtype=np.float32)
    B = np.asarray(T_kf, np.float32).reshape(4, 4) if which == 0 else I
    M = np.asarray(M, np.float32).reshape(4, 4)
    hints = [np.asarray(h, np.float32).reshape(4, 4) for h in hints]
    if mode == MODE_KEYFRAME_POSE:
        listed = [(KIND_IDENTITY, None)]
    elif mode == MODE_CONSTANT_VELOCITY:
        listed = [(KIND_HINT, hints[0])] if hints else [(KIND_LAST_MOTION, M)]
    else:
        listed = [(KIND_IDENTITY, None), (KIND_LAST_MOTION, M), (KIND_LAST_MOTION_TWICE, m44_mul(M, M))] + [(KIND_HINT, h) for h in hints]
    poses = [B.copy() if kind == KIND_IDENTITY else (m44_mul(c, B) if which == 0 else c.copy()) for kind, c in listed]
    return np.stack(poses).astype(np.float32), [kind for kind, _ in listed]


def argmin(scores):
    """pose_score_argmin: the lowest score, ties to the lowest index, a NaN never wins; all NaN: 0."""
    best = -1
    for i, s in enumerate(scores):
        if s != s:
            continue
        if best < 0 or s < scores[best]:
            best = i
    return max(best, 0)


def pooled_record(records, n_points, C, tau):
    """A rig's record of one body candidate from its members' records of it (dicts or POSE_SCORE records) and their templates' point counts:
    (cost_sum, score, n_valid, n_below); one member: its own record."""
    if len(records) == 1:
        r = records[0]
        return float(r["cost_sum"]), float(r["score"]), int(r["n_valid"]), int(r["n_below"])
    tau = float(np.float32(tau))
    cost, charged, terms, nv, nb = 0.0, 0.0, 0.0, 0, 0
    for r, N in zip(records, n_points):
        cost += float(r["cost_sum"])
        nv += int(r["n_valid"])
        nb += int(r["n_below"])
        charged += float(C * (int(N) - int(r["n_valid"])))
        terms += float(C * int(N))
    score = (cost + tau * charged) / terms if terms > 0 else tau
    return cost, score, nv, nb


def _inverse_at(X, r, c):
    if r == 3:
        return 1.0 if c == 3 else 0.0
    if c < 3:
        return float(X[c, r])
    v = float(X[0, r]) * float(X[0, 3])
    v += float(X[1, r]) * float(X[1, 3])
    v += float(X[2, r]) * float(X[2, 3])
    return -v


def rig_member_pose(X, T):
    """rig_math.h rig_member_pose: X T X^-1 as I + X (T - I) X^-1, f64 sums in index order from the f32 inputs, narrowed to f32."""
    X = np.asarray(X, np.float32).reshape(4, 4)
    T = np.asarray(T, np.float32).reshape(4, 4)
    out = np.empty((4, 4), np.float32)
    for r in range(4):
        for c in range(4):
            v = 0.0
            for k in range(4):
                xt = 0.0
                for l in range(4):
                    xt += float(X[r, l]) * (float(T[l, k]) - (1.0 if l == k else 0.0))
                v += xt * _inverse_at(X, k, c)
            out[r, c] = np.float32(v + (1.0 if r == c else 0.0))
    out[3] = (0.0, 0.0, 0.0, 1.0)
    return out
