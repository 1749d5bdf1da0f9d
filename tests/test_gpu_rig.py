"""Rig mode (bpvo_hip_*_rig): the cameras of a rigid rig estimated as ONE body pose.  The joint normal equations against a numpy float64 combination
of the members' own bpvo_hip_linearize results (B_p = A_p^-1 Ad(X_p)), a rig of one against that camera's bpvo_hip_estimate_pose, three members
against a float64 joint Gauss-Newton written here, the joint estimate against ground truth on noisy frames, bpvo_hip_add_frames_rig against
bpvo_hip_add_frame, and every refusal.  Scene: synth.make_pair's plane at index 3 (seed 1003), 120x160, seen through three extrinsics."""
import re

import numpy as np
import pytest

from bpvo_amd import capi, synth
from util import ROT_TOL, TRANS_TOL, bits_equal, make_params, perturbed_pose, pose_error

pytestmark = pytest.mark.gpu

ROWS, COLS, INDEX = 120, 160, 3
EXTRINSIC_TWISTS = ((0, 0, 0, 0, 0, 0), (0, 0.14, 0.02, 0.3, 0.02, 0.1), (0.03, -0.2, 0, -0.4, 0, 0.05))
ERR_INVALID_ARG, ERR_UNSUPPORTED, ERR_NO_TEMPLATE = -1, -2, -4      # c_api.h BPVO_ERR_*
PLANE = (10.0, (0.1, -0.15))      # synth.make_pair's plane


def extrinsics(which=(0, 1, 2)):
    return [np.ascontiguousarray(synth.twist_to_matrix(EXTRINSIC_TWISTS[k]), np.float32) for k in which]


@pytest.fixture(scope="module")
def scene():
    """Member p sees make_pair(index 3)'s plane from X_p (template) and from X_p T_gt (current frame); noisy: sigma = 2 grey levels of seeded
    Gaussian noise on the current frames."""
    d = synth.make_pair(ROWS, COLS, INDEX)
    K, b, T_gt, seed = d["K"], d["b"], d["T_gt"], d["seed"]
    members = []
    for p, X in enumerate(extrinsics()):
        Xd = X.astype(np.float64)
        imgA, dispA = synth._render(K, b, ROWS, COLS, Xd, seed, *PLANE)
        imgB, dispB = synth._render(K, b, ROWS, COLS, Xd @ T_gt, seed, *PLANE)
        noise = np.random.default_rng([seed, 77, p]).normal(0.0, 2.0, imgB.shape)
        noisy = np.clip(np.rint(imgB.astype(np.float64) + noise), 0, 255).astype(np.uint8)
        members.append(dict(X=X, imgA=imgA, dispA=dispA, imgB=imgB, dispB=dispB, noisyB=noisy))
    return dict(K=K, b=b, T_gt=T_gt, members=members)


def rig_context(hip, scene, which, levels=3, noisy=False, **pk):
    """A context with member i of the rig on workspace i, template in slot 2 i, current frame in slot 2 i + 1."""
    n = len(which)
    p = make_params(hip, levels=levels, **pk)
    ctx = hip.create(scene["K"], scene["b"], ROWS, COLS, p, device=0, n_frames=2 * n, n_pairs=n)
    for i, k in enumerate(which):
        m = scene["members"][k]
        ctx.frame_set_data(2 * i, m["imgA"], m["dispA"])
        ctx.frame_set_template(2 * i)
        ctx.frame_set_data(2 * i + 1, m["noisyB"] if noisy else m["imgB"], m["dispB"])
    X = np.stack([scene["members"][k]["X"] for k in which])
    return ctx, list(range(n)), [2 * i for i in range(n)], [2 * i + 1 for i in range(n)], X


def skew(v):
    return np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]], np.float64)


def body_map(ctx, ref_slot, level, X):
    """B_p = A_p^-1 Ad(X_p) in float64, (s, c) read from the template's normalisation"""
    N, Ni = ctx.get_normalization(ref_slot, level)
    s, c = float(N[0, 0]), Ni[:3, 3].astype(np.float64)
    Ai = np.eye(6)
    Ai[3:, :3] = -s * skew(c)
    Ai[3:, 3:] = s * np.eye(3)
    Xd = np.asarray(X, np.float64)
    Ad = np.zeros((6, 6))
    Ad[:3, :3] = Xd[:3, :3]
    Ad[3:, :3] = skew(Xd[:3, 3]) @ Xd[:3, :3]
    Ad[3:, 3:] = Xd[:3, :3]
    return Ai @ Ad


def member_pose(X, T):
    Xd = np.asarray(X, np.float64)
    return Xd @ np.asarray(T, np.float64) @ np.linalg.inv(Xd)


def joint_f64(ctx, wss, refs, curs, X, level, T, reset_scale):
    """the joint system from the members' own bpvo_hip_linearize results, combined in float64"""
    H, G, f2, nv = np.zeros((6, 6)), np.zeros(6), 0.0, 0
    for w, r, c, Xp in zip(wss, refs, curs, X):
        lin = ctx.linearize(w, r, c, level, member_pose(Xp, T).astype(np.float32), reset_scale=reset_scale)
        B = body_map(ctx, r, level, Xp)
        H += B.T @ lin["H"].astype(np.float64) @ B
        G += B.T @ lin["G"].astype(np.float64)
        f2 += float(lin["f_norm"]) ** 2
        nv += lin["num_valid"]
    return H, G, np.sqrt(f2), nv


def gauss_newton_f64(ctx, wss, refs, curs, X, T0=None):
    """the reference of this file: coarse to fine, per level at most 30 iterations of (members' linearize, float64 combine, solve, T <- T exp(-zeta))
    until |zeta| < 1e-7, the robust scales reset on the first iteration of each level"""
    T = np.eye(4) if T0 is None else np.asarray(T0, np.float64)
    for level in range(ctx.L - 1, -1, -1):
        for it in range(30):
            H, G, _, _ = joint_f64(ctx, wss, refs, curs, X, level, T, reset_scale=(it == 0))
            zeta = np.linalg.solve(H, G)
            T = T @ synth.twist_to_matrix(-zeta)
            if np.linalg.norm(zeta) < 1e-7:
                break
    return T


def test_joint_system_is_the_f64_combination_of_the_members_systems(hip, scene):
    ctx, wss, refs, curs, X = rig_context(hip, scene, (0, 1, 2))
    for T in (np.eye(4, dtype=np.float32), perturbed_pose(1)):
        for level in range(ctx.L):
            rig = ctx.linearize_rig(wss, refs, curs, X, level, T, reset_scale=True)
            H, G, f2, nv = np.zeros((6, 6)), np.zeros(6), 0.0, 0
            for i in range(3):
                ref = member_pose(X[i], T)
                assert np.abs(rig["T_members"][i] - ref).max() <= 2e-6 * max(1.0, np.abs(ref[:3, 3]).max()), (level, i)
                lin = ctx.linearize(wss[i], refs[i], curs[i], level, rig["T_members"][i], reset_scale=True)
                B = body_map(ctx, refs[i], level, X[i])
                H += B.T @ lin["H"].astype(np.float64) @ B
                G += B.T @ lin["G"].astype(np.float64)
                f2 += float(lin["f_norm"]) ** 2
                nv += lin["num_valid"]
            dH, dG = np.abs(rig["H"] - H).max() / np.abs(H).max(), np.abs(rig["G"] - G).max() / np.abs(G).max()
            print(f"level {level}: |dH|/max|H| = {dH:.2e}, |dG|/max|G| = {dG:.2e}, f {rig['f_norm']} vs {np.sqrt(f2)}, valid {rig['num_valid']} vs {nv}")
            assert dH <= 1e-6 and dG <= 1e-6, (level, dH, dG)
            assert abs(rig["f_norm"] - np.sqrt(f2)) <= 1e-6 * np.sqrt(f2), (level, rig["f_norm"], np.sqrt(f2))
            assert rig["num_valid"] == nv
    ctx.close()


@pytest.mark.parametrize("descriptor,loss", [("bitplanes", "tukey"), ("intensity", "huber")])
@pytest.mark.parametrize("member", [0, 1])
def test_a_rig_of_one_is_that_cameras_own_estimate(hip, scene, descriptor, loss, member):
    """X^-1 T_p X of the camera's own bpvo_hip_estimate_pose against the body estimate of a rig of that one camera, within the project's pose bar.
    The estimate iterates on the reference member's pose in that member's normalised twist, so a rig of one takes the camera's own steps —
    also where that run never settles: bit-planes / Tukey on this scene ends at maxIterations on two pyramid levels, 9e-2 m from ground truth.
    Measured on an MI355X: 0 / 0 with X = I (both configurations), 5.1e-8 rad / 5.8e-7 m (bit-planes / Tukey) and 4.2e-9 rad / 1.5e-7 m
    (intensity / Huber) with the second extrinsic: the rounding of the conjugation."""
    ctx, wss, refs, curs, X = rig_context(hip, scene, (member,), descriptor=descriptor, loss=loss)
    T_cam, _ = ctx.estimate_pose(0, 0, 1)
    T_body, stats = ctx.estimate_pose_rig(wss, refs, curs, X)
    Xd = X[0].astype(np.float64)
    want = np.linalg.inv(Xd) @ T_cam.astype(np.float64) @ Xd
    dr, dt = pose_error(T_body, want)
    print(f"member {member} {descriptor}/{loss}: rig of one against the camera's own estimate {dr:.2e} rad {dt:.2e} m; iterations {[s['numIterations'] for s in stats]}")
    assert dr <= ROT_TOL and dt <= TRANS_TOL, (dr, dt)
    assert all(s["numIterations"] >= 1 and s["finalError"] >= 0 for s in stats)
    ctx.close()


def test_three_members_against_an_f64_joint_gauss_newton(hip, scene):
    ctx, wss, refs, curs, X = rig_context(hip, scene, (0, 1, 2), descriptor="intensity", loss="huber")
    T_rig, _ = ctx.estimate_pose_rig(wss, refs, curs, X)
    T_ref = gauss_newton_f64(ctx, wss, refs, curs, X)
    dr, dt = pose_error(T_rig, T_ref)
    # the same loop for ONE camera against bpvo_hip_estimate_pose: the gap the stopping rule alone leaves
    T_one, _ = ctx.estimate_pose(0, 0, 1)
    T_one_ref = gauss_newton_f64(ctx, wss[:1], refs[:1], curs[:1], X[:1])
    dr1, dt1 = pose_error(T_one, T_one_ref)
    print(f"three members against the f64 joint Gauss-Newton: {dr:.2e} rad {dt:.2e} m; one camera against the same loop: {dr1:.2e} rad {dt1:.2e} m")
    assert dr1 <= ROT_TOL and dt1 <= TRANS_TOL, (dr1, dt1)
    assert dr <= ROT_TOL and dt <= TRANS_TOL, (dr, dt)
    ctx.close()


def test_joint_estimate_on_noisy_frames_is_no_worse_than_the_worst_camera(hip, scene):
    ctx, wss, refs, curs, X = rig_context(hip, scene, (0, 1, 2), noisy=True, descriptor="intensity", loss="huber")
    T_rig, _ = ctx.estimate_pose_rig(wss, refs, curs, X)
    er, et = pose_error(T_rig, scene["T_gt"])
    singles = []
    for i in range(3):
        T_cam, _ = ctx.estimate_pose(wss[i], refs[i], curs[i])
        Xd = X[i].astype(np.float64)
        singles.append(pose_error(np.linalg.inv(Xd) @ T_cam.astype(np.float64) @ Xd, scene["T_gt"]))
    print(f"joint {er:.2e} rad {et:.2e} m; singles {[(f'{a:.2e}', f'{b:.2e}') for a, b in singles]}")
    assert er <= max(s[0] for s in singles) and et <= max(s[1] for s in singles), (er, et, singles)
    ctx.close()


# ---- addFrame level
KF = dict(minTranslationMagToKeyFrame=0.02, minRotationMagToKeyFrame=2.5, maxFractionOfGoodPointsToKeyFrame=0.0, goodPointThreshold=0.8)
N_FRAMES = 6


def rig_sequence(which):
    return synth.make_rig_sequence(ROWS, COLS, N_FRAMES, [x.astype(np.float64) for x in extrinsics(which)], index=INDEX)


def sequences_context(hip, seq, n, capacity=None, **kw):
    p = make_params(hip, levels=3, **dict(KF, **kw))
    cams = [(seq["K"][0], seq["b"][0], ROWS, COLS)] * (capacity or n)
    return hip.create_sequences(cams, p), p


def run_alone(hip, seq, member, p):
    """member's frames through bpvo_hip_add_frame on a context of its own"""
    ctx = hip.create(seq["K"][member], seq["b"][member], ROWS, COLS, p, n_frames=3, n_pairs=1)
    res = [ctx.add_frame(*frames[member]) for frames in seq["frames"]]
    traj = ctx.trajectory()
    ctx.close()
    return res, traj


def test_add_frames_rig_of_one_at_the_origin_follows_add_frame(hip):
    seq = rig_sequence((0,))
    ctx, p = sequences_context(hip, seq, 1)
    ctx.rig_set(extrinsics((0,)))
    ids, X = ctx.rig_get()
    assert ids.tolist() == [0] and bits_equal(X[0], np.eye(4, dtype=np.float32))
    rig = [ctx.add_frames_rig([frames[0][0]], [frames[0][1]]) for frames in seq["frames"]]
    alone, traj = run_alone(hip, seq, 0, p)
    assert sum(r["isKeyFrame"] for r in rig[1:]) >= 1, "no key frame after the first: the sequence does not test the key-frame path"
    for k, (a, b) in enumerate(zip(rig, alone)):
        assert a["isKeyFrame"] == b["isKeyFrame"] and a["keyFramingReason"] == b["keyFramingReason"], (k, a["keyFramingReason"], b["keyFramingReason"])
        dr, dt = pose_error(a["pose"], b["pose"])
        assert dr <= ROT_TOL and dt <= TRANS_TOL, (k, dr, dt)
        assert bits_equal(a["covariance"], np.eye(6, dtype=np.float32))
    assert ctx.rig_trajectory().shape == traj.shape
    dr, dt = pose_error(ctx.rig_trajectory()[-1], traj[-1])
    assert dr <= ROT_TOL * N_FRAMES and dt <= TRANS_TOL * N_FRAMES, (dr, dt)
    ctx.close()


def test_add_frames_rig_of_two(hip):
    which = (0, 1)
    seq = rig_sequence(which)
    X = extrinsics(which)
    ctx, p = sequences_context(hip, seq, 2)
    ctx.rig_set(X)
    lvl = p.maxTestLevel
    key_frames = 0
    for k, frames in enumerate(seq["frames"]):
        r = ctx.add_frames_rig([f[0] for f in frames], [f[1] for f in frames])
        if k == 0:
            assert r["isKeyFrame"] and r["keyFramingReason"] == capi.KF_FIRST_FRAME and not r["hasPointCloud"]
            continue
        key_frames += int(r["isKeyFrame"])
        assert r["hasPointCloud"] == r["isKeyFrame"]
        if r["isKeyFrame"]:
            W_kf = ctx.rig_trajectory()[-1].astype(np.float64)
            for s in range(2):
                assert ctx.seq_num_points_at_level(s, lvl) > 0
                pts, pose = ctx.seq_point_cloud(s)
                assert len(pts) > 0
                want = W_kf @ np.linalg.inv(X[s].astype(np.float64))
                assert np.abs(pose - want).max() <= 1e-5, (k, s, np.abs(pose - want).max())
    assert key_frames >= 1, "no key frame after the first: the sequence does not test the key-frame path"
    traj = ctx.rig_trajectory()
    assert traj.shape == (N_FRAMES, 4, 4)
    truth = np.linalg.inv(seq["poses"][-1])      # the trajectory holds body_0 from body_k
    er, et = pose_error(traj[-1], truth)
    singles = []
    for s in range(2):
        _, t = run_alone(hip, seq, s, p)
        Xd = X[s].astype(np.float64)
        singles.append(pose_error(np.linalg.inv(Xd) @ t[-1].astype(np.float64) @ Xd, truth))      # the camera's trajectory carried to the body
    print(f"rig of two, final pose: {er:.2e} rad {et:.2e} m; the cameras alone {[(f'{a:.2e}', f'{b:.2e}') for a, b in singles]}")
    assert er <= max(s[0] for s in singles) and et <= max(s[1] for s in singles), (er, et, singles)
    ctx.close()


# ---- refusals
def refused(code, fn, *args, **kw):
    with pytest.raises(capi.BpvoError) as e:
        fn(*args, **kw)
    assert re.match(rf"status {code}:", str(e.value)), (code, str(e.value))
    return str(e.value)


def bad_extrinsics():
    X = extrinsics((1,))[0]
    out = {}
    for name in ("not finite", "last row", "not orthonormal"):
        Y = X.copy()
        if name == "not finite":
            Y[1, 3] = np.nan
        elif name == "last row":
            Y[3, 1] = 0.5
        else:
            Y[:3, :3] *= np.float32(1.001)
        out[name] = Y
    return out


@pytest.mark.parametrize("what", ["not finite", "last row", "not orthonormal"])
def test_rig_set_refuses_an_extrinsic_that_is_not_rigid(hip, what):
    seq = rig_sequence((0, 1))
    ctx, _ = sequences_context(hip, seq, 2)
    refused(ERR_INVALID_ARG, ctx.rig_set, [np.eye(4, dtype=np.float32), bad_extrinsics()[what]])
    assert ctx.rig_get()[0].size == 0
    ctx.close()


def test_rig_set_refuses_bad_member_lists(hip):
    seq = rig_sequence((0, 1))
    ctx, p = sequences_context(hip, seq, 2)
    X = extrinsics((0, 1, 2))
    refused(ERR_INVALID_ARG, ctx.rig_set, np.zeros((0, 4, 4), np.float32))                      # n < 1
    refused(ERR_INVALID_ARG, ctx.rig_set, X)                                                  # n above the sequence capacity
    refused(ERR_INVALID_ARG, ctx.rig_set, X[:2], seq=[1, 1])                                  # an id twice
    refused(ERR_INVALID_ARG, ctx.rig_set, X[:2], seq=[0, 2])                                  # no such sequence
    own = make_params(hip, levels=3, **dict(KF, maxIterations=7))
    ctx.seq_set_params(1, own)
    refused(ERR_INVALID_ARG, ctx.rig_set, X[:2])                                              # a member with parameters of its own
    ctx.seq_set_params(1, p)
    assert ctx.rig_get()[0].size == 0
    ctx.rig_set(X[:2])
    frames = seq["frames"][0]
    ctx.add_frames_rig([f[0] for f in frames], [f[1] for f in frames])
    refused(ERR_INVALID_ARG, ctx.rig_set, X[:2])                                              # the members hold frames
    ctx.close()


def test_a_rig_context_serves_add_frames_rig_only_and_goes_on_after_refusals(hip):
    seq = rig_sequence((0, 1))
    X = extrinsics((0, 1))
    p = make_params(hip, levels=3, **KF)

    def run(disturb):
        ctx = hip.create(seq["K"][0], seq["b"][0], ROWS, COLS, p, n_frames=6, n_pairs=2)
        ctx.rig_set(X)
        out = []
        for frames in seq["frames"][:4]:
            imgs, disps = [f[0] for f in frames], [f[1] for f in frames]
            if disturb:
                msg = refused(ERR_INVALID_ARG, ctx.add_frame, imgs[0], disps[0])
                assert "rig" in msg
                refused(ERR_INVALID_ARG, ctx.add_frames, np.stack(imgs), np.stack(disps))
                refused(ERR_INVALID_ARG, ctx.add_frames_stereo, imgs, imgs, ctx.default_stereo_params(16))
                refused(ERR_INVALID_ARG, ctx.rig_set, [X[0], bad_extrinsics()["last row"]])
                if not any(any(ctx.frame_state(slot)) for slot in (3, 4, 5)):
                    # (sequence 1 is still fresh: its parameters may change — and the rig then refuses its frames)
                    ctx.seq_set_params(1, make_params(hip, levels=3, **dict(KF, maxIterations=7)))
                    refused(ERR_INVALID_ARG, ctx.add_frames_rig, imgs, disps)
                    ctx.seq_set_params(1, p)
            out.append(ctx.add_frames_rig(imgs, disps))
        traj = ctx.rig_trajectory()
        ctx.close()
        return out, traj

    clean, traj_clean = run(False)
    disturbed, traj_disturbed = run(True)
    assert bits_equal(traj_clean, traj_disturbed)
    for a, b in zip(clean, disturbed):
        assert bits_equal(a["pose"], b["pose"]) and a["isKeyFrame"] == b["isKeyFrame"] and a["keyFramingReason"] == b["keyFramingReason"]


def test_estimate_rig_refusals(hip, scene):
    ctx, wss, refs, curs, X = rig_context(hip, scene, (0, 1), descriptor="intensity", loss="huber")
    T_before, _ = ctx.estimate_pose_rig(wss, refs, curs, X)
    for name, Y in bad_extrinsics().items():
        refused(ERR_INVALID_ARG, ctx.estimate_pose_rig, wss, refs, curs, np.stack([X[0], Y]))
        refused(ERR_INVALID_ARG, ctx.linearize_rig, wss, refs, curs, np.stack([X[0], Y]), 0, np.eye(4))
    refused(ERR_INVALID_ARG, ctx.estimate_pose_rig, [0, 0], refs, curs, X)                    # a workspace twice
    refused(ERR_INVALID_ARG, ctx.estimate_pose_rig, [0, 1, 1], [0, 2, 2], [1, 3, 3], np.stack([X[0], X[1], X[1]]))      # n above the workspaces
    refused(ERR_INVALID_ARG, ctx.estimate_pose_rig, [], [], [], np.zeros((0, 4, 4), np.float32))
    # a member whose template is empty (no valid disparity): BPVO_ERR_NO_TEMPLATE, as the single-pair entry points answer
    m = scene["members"][1]
    ctx.frame_set_data(2, m["imgA"], np.zeros_like(m["dispA"]))
    ctx.frame_set_template(2)
    refused(ERR_NO_TEMPLATE, ctx.estimate_pose_rig, wss, refs, curs, X)
    refused(ERR_NO_TEMPLATE, ctx.linearize_rig, wss, refs, curs, X, 0, np.eye(4))
    ctx.frame_set_data(2, m["imgA"], m["dispA"])
    ctx.frame_set_template(2)
    T_after, _ = ctx.estimate_pose_rig(wss, refs, curs, X)
    assert bits_equal(T_before, T_after)          # the context goes on as if the refused calls had not been made
    # DisparitySpaceWarp is not served
    ctx.set_warp_formulation(2)
    for i in range(2):
        ctx.frame_set_template(2 * i)
    refused(ERR_UNSUPPORTED, ctx.estimate_pose_rig, wss, refs, curs, X)
    refused(ERR_UNSUPPORTED, ctx.linearize_rig, wss, refs, curs, X, 0, np.eye(4))
    ctx.close()
