"""The start policy on the device (c_api.h "start policy"; the rule: bpvo_amd/csrc/vo_state.h, its numpy statement: tests/start_policy_ref.py).

Scenario S (an accelerating camera: the reference's start fails on frames 4 - 7, tests/test_start_policy_cpu.py pins that on the oracle), scenario
Q (small steps, no key-framing: T_kf accumulates) and scenario R (every branch of addFrame, the re-estimate among them), 120x160, 3 levels,
Tukey.  What is checked: the rescue; that every estimate is bit for bit a plain bpvo_hip_estimate_pose from the start the record reports, and
that start and its scores are the numpy rule applied to the earlier Results and to bpvo_hip_score_poses; hints; many sequences in one context
against contexts of their own; rigs; that the default policy changes no byte; every
refusal."""
import ctypes as C
import re

import numpy as np
import pytest

import start_policy_ref as ref
from bpvo_amd import capi, synth
from util import bits_equal, make_params

pytestmark = pytest.mark.gpu

I4 = np.eye(4, dtype=np.float32)
INVALID, UNSUPPORTED = -1, -2
SCORED = dict(mode=ref.MODE_SCORED, score_level=ref.SCORE_LEVEL, tau=0.5)
VELOCITY = dict(mode=ref.MODE_CONSTANT_VELOCITY, score_level=-1, tau=0.0)
REFERENCE = dict(mode=ref.MODE_KEYFRAME_POSE, score_level=-1, tau=0.0)


def params_for(hip, scenario, descriptor="bitplanes"):
    return make_params(hip, descriptor=descriptor, levels=ref.LEVELS, **(ref.Q_PARAMS if scenario == "Q" else {}))


def scenario(name):
    return {"S": ref.scenario_S, "Q": ref.scenario_Q, "R": ref.scenario_R}[name]()


def stats_key(st):
    return [(s["numIterations"], s["status"], np.float32(s["finalError"]).tobytes(), np.float32(s["firstOrderOptimality"]).tobytes()) for s in st]


def info_key(info):
    return (info["n_candidates"], info["chosen"], tuple(info["kind"]), info["T_start"].tobytes(), info["scores"].tobytes())


def run_add_frame(hip, name, policy, descriptor="bitplanes", options=None, hints=None, set_policy=True):
    """Scenario `name` through add_frame on a context of its own: per frame dict(res, cloud, npts, info [2], cov T), and the trajectory.  hints:
    {frame: [poses]} set before that frame."""
    seq = scenario(name)
    ctx = hip.create(seq["K"], seq["b"], ref.ROWS, ref.COLS, params_for(hip, name, descriptor), n_frames=3, n_pairs=1)
    for k, v in (options or {}).items():
        ctx.set_option(k, v)
    if set_policy:
        ctx.set_start_policy(policy)
    out = []
    for k, (img, disp) in enumerate(seq["frames"]):
        if hints and k in hints:
            ctx.vo_set_start_hints(hints[k])
        res = ctx.add_frame(img, disp)
        out.append(dict(res=res, cloud=ctx.get_point_cloud() if res["hasPointCloud"] else None, npts=ctx.vo_num_points_at_level(),
                        info=[ctx.vo_start_info(0), ctx.vo_start_info(1)],
                        cov_T=ctx.vo_pose_covariance()["T"] if (options or {}).get("pose_covariance") else None))
    traj = ctx.trajectory()
    ctx.close()
    return out, traj


def assert_same_frame(a, b, what):
    ra, rb = a["res"], b["res"]
    assert bits_equal(ra["pose"], rb["pose"]), (what, "pose", ra["pose"], rb["pose"])
    assert bits_equal(ra["covariance"], rb["covariance"]), (what, "covariance")
    assert stats_key(ra["stats"]) == stats_key(rb["stats"]), (what, "stats")
    for k in ("isKeyFrame", "keyFramingReason", "hasPointCloud"):
        assert ra[k] == rb[k], (what, k, ra[k], rb[k])
    assert a["npts"] == b["npts"], (what, "num_points_at_level")
    assert (a["cloud"] is None) == (b["cloud"] is None), (what, "cloud")
    if a["cloud"] is not None:
        assert np.array_equal(a["cloud"][0].view(np.uint8), b["cloud"][0].view(np.uint8)) and bits_equal(a["cloud"][1], b["cloud"][1]), (what, "point cloud")
    for w in (0, 1):
        assert info_key(a["info"][w]) == info_key(b["info"][w]), (what, "start info", w, a["info"][w], b["info"][w])


def final_info(frame):
    """the record of the estimate the result's pose came from: the re-estimate's where it ran"""
    return frame["info"][1] if frame["info"][1]["n_candidates"] else frame["info"][0]


def errors(name, out):
    seq = scenario(name)
    return {k: ref.translation_error(out[k]["res"]["pose"], ref.true_motion(seq, k)) for k in range(1, len(out))}


@pytest.fixture(scope="module")
def S_runs(hip):
    return {mode: run_add_frame(hip, "S", pol) for mode, pol in ((0, REFERENCE), (1, VELOCITY), (2, SCORED))}


# ---- 1. the rescue ------------------------------------------------------------------------------------------------------------------------------
def test_rescue(S_runs):
    """Scenario S, bit-planes, add_frame: the reference's start ends metres off on frames 4 - 7, a start at the last motion (mode 1) or at the
    best-scoring candidate (mode 2) within 0.05 m; mode 2 chooses the last motion there and — M being the Identity — the reference's start on frame 1."""
    err = {mode: errors("S", S_runs[mode][0]) for mode in (0, 1, 2)}
    for mode in (0, 1, 2):
        print("mode", mode, "translation errors [m]", {k: round(v, 4) for k, v in err[mode].items()})
    out2 = S_runs[2][0]
    print("mode 2 chosen", [final_info(f)["chosen"] for f in out2[1:]], "scores", [np.round(final_info(f)["scores"]["score"], 4).tolist() for f in out2[1:]])
    for k in ref.S_HARD:
        assert err[0][k] > 0.5, (k, err[0][k])
        assert err[1][k] < 0.05, (k, err[1][k])
        assert err[2][k] < 0.05, (k, err[2][k])
        assert final_info(out2[k])["chosen"] == 1, (k, final_info(out2[k]))
    first = final_info(out2[1])
    assert first["chosen"] == 0 and first["kind"] == [0, 1, 2] and first["scores"]["score"][0] == first["scores"]["score"][1] == first["scores"]["score"][2]
    assert out2[0]["info"][0]["n_candidates"] == 0 and out2[0]["info"][1]["n_candidates"] == 0      # a first frame estimates nothing
    # modes 0 and 1 report their one candidate with zeroed records
    for mode, kind in ((0, ref.KIND_IDENTITY), (1, ref.KIND_LAST_MOTION)):
        info = final_info(S_runs[mode][0][4])
        assert info["n_candidates"] == 1 and info["chosen"] == 0 and info["kind"] == [kind]
        assert info["scores"].tobytes() == np.zeros(1, capi.POSE_SCORE).tobytes()


# ---- 2. replay, bit for bit -------------------------------------------------------------------------------------------------------------------
def check_record(info, mode, which, T_kf, M, hints, plain, policy, what):
    """The record against the numpy rule: candidates from (T_kf, M, hints), scores from score_poses on the plain context's slots (0, 1)."""
    cands, kinds = ref.candidates(mode, which, T_kf, M, hints)
    assert info["n_candidates"] == len(kinds) and info["kind"] == kinds, (what, info["kind"], kinds)
    if mode == ref.MODE_SCORED:
        level = plain.L - 1 if policy["score_level"] < 0 else policy["score_level"]
        want = plain.score_poses(0, 1, level, cands, policy["tau"])
        assert info["scores"].tobytes() == want.tobytes(), (what, info["scores"], want)
        chosen = ref.argmin([float(s) for s in want["score"]])
    else:
        assert info["scores"].tobytes() == np.zeros(1, capi.POSE_SCORE).tobytes(), what
        chosen = 0
    assert info["chosen"] == chosen, (what, info["chosen"], chosen)
    assert bits_equal(info["T_start"], cands[chosen]), (what, info["T_start"], cands[chosen])


@pytest.mark.parametrize("reference_reduction", [0, 1])
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("name", ["S", "Q", "R"])
def test_replay(hip, name, mode, reference_reduction):
    """Every estimate of an add_frame run, replayed on a plain context (the same n_frames / n_pairs) as bpvo_hip_estimate_pose from the start the
    record reports, and every record against the numpy rule applied to the earlier Results — all bit for bit.  Option pose_covariance is on to read
    the pose of the estimate the result came from AGAINST ITS KEY FRAME (the record's T).  The test follows addFrame's state machine:
      S  every frame key-frames and none has a previous frame that was no key frame, so only which = 0 runs, against frame k - 1 with
         T_kf = Identity: Result.pose of frame k is that estimate
      Q  no frame key-frames: which = 0 against frame 0, T_kf accumulates (the rule's product is exercised)
      R  frames 1, 2 are no key frames, frame 3 key-frames with the re-estimate (which = 1, against frame 2, whose pose the result carries), frame 4
         key-frames against frame 2 with T_kf the re-estimate's pose, frame 5 against frame 4"""
    policy = (SCORED if name != "Q" else dict(mode=ref.MODE_SCORED, score_level=-1, tau=0.4)) if mode == 2 else VELOCITY
    options = {"pose_covariance": 1}
    if reference_reduction:
        options["reference_reduction"] = 1
    out, _ = run_add_frame(hip, name, policy, options=options)
    seq = scenario(name)
    plain = hip.create(seq["K"], seq["b"], ref.ROWS, ref.COLS, params_for(hip, name), n_frames=3, n_pairs=1)
    if reference_reduction:
        plain.set_option("reference_reduction", 1)

    def pair(a, b):
        plain.frame_set_data(0, *seq["frames"][a])
        plain.frame_set_template(0)
        plain.frame_set_data(1, *seq["frames"][b])

    kf, prev_has_data, T_kf, M = 0, False, I4, I4
    branches = set()
    for k in range(1, len(out)):
        f = out[k]
        pair(kf, k)
        check_record(f["info"][0], mode, 0, T_kf, M, [], plain, policy, (name, k, 0))
        T, st = plain.estimate_pose(0, 0, 1, f["info"][0]["T_start"])
        if not f["res"]["isKeyFrame"]:
            branches.add("no key frame")
            assert f["info"][1]["n_candidates"] == 0
            prev_has_data, T_kf_next = True, T
        elif not prev_has_data:
            branches.add("key frame")
            assert f["info"][1]["n_candidates"] == 0
            if bits_equal(T_kf, I4):      # (T_est T_kf^-1 with T_kf = Identity is T_est: the issue's statement for S)
                assert np.array_equal(f["res"]["pose"], T), (name, k)
            kf, T_kf_next = k, I4
        else:
            branches.add("key frame, re-estimate")
            pair(k - 1, k)
            check_record(f["info"][1], mode, 1, I4, M, [], plain, policy, (name, k, 1))
            T, st = plain.estimate_pose(0, 0, 1, f["info"][1]["T_start"])
            assert bits_equal(f["res"]["pose"], T), (name, k)
            kf, prev_has_data, T_kf_next = k - 1, False, T
        assert bits_equal(T, f["cov_T"]), (name, k, T, f["cov_T"])
        assert stats_key(st) == stats_key(f["res"]["stats"]), (name, k)
        T_kf, M = T_kf_next, f["res"]["pose"]
    assert branches == {"S": {"key frame"}, "Q": {"no key frame"}, "R": {"no key frame", "key frame", "key frame, re-estimate"}}[name], branches
    plain.close()


# ---- 3. hints -----------------------------------------------------------------------------------------------------------------------------------
def test_hints(hip, S_runs):
    seq = scenario("S")
    truth4 = ref.true_motion(seq, 4).astype(np.float32)
    out, _ = run_add_frame(hip, "S", VELOCITY, hints={4: [truth4]})
    info = out[4]["info"][0]      # (S: the one estimate of a frame is which = 0, with T_kf = Identity)
    assert info["n_candidates"] == 1 and info["kind"] == [ref.KIND_HINT] and out[4]["info"][1]["n_candidates"] == 0, info
    assert bits_equal(info["T_start"], ref.m44_mul(truth4, I4)) and np.array_equal(info["T_start"], truth4)
    assert ref.translation_error(out[4]["res"]["pose"], truth4) < 0.05
    assert out[5]["info"][0]["kind"] == [ref.KIND_LAST_MOTION]      # gone on frame 5
    assert bits_equal(out[5]["info"][0]["T_start"], ref.m44_mul(out[4]["res"]["pose"], I4))
    # mode 2: a hint 2 m backwards is listed, scored and not chosen
    wrong = np.eye(4, dtype=np.float32)
    wrong[:3, 3] = -2.0 * ref.DIRECTION
    out2, _ = run_add_frame(hip, "S", SCORED, hints={4: [wrong]})
    info = out2[4]["info"][0]
    assert info["n_candidates"] == 4 and info["kind"] == [0, 1, 2, 3], info
    assert info["scores"]["score"][3] > info["scores"]["score"][info["chosen"]] > 0.0 and info["chosen"] == 1, info
    # ... and changes nothing of the frame: the other three records and the result are those of the run without the hint
    base = S_runs[2][0]
    assert out2[4]["info"][0]["scores"][:3].tobytes() == base[4]["info"][0]["scores"].tobytes()
    assert bits_equal(out2[4]["res"]["pose"], base[4]["res"]["pose"])
    assert out2[5]["info"][0]["kind"] == [0, 1, 2]
    assert_same_frame(out2[7], base[7], "after the hint")
    # R, frame 3 (a key frame with the re-estimate): both estimates of the call list the hint, then it is dropped
    out3, _ = run_add_frame(hip, "R", SCORED, hints={3: [wrong]})
    assert out3[3]["info"][0]["kind"] == [0, 1, 2, 3] and out3[3]["info"][1]["kind"] == [0, 1, 2, 3]
    assert out3[4]["info"][0]["kind"] == [0, 1, 2]


# ---- 4. one context for many --------------------------------------------------------------------------------------------------------------------
class Many:
    """add_frames on one context of S sequences: per sequence the frames' snapshots in run_add_frame's format"""

    def __init__(self, hip, seq0, params, S, options=None):
        self.ctx = hip.create(seq0["K"], seq0["b"], ref.ROWS, ref.COLS, params, n_frames=3 * S, n_pairs=S)
        for k, v in (options or {}).items():
            self.ctx.set_option(k, v)
        self.out = [[] for _ in range(S)]

    def call(self, ids, frames):
        res = self.ctx.add_frames(np.stack([f[0] for f in frames]), np.stack([f[1] for f in frames]), seq=ids)
        for s, r in zip(ids, res):
            self.out[s].append(dict(res=r, cloud=self.ctx.seq_point_cloud(s) if r["hasPointCloud"] else None, npts=self.ctx.seq_num_points_at_level(s),
                                    info=[self.ctx.seq_start_info(s, 0), self.ctx.seq_start_info(s, 1)]))


def test_one_context_for_many_sequences(hip, S_runs):
    """Five sequences in one context — S scored at level 2 with tau 0.5; Q with parameters of its own (no key-framing) under the CONTEXT's policy,
    constant velocity; S scored at the coarsest level with tau 0.4 (a second launch of the call); S in mode 0; R (the re-estimate runs) scored like
    sequence 0 — each bit for bit the add_frame context with that policy."""
    S, Q, R = scenario("S"), scenario("Q"), scenario("R")
    m = Many(hip, S, params_for(hip, "S"), 5)
    other = dict(mode=ref.MODE_SCORED, score_level=-1, tau=0.4)
    m.ctx.seq_set_params(1, params_for(hip, "Q"))
    m.ctx.set_start_policy(VELOCITY)
    m.ctx.seq_set_start_policy(0, SCORED)
    m.ctx.seq_set_start_policy(2, other)
    m.ctx.seq_set_start_policy(3, REFERENCE)
    m.ctx.seq_set_start_policy(4, SCORED)
    assert m.ctx.seq_get_start_policy(0) == (SCORED, True) and m.ctx.seq_get_start_policy(1) == (VELOCITY, False)
    assert m.ctx.seq_get_start_policy(2)[0]["tau"] == float(np.float32(0.4)) and m.ctx.seq_get_start_policy(3) == (REFERENCE, True)
    frames = [S["frames"], Q["frames"], S["frames"], S["frames"], R["frames"]]
    for k in range(8):
        ids = [s for s in range(5) if k < len(frames[s])]
        m.call(ids, [frames[s][k] for s in ids])
    trajs = [m.ctx.seq_trajectory(s) for s in range(5)]
    m.ctx.close()
    singles = [S_runs[2], run_add_frame(hip, "Q", VELOCITY), run_add_frame(hip, "S", other), S_runs[0], run_add_frame(hip, "R", SCORED)]
    assert singles[4][0][3]["info"][1]["n_candidates"] == 3      # (R's frame 3 did re-estimate)
    for s in range(5):
        out, traj = singles[s]
        assert len(m.out[s]) == len(out)
        for k, (a, b) in enumerate(zip(m.out[s], out)):
            assert_same_frame(a, b, f"sequence {s} frame {k}")
        assert bits_equal(trajs[s], traj), s
    assert m.out[1][3]["info"][0]["kind"] == [ref.KIND_LAST_MOTION]      # (sequence 1 did run the context's policy)


def test_intensity_sequences_in_one_context(hip):
    """... and with the intensity descriptor (tau in grey levels): S scored with tau 30 and S at constant velocity."""
    S = scenario("S")
    scored = dict(mode=ref.MODE_SCORED, score_level=ref.SCORE_LEVEL, tau=30.0)
    m = Many(hip, S, params_for(hip, "S", "intensity"), 2)
    m.ctx.seq_set_start_policy(0, scored)
    m.ctx.seq_set_start_policy(1, VELOCITY)
    for k in range(8):
        m.call([0, 1], [S["frames"][k], S["frames"][k]])
    trajs = [m.ctx.seq_trajectory(s) for s in range(2)]
    m.ctx.close()
    for s, pol in enumerate((scored, VELOCITY)):
        out, traj = run_add_frame(hip, "S", pol, descriptor="intensity")
        for k, (a, b) in enumerate(zip(m.out[s], out)):
            assert_same_frame(a, b, f"intensity sequence {s} frame {k}")
        assert bits_equal(trajs[s], traj), s
        err = errors("S", out)
        print("intensity", pol["mode"], {k: round(v, 4) for k, v in err.items()})
        assert err[6] < 0.05, err      # (the frame the reference's start loses with this descriptor: 10.77 m on the oracle)


def test_stereo_sequences(hip):
    """add_frames_stereo: two sequences with policies of their own against add_frame_stereo contexts with those policies."""
    rows, cols, ndisp, n_frames = 240, 320, 64, 4
    K, _ = synth.calibration(rows, cols)
    seqs = [synth.make_stereo_sequence(rows, cols, n_frames, index=i, step_rot=0.006, step_trans=0.1, camera=(K, 0.6)) for i in (0, 1)]
    policies = [dict(mode=ref.MODE_SCORED, score_level=-1, tau=0.5), VELOCITY]
    p = make_params(hip, descriptor="bitplanes", levels=ref.LEVELS)
    multi = hip.create(K, 0.6, rows, cols, p, n_frames=6, n_pairs=2)
    sp = multi.default_stereo_params(ndisp)
    for s in range(2):
        multi.seq_set_start_policy(s, policies[s])
    got = [[], []]
    for k in range(n_frames):
        res = multi.add_frames_stereo([seqs[0]["frames"][k][0], seqs[1]["frames"][k][0]], [seqs[0]["frames"][k][1], seqs[1]["frames"][k][1]], sp)
        for s in range(2):
            got[s].append((res[s], multi.seq_start_info(s, 0), multi.seq_start_info(s, 1)))
    trajs = [multi.seq_trajectory(s) for s in range(2)]
    multi.close()
    for s in range(2):
        one = hip.create(K, 0.6, rows, cols, p, n_frames=3, n_pairs=1)
        one.set_start_policy(policies[s])
        for k in range(n_frames):
            res = one.add_frame_stereo(*seqs[s]["frames"][k], sp)
            a = got[s][k]
            assert bits_equal(a[0]["pose"], res["pose"]) and stats_key(a[0]["stats"]) == stats_key(res["stats"]) and a[0]["isKeyFrame"] == res["isKeyFrame"], (s, k)
            assert info_key(a[1]) == info_key(one.vo_start_info(0)) and info_key(a[2]) == info_key(one.vo_start_info(1)), (s, k)
        assert bits_equal(trajs[s], one.trajectory()), s
        if s == 0:
            assert one.vo_start_info(0)["n_candidates"] == 3
        one.close()


# ---- 5. rigs ------------------------------------------------------------------------------------------------------------------------------------
RIG_X = [np.eye(4), synth.twist_to_matrix((0, 0.14, 0.02, 0.3, 0.02, 0.1))]      # tests/test_gpu_rig.py's first two extrinsics


def test_a_rig_of_one_camera_is_the_sequence(hip, S_runs):
    S = scenario("S")
    ctx = hip.create(S["K"], S["b"], ref.ROWS, ref.COLS, params_for(hip, "S"), n_frames=3, n_pairs=1)
    ctx.rigs_set([I4[None]])
    ctx.rigs_set_start_policy(0, SCORED)
    assert ctx.rigs_get_start_policy(0) == (SCORED, True)
    base = S_runs[2][0]
    for k, (img, disp) in enumerate(S["frames"]):
        res = ctx.add_frames_rigs([[img]], [[disp]])[0]
        assert bits_equal(res["pose"], base[k]["res"]["pose"]) and stats_key(res["stats"]) == stats_key(base[k]["res"]["stats"]), k
        assert res["isKeyFrame"] == base[k]["res"]["isKeyFrame"]
        for w in (0, 1):
            assert info_key(ctx.rigs_start_info(0, w)) == info_key(base[k]["info"][w]), (k, w)
    assert bits_equal(ctx.rigs_trajectory(0), S_runs[2][1])
    ctx.close()


def run_rig(hip, seq, policy):
    X = np.stack([x.astype(np.float32) for x in RIG_X])
    ctx = hip.create(seq["K"][0], seq["b"][0], ref.ROWS, ref.COLS, params_for(hip, "S"), n_frames=6, n_pairs=2)
    ctx.rigs_set([X])
    ctx.rigs_set_start_policy(0, policy)
    out = []
    for k, members in enumerate(seq["frames"]):
        res = ctx.add_frames_rigs([[m[0] for m in members]], [[m[1] for m in members]])[0]
        out.append(dict(res=res, info=[ctx.rigs_start_info(0, 0), ctx.rigs_start_info(0, 1)]))
    ctx.close()
    return out


def test_a_two_camera_rig(hip):
    """Two cameras over S: modes 1 and 2 end within 0.05 m of the body's truth on frames 4 - 7 (mode 0 is only reported: nobody has measured whether
    the reference's start fails on the rig); the pooled scores of the records are the formula on per-member score_poses records at the member poses
    of the numpy rule's body candidates."""
    seq = ref.scenario_S_rig(tuple(tuple(x.reshape(-1)) for x in RIG_X))
    X = [x.astype(np.float32) for x in RIG_X]
    runs = {mode: run_rig(hip, seq, pol) for mode, pol in ((0, REFERENCE), (1, VELOCITY), (2, SCORED))}
    err = {mode: {k: ref.translation_error(runs[mode][k]["res"]["pose"], ref.true_motion(seq, k)) for k in range(1, 8)} for mode in runs}
    for mode in (0, 1, 2):
        print("rig mode", mode, "translation errors [m]", {k: round(v, 4) for k, v in err[mode].items()})
    print("rig mode 0 fails on frames", [k for k in range(1, 8) if err[0][k] > 0.5], "(reported, not asserted)")
    for k in ref.S_HARD:
        assert err[1][k] < 0.05, (k, err[1][k])
        assert err[2][k] < 0.05, (k, err[2][k])
    # the records of mode 2 against per-member score_poses on a plain context: member p's pair in slots (2p, 2p + 1)
    out = runs[2]
    plain = hip.create(seq["K"][0], seq["b"][0], ref.ROWS, ref.COLS, params_for(hip, "S"), n_frames=4, n_pairs=2)
    checked = 0
    for k in range(1, 8):
        f = out[k]
        assert f["res"]["isKeyFrame"], k
        which = 0      # (S: one estimate per frame, against frame k - 1 with T_kf = Identity)
        assert f["info"][1]["n_candidates"] == 0
        M = out[k - 1]["res"]["pose"] if k > 1 else I4
        for p in range(2):
            plain.frame_set_data(2 * p, *seq["frames"][k - 1][p])
            plain.frame_set_template(2 * p)
            plain.frame_set_data(2 * p + 1, *seq["frames"][k][p])
        cands, kinds = ref.candidates(ref.MODE_SCORED, which, I4, M)
        info = f["info"][which]
        assert info["kind"] == kinds == [0, 1, 2]
        member = [plain.score_poses(2 * p, 2 * p + 1, ref.SCORE_LEVEL, np.stack([ref.rig_member_pose(X[p], T) for T in cands]), 0.5) for p in range(2)]
        n_points = [plain.num_points(2 * p, ref.SCORE_LEVEL) for p in range(2)]
        want = np.zeros(3, capi.POSE_SCORE)
        for j in range(3):
            want[j] = ref.pooled_record([member[0][j], member[1][j]], n_points, plain.Cn, 0.5)
        assert info["scores"].tobytes() == want.tobytes(), (k, info["scores"], want)
        assert info["chosen"] == ref.argmin([float(s) for s in want["score"]]) and bits_equal(info["T_start"], cands[info["chosen"]]), k
        checked += 1
    assert checked == 7
    plain.close()


# ---- 6. off means off -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["S", "Q", "R"])
def test_the_default_policy_changes_no_byte(hip, S_runs, name):
    """A context whose policy was never set and one set to mode 0 explicitly: identical results, trajectories and point clouds."""
    never, traj_never = run_add_frame(hip, name, None, set_policy=False)
    explicit, traj_explicit = S_runs[0] if name == "S" else run_add_frame(hip, name, REFERENCE)
    assert len(never) == len(explicit)
    for k, (a, b) in enumerate(zip(never, explicit)):
        assert_same_frame(a, b, (name, k))
        for w in (0, 1):      # mode 0 starts at T_kf / the Identity themselves
            if a["info"][w]["n_candidates"]:
                assert a["info"][w]["kind"] == [ref.KIND_IDENTITY]
        if k and name == "S":
            assert bits_equal(a["info"][0]["T_start"], I4)
    assert bits_equal(traj_never, traj_explicit)


# ---- 7. every refusal ---------------------------------------------------------------------------------------------------------------------------
def refused(ctx, code, fn, *args):
    with pytest.raises(capi.BpvoError) as e:
        fn(*args)
    text = str(e.value)
    assert re.match(r"status %d:" % code, text), text
    msg = ctx.b.fn("last_error", C.c_char_p)(ctx.h)
    assert msg and msg.decode() in text
    return text


def test_refusals(hip):
    S = scenario("S")
    p = params_for(hip, "S")
    ctx = hip.create(S["K"], S["b"], ref.ROWS, ref.COLS, p, n_frames=9, n_pairs=3)
    assert ctx.get_start_policy() == REFERENCE and ctx.seq_get_start_policy(1) == (REFERENCE, False)
    ctx.set_start_policy(SCORED)
    # a mode outside 0 .. 2, a mode-2 tau that is not finite and positive, a score level the context does not have
    bad = [dict(mode=3, score_level=-1, tau=0.5), dict(mode=-1, score_level=-1, tau=0.5)]
    bad += [dict(mode=2, score_level=-1, tau=t) for t in (0.0, -0.5, float("nan"), float("inf"))]
    bad += [dict(mode=2, score_level=l, tau=0.5) for l in (3, -2, 99)]
    for pol in bad:
        refused(ctx, INVALID, ctx.set_start_policy, pol)
        assert ctx.get_start_policy() == SCORED
        refused(ctx, INVALID, ctx.seq_set_start_policy, 1, pol)
        assert ctx.seq_get_start_policy(1) == (SCORED, False)
    ctx.seq_set_start_policy(1, VELOCITY)
    refused(ctx, INVALID, ctx.seq_set_start_policy, 1, bad[0])
    assert ctx.seq_get_start_policy(1) == (VELOCITY, True)
    refused(ctx, INVALID, ctx.seq_set_start_policy, 3, SCORED)      # no such sequence
    # hints: a 14th, a non-rigid one, a non-finite one, two in mode 1, any in mode 0 — the pending ones stay
    hint = ref.true_motion(S, 4).astype(np.float32)
    ctx.seq_set_start_hints(0, [hint] * 13)
    refused(ctx, INVALID, ctx.seq_set_start_hints, 0, [hint] * 14)
    skewed = hint.copy()
    skewed[0, 0] = 1.5
    refused(ctx, INVALID, ctx.seq_set_start_hints, 0, [skewed])
    nan = hint.copy()
    nan[2, 3] = np.nan
    refused(ctx, INVALID, ctx.seq_set_start_hints, 0, [nan])
    refused(ctx, INVALID, ctx.seq_set_start_hints, 1, [hint, hint])
    ctx.seq_set_start_hints(1, [hint])
    ctx.seq_set_start_policy(2, REFERENCE)
    refused(ctx, INVALID, ctx.seq_set_start_hints, 2, [hint])
    # the pending hints are used by the next estimate: 13 of them, sixteen candidates in all
    ctx.add_frames(np.stack([S["frames"][0][0]] * 3), np.stack([S["frames"][0][1]] * 3))
    assert ctx.seq_start_info(0, 0)["n_candidates"] == 0
    # a policy change while the body holds frames is allowed and takes effect at the next call
    ctx.seq_set_start_policy(2, SCORED)
    ctx.add_frames(np.stack([S["frames"][1][0]] * 3), np.stack([S["frames"][1][1]] * 3))
    info = ctx.seq_start_info(0, 0)
    assert info["n_candidates"] == 16 and info["kind"] == [0, 1, 2] + [3] * 13
    assert ctx.seq_start_info(1, 0)["kind"] == [ref.KIND_HINT] and ctx.seq_start_info(2, 0)["kind"] == [0, 1, 2]
    # a policy outlives seq_reset; the motion and the hints do not
    ctx.seq_set_start_hints(1, [hint])
    ctx.seq_reset(1)
    assert ctx.seq_get_start_policy(1) == (VELOCITY, True) and ctx.seq_start_info(1, 0)["n_candidates"] == 0
    ctx.add_frames(S["frames"][0][0][None], S["frames"][0][1][None], seq=[1])
    ctx.add_frames(S["frames"][1][0][None], S["frames"][1][1][None], seq=[1])
    info = ctx.seq_start_info(1, 0)
    assert info["kind"] == [ref.KIND_LAST_MOTION] and bits_equal(info["T_start"], I4)
    for which in (-1, 2):
        refused(ctx, INVALID, ctx.seq_start_info, 0, which)
    ctx.close()
    # add_frame's own state
    one = hip.create(S["K"], S["b"], ref.ROWS, ref.COLS, p, n_frames=3, n_pairs=1)
    refused(one, INVALID, one.vo_set_start_hints, [hint])      # mode 0 takes none
    one.set_start_policy(VELOCITY)
    refused(one, INVALID, one.vo_set_start_hints, [hint, hint])
    one.vo_set_start_hints([hint])
    refused(one, INVALID, one.vo_start_info, 2)
    one.close()
    # mode 2 on a context pose scoring does not serve: the scorer's message, the earlier policy stays
    cubic = hip.create(S["K"], S["b"], ref.ROWS, ref.COLS, make_params(hip, descriptor="bitplanes", levels=3, interp=capi.INTERP_CUBIC), n_frames=3, n_pairs=1)
    cubic.set_start_policy(VELOCITY)
    assert "pose score" in refused(cubic, UNSUPPORTED, cubic.set_start_policy, SCORED) and "kCubic" in str(cubic.b.fn("last_error", C.c_char_p)(cubic.h))
    assert cubic.get_start_policy() == VELOCITY
    refused(cubic, UNSUPPORTED, cubic.seq_set_start_policy, 0, SCORED)
    cubic.close()
    wide = hip.create(S["K"], S["b"], ref.ROWS, ref.COLS, make_params(hip, descriptor="latch", levels=2, latchNumBytes=16), n_frames=3, n_pairs=1)
    assert wide.Cn == 128 and "128" in refused(wide, UNSUPPORTED, wide.set_start_policy, dict(mode=2, score_level=-1, tau=0.5))
    assert wide.get_start_policy() == REFERENCE
    wide.close()
    # a member of a rig takes neither a policy nor hints of its own; the rig's body does
    rig = hip.create(S["K"], S["b"], ref.ROWS, ref.COLS, p, n_frames=6, n_pairs=2)
    rig.rigs_set([np.stack([x.astype(np.float32) for x in RIG_X])])
    refused(rig, INVALID, rig.seq_set_start_policy, 1, VELOCITY)
    refused(rig, INVALID, rig.seq_set_start_hints, 0, [hint])
    assert rig.rigs_get_start_policy(0) == (REFERENCE, False)
    rig.rigs_set_start_policy(0, VELOCITY)
    refused(rig, INVALID, rig.rigs_set_start_policy, 0, bad[0])
    refused(rig, INVALID, rig.rigs_set_start_policy, 1, VELOCITY)      # no such rig
    refused(rig, INVALID, rig.rigs_set_start_hints, 0, [hint, hint])
    assert rig.rigs_get_start_policy(0) == (VELOCITY, True)
    rig.rigs_set_start_hints(0, [hint])
    rig.close()
