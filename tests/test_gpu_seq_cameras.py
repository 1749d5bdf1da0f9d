"""Per-sequence cameras in bpvo_hip_add_frames (bpvo_hip_create_sequences, bpvo_hip_seq_set_camera): every sequence, with its own calibration
and image size, is compared bit for bit with a bpvo_hip_create context of its camera driven by bpvo_hip_add_frame on the same frames — poses,
per-level statistics, key-frame decisions, point clouds fetched after each key frame, point counts and trajectories."""
import ctypes as C

import numpy as np
import pytest

from bpvo_amd import capi, synth
from test_gpu_multi_sequence import KF, Multi, assert_same_result, assert_sequence_equal, run_single
from util import make_params

pytestmark = pytest.mark.gpu

ERR_INVALID_ARG, ERR_UNSUPPORTED = -1, -2      # c_api.h BPVO_ERR_*
ROWS, COLS = 480, 640

# the three KITTI odometry geometries: (rows, cols, fx, cx, cy, baseline)
KITTI = [(376, 1241, 718.856, 607.1928, 185.2157, 0.5372), (375, 1242, 721.5377, 609.5593, 172.854, 0.5371),
         (370, 1226, 707.0912, 601.8873, 183.1104, 0.5372)]


def K_of(fx, fy, cx, cy):
    return np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], np.float32)


def calib_cameras(n, rows=ROWS, cols=COLS, seed=7):
    """n cameras of one size, each with its own fx / fy in 560 - 680, a principal point up to 12 px off the centre and a baseline of 0.08 - 0.16"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        fx, fy = rng.uniform(560, 680, 2)
        cx, cy = cols / 2 + rng.uniform(-12, 12), rows / 2 + rng.uniform(-12, 12)
        out.append((K_of(fx, fy, cx, cy), float(np.float32(rng.uniform(0.08, 0.16))), rows, cols))
    return out


def frames_for(cams, n_frames, scene="plane", first_index=0):
    specs = [(0.006, 0.05), (0.01, 0.06), (0.004, 0.03), (0.01, 0.08), (0.002, 0.16), (0.008, 0.04)]
    out = []
    for s, (K, b, r, c) in enumerate(cams):
        rot, tr = specs[s % len(specs)]
        out.append(synth.make_sequence(r, c, n_frames, index=first_index + s, step_rot=rot, step_trans=tr, scene=scene, camera=(K, b))["frames"])
    return out


class MultiCam:
    """one context serving S sequences with cameras of their own; records per sequence what run_single's snapshots record"""

    def __init__(self, ctx, S):
        self.ctx = ctx
        self.out = [[] for _ in range(S)]
        self.trajs = [[] for _ in range(S)]

    def call(self, ids, frames, device=False):
        imgs, disps = [f[0] for f in frames], [f[1] for f in frames]
        if device:
            import torch
            img, disp, _ = capi.pack_frames(imgs, disps)
            ti, td = torch.from_numpy(img).cuda(), torch.from_numpy(disp).cuda()
            res = self.ctx.add_frames_device(len(ids), ti.data_ptr(), td.data_ptr(), seq=ids)
            torch.cuda.synchronize()
        else:
            res = self.ctx.add_frames(imgs, disps, seq=ids)
        for s, r in zip(ids, res):
            cloud = self.ctx.seq_point_cloud(s) if r["hasPointCloud"] else None
            self.out[s].append(dict(res=r, cloud=cloud, npts=self.ctx.seq_num_points_at_level(s)))
        return res

    def reset(self, s):
        self.trajs[s].append(self.ctx.seq_trajectory(s))
        self.ctx.seq_reset(s)

    def finish(self):
        for s in range(len(self.out)):
            self.trajs[s].append(self.ctx.seq_trajectory(s))


def drive(m, seqs, schedule, device=False):
    """schedule 'lockstep': every sequence in every call, in order; 'subsets': shuffled subsets until every sequence has had all its frames"""
    S = len(seqs)
    nxt = [0] * S
    rng = np.random.default_rng(11)
    while any(nxt[s] < len(seqs[s]) for s in range(S)):
        live = [s for s in range(S) if nxt[s] < len(seqs[s])]
        if schedule == "subsets":
            live = [int(s) for s in rng.permutation(live)[: max(1, int(rng.integers(1, len(live) + 1)))]]
        m.call(live, [seqs[s][nxt[s]] for s in live], device=device)
        for s in live:
            nxt[s] += 1
    m.finish()


def singles_for(hip, cams, params, seqs, options=None):
    return [run_single(hip, K, b, r, c, params, seqs[s], options) for s, (K, b, r, c) in enumerate(cams)]


def check_all(m, singles):
    for s in range(len(singles)):
        assert_sequence_equal(m, s, *singles[s])


def set_options(ctx, options):
    for k, v in (options or {}).items():
        ctx.set_option(k, v)


def rc_and_error(ctx, name, *args):
    rc = ctx.b.fn(name)(ctx.h, *args)
    return rc, ctx.b.fn("last_error", C.c_char_p)(ctx.h).decode()


# ---- 1. mixed calibrations, one size --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("desc,loss", [("bitplanes", "tukey"), ("intensity", "huber")])
@pytest.mark.parametrize("mode", ["default", "reference_reduction"])
def test_mixed_calibrations_equal_contexts_of_their_own(hip, desc, loss, mode):
    cams = calib_cameras(6)
    assert len({(float(K[0, 0]), float(K[0, 2]), b) for K, b, _, _ in cams}) == 6
    seqs = frames_for(cams, 6)
    p = make_params(hip, descriptor=desc, loss=loss, levels=4, **KF)
    options = {"reference_reduction": 1} if mode == "reference_reduction" else None
    singles = singles_for(hip, cams, p, seqs, options)
    for device, schedule in ((False, "subsets"), (True, "lockstep")):
        ctx = hip.create_sequences(cams, p)
        set_options(ctx, options)
        assert ctx.seq_capacity() == 6 and ctx.level_size(0) == (ROWS, COLS)
        for s, (K, b, r, c) in enumerate(cams):
            got = ctx.seq_get_camera(s)
            assert np.array_equal(np.array(got.K, np.float32), K.reshape(9)) and got.baseline == np.float32(b) and (got.rows, got.cols) == (r, c)
        m = MultiCam(ctx, 6)
        drive(m, seqs, schedule, device=device)
        check_all(m, singles)
        kf = [sum(o["res"]["isKeyFrame"] for o in m.out[s][1:]) for s in range(6)]
        assert any(kf), "the sequences should key-frame"
        ctx.close()


# ---- 2. mixed sizes ---------------------------------------------------------------------------------------------------------------------
def kitti_cameras():
    return [(K_of(fx, fx, cx, cy), b, r, c) for r, c, fx, cx, cy, b in KITTI for _ in range(2)]


@pytest.mark.parametrize("scene,desc,loss", [("plane", "bitplanes", "tukey"), ("layered", "intensity", "huber")])
def test_kitti_geometries_in_one_context(hip, scene, desc, loss):
    cams = kitti_cameras()
    seqs = frames_for(cams, 8, scene=scene)
    p = make_params(hip, descriptor=desc, loss=loss, levels=4, **KF)
    singles = singles_for(hip, cams, p, seqs)
    for device, schedule in ((False, "subsets"), (True, "lockstep")):
        ctx = hip.create_sequences(cams, p)
        assert ctx.level_size(0) == (376, 1242)
        m = MultiCam(ctx, len(cams))
        drive(m, seqs, schedule, device=device)
        check_all(m, singles)
        ctx.close()


def test_sizes_across_the_nms_threshold(hip):
    """640x480 / 632x474 / 616x462 at 4 levels: the level 1 of the last two falls under minNumPixelsForNonMaximaSuppression (320 x 240) and
    is dense, the first camera's is not; every geometry group is equipped in the same calls"""
    sizes = [(480, 640), (474, 632), (462, 616)]
    cams = [(K_of(600.0 + 7 * i, 602.0 + 5 * i, c / 2 + 3 - i, r / 2 - 2 + i), 0.1 + 0.01 * i, r, c) for i, (r, c) in enumerate(sizes * 2)]
    seqs = frames_for(cams, 8)
    p = make_params(hip, descriptor="intensity", loss="huber", levels=4, **KF)
    singles = singles_for(hip, cams, p, seqs)
    ctx = hip.create_sequences(cams, p)
    m = MultiCam(ctx, len(cams))
    drive(m, seqs, "lockstep")
    check_all(m, singles)
    n1 = [ctx.seq_num_points_at_level(s, 1) for s in range(len(cams))]
    cap_nms = 160 * 120
    assert n1[0] <= cap_nms and n1[3] <= cap_nms, n1
    assert min(n1[1], n1[2], n1[4], n1[5]) > cap_nms, n1      # dense: more points than any NMS template of the context could hold
    ctx.close()


# ---- 3. no behaviour change ---------------------------------------------------------------------------------------------------------------
def test_the_context_camera_changes_nothing(hip):
    S = 4
    K, b = synth.calibration(ROWS, COLS)
    seqs = frames_for([(K, b, ROWS, COLS)] * S, 6)
    p = make_params(hip, descriptor="bitplanes", loss="tukey", levels=4, **KF)
    plain = Multi(hip, K, b, ROWS, COLS, p, S)
    cammed = Multi(hip, K, b, ROWS, COLS, p, S)
    for s in range(S):
        cammed.ctx.seq_set_camera(s, (K, b, ROWS, COLS))
        got = cammed.ctx.seq_get_camera(s)
        assert np.array_equal(np.array(got.K, np.float32), K.reshape(9)) and got.baseline == np.float32(b)
    for k in range(6):
        plain.call(list(range(S)), [seqs[s][k] for s in range(S)])
        cammed.call(list(range(S)), [seqs[s][k] for s in range(S)])
    plain.finish()
    cammed.finish()
    for s in range(S):
        for k, (a, c) in enumerate(zip(cammed.out[s], plain.out[s])):
            assert_same_result(a, c, f"sequence {s} frame {k}")
        assert np.array_equal(cammed.trajs[s][0].view(np.uint32), plain.trajs[s][0].view(np.uint32))


# ---- 4. reconfiguration ------------------------------------------------------------------------------------------------------------------
def test_reset_then_new_camera(hip):
    cams = [(K_of(600, 600, 320, 240), 0.1, 480, 640), (K_of(640, 636, 318, 243), 0.12, 480, 640), (K_of(590, 592, 308, 231), 0.09, 462, 616)]
    new = (K_of(575, 579, 306, 229), 0.14, 462, 616)
    seqs = frames_for(cams, 8)
    seq0_new = synth.make_sequence(462, 616, 5, index=20, step_rot=0.01, step_trans=0.06, camera=(new[0], new[1]))["frames"]
    p = make_params(hip, descriptor="bitplanes", loss="tukey", levels=4, **KF)
    ctx = hip.create_sequences(cams, p)
    m = MultiCam(ctx, 3)
    for k in range(3):
        m.call([0, 1, 2], [seqs[s][k] for s in range(3)])
    m.reset(0)
    ctx.seq_set_camera(0, new)
    got = ctx.seq_get_camera(0)
    assert (got.rows, got.cols) == (462, 616) and got.baseline == np.float32(0.14)
    for k in range(3, 8):
        m.call([2, 0, 1], [seqs[2][k], seq0_new[k - 3], seqs[1][k]])
    m.finish()
    # sequence 0: its first three frames with the first camera, then a fresh context of the new one
    first, first_t = run_single(hip, *cams[0][:2], 480, 640, p, seqs[0][:3])
    after, after_t = run_single(hip, new[0], new[1], 462, 616, p, seq0_new)
    for k, (a, b) in enumerate(zip(m.out[0], first + after)):
        assert_same_result(a, b, f"sequence 0 frame {k}")
    assert np.array_equal(m.trajs[0][0].view(np.uint32), first_t[0].view(np.uint32))
    assert np.array_equal(m.trajs[0][1].view(np.uint32), after_t[0].view(np.uint32))
    for s in (1, 2):
        assert_sequence_equal(m, s, *run_single(hip, *cams[s][:2], cams[s][2], cams[s][3], p, seqs[s]))
    ctx.close()


# ---- 5. errors -----------------------------------------------------------------------------------------------------------------------------
def test_camera_errors_leave_every_sequence_unchanged(hip):
    K, b = synth.calibration(ROWS, COLS)
    p = make_params(hip, descriptor="intensity", loss="huber", levels=4, **KF)
    seqs = frames_for([(K, b, ROWS, COLS)] * 2, 4)
    ctx = hip.create(K, b, ROWS, COLS, p, n_frames=6, n_pairs=2)
    m = MultiCam(ctx, 2)
    m.call([0], [seqs[0][0]])      # sequence 0 holds a frame, sequence 1 is fresh

    def refused(s, cam, code, *words):
        rc, msg = rc_and_error(ctx, "seq_set_camera", int(s), C.byref(capi.camera(*cam)))
        assert rc == code, (cam[2:], rc, msg)
        for w in words:
            assert w in msg, (w, msg)
        got = ctx.seq_get_camera(s)
        assert np.array_equal(np.array(got.K, np.float32), K.reshape(9)) and got.baseline == np.float32(b) and (got.rows, got.cols) == (ROWS, COLS)

    other = K_of(600, 600, 310, 235)
    refused(0, (other, 0.1, ROWS, COLS), ERR_INVALID_ARG, "sequence 0", "holds frames")
    refused(1, (other, 0.1, ROWS, 648), ERR_UNSUPPORTED, "larger", "648x480")
    refused(1, (other, 0.1, 40, 40), ERR_UNSUPPORTED, "smaller than 8 pixels")
    # 624x468: level 1 (312 x 234) falls under the NMS pixel count, a dense template of 73 008 points (73 728 in whole tiles) where the
    # context's NMS template holds 160 x 120 = 19 200 (20 480)
    refused(1, (other, 0.1, 468, 624), ERR_UNSUPPORTED, "level 1", "73728", "20480")
    nan = other.copy()
    nan[0, 2] = np.nan
    bad8 = other.copy()
    bad8[2, 2] = 2.0
    negf = other.copy()
    negf[1, 1] = -600.0
    refused(1, (nan, 0.1, ROWS, COLS), ERR_INVALID_ARG, "finite")
    refused(1, (bad8, 0.1, ROWS, COLS), ERR_INVALID_ARG, "K[8]")
    refused(1, (negf, 0.1, ROWS, COLS), ERR_INVALID_ARG, "fx and fy")
    refused(1, (other, 0.0, ROWS, COLS), ERR_INVALID_ARG, "baseline")
    refused(1, (other, -0.1, ROWS, COLS), ERR_INVALID_ARG, "baseline")
    # nothing changed: both sequences go on as contexts of their own
    for k in range(1, 4):
        m.call([1, 0], [seqs[1][k - 1], seqs[0][k]])
    m.call([1], [seqs[1][3]])
    m.finish()
    for s in range(2):
        assert_sequence_equal(m, s, *run_single(hip, K, b, ROWS, COLS, p, seqs[s]))
    ctx.close()

    # the automatic level count: 640x480 has 5 levels, 600x450 4
    pa = make_params(hip, descriptor="intensity", loss="huber", levels=0, **KF)
    auto = hip.create(K, b, ROWS, COLS, pa, n_frames=3, n_pairs=1)
    assert auto.L == 5
    rc, msg = rc_and_error(auto, "seq_set_camera", 0, C.byref(capi.camera(other, 0.1, 450, 600)))
    assert rc == ERR_UNSUPPORTED and "4 levels" in msg and "5" in msg, msg
    auto.close()
    cams = (capi.Camera * 2)(capi.camera(K, b, ROWS, COLS), capi.camera(other, 0.1, 450, 600))
    h = C.c_void_p()
    rc = hip.fn("create_sequences")(C.byref(h), 2, cams, C.byref(pa), 0)
    msg = hip.fn("last_error", C.c_char_p)(None).decode()
    assert rc == ERR_UNSUPPORTED and "sequence 1" in msg and "4 levels" in msg and "5" in msg, (rc, msg)
    cams = (capi.Camera * 1)(capi.camera(K, 0.0, ROWS, COLS))
    rc = hip.fn("create_sequences")(C.byref(h), 1, cams, C.byref(p), 0)
    assert rc == ERR_INVALID_ARG and "baseline" in hip.fn("last_error", C.c_char_p)(None).decode()

    # a context that runs add_frame takes no per-sequence camera, and its add_frame path is unaffected
    single = hip.create(K, b, ROWS, COLS, p, n_frames=3, n_pairs=1)
    r0 = single.add_frame(*seqs[0][0])
    rc, msg = rc_and_error(single, "seq_set_camera", 0, C.byref(capi.camera(K, b, ROWS, COLS)))
    assert rc == ERR_INVALID_ARG and "add_frame" in msg, msg
    r1 = single.add_frame(*seqs[0][1])
    cammed = hip.create(K, b, ROWS, COLS, p, n_frames=3, n_pairs=1)
    cammed.seq_set_camera(0, (other, 0.1, ROWS, COLS))      # ... and a context with a per-sequence camera serves add_frames only
    with pytest.raises(capi.BpvoError, match="add_frames"):
        cammed.add_frame(*seqs[0][0])
    cammed.close()
    ref, _ = run_single(hip, K, b, ROWS, COLS, p, seqs[0][:2])
    assert r0["isKeyFrame"] and np.array_equal(np.asarray(r1["pose"]).view(np.uint32), np.asarray(ref[1]["res"]["pose"]).view(np.uint32))
    single.close()
