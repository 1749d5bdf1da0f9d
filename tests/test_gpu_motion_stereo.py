"""Motion stereo on the device (c_api.h "motion stereo") against the numpy statement of the rule (tests/motion_stereo_ref.py), bit for bit: the
kernel alone through bpvo_hip_motion_stereo_frames; the addFrame drivers as "splat, motion stereo, update" replayed in numpy from what the calls
returned; the feature off; the refusals; the C++ facade.

The library serves cameras of at least 8 x 8 pixels, so the smallest shape here is 9 x 11, where the CPU test runs 5 x 7 and 1 x 1."""
import os
import subprocess

import numpy as np
import pytest

import disparity_fusion_ref as fref
import motion_stereo_ref as ref
from bpvo_amd import capi, synth
from util import bits_equal, make_params

pytestmark = pytest.mark.gpu
F32 = np.float32

FUSION = dict(mode=1, measurement_sigma=0.5, process_sigma=0.1, gate=3.0, max_fill_sigma=2.0)
FPRM = fref.rule(0.5, 0.1, 3.0, 2.0)
MS = ref.rule(2, 2, 0.25, 2.0, 0.02, 2.0, 3.0)
MS_B = ref.rule(1, 4, 0.5, 3.0, 0.05, 1.0, 2.5)      # a second sequence's own setting, unlike in every field
SHAPES = [(9, 11), (24, 40), (37, 53)]
SETTINGS = [(1, 1), (3, 8), (1, 8), (3, 1)]      # (radius, steps): both radii with both step counts
MOTIONS = ("sideways", "forward", "rotation", "general")


def _K(cam):
    return np.array([[cam["fx"], 0, cam["cx"]], [0, cam["fy"], cam["cy"]], [0, 0, 1]], F32)


def _capi_cam(cam):
    return (_K(cam), float(cam["b"]), cam["rows"], cam["cols"])


def _rule_ctx(hip, prm, lo=0.001, hi=64.0):
    """A context whose parameters carry the gate of the rule-alone calls, with the setting on."""
    cam = fref.camera(9, 11, lo=lo, hi=hi)
    p = make_params(hip, levels=1, minValidDisparity=float(lo), maxValidDisparity=float(hi))
    ctx = hip.create(_K(cam), float(cam["b"]), 9, 11, p, n_frames=3, n_pairs=1)
    ctx.set_motion_stereo(ref.setting(prm))
    return ctx


def _run_cases(ctx, prm, cases):
    """One call for all the cases (cam, C, K, Q, pd, pv): the three maps of each against numpy, and the counters of the call against numpy's."""
    l0, p0, t0, c0 = ctx.motion_stereo_counts()
    Ds, Vs, Cs = ctx.motion_stereo_frames([_capi_cam(c[0]) for c in cases], [c[1] for c in cases], [c[2] for c in cases], [c[3] for c in cases],
                                          [c[4] for c in cases], [c[5] for c in cases])
    l1, p1, t1, c1 = ctx.motion_stereo_counts()
    total = {k: 0 for k in ref.CLASSES}
    tiles = [0, 0, 0]
    for i, (cam, C, K, Q, pd, pv) in enumerate(cases):
        D, V, cls, counts = ref.refine(cam, prm, C, K, Q, pd, pv)
        assert ref.same_bits(Ds[i], D), (i, "D", np.argwhere(ref.bits(Ds[i]) != ref.bits(D))[:5])
        assert ref.same_bits(Vs[i], V), (i, "V", np.argwhere(ref.bits(Vs[i]) != ref.bits(V))[:5])
        assert np.array_equal(Cs[i], cls), (i, "class", np.argwhere(Cs[i] != cls)[:5])
        for k in ref.CLASSES:
            total[k] += counts[k]
        for k, v in enumerate(ref.tile_paths(cam, prm, Q, pd, pv)):
            tiles[k] += v
    assert l1 - l0 == 1 and p1 - p0 == sum(c[4].size for c in cases)      # ONE launch for the frames of unlike sizes
    assert {k: c1[k] - c0[k] for k in ref.CLASSES} == total, (c0, c1, total)
    assert tuple(b - a for a, b in zip(t0, t1)) == tuple(tiles), (t0, t1, tiles)
    return total, tuple(tiles)


# ---- 1. the rule alone -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius,steps", SETTINGS)
def test_rule_every_shape_and_motion_in_one_call(hip, radius, steps):
    """Twelve frames of three unlike sizes in one call: 9 x 11, 24 x 40 and 37 x 53 (more than one tile both ways, no multiple of the tile) under
    the four motions, with ref.hostile_prior's holes, NaN, values outside the gate and zero variances."""
    prm = ref.rule(radius, steps, 0.25, 2.0, 0.02, 2.0, 3.0)
    cases = [ref.rule_case(rows, cols, name) for rows, cols in SHAPES for name in MOTIONS]
    ctx = _rule_ctx(hip, prm)
    total, tiles = _run_cases(ctx, prm, cases)
    assert total["no_prior"] > 0 and total["low_parallax"] > 0 and total["border"] > 0
    if (radius, steps) == (1, 1):
        assert total["edge"] > 0 and total["fused"] > 0 and total["rejected"] > 0
    assert tiles[1] == 0      # (no image here is larger than the staged box)
    ctx.close()


def test_rule_rotation_only_is_all_low_parallax(hip):
    prm = ref.rule(2, 4, 0.25, 2.0, 0.02, 2.0, 3.0)
    cam, C, K, Q, pd, pv = ref.rule_case(37, 53, "rotation")
    pd, pv = np.full(pd.shape, 5.0, F32), np.full(pv.shape, 0.25, F32)
    ctx = _rule_ctx(hip, prm)
    total, tiles = _run_cases(ctx, prm, [(cam, C, K, Q, pd, pv)])
    assert total["low_parallax"] == 37 * 53 and tiles == (0, 0, 10)
    ctx.close()


@pytest.mark.parametrize("radius,steps", [(3, 8), (1, 8)])
def test_rule_a_quarter_turn_takes_both_tile_paths(hip, radius, steps):
    """72 x 96 under a quarter turn about the optical axis: a tile's row of 32 pixels becomes a column of the second image, taller than the box
    the kernel stages, so the tiles inside read the second image directly — the same integers; the tiles at the rim, where few lanes go on,
    still fit."""
    prm = ref.rule(radius, steps, 0.25, 2.0, 0.02, 2.0, 3.0)
    case = ref.rule_case(72, 96, "roll")
    ctx = _rule_ctx(hip, prm)
    total, tiles = _run_cases(ctx, prm, [case, ref.rule_case(24, 40, "general")])
    assert tiles[0] > 0 and tiles[1] > 0 and total["fused"] > 0, (tiles, total)
    ctx.close()


def test_rule_needs_the_setting_and_sane_cameras(hip):
    cam, C, K, Q, pd, pv = ref.rule_case(9, 11, "sideways")
    p = make_params(hip, levels=1)
    ctx = hip.create(_K(cam), float(cam["b"]), 9, 11, p, n_frames=3, n_pairs=1)
    with pytest.raises(capi.BpvoError, match="status -1:"):
        ctx.motion_stereo_frames([_capi_cam(cam)], [C], [K], [Q], [pd], [pv])      # mode 0
    ctx.set_motion_stereo(ref.setting(MS))
    with pytest.raises(capi.BpvoError, match="status -1:"):
        ctx.motion_stereo_frames([(_K(cam), 0.0, 9, 11)], [C], [K], [Q], [pd], [pv])      # no baseline
    assert ctx.motion_stereo_counts()[0] == 0
    ctx.close()


# ---- 2. the drivers: splat, motion stereo, update ----------------------------------------------------------------------------------------------
FRAMES = 8
# Images this small see synth's plane (10 m away) with a parallax of a fraction of a pixel per frame under synth's own calibration and steps,
# and the search needs `steps` pixels of it: the sequences are rendered with a longer focal length and steps of up to 0.15 m (24 x 40) and
# 0.08 m (48 x 64), which move the plane's image by a few pixels per frame.  The estimates on such images are poor; what is compared is the
# library against the numpy replay from the poses it returned, bit for bit.  Key frames from the translation alone; the sequences and
# thresholds are those at which both key-frame branches occur and pixels are fused (found by running them) — the tests assert that they did.
VO_KW = dict(loss="huber", levels=2, minRotationMagToKeyFrame=100.0, maxFractionOfGoodPointsToKeyFrame=0.0)
# rows, cols, the (first) sequence's index, minTranslationMagToKeyFrame
SINGLE_CASES = [(24, 40, 1, 0.2), (48, 64, 2, 0.15)]
DRIVER_CASES = [(24, 40, 0, 0.2), (48, 64, 0, 0.15)]
STEREO_CASES = [(24, 40, 2, 0.1), (48, 64, 2, 0.1)]
FOCAL = {(24, 40): 150.0, (48, 64): 200.0}
STEP_TRANS = {(24, 40): 0.15, (48, 64): 0.08}


def _sequence(rows, cols, n_frames, index, stereo=False):
    fx = FOCAL[(rows, cols)]
    camera = (np.array([[fx, 0, cols / 2.0], [0, fx, rows / 2.0], [0, 0, 1]], F32), 0.1)
    make = synth.make_stereo_sequence if stereo else synth.make_sequence
    return make(rows, cols, n_frames, index=index, step_trans=STEP_TRANS[(rows, cols)], camera=camera)


def _cam_of(seq, rows, cols, p):
    K = np.asarray(seq["K"], F32)
    return fref.camera(rows, cols, fx=K[0, 0], fy=K[1, 1], cx=K[0, 2], cy=K[1, 2], b=seq["b"], lo=p.minValidDisparity, hi=p.maxValidDisparity)


class Replay:
    """One sequence's numpy replay: the carried maps, and which frame is the key frame of the call's last estimate (the state machine of
    vo_state.h followed from the results: a key frame with re-estimation makes the PREVIOUS frame the key frame, a plain one the current)."""

    def __init__(self, cam, ms, fprm=FPRM):
        self.cam, self.ms, self.fprm = cam, ms, fprm
        self.D = self.V = None
        self.images, self.key, self.T_key = [], 0, np.eye(4)
        self.branches, self.classes = set(), {k: 0 for k in ref.CLASSES}

    def step(self, img, M, res, reest, info):
        """The call's frame: returns the numpy (D, V, fusion counts).  info: the sequence's motion-stereo record (None: the feature is off)."""
        f = len(self.images)
        self.images.append(img)
        cam = self.cam
        if f == 0:
            z = np.zeros((cam["rows"], cam["cols"]), np.uint64)
            assert info is None or not info["launched"]
        else:
            z = fref.splat(cam, self.fprm, self.D, self.V, res["pose"])
            pose = np.asarray(res["pose"], np.float64)
            if res["isKeyFrame"] and reest:
                view, T = f - 1, pose      # the new key frame is the previous frame: the estimate against it is the frame's motion
                self.branches.add("reest")
            else:
                view, T = self.key, pose @ self.T_key
                if res["isKeyFrame"]:
                    self.branches.add("plain")
            if info is not None:
                assert info["launched"] == 1
                Q = info["motion"]      # the library's f32 inverse of its estimate: its bits are the rule's input, its value is checked here
                assert np.allclose(Q.astype(np.float64) @ T, np.eye(4), atol=2e-4), (f, Q, T)
                z, _, counts = ref.refine_words(cam, self.ms, img, self.images[view], Q, z)
                assert {k: info[k] for k in ref.CLASSES} == counts, (f, info, counts)
                for k in ref.CLASSES:
                    self.classes[k] += counts[k]
            # the key frame of the NEXT call's first estimate, and the motion from it to this frame
            if res["isKeyFrame"]:
                self.key, self.T_key = (f - 1, pose) if reest else (f, np.eye(4))
            else:
                self.T_key = T
        self.D, self.V, counts = fref.update(cam, self.fprm, M, z)
        return self.D, self.V, counts


def _assert_maps(got_D, got_V, want_D, want_V, what):
    assert ref.same_bits(got_D, want_D), (what, "D", np.argwhere(ref.bits(got_D) != ref.bits(want_D))[:5])
    assert ref.same_bits(got_V, want_V), (what, "V", np.argwhere(ref.bits(got_V) != ref.bits(want_V))[:5])


def _same_results(ra, rb, what):
    assert bits_equal(ra["pose"], rb["pose"]) and ra["stats"] == rb["stats"], (what, ra["stats"], rb["stats"])
    assert ra["isKeyFrame"] == rb["isKeyFrame"] and ra["keyFramingReason"] == rb["keyFramingReason"] and ra["hasPointCloud"] == rb["hasPointCloud"], what


@pytest.mark.parametrize("rows,cols,index,thr", SINGLE_CASES)
def test_add_frame_is_splat_motion_stereo_update(hip, rows, cols, index, thr):
    seq = _sequence(rows, cols, FRAMES, index)
    p = make_params(hip, descriptor="bitplanes", minTranslationMagToKeyFrame=thr, **VO_KW)
    cam = _cam_of(seq, rows, cols, p)
    A = hip.create(seq["K"], seq["b"], rows, cols, p, n_frames=3, n_pairs=1)
    B = hip.create(seq["K"], seq["b"], rows, cols, p, n_frames=3, n_pairs=1)
    A.set_disparity_fusion(FUSION)
    A.set_motion_stereo(ref.setting(MS))
    rp = Replay(cam, MS)
    for f, (img, M) in enumerate(seq["frames"]):
        ra = A.add_frame(img, M)
        D, V, counts = rp.step(img, M, ra, A.vo_start_info(1)["n_candidates"] > 0, A.vo_motion_stereo_info())
        Da, Va = A.vo_get_fused_disparity()
        _assert_maps(Da, Va, D, V, f)
        finfo = A.vo_disparity_fusion_info()
        assert {k: finfo[k] for k in fref.CLASSES} == counts and ref.same_bits(A.get_disparity(finfo["slot"]), D), f
        _same_results(ra, B.add_frame(img, D), f)      # a context in mode 0 fed the fused maps returns the same results
    assert bits_equal(A.trajectory(), B.trajectory())
    assert rp.branches == {"reest", "plain"}, rp.branches
    assert A.motion_stereo_counts()[0] == FRAMES - 1 and B.motion_stereo_counts()[0] == 0
    assert rp.classes["fused"] > 0, rp.classes
    A.close(); B.close()


@pytest.mark.parametrize("rows,cols,index,thr", DRIVER_CASES)
def test_add_frames_three_sequences_one_off_two_on_with_unlike_settings(hip, rows, cols, index, thr):
    seqs = [_sequence(rows, cols, FRAMES, index + i) for i in range(3)]
    p = make_params(hip, descriptor="bitplanes", minTranslationMagToKeyFrame=thr, **VO_KW)
    cams = [_cam_of(s, rows, cols, p) for s in seqs]
    A = hip.create(seqs[0]["K"], seqs[0]["b"], rows, cols, p, n_frames=9, n_pairs=3)
    B = hip.create(seqs[0]["K"], seqs[0]["b"], rows, cols, p, n_frames=9, n_pairs=3)
    A.set_disparity_fusion(FUSION)
    A.seq_set_motion_stereo(1, ref.setting(MS))
    A.seq_set_motion_stereo(2, ref.setting(MS_B))
    settings = [None, MS, MS_B]
    rps = [Replay(cams[s], settings[s]) for s in range(3)]
    launches = 0
    for f in range(FRAMES):
        imgs = np.stack([s["frames"][f][0] for s in seqs])
        Ms = [s["frames"][f][1] for s in seqs]
        ra = A.add_frames(imgs, np.stack(Ms))
        fused = []
        for s in range(3):
            info = A.seq_motion_stereo_info(s)
            if settings[s] is None:
                assert not info["launched"] and all(info[k] == 0 for k in ref.CLASSES)
            D, V, counts = rps[s].step(imgs[s], Ms[s], ra[s], A.seq_start_info(s, 1)["n_candidates"] > 0, info if settings[s] is not None else None)
            Da, Va = A.seq_get_fused_disparity(s)
            _assert_maps(Da, Va, D, V, (f, s))
            fused.append(D)
        rb = B.add_frames(imgs, np.stack(fused))
        for s in range(3):
            _same_results(ra[s], rb[s], (f, s))
    for s in range(3):
        assert bits_equal(A.seq_trajectory(s), B.seq_trajectory(s))
    seen = set().union(*(rp.branches for rp in rps[1:]))
    assert seen == {"reest", "plain"}, [rp.branches for rp in rps]
    assert rps[1].classes["fused"] + rps[2].classes["fused"] > 0, [rp.classes for rp in rps]
    # at most two fusion stages per call (in front of the key frames' templates, and at the end): one launch each where a sequence with the
    # feature on predicts
    launches = A.motion_stereo_counts()[0]
    assert FRAMES - 1 <= launches <= 2 * (FRAMES - 1) and B.motion_stereo_counts()[0] == 0
    A.close(); B.close()


@pytest.mark.parametrize("driver", ["add_frames_stereo", "add_frame_stereo"])
@pytest.mark.parametrize("rows,cols,index,thr", STEREO_CASES)
def test_the_stereo_drivers_are_splat_motion_stereo_update(hip, rows, cols, index, thr, driver):
    """Block matching (16 disparities) serves both sizes: the measured map is the front-end's own, taken from a call of its own.  The batched
    driver and the single-sequence driver take both key-frame branches on these sequences."""
    single = driver == "add_frame_stereo"
    seq = _sequence(rows, cols, FRAMES, index, stereo=True)
    p = make_params(hip, descriptor="bitplanes", minTranslationMagToKeyFrame=thr, **VO_KW)
    cam = _cam_of(seq, rows, cols, p)
    A = hip.create(seq["K"], seq["b"], rows, cols, p, n_frames=3, n_pairs=1)
    B = hip.create(seq["K"], seq["b"], rows, cols, p, n_frames=3, n_pairs=1)
    A.set_disparity_fusion(FUSION)
    A.set_motion_stereo(ref.setting(MS))
    sp = A.default_stereo_params(ndisp=16)
    rp = Replay(cam, MS)
    pattern = ""
    for f, (left, right) in enumerate(seq["frames"]):
        M = B.stereo_frames([(rows, cols)], [left], [right], sp)[0]
        if single:
            ra = A.add_frame_stereo(left, right, sp)
            reest, info, (Da, Va) = A.vo_start_info(1)["n_candidates"] > 0, A.vo_motion_stereo_info(), A.vo_get_fused_disparity()
        else:
            ra = A.add_frames_stereo([left], [right], sp)[0]
            reest, info, (Da, Va) = A.seq_start_info(0, 1)["n_candidates"] > 0, A.seq_motion_stereo_info(0), A.seq_get_fused_disparity(0)
        D, V, counts = rp.step(left, M, ra, reest, info)
        _assert_maps(Da, Va, D, V, f)
        _same_results(ra, B.add_frames([left], [D])[0], f)
        pattern += "F" if f == 0 else ("R" if ra["isKeyFrame"] and reest else "P" if ra["isKeyFrame"] else ".")
    assert bits_equal(A.trajectory() if single else A.seq_trajectory(0), B.seq_trajectory(0))
    assert rp.branches == {"reest", "plain"} and rp.classes["fused"] > 0, (pattern, rp.classes)
    assert FRAMES - 1 <= A.motion_stereo_counts()[0] <= 2 * (FRAMES - 1)
    A.close(); B.close()


def test_a_word_without_a_candidate_stays_empty_and_a_first_frame_launches_nothing(hip):
    """Holes in the measured maps of every frame: where no candidate arrives the pixel is "none" or "measured", as without the feature."""
    rows, cols, index, thr = DRIVER_CASES[0]
    seq = _sequence(rows, cols, 3, index)
    p = make_params(hip, descriptor="bitplanes", minTranslationMagToKeyFrame=thr, **VO_KW)
    cam = _cam_of(seq, rows, cols, p)
    A = hip.create(seq["K"], seq["b"], rows, cols, p, n_frames=3, n_pairs=1)
    A.set_disparity_fusion(dict(FUSION, max_fill_sigma=0.0))
    A.set_motion_stereo(ref.setting(MS))
    rp = Replay(cam, MS, fref.rule(0.5, 0.1, 3.0, 0.0))
    for f, (img, M) in enumerate(seq["frames"]):
        M = M.copy()
        M[::3, ::2] = -1.0
        ra = A.add_frame(img, M)
        info = A.vo_motion_stereo_info()
        D, V, counts = rp.step(img, M, ra, A.vo_start_info(1)["n_candidates"] > 0, info)
        _assert_maps(*A.vo_get_fused_disparity(), D, V, f)
        if f == 0:
            assert not info["launched"] and A.motion_stereo_counts()[0] == 0
        else:
            assert info["no_prior"] > 0
    A.close()


# ---- 3. the feature off ------------------------------------------------------------------------------------------------------------------------
def test_mode_0_is_the_fusion_only_run(hip):
    rows, cols, index, thr = DRIVER_CASES[0]
    seq = _sequence(rows, cols, 4, index)
    p = make_params(hip, descriptor="bitplanes", minTranslationMagToKeyFrame=thr, **VO_KW)
    live0 = hip.debug_live_resources()
    plain = hip.create(seq["K"], seq["b"], rows, cols, p, n_frames=3, n_pairs=1)
    plain.set_disparity_fusion(FUSION)
    want = []
    for img, M in seq["frames"]:
        r = plain.add_frames([img], [M])[0]
        want.append((r, plain.seq_get_fused_disparity(0)))
    live_plain = hip.debug_live_resources()
    off = hip.create(seq["K"], seq["b"], rows, cols, p, n_frames=3, n_pairs=1)
    off.set_disparity_fusion(FUSION)
    off.set_motion_stereo(dict(ref.setting(MS), mode=0))
    off.seq_set_motion_stereo(0, dict(mode=0))
    for (img, M), (ra, (D, V)) in zip(seq["frames"], want):
        _same_results(ra, off.add_frames([img], [M])[0], "mode 0")
        _assert_maps(*off.seq_get_fused_disparity(0), D, V, "mode 0")
    assert bits_equal(plain.seq_trajectory(0), off.seq_trajectory(0))
    assert off.motion_stereo_counts() == (0, 0, (0, 0, 0), {k: 0 for k in ref.CLASSES})
    info = off.seq_motion_stereo_info(0)
    assert not info["launched"] and all(info[k] == 0 for k in ref.CLASSES)
    live_both = hip.debug_live_resources()
    assert tuple(b - a for a, b in zip(live_plain, live_both)) == tuple(b - a for a, b in zip(live0, live_plain))      # mode 0 holds what the fusion-only context holds
    # motion stereo on and fusion off: nothing runs either
    alone = hip.create(seq["K"], seq["b"], rows, cols, p, n_frames=3, n_pairs=1)
    alone.set_motion_stereo(ref.setting(MS))
    for img, M in seq["frames"]:
        alone.add_frames([img], [M])
    assert alone.motion_stereo_counts()[0] == 0
    plain.close(); off.close(); alone.close()
    assert hip.debug_live_resources() == live0


# ---- 4. refusals -------------------------------------------------------------------------------------------------------------------------------
BAD = [(dict(radius=0), "radius"), (dict(radius=4), "radius"), (dict(steps=0), "steps"), (dict(steps=9), "steps"), (dict(min_gain=0.0), "min_gain"),
       (dict(min_gain=np.nan), "min_gain"), (dict(noise_sigma=0.0), "noise_sigma"), (dict(noise_sigma=np.inf), "noise_sigma"), (dict(min_sigma=0.0), "min_sigma"),
       (dict(min_sigma=3.0), "max_sigma"), (dict(max_sigma=np.inf), "max_sigma"), (dict(gate=0.0), "gate"), (dict(gate=np.nan), "gate"), (dict(mode=2), "mode"),
       (dict(mode=-1), "mode")]


@pytest.mark.parametrize("bad,field", BAD)
def test_invalid_parameters_are_refused_by_name_and_nothing_changes(hip, bad, field):
    cam = fref.camera(9, 11)
    p = make_params(hip, levels=1)
    ctx = hip.create_sequences([_capi_cam(cam), _capi_cam(cam)], p)
    ctx.seq_set_motion_stereo(1, ref.setting(MS))
    before = ctx.get_motion_stereo(), ctx.seq_get_motion_stereo(0), ctx.seq_get_motion_stereo(1)
    for call in (lambda: ctx.set_motion_stereo(dict(ref.setting(MS), **bad)), lambda: ctx.seq_set_motion_stereo(1, dict(ref.setting(MS), **bad))):
        with pytest.raises(capi.BpvoError, match="status -1:.*motion stereo: .*" + field):      # BPVO_ERR_INVALID_ARG, and the field by name
            call()
    assert (ctx.get_motion_stereo(), ctx.seq_get_motion_stereo(0), ctx.seq_get_motion_stereo(1)) == before
    assert before[0]["mode"] == 0 and before[1] == (before[0], False) and before[2][1] and before[2][0]["mode"] == 1
    ctx.seq_set_motion_stereo(1, None)
    assert ctx.seq_get_motion_stereo(1) == (before[0], False)
    ctx.close()


def test_rig_contexts_refuse_mode_1(hip):
    cam = fref.camera(33, 65)
    p = make_params(hip, levels=1)
    ctx = hip.create_sequences([_capi_cam(cam), _capi_cam(cam)], p)
    X = np.stack([np.eye(4, dtype=F32)] * 2)
    ctx.rig_set(X)
    for call in (lambda: ctx.set_motion_stereo(ref.setting(MS)), lambda: ctx.seq_set_motion_stereo(0, ref.setting(MS))):
        with pytest.raises(capi.BpvoError, match="status -2:.*motion stereo"):      # BPVO_ERR_UNSUPPORTED, the cause in the message
            call()
    assert ctx.get_motion_stereo()["mode"] == 0 and ctx.seq_get_motion_stereo(0) == (ctx.get_motion_stereo(), False)
    ctx.set_motion_stereo(dict(mode=0))      # mode 0 is what the context runs anyway
    ctx.close()
    other = hip.create_sequences([_capi_cam(cam), _capi_cam(cam)], p)
    other.set_motion_stereo(ref.setting(MS))
    with pytest.raises(capi.BpvoError, match="status -2:.*motion stereo"):
        other.rig_set(X)      # ... and a context in mode 1 declares no rig
    other.close()


# ---- 5. the C++ facade -------------------------------------------------------------------------------------------------------------------------
def test_set_motion_stereo_through_the_facade(hip, tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, "bpvo_amd", "csrc")
    exe = str(tmp_path / "motion_stereo_facade")
    r = subprocess.run(["g++", "-std=c++11", "-O2", "-I", os.path.join(root, "include"), os.path.join(root, "tests", "cpp", "motion_stereo_facade.cc"),
                        "-o", exe, "-L", csrc, "-lbpvo_hip", f"-Wl,-rpath,{csrc}"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    rows, cols, n_frames = 48, 64, 4
    seq = _sequence(rows, cols, n_frames, 0)
    for k, (img, M) in enumerate(seq["frames"]):
        img.tofile(tmp_path / f"img_{k}.u8")
        M.astype(F32).tofile(tmp_path / f"disp_{k}.f32")
    K = seq["K"]
    s = ref.setting(MS)
    r = subprocess.run([exe, str(tmp_path), str(rows), str(cols), repr(float(K[0, 0])), repr(float(K[1, 1])), repr(float(K[0, 2])), repr(float(K[1, 2])),
                        repr(float(seq["b"])), str(n_frames), "0.5", "0.1", "3.0", "2.0", str(s["radius"]), str(s["steps"]), repr(s["min_gain"]),
                        repr(s["noise_sigma"]), repr(s["min_sigma"]), repr(s["max_sigma"]), repr(s["gate"])], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    poses = np.fromfile(tmp_path / "poses.bin", F32).reshape(n_frames, 4, 4)
    poses_seq = np.fromfile(tmp_path / "poses_seq.bin", F32).reshape(n_frames, 2, 4, 4)
    lines = [[int(v) for v in line.split()] for line in r.stdout.strip().splitlines()]
    # the same through the ctypes binding, with the facade's parameters (the defaults but two levels, bit-planes, Huber)
    p = make_params(hip, descriptor="bitplanes", loss="huber", levels=2)
    one = hip.create(K, seq["b"], rows, cols, p, n_frames=3, n_pairs=1)
    one.set_disparity_fusion(FUSION)
    one.set_motion_stereo(s)
    two = hip.create(K, seq["b"], rows, cols, p, n_frames=6, n_pairs=2)
    two.set_disparity_fusion(FUSION)
    two.seq_set_motion_stereo(1, s)
    for k, (img, M) in enumerate(seq["frames"]):
        assert bits_equal(one.add_frame(img, M)["pose"], poses[k]), k
        info = one.vo_motion_stereo_info()
        assert lines[k] == [info[c] for c in ref.CLASSES] + [int(info["launched"])], k
        res = two.add_frames(np.stack([img, img]), np.stack([M, M]))
        assert bits_equal(res[0]["pose"], poses_seq[k, 0]) and bits_equal(res[1]["pose"], poses_seq[k, 1]), k
    one.close(); two.close()
