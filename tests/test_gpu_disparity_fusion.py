"""Disparity fusion on the device (c_api.h "disparity fusion") against the numpy statement of the rule (tests/disparity_fusion_ref.py), bit for bit:
the kernels through bpvo_hip_fuse_disparities with exact motions; order-freedom; the VO as "the filter plus today's VO" on every driver; the edges.

The library serves cameras of at least 8 x 8 pixels (a rule older than this feature: every pyramid level has at least 8 rows and columns), so the
smallest shape here is 9 x 11 — 99 pixels, odd, no multiple of the splat's four pixels per lane — where the CPU test runs 5 x 7 and 1 x 1, and the
1 x 8 collision case is run as 8 equal rows."""
import numpy as np
import pytest

import disparity_fusion_ref as ref
from bpvo_amd import capi, synth
from util import bits_equal, make_params

pytestmark = pytest.mark.gpu
F32 = np.float32

FUSION = dict(mode=1, measurement_sigma=0.5, process_sigma=0.1, gate=3.0, max_fill_sigma=2.0)
PRM = ref.rule(0.5, 0.1, 3.0, 2.0)


def _K(cam):
    return np.array([[cam["fx"], 0, cam["cx"]], [0, cam["fy"], cam["cy"]], [0, 0, 1]], F32)


def _ctx(hip, cams, fusion=FUSION, **kw):
    """A context of len(cams) sequences, sequence s with the camera cams[s] (a ref.camera) and its gate, one pyramid level."""
    p = make_params(hip, levels=1, minValidDisparity=float(cams[0]["lo"]), maxValidDisparity=float(cams[0]["hi"]), **kw)
    ctx = hip.create_sequences([(_K(c), float(c["b"]), c["rows"], c["cols"]) for c in cams], p)
    if fusion is not None:
        ctx.set_disparity_fusion(fusion)
    return ctx


def _state(ctx, s, cam):
    D, V = ctx.seq_get_fused_disparity(s)
    info = ctx.seq_disparity_fusion_info(s)
    return D, V, info, ctx.get_disparity(info["slot"], (cam["rows"], cam["cols"]))


def _assert_step(got, want, M, what):
    D, V, info, slot = got
    rD, rV, rcounts = want
    assert ref.same_bits(D, rD), (what, "D", np.argwhere(ref.bits(D) != ref.bits(rD))[:5])
    assert ref.same_bits(V, rV), (what, "V", np.argwhere(ref.bits(V) != ref.bits(rV))[:5])
    assert ref.same_bits(slot, rD), (what, "slot")
    assert {k: info[k] for k in ref.CLASSES} == rcounts, (what, info, rcounts)


def _chain(ctx, cams, prms, steps, seq=None):
    """steps[k] = ([M per sequence], [P per sequence]): every step against the numpy statement; returns the final (D, V) per sequence."""
    ids = list(range(len(cams))) if seq is None else list(seq)
    carried = [(None, None)] * len(cams)
    for k, (Ms, Ps) in enumerate(steps):
        ctx.fuse_disparities(Ms, Ps, seq=seq)
        for i, s in enumerate(ids):
            want = ref.step(cams[i], prms[i], Ms[i], carried[i][0], carried[i][1], None if k == 0 else Ps[i])
            got = _state(ctx, s, cams[i])
            _assert_step(got, want, Ms[i], (k, s))
            assert got[2]["predicted"] == (k > 0) and bits_equal(got[2]["motion"], np.asarray(Ps[i], F32))
            carried[i] = (want[0], want[1])
    return carried


SHAPES = [(9, 11), (33, 65), (120, 160)]


# ---- 1. the rule -----------------------------------------------------------------------------------------------------------------------------
def test_rule_three_chained_steps_three_unlike_cameras_in_one_call(hip):
    cases = [ref.chain_case(r, c, seed=c) for r, c in SHAPES]
    cams = [c[0] for c in cases]
    steps = [([c[1][k] for c in cases], [c[2][k] for c in cases]) for k in range(3)]
    steps[2][0][1] = ref.hostile_measurement(cams[1], seed=3)      # the hostile values, on carried maps two steps old
    ctx = _ctx(hip, cams)
    launches0, _ = ctx.disparity_fusion_counts()
    final = _chain(ctx, cams, [PRM] * 3, steps)
    launches, pixels = ctx.disparity_fusion_counts()
    assert launches0 == 0 and launches == 1 + 2 + 2 and pixels == 3 * sum(r * c for r, c in SHAPES)      # one launch per stage for all sequences
    M = steps[2][0][1]
    D, V = final[1]
    untouched = V == -1
    assert untouched.any() and np.array_equal(ref.bits(D)[untouched], ref.bits(M)[untouched])      # the caller's bits, NaN payloads too
    with np.errstate(invalid="ignore"):
        for (D, V), cam, Ms in zip(final, cams, steps[2][0]):
            assert np.all(ref.valid(D, cam["lo"], cam["hi"])[ref.valid(Ms, cam["lo"], cam["hi"])])      # wherever M is valid the output is valid
    ctx.close()


def test_rule_collision_and_ties(hip):
    """The collision case as 8 equal rows.  The carried variances a device context can hold come from its own steps: a first frame (V = r2), then
    an identity step that fuses every pixel but source 1, which it fills (V stays r2, the others halve) — so the two sources that tie at target 2
    with equal d' carry unlike variances, and the larger must win."""
    cam, Dc, Vc, P, M = ref.collision_case(rows=8)
    prm = ref.rule(0.5, 0.0, 3.0, 2.0)
    M0 = np.where(Vc >= 0, Dc, F32(-1)).astype(F32)
    M1 = M0.copy()
    M1[:, 1] = -1
    ctx = _ctx(hip, [cam], dict(FUSION, process_sigma=0.0))
    (D, V), = _chain(ctx, [cam], [prm], [([M0], [ref.motion()]), ([M1], [ref.motion()])])
    assert np.all(V[:, 0] == 0.125) and np.all(V[:, 1] == 0.25) and np.all(D[:, :2] == 2.0)
    z = ref.splat(cam, prm, D, V, P)
    assert np.all(z[:, 2] == (int(ref.bits([F32(2.0)])[0]) << 32 | int(ref.bits([F32(0.25)])[0])))      # ties to even, then the larger variance
    assert np.all(z[:, 7] >> np.uint64(32) == int(ref.bits([F32(4.0)])[0])) and np.count_nonzero(z) == 2 * 8      # the nearer surface
    ctx.fuse_disparities([M], [P])
    want = ref.step(cam, prm, M, D, V, P)
    _assert_step(_state(ctx, 0, cam), want, M, "collision")
    assert want[2] == dict(fused=8, replaced=8, measured=24, filled=0, none=24)
    ctx.close()


def test_rule_edges_of_the_gate_the_bound_and_the_fill(hip):
    """ref.edge_case's carried variances cannot be put into a device context from outside; its measurements at the gate's ends and the NaN can: the
    gate is inclusive on the device too (the comparison with the numpy statement), and a non-finite motion predicts nothing."""
    cam = ref.camera(9, 11, lo=1.0, hi=64.0)
    M0 = np.full((9, 11), 4.0, F32)
    M0[0, :6] = [1.0, np.nextafter(F32(1.0), F32(0.0)), 64.0, np.nextafter(F32(64.0), F32(65.0)), np.nan, -np.inf]
    M1 = np.roll(M0, 3, axis=1)
    Pn = ref.motion()
    Pn[2, 3] = np.nan
    ctx = _ctx(hip, [cam])
    ctx.fuse_disparities([M0], [ref.motion()])
    first = ref.step(cam, PRM, M0)
    _assert_step(_state(ctx, 0, cam), first, M0, "first")
    assert first[2]["measured"] == 99 - 4 and first[2]["none"] == 4
    ctx.fuse_disparities([M1], [Pn])
    _assert_step(_state(ctx, 0, cam), ref.step(cam, PRM, M1), M1, "nan motion")
    assert not ctx.seq_disparity_fusion_info(0)["predicted"]
    ctx.close()


# ---- 2. order-freedom ------------------------------------------------------------------------------------------------------------------------
def test_a_sequence_alone_and_among_five_and_the_same_call_twice(hip):
    shapes = [(33, 65), (120, 160), (120, 160), (9, 11), (33, 65)]
    cases = [ref.chain_case(r, c, seed=10 + i) for i, (r, c) in enumerate(shapes)]
    cams = [c[0] for c in cases]
    steps = [([c[1][k] for c in cases], [c[2][k] for c in cases]) for k in range(3)]
    finals = []
    for _ in range(2):      # the same calls on two fresh contexts
        ctx = _ctx(hip, cams)
        for Ms, Ps in steps:
            ctx.fuse_disparities(Ms, Ps)
        finals.append([ctx.seq_get_fused_disparity(s) for s in range(5)])
        ctx.close()
    for (Da, Va), (Db, Vb) in zip(*finals):
        assert ref.same_bits(Da, Db) and ref.same_bits(Va, Vb)
    alone = _ctx(hip, cams)
    for Ms, Ps in steps:
        alone.fuse_disparities([Ms[2]], [Ps[2]], seq=[2])
    D, V = alone.seq_get_fused_disparity(2)
    assert ref.same_bits(D, finals[0][2][0]) and ref.same_bits(V, finals[0][2][1])
    assert alone.seq_disparity_fusion_info(3)["measured"] == 0      # (a sequence no call named has fused nothing)
    alone.close()


# ---- 3. the VO is the filter plus today's VO ---------------------------------------------------------------------------------------------------
ROWS, COLS, FRAMES = 120, 160, 6
# key frames from the translation alone; 0.035 m: on these sequences both key-frame branches occur (found with the CPU oracle: the plane sequence
# runs first . reest plain . reest, the layered one first . . reest plain .) — the tests assert that they did
VO_KW = dict(loss="huber", levels=3, minTranslationMagToKeyFrame=0.035, minRotationMagToKeyFrame=100.0, maxFractionOfGoodPointsToKeyFrame=0.0)
SEQS = dict(bitplanes=[("plane", 0), ("layered", 2)], intensity=[("layered", 2)])


def _cam_of(seq, p):
    K = np.asarray(seq["K"], F32)
    return ref.camera(ROWS, COLS, fx=K[0, 0], fy=K[1, 1], cx=K[0, 2], cy=K[1, 2], b=seq["b"], lo=p.minValidDisparity, hi=p.maxValidDisparity)


def _same_results(ra, rb, what):
    assert bits_equal(ra["pose"], rb["pose"]) and ra["stats"] == rb["stats"], (what, ra["stats"], rb["stats"])
    assert ra["isKeyFrame"] == rb["isKeyFrame"] and ra["keyFramingReason"] == rb["keyFramingReason"] and ra["hasPointCloud"] == rb["hasPointCloud"], what


def _same_cloud(a, b, what):
    (pa, Pa), (pb, Pb) = a, b
    assert all(bits_equal(pa[k], pb[k]) for k in ("xyzw", "rgba", "weight")) and bits_equal(Pa, Pb), what


def _branches(results, reest):
    """The key-frame branches a sequence took: {"reest", "plain"}; reest[k]: the second estimate of call k ran (its start record exists)."""
    seen = set()
    for k, r in enumerate(results):
        if k > 0 and r["isKeyFrame"]:
            seen.add("reest" if reest[k] else "plain")
        else:
            assert not reest[k]
    return seen


@pytest.mark.parametrize("descriptor", sorted(SEQS))
def test_add_frames_is_the_filter_plus_todays_vo(hip, descriptor):
    seqs = [synth.make_sequence(ROWS, COLS, FRAMES, index=i, scene=scene) for scene, i in SEQS[descriptor]]
    n = len(seqs)
    p = make_params(hip, descriptor=descriptor, **VO_KW)
    cams = [_cam_of(s, p) for s in seqs]
    A = hip.create(seqs[0]["K"], seqs[0]["b"], ROWS, COLS, p, n_frames=3 * n, n_pairs=n)
    B = hip.create(seqs[0]["K"], seqs[0]["b"], ROWS, COLS, p, n_frames=3 * n, n_pairs=n)
    A.set_disparity_fusion(FUSION)
    carried = [(None, None)] * n
    results, reest, filled = [[] for _ in range(n)], [[] for _ in range(n)], 0
    for f in range(FRAMES):
        imgs = np.stack([s["frames"][f][0] for s in seqs])
        Ms = [s["frames"][f][1] for s in seqs]
        ra = A.add_frames(imgs, np.stack(Ms))
        fusedD = []
        for s in range(n):
            # (i) the carried maps: the numpy statement on the previous ones, the call's measured map and the pose the call returned
            want = ref.step(cams[s], PRM, Ms[s], carried[s][0], carried[s][1], None if f == 0 else ra[s]["pose"])
            got = _state(A, s, cams[s])
            _assert_step(got, want, Ms[s], (f, s))
            assert bits_equal(got[2]["motion"], ra[s]["pose"] if f else np.eye(4, dtype=F32))
            carried[s] = want[:2]
            fusedD.append(want[0])
            filled += want[2]["filled"]
            results[s].append(ra[s])
            reest[s].append(A.seq_start_info(s, 1)["n_candidates"] > 0)
        # (ii) a context in mode 0 fed A's carried disparity returns A's results
        rb = B.add_frames(imgs, np.stack(fusedD))
        for s in range(n):
            _same_results(ra[s], rb[s], (f, s))
            for level in range(A.L):
                assert A.seq_num_points_at_level(s, level) == B.seq_num_points_at_level(s, level), (f, s, level)
            if ra[s]["hasPointCloud"]:
                _same_cloud(A.seq_point_cloud(s), B.seq_point_cloud(s), (f, s))
    for s in range(n):
        assert bits_equal(A.seq_trajectory(s), B.seq_trajectory(s))
        assert _branches(results[s], reest[s]) == {"reest", "plain"}, (s, [r["isKeyFrame"] for r in results[s]], reest[s])
    if descriptor == "bitplanes":
        assert filled > 0      # (the layered sequence's holes, filled by prediction; the parameters' default gate)
    assert B.disparity_fusion_counts() == (0, 0)
    A.close(); B.close()


def test_add_frame_is_the_filter_plus_todays_vo(hip):
    seq = synth.make_sequence(ROWS, COLS, FRAMES, index=2, scene="layered")
    p = make_params(hip, descriptor="bitplanes", **VO_KW)
    cam = _cam_of(seq, p)
    A = hip.create(seq["K"], seq["b"], ROWS, COLS, p, n_frames=3, n_pairs=1)
    B = hip.create(seq["K"], seq["b"], ROWS, COLS, p, n_frames=3, n_pairs=1)
    A.set_disparity_fusion(FUSION)
    D = V = None
    results, reest = [], []
    for f, (img, M) in enumerate(seq["frames"]):
        ra = A.add_frame(img, M)
        want = ref.step(cam, PRM, M, D, V, None if f == 0 else ra["pose"])
        Da, Va = A.vo_get_fused_disparity()
        info = A.vo_disparity_fusion_info()
        _assert_step((Da, Va, info, A.get_disparity(info["slot"])), want, M, f)
        D, V = want[:2]
        results.append(ra)
        reest.append(A.vo_start_info(1)["n_candidates"] > 0)
        rb = B.add_frame(img, D)
        _same_results(ra, rb, f)
        for level in range(A.L):
            assert A.vo_num_points_at_level(level) == B.vo_num_points_at_level(level), (f, level)
        if ra["hasPointCloud"]:
            _same_cloud(A.get_point_cloud(), B.get_point_cloud(), f)
    assert bits_equal(A.trajectory(), B.trajectory())
    assert _branches(results, reest) == {"reest", "plain"}
    A.close(); B.close()


def test_add_frames_stereo_is_the_filter_plus_todays_vo(hip):
    seq = synth.make_stereo_sequence(ROWS, COLS, FRAMES, index=0)
    p = make_params(hip, descriptor="bitplanes", **VO_KW)
    cam = _cam_of(seq, p)
    A = hip.create(seq["K"], seq["b"], ROWS, COLS, p, n_frames=3, n_pairs=1)
    B = hip.create(seq["K"], seq["b"], ROWS, COLS, p, n_frames=3, n_pairs=1)
    A.set_disparity_fusion(FUSION)
    sp = A.default_stereo_params(ndisp=32)
    D = V = None
    fused_some = 0
    for f, (left, right) in enumerate(seq["frames"]):
        M = B.stereo_frames([(ROWS, COLS)], [left], [right], sp)[0]      # the measured map: the front-end's own, from a call of its own
        ra = A.add_frames_stereo([left], [right], sp)[0]
        want = ref.step(cam, PRM, M, D, V, None if f == 0 else ra["pose"])
        _assert_step(_state(A, 0, cam), want, M, f)
        D, V = want[:2]
        fused_some += want[2]["fused"]
        rb = B.add_frames([left], [D])[0]
        _same_results(ra, rb, f)
        assert A.seq_num_points_at_level(0) == B.seq_num_points_at_level(0)
    assert fused_some > 0 and bits_equal(A.seq_trajectory(0), B.seq_trajectory(0))
    A.close(); B.close()


# ---- 4. edges --------------------------------------------------------------------------------------------------------------------------------
def test_first_frames_reset_and_a_lower_gate(hip):
    """The first frame's slot keeps the caller's bits, and after seq_reset the next frame is a first frame again.  With minValidDisparity = 1
    (the CPU emulation's gate; the parameters' default 0.001 is checked by the add_frames test above) the layered sequence fills holes, too."""
    seq = synth.make_sequence(ROWS, COLS, 3, index=2, scene="layered")
    p = make_params(hip, descriptor="bitplanes", minValidDisparity=1.0, **VO_KW)
    cam = _cam_of(seq, p)
    ctx = hip.create(seq["K"], seq["b"], ROWS, COLS, p, n_frames=3, n_pairs=1)
    ctx.set_disparity_fusion(FUSION)
    hostile = ref.hostile_measurement(cam, seed=5)
    hostile[::2] = seq["frames"][0][1][::2]      # (enough valid rows for a template)
    for first in (hostile, seq["frames"][0][1]):
        ctx.add_frames([seq["frames"][0][0]], [first])
        D, V, info, slot = _state(ctx, 0, cam)
        assert ref.same_bits(slot, first) and ref.same_bits(D, first) and not info["predicted"]
        assert info["fused"] == info["replaced"] == info["filled"] == 0 and info["measured"] == int(ref.valid(first, cam["lo"], cam["hi"]).sum())
        ctx.seq_reset(0)
        with pytest.raises(capi.BpvoError, match="status -?\\d+"):
            ctx.seq_get_fused_disparity(0)      # the carried maps do not outlive the reset
        assert ctx.seq_get_disparity_fusion(0)[0]["mode"] == 1      # the setting does
    filled = 0
    for img, M in seq["frames"]:
        ctx.add_frames([img], [M])
        filled += ctx.seq_disparity_fusion_info(0)["filled"]
    assert filled > 0
    ctx.close()


def test_mode_0_is_a_context_that_never_heard_of_the_feature(hip):
    seq = synth.make_sequence(ROWS, COLS, 4, index=0)
    p = make_params(hip, descriptor="bitplanes", **VO_KW)
    live0 = hip.debug_live_resources()
    plain = hip.create(seq["K"], seq["b"], ROWS, COLS, p, n_frames=3, n_pairs=1)
    want = [plain.add_frames([img], [M])[0] for img, M in seq["frames"]]
    live_plain = hip.debug_live_resources()
    off = hip.create(seq["K"], seq["b"], ROWS, COLS, p, n_frames=3, n_pairs=1)
    off.set_disparity_fusion(dict(FUSION, mode=0))
    off.seq_set_disparity_fusion(0, dict(mode=0))
    for (img, M), ra in zip(seq["frames"], want):
        _same_results(ra, off.add_frames([img], [M])[0], "mode 0")
    assert bits_equal(plain.seq_trajectory(0), off.seq_trajectory(0))
    assert off.disparity_fusion_counts() == (0, 0)
    info = off.seq_disparity_fusion_info(0)
    assert all(info[k] == 0 for k in ref.CLASSES)
    live_both = hip.debug_live_resources()
    assert tuple(b - a for a, b in zip(live_plain, live_both)) == tuple(b - a for a, b in zip(live0, live_plain))      # mode 0 holds what a plain context holds
    with pytest.raises(capi.BpvoError):
        off.fuse_disparities([seq["frames"][0][1]], [np.eye(4)])      # needs mode 1
    plain.close(); off.close()
    assert hip.debug_live_resources() == live0


@pytest.mark.parametrize("bad", [dict(measurement_sigma=0.0), dict(measurement_sigma=-1.0), dict(measurement_sigma=np.nan), dict(process_sigma=-0.1),
                                 dict(process_sigma=np.inf), dict(gate=0.0), dict(gate=np.nan), dict(max_fill_sigma=-1.0), dict(mode=2), dict(mode=-1)])
def test_invalid_parameters_are_refused_and_nothing_changes(hip, bad):
    cam = ref.camera(9, 11)
    ctx = _ctx(hip, [cam, cam], fusion=None)
    ctx.seq_set_disparity_fusion(1, FUSION)
    before = ctx.get_disparity_fusion(), ctx.seq_get_disparity_fusion(0), ctx.seq_get_disparity_fusion(1)
    for call in (lambda: ctx.set_disparity_fusion(dict(FUSION, **bad)), lambda: ctx.seq_set_disparity_fusion(1, dict(FUSION, **bad))):
        with pytest.raises(capi.BpvoError, match="status -1:"):      # BPVO_ERR_INVALID_ARG
            call()
    assert (ctx.get_disparity_fusion(), ctx.seq_get_disparity_fusion(0), ctx.seq_get_disparity_fusion(1)) == before
    assert before[0]["mode"] == 0 and before[1] == (before[0], False) and before[2][1] and before[2][0]["mode"] == 1
    ctx.seq_set_disparity_fusion(1, None)
    assert ctx.seq_get_disparity_fusion(1) == (before[0], False)
    ctx.close()


def test_rig_contexts_refuse_mode_1(hip):
    cam = ref.camera(33, 65)
    ctx = _ctx(hip, [cam, cam], fusion=None)
    X = np.stack([np.eye(4, dtype=F32)] * 2)
    ctx.rig_set(X)
    for call in (lambda: ctx.set_disparity_fusion(FUSION), lambda: ctx.seq_set_disparity_fusion(0, FUSION)):
        with pytest.raises(capi.BpvoError, match="status -2:"):
            call()
    assert ctx.get_disparity_fusion()["mode"] == 0 and ctx.seq_get_disparity_fusion(0) == (ctx.get_disparity_fusion(), False)
    ctx.set_disparity_fusion(dict(mode=0))      # mode 0 is what the context runs anyway
    ctx.close()
    other = _ctx(hip, [cam, cam])
    with pytest.raises(capi.BpvoError, match="status -2:"):
        other.rig_set(X)      # ... and a context in mode 1 declares no rig
    other.close()


# ---- 5. the C++ facade -----------------------------------------------------------------------------------------------------------------------
def test_set_disparity_fusion_through_the_facade(hip, tmp_path):
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, "bpvo_amd", "csrc")
    exe = str(tmp_path / "disparity_fusion_facade")
    r = subprocess.run(["g++", "-std=c++11", "-O2", "-I", os.path.join(root, "include"), os.path.join(root, "tests", "cpp", "disparity_fusion_facade.cc"),
                        "-o", exe, "-L", csrc, "-lbpvo_hip", f"-Wl,-rpath,{csrc}"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    n_frames = 4
    seq = synth.make_sequence(ROWS, COLS, n_frames, index=2, scene="layered")
    for k, (img, M) in enumerate(seq["frames"]):
        img.tofile(tmp_path / f"img_{k}.u8")
        M.astype(F32).tofile(tmp_path / f"disp_{k}.f32")
    K = seq["K"]
    r = subprocess.run([exe, str(tmp_path), str(ROWS), str(COLS), repr(float(K[0, 0])), repr(float(K[1, 1])), repr(float(K[0, 2])), repr(float(K[1, 2])),
                        repr(float(seq["b"])), str(n_frames), "0.5", "0.1", "3.0", "2.0"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    poses = np.fromfile(tmp_path / "poses.bin", F32).reshape(n_frames, 4, 4)
    poses_seq = np.fromfile(tmp_path / "poses_seq.bin", F32).reshape(n_frames, 2, 4, 4)
    lines = [[int(v) for v in line.split()] for line in r.stdout.strip().splitlines()]
    # the same through the ctypes binding, with the facade's parameters (the defaults but three levels, bit-planes, Huber)
    p = make_params(hip, descriptor="bitplanes", loss="huber", levels=3)
    one = hip.create(K, seq["b"], ROWS, COLS, p, n_frames=3, n_pairs=1)
    one.set_disparity_fusion(FUSION)
    two = hip.create(K, seq["b"], ROWS, COLS, p, n_frames=6, n_pairs=2)
    two.seq_set_disparity_fusion(1, FUSION)
    for k, (img, M) in enumerate(seq["frames"]):
        assert bits_equal(one.add_frame(img, M)["pose"], poses[k]), k
        info = one.vo_disparity_fusion_info()
        assert lines[k] == [info[c] for c in ref.CLASSES] + [int(info["predicted"])], k
        res = two.add_frames(np.stack([img, img]), np.stack([M, M]))
        assert bits_equal(res[0]["pose"], poses_seq[k, 0]) and bits_equal(res[1]["pose"], poses_seq[k, 1]), k
    for ctx_maps, name in ((one.vo_get_fused_disparity(), "fused.bin"), (two.seq_get_fused_disparity(1), "fused_seq1.bin")):
        got = np.fromfile(tmp_path / name, F32).reshape(2, ROWS, COLS)
        assert ref.same_bits(got[0], ctx_maps[0]) and ref.same_bits(got[1], ctx_maps[1]), name
    one.close(); two.close()
