"""Several rigs in one call (bpvo_hip_rigs_set ... bpvo_hip_add_frames_rigs, bpvo_hip_estimate_pose_rigs), each with its own parameters.  One statement
carries every test: a rig advanced by the plural calls is BIT-IDENTICAL to the same rig alone in a context of its own, built the way a one-rig
context has always been built — bpvo_hip_create_sequences + bpvo_hip_rig_set + bpvo_hip_add_frames_rig with the rig's parameters as the
context's.  Compared per frame: pose, covariance, every level's statistics, the key-frame flags, every member's point count per level and point
cloud; at the end the whole body trajectory.  No tolerance anywhere.
Scenes: synth.make_rig_sequence's plane (index 3) through tests/test_gpu_rig.py's three extrinsics, 6 frames, at 120x160 and at 96x128, 3 levels.
Key frames.  The body moves 0.022 - 0.038 m per frame and lies 0.0224, 0.0236, 0.0067, 0.0304, 0.0123 m from its first pose.  Intensity / Huber
estimates that to a millimetre at both sizes, so there the ground truth plans the key frames: minTranslationMagToKeyFrame = 0.02 (KF) makes
every frame a key frame, none with re-estimation; 0.027 (KF_RE) gives frames 1 - 3 no key frame and frame 4 a key frame WITH re-estimation, its
previous frame holding data.  Bit-planes / Tukey does not follow this scene (it ends at maxIterations, centimetres off, at
96x128 it barely moves): its tests take 1e-4 m (KF_LOW), which any estimated motion exceeds, and assert the key frame they need."""
import re

import numpy as np
import pytest

from bpvo_amd import capi, synth
from util import bits_equal, make_params, perturbed_pose

pytestmark = pytest.mark.gpu

EXTRINSIC_TWISTS = ((0, 0, 0, 0, 0, 0), (0, 0.14, 0.02, 0.3, 0.02, 0.1), (0.03, -0.2, 0, -0.4, 0, 0.05))      # tests/test_gpu_rig.py's
LARGE, SMALL = (120, 160), (96, 128)
INDEX, N_FRAMES, LEVELS = 3, 6, 3
KF = dict(minTranslationMagToKeyFrame=0.02, minRotationMagToKeyFrame=2.5, maxFractionOfGoodPointsToKeyFrame=0.0, goodPointThreshold=0.8)
KF_RE = dict(KF, minTranslationMagToKeyFrame=0.027)
KF_LOW = dict(KF, minTranslationMagToKeyFrame=1e-4)
PLANNED = dict(descriptor="intensity", loss="huber")      # the configuration whose key frames the ground truth plans
KF_NEVER = dict(KF, minTranslationMagToKeyFrame=10.0, minRotationMagToKeyFrame=10.0)
ERR_INVALID_ARG, ERR_UNSUPPORTED = -1, -2      # c_api.h BPVO_ERR_*


def extrinsics(which=(0, 1, 2)):
    return [np.ascontiguousarray(synth.twist_to_matrix(EXTRINSIC_TWISTS[k]), np.float32) for k in which]


@pytest.fixture(scope="module")
def scenes():
    """the three cameras' frames at both sizes, rendered once: scenes[size]["frames"][k][e] = (image, disparity) of extrinsic e at frame k"""
    return {size: synth.make_rig_sequence(size[0], size[1], N_FRAMES, [x.astype(np.float64) for x in extrinsics()], index=INDEX) for size in (LARGE, SMALL)}


def rig_spec(scenes, which, size=LARGE, frames=None, **params):
    """One rig: members `which` (indices of the extrinsics) at `size`, fed frames[k] of the scene at its k-th call, its parameters as keywords of
    util.make_params over KF."""
    order = list(range(N_FRAMES)) if frames is None else list(frames)
    sc = scenes[size]
    return dict(X=np.stack(extrinsics(which)), cams=[(sc["K"][e], sc["b"][e], size[0], size[1]) for e in which],
                frames=[[sc["frames"][k][e] for e in which] for k in order], params=dict(KF, **params))


def params_of(hip, spec):
    return make_params(hip, levels=LEVELS, **spec["params"])


def snapshot(ctx, res, seq_ids, cov):
    """everything a frame leaves behind that a caller can read"""
    rec = dict(res=res, cov=cov, counts=[[ctx.seq_num_points_at_level(int(s), l) for l in range(ctx.L)] for s in seq_ids], clouds=None)
    if res["hasPointCloud"]:
        rec["clouds"] = [ctx.seq_point_cloud(int(s)) for s in seq_ids]
    return rec


def alone(hip, spec, n_calls=None, options=()):
    """the rig in a context of its own: create_sequences + rig_set + add_frames_rig, its parameters the context's"""
    ctx = hip.create_sequences(spec["cams"], params_of(hip, spec))
    for k, v in options:
        ctx.set_option(k, v)
    ctx.rig_set(spec["X"])
    recs = []
    for frames in spec["frames"][:n_calls]:
        res = ctx.add_frames_rig([f[0] for f in frames], [f[1] for f in frames])
        recs.append(snapshot(ctx, res, range(len(spec["cams"])), ctx.rig_pose_covariance()))
    traj = ctx.rig_trajectory()
    ctx.close()
    return recs, traj


def together_context(hip, specs, seq_ids, base, options=()):
    """one context for all the rigs: rig r's members are sequences seq_ids[r]; parameters that differ from the base's through rigs_set_params"""
    n_seq = sum(len(q) for q in seq_ids)
    cams = [None] * n_seq
    for sp, ids in zip(specs, seq_ids):
        for cam, s in zip(sp["cams"], ids):
            cams[s] = cam
    ctx = hip.create_sequences(cams, make_params(hip, levels=LEVELS, **base))
    for k, v in options:
        ctx.set_option(k, v)
    ctx.rigs_set([sp["X"] for sp in specs], seqs=seq_ids)
    for r, sp in enumerate(specs):
        if sp["params"] != base:
            ctx.rigs_set_params(r, params_of(hip, sp))
    return ctx


def advance(ctx, specs, seq_ids, call, done, recs):
    """one add_frames_rigs call naming the rigs `call` in that order, each fed its next frame"""
    imgs = [[f[0] for f in specs[r]["frames"][done[r]]] for r in call]
    disps = [[f[1] for f in specs[r]["frames"][done[r]]] for r in call]
    out = ctx.add_frames_rigs(imgs, disps, rigs=call)
    for r, res in zip(call, out):
        recs[r].append(snapshot(ctx, res, seq_ids[r], ctx.rigs_pose_covariance(r)))
        done[r] += 1


def together(hip, specs, seq_ids, base=KF, schedule=None, options=()):
    ctx = together_context(hip, specs, seq_ids, base, options)
    recs, done = [[] for _ in specs], [0] * len(specs)
    for call in (schedule or [list(range(len(specs)))] * N_FRAMES):
        advance(ctx, specs, seq_ids, call, done, recs)
    trajs = [ctx.rigs_trajectory(r) for r in range(len(specs))]
    ctx.close()
    return recs, trajs


def stats_array(stats):
    return (np.array([(s["numIterations"], s["status"]) for s in stats], np.int32),
            np.array([(s["finalError"], s["firstOrderOptimality"]) for s in stats], np.float32))


def assert_same_frames(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    for k, (a, b) in enumerate(zip(got, want)):
        ra, rb = a["res"], b["res"]
        assert bits_equal(ra["pose"], rb["pose"]), (what, k, "pose", ra["pose"], rb["pose"])
        assert bits_equal(ra["covariance"], rb["covariance"]), (what, k, "covariance")
        for x, y in zip(stats_array(ra["stats"]), stats_array(rb["stats"])):
            assert bits_equal(x, y), (what, k, "optimizerStatistics", ra["stats"], rb["stats"])
        for key in ("isKeyFrame", "keyFramingReason", "hasPointCloud"):
            assert ra[key] == rb[key], (what, k, key, ra[key], rb[key])
        assert a["counts"] == b["counts"], (what, k, "point counts", a["counts"], b["counts"])
        assert (a["clouds"] is None) == (b["clouds"] is None), (what, k)
        for p, ((pa, Ta), (pb, Tb)) in enumerate(zip(a["clouds"] or [], b["clouds"] or [])):
            assert bits_equal(Ta, Tb), (what, k, p, "cloud pose")
            assert len(pa) == len(pb) and len(pa) > 0, (what, k, p, len(pa), len(pb))
            for field in ("xyzw", "rgba", "weight"):
                assert bits_equal(pa[field], pb[field]), (what, k, p, "cloud", field)
        for field in ("T", "covariance"):
            assert bits_equal(a["cov"][field], b["cov"][field]), (what, k, "pose covariance record", field)
        assert bits_equal(np.float32(a["cov"]["sigma"]), np.float32(b["cov"]["sigma"])), (what, k, "sigma")
        assert [a["cov"][f] for f in ("num_valid", "level", "status")] == [b["cov"][f] for f in ("num_valid", "level", "status")], (what, k, a["cov"], b["cov"])


def assert_rigs_equal_their_own_contexts(hip, specs, seq_ids, key_frames=True, **kw):
    recs, trajs = together(hip, specs, seq_ids, **kw)
    for r, sp in enumerate(specs):
        want, traj = alone(hip, sp, options=kw.get("options", ()))
        if key_frames is True or (key_frames and key_frames[r]):
            assert sum(x["res"]["isKeyFrame"] for x in want[1:]) >= 1, "no key frame after the first: the sequence does not test the key-frame path"
        assert_same_frames(recs[r], want, f"rig {r}")
        assert bits_equal(trajs[r], traj), (r, "trajectory")
    return recs


UNLIKE_IDS = [[4], [0, 3], [5, 1, 2]]      # the members' sequence ids, interleaved in the context


def unlike_rigs(scenes, **params):
    return [rig_spec(scenes, (0,), **params), rig_spec(scenes, (0, 1), size=SMALL, **params), rig_spec(scenes, (0, 1, 2), **params)]


def test_unlike_rigs_in_one_call(hip, scenes):
    """Rigs of 1, 2 and 3 members, the rig of two at 96x128, the others at 120x160, sequence ids interleaved: the member ranges of the batched
    step, each rig's own reference member, mixed sizes in the shared launches."""
    assert_rigs_equal_their_own_contexts(hip, unlike_rigs(scenes, **KF_LOW), UNLIKE_IDS, base=KF_LOW)


def test_unlike_rigs_intensity_huber(hip, scenes):
    """the same shape with one channel"""
    kw = dict(KF_LOW, descriptor="intensity", loss="huber")
    assert_rigs_equal_their_own_contexts(hip, unlike_rigs(scenes, **kw), UNLIKE_IDS, base=kw)


def test_rigs_that_finish_at_different_iterations(hip, scenes):
    """Rig 0 sees every frame twice (its every second estimate converges in its first iterations), rig 1 make_rig_sequence's motion, which under
    bit-planes / Tukey at this size runs to maxIterations: the finished rig's body and members must stay frozen while the other iterates."""
    specs = [rig_spec(scenes, (0, 1), frames=(0, 0, 1, 1, 2, 2), **KF_LOW), rig_spec(scenes, (1, 2), **KF_LOW)]
    recs = assert_rigs_equal_their_own_contexts(hip, specs, [[0, 1], [2, 3]], base=KF_LOW)
    its = [[sum(s["numIterations"] for s in x["res"]["stats"]) for x in recs[r][1:]] for r in range(2)]
    print(f"iterations per frame (all levels): still rig {its[0]}, moving rig {its[1]}")
    assert any(a < b for a, b in zip(its[0], its[1])), "the rigs never finish at different iterations"


def test_rigs_out_of_step(hip, scenes):
    """Rig 0 starts two frames before rig 1, whose first frame arrives while rig 0 estimates; a call that names only rig 1 leaves rig 0 untouched;
    at rig 0's frame 4 exactly one rig takes a key frame with re-estimation (rig 0: KF_RE, its frame 3 was no key frame, so the previous slot
    holds data and the new key frame is estimated against; rig 1 never takes a key frame)."""
    specs = [rig_spec(scenes, (0, 1), **dict(KF_RE, **PLANNED)), rig_spec(scenes, (2, 0), **dict(KF_NEVER, **PLANNED))]
    seq_ids = [[0, 2], [3, 1]]
    schedule = [[0], [0], [1, 0], [0, 1], [1], [0, 1], [0]]
    ctx = together_context(hip, specs, seq_ids, dict(KF, **PLANNED))
    recs, done = [[], []], [0, 0]
    for i, call in enumerate(schedule):
        before = (ctx.rigs_trajectory(0), snapshot(ctx, dict(hasPointCloud=False), seq_ids[0], ctx.rigs_pose_covariance(0)))
        advance(ctx, specs, seq_ids, call, done, recs)
        if call == [1]:
            after = snapshot(ctx, dict(hasPointCloud=False), seq_ids[0], None)
            assert bits_equal(before[0], ctx.rigs_trajectory(0)) and before[1]["counts"] == after["counts"], "a call that names only rig 1 touched rig 0"
        if call == [0, 1] and done[0] == 5:
            a, b = recs[0][-1]["res"], recs[1][-1]["res"]
            assert a["isKeyFrame"] and not recs[0][-2]["res"]["isKeyFrame"], "rig 0 takes no key frame with re-estimation at its frame 4"
            assert not b["isKeyFrame"], "rig 1 takes a key frame too"
    trajs = [ctx.rigs_trajectory(r) for r in range(2)]
    ctx.close()
    for r in range(2):
        want, traj = alone(hip, specs[r], n_calls=done[r])
        assert_same_frames(recs[r], want, f"rig {r}")
        assert bits_equal(trajs[r], traj), (r, "trajectory")


def test_per_rig_parameters(hip, scenes):
    """Huber, Tukey, Tukey with 5 iterations, Tukey with a translation threshold no motion reaches, over the same frames in one context (the
    context's: Tukey, KF_LOW): two estimates per call, one per loss; the last rig, alone, never takes a key frame."""
    variants = [dict(KF_LOW, loss="huber"), KF_LOW, dict(KF_LOW, maxIterations=5), dict(KF_LOW, minTranslationMagToKeyFrame=10.0)]
    specs = [rig_spec(scenes, (0, 1), **v) for v in variants]
    seq_ids = [[0, 1], [2, 3], [4, 5], [6, 7]]
    recs = assert_rigs_equal_their_own_contexts(hip, specs, seq_ids, key_frames=[True, True, True, False], base=KF_LOW)
    assert not any(x["res"]["isKeyFrame"] for x in recs[3][1:]), "the key-frame thresholds are not the rigs' own"
    ctx = together_context(hip, specs, seq_ids, KF_LOW)
    for r in (0, 2, 3):
        assert bytes(ctx.rigs_get_params(r)) == bytes(params_of(hip, specs[r])), r
    before = bytes(ctx.rigs_get_params(1))
    for field, value in (("maxTestLevel", 1), ("nonMaxSuppRadius", 2), ("descriptor", "intensity")):
        with pytest.raises(capi.BpvoError) as e:
            ctx.rigs_set_params(1, make_params(hip, levels=LEVELS, **dict(KF, **{field: value})))
        assert re.match(rf"status {ERR_UNSUPPORTED}:", str(e.value)) and field in str(e.value), (field, str(e.value))
    assert bytes(ctx.rigs_get_params(1)) == before
    ctx.close()


def test_pose_covariance_of_every_rig(hip, scenes):
    """option "pose_covariance": the records and result.covariance of two rigs of two members, through a key frame with re-estimation (KF_RE);
    option off: the Identity (assert_same_frames compares the records either way)."""
    specs = [rig_spec(scenes, (0, 1), **dict(KF_RE, **PLANNED)), rig_spec(scenes, (2, 1), **PLANNED)]
    base = dict(KF, **PLANNED)
    on = assert_rigs_equal_their_own_contexts(hip, specs, [[1, 2], [0, 3]], base=base, options=(("pose_covariance", 1),))
    eye = np.eye(6, dtype=np.float32)
    assert all(x["cov"]["status"] != capi.COV_NONE for r in range(2) for x in on[r][1:])
    assert all(not bits_equal(x["res"]["covariance"], eye) for r in range(2) for x in on[r][1:] if x["cov"]["status"] == capi.COV_OK)
    assert any(x["cov"]["status"] == capi.COV_OK for r in range(2) for x in on[r][1:])
    assert any(x["res"]["isKeyFrame"] and not on[0][k]["res"]["isKeyFrame"] for k, x in enumerate(on[0][1:]) if k >= 1), "no key frame with re-estimation"
    recs, _ = together(hip, specs, [[1, 2], [0, 3]], base=base)
    assert all(bits_equal(x["res"]["covariance"], eye) and x["cov"]["status"] == capi.COV_NONE for r in range(2) for x in recs[r])


def test_estimate_pose_rigs_is_estimate_pose_rig_per_rig(hip, scenes):
    """the stateless form: two rigs of two members from perturbed starts against two bpvo_hip_estimate_pose_rig calls on the same context"""
    sc = scenes[LARGE]
    ctx = hip.create(sc["K"][0], sc["b"][0], LARGE[0], LARGE[1], make_params(hip, levels=LEVELS), device=0, n_frames=8, n_pairs=4)
    members = [(0, 1), (2, 1)]
    for i, e in enumerate(members[0] + members[1]):
        ctx.frame_set_data(2 * i, *sc["frames"][0][e])
        ctx.frame_set_template(2 * i)
        ctx.frame_set_data(2 * i + 1, *sc["frames"][2][e])
    wss, refs, curs = [[0, 1], [2, 3]], [[0, 2], [4, 6]], [[1, 3], [5, 7]]
    X = [np.stack(extrinsics(m)) for m in members]
    T0 = np.stack([perturbed_pose(1), perturbed_pose(0.5)])
    single = [ctx.estimate_pose_rig(wss[r], refs[r], curs[r], X[r], T0[r]) for r in range(2)]
    T, stats = ctx.estimate_pose_rigs(wss, refs, curs, X, T0)
    again = [ctx.estimate_pose_rig(wss[r], refs[r], curs[r], X[r], T0[r]) for r in range(2)]
    for r in range(2):
        for Ts, ss in (single[r], again[r]):
            assert bits_equal(T[r], Ts), (r, T[r], Ts)
            for x, y in zip(stats_array(stats[r]), stats_array(ss)):
                assert bits_equal(x, y), (r, stats[r], ss)
        assert not bits_equal(T[r], T0[r]) and all(s["numIterations"] >= 1 for s in stats[r])
    with pytest.raises(capi.BpvoError, match=rf"status {ERR_INVALID_ARG}:"):
        ctx.estimate_pose_rigs([[0, 1], [1, 3]], refs, curs, X, T0)      # a workspace in two rigs
    ctx.close()


# ---- refusals and recovery
def refused(code, fn, *args, **kw):
    with pytest.raises(capi.BpvoError) as e:
        fn(*args, **kw)
    assert re.match(rf"status {code}:", str(e.value)), (code, str(e.value))
    return str(e.value)


def test_refusals_leave_the_rigs_as_they_were(hip, scenes):
    specs = [rig_spec(scenes, (0, 1), **KF_RE), rig_spec(scenes, (2,), loss="huber")]
    seq_ids = [[0, 2], [1]]
    Xs = [sp["X"] for sp in specs]
    bad = Xs[0].copy()
    bad[1, :3, :3] *= np.float32(1.001)
    own = make_params(hip, levels=LEVELS, **dict(KF, maxIterations=7))

    def run(disturb):
        ctx = together_context(hip, specs, seq_ids, KF)
        base = make_params(hip, levels=LEVELS, **KF)
        recs, done = [[], []], [0, 0]
        for k in range(4):
            imgs = [[f[0] for f in specs[r]["frames"][k]] for r in range(2)]
            disps = [[f[1] for f in specs[r]["frames"][k]] for r in range(2)]
            if disturb:
                refused(ERR_INVALID_ARG, ctx.add_frames_rigs, [imgs[0], imgs[0]], [disps[0], disps[0]], rigs=[0, 0])      # a rig named twice
                refused(ERR_INVALID_ARG, ctx.add_frames_rigs, imgs, disps, rigs=[0, 2])                                  # a rig id out of range
                refused(ERR_INVALID_ARG, ctx.add_frames_rigs, imgs[:1], disps[:1], rigs=[-1])
                refused(ERR_INVALID_ARG, ctx.rigs_set, [Xs[0], Xs[0]], seqs=[[0, 1], [1, 2]])                           # a sequence in two rigs
                refused(ERR_INVALID_ARG, ctx.rigs_set, [bad, Xs[1]], seqs=seq_ids)                                       # an extrinsic that is not rigid
                # the one-rig entry points on a context of several rigs
                for name, args in (("rig_get", ()), ("rig_trajectory", ()), ("rig_pose_covariance", ())):
                    refused(ERR_INVALID_ARG, getattr(ctx, name), *args)
                img, disp, _ = capi.pack_frames(imgs[0], disps[0])
                msg = refused(ERR_INVALID_ARG, ctx.call, "add_frames_rig", capi.C.c_void_p(img.ctypes.data), capi.C.c_void_p(disp.ctypes.data), 0, capi.C.byref(capi.Result()))
                assert "add_frames_rigs" in msg, msg
                refused(ERR_INVALID_ARG, ctx.add_frames, np.stack(imgs[0]), np.stack(disps[0]))                          # a rig context serves the rig calls only
                if k == 0:
                    # (the sequences are fresh: a member's own parameters may be set — and its rig then refuses its frames, as rigs_set refuses it)
                    ctx.seq_set_params(2, own)
                    refused(ERR_INVALID_ARG, ctx.add_frames_rigs, imgs, disps)
                    refused(ERR_INVALID_ARG, ctx.rigs_set, Xs, seqs=seq_ids)
                    ctx.seq_set_params(2, base)
                    ctx.set_warp_formulation(2)
                    refused(ERR_UNSUPPORTED, ctx.add_frames_rigs, imgs, disps)                                           # BPVO_WARP_DISPARITY_SPACE_F32
                    ctx.set_warp_formulation(0)
                else:
                    refused(ERR_INVALID_ARG, ctx.rigs_set, Xs, seqs=seq_ids)                                             # membership changes on sequences that hold frames
                    refused(ERR_INVALID_ARG, ctx.rigs_set_params, 0, own)
            advance(ctx, specs, seq_ids, [0, 1], done, recs)
        trajs = [ctx.rigs_trajectory(r) for r in range(2)]
        ctx.close()
        return recs, trajs

    clean, traj_clean = run(False)
    disturbed, traj_disturbed = run(True)
    for r in range(2):
        assert_same_frames(disturbed[r], clean[r], f"rig {r} after refusals")
        assert bits_equal(traj_disturbed[r], traj_clean[r])
        want, traj = alone(hip, specs[r], n_calls=4)
        assert_same_frames(clean[r], want, f"rig {r}")
        assert bits_equal(traj_clean[r], traj)


def test_one_rig_declared_by_rigs_set_serves_both_forms(hip, scenes):
    spec = rig_spec(scenes, (0, 1), **KF_RE)
    ctx = hip.create_sequences(spec["cams"], params_of(hip, spec))
    ctx.rigs_set([spec["X"]])
    ids, X = ctx.rig_get()
    assert ids.tolist() == [0, 1] and bits_equal(X, spec["X"])
    (ids2, X2), = ctx.rigs_get()
    assert ids2.tolist() == [0, 1] and bits_equal(X2, spec["X"])
    recs = []
    for k, frames in enumerate(spec["frames"]):
        imgs, disps = [f[0] for f in frames], [f[1] for f in frames]
        res = ctx.add_frames_rig(imgs, disps) if k % 2 else ctx.add_frames_rigs([imgs], [disps])[0]
        assert bits_equal(ctx.rig_trajectory(), ctx.rigs_trajectory(0))
        recs.append(snapshot(ctx, res, [0, 1], ctx.rigs_pose_covariance(0) if k % 2 else ctx.rig_pose_covariance()))
    traj = ctx.rig_trajectory()
    ctx.close()
    want, traj_alone = alone(hip, spec)
    assert_same_frames(recs, want, "one rig, both forms")
    assert bits_equal(traj, traj_alone)
