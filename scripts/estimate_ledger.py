"""The ledger of the estimate driver (bpvo_amd/csrc/estimate.hip): for every path a group of pairs can take — persistent kernel, team kernel
(one launch and split), the four-kernel chain in its forms, reference order, channel groups, rigs, add_frames with two losses, the fall-back
reruns — what came out (iterations and status per level, a digest of the pose bytes) and what was launched to get there (persistent levels,
team launches / joins / give-ups, median selections by path, fused points, and at profiling level 2 the launches per kernel class).  The host
decides its rounds from device results it has waited for, so every number is exact: tests/test_gpu_estimate_ledger.py compares a run against
tests/golden/estimate_ledger.json key by key.  Through bpvo_amd.capi only, on 120x160 synthetic pairs with 3 levels.

    python scripts/estimate_ledger.py [out.json]
"""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from bpvo_amd import capi, synth  # noqa: E402

ROWS, COLS, LEVELS = 120, 160, 3
DESC = {"bitplanes": capi.DESC_BITPLANES, "intensity": capi.DESC_INTENSITY, "centraldiff": capi.DESC_CENTRAL_DIFFERENCE}
LOSS = {"tukey": capi.LOSS_TUKEY, "huber": capi.LOSS_HUBER, "l2": capi.LOSS_L2}
RIG_TWISTS = ((0, 0, 0, 0, 0, 0), (0, 0.14, 0.02, 0.3, 0.02, 0.1), (0.03, -0.2, 0, -0.4, 0, 0.05))


def params(hip, descriptor="bitplanes", loss="tukey", **kw):
    p = hip.default_params()
    p.numPyramidLevels = LEVELS
    p.descriptor = DESC[descriptor]
    p.lossFunction = LOSS[loss]
    p.verbosity = capi.VERB_SILENT
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a, np.float32).tobytes()).hexdigest()[:16]


def levels_of(stats):
    """[numIterations per level], [status per level] of one estimate: a list of dicts or a row of batch statistics"""
    if isinstance(stats, np.ndarray):
        return [int(v) for v in stats["numIterations"]], [int(v) for v in stats["status"]]
    return [int(s["numIterations"]) for s in stats], [int(s["status"]) for s in stats]


def estimates(poses, stats):
    out = []
    for T, st in zip(poses, stats):
        its, status = levels_of(st)
        out.append(dict(numIterations=its, status=status, pose=digest(T)))
    return out


def counters(ctx, device_work=True, profiled=False):
    """device_work = False: a launch that gave up at a barrier did some of its work first, how much depends on when the budget ran out"""
    levels_pk, gave_up = ctx.persistent_counts()
    rec = dict(persistent_counts=[int(levels_pk), int(gave_up)], team_launches=int(ctx.team_counts()), team_joins=int(ctx.get_option("team_joins_seen")))
    if device_work:
        rec["median_path_counts"] = [int(v) for v in ctx.median_path_counts()]
        rec["fused_point_counts"] = [int(v) for v in ctx.fused_point_counts()]
    if profiled:
        rec["launches"] = {k["name"]: int(k["launches"]) for k in ctx.kernel_stats()}
    return rec


def make(hip, data, p, n, options, profiling):
    ctx = hip.create(data["K"], data["b"], ROWS, COLS, p, device=0, n_frames=2 * n, n_pairs=n)
    for k, v in options.items():
        ctx.set_option(k, v)
    if profiling:
        ctx.profiling(profiling)
    return ctx


def single(hip, pair, p, options=None, profiling=0, device_work=True):
    ctx = make(hip, pair, p, 1, options or {}, profiling)
    ctx.frame_set_data(0, pair["imgA"], pair["dispA"])
    ctx.frame_set_template(0)
    ctx.frame_set_data(1, pair["imgB"], pair["dispB"])
    T, st = ctx.estimate_pose(0, 0, 1)
    T2, st2 = ctx.estimate_pose(0, 0, 1, T)      # (a warm start: few iterations, early exits)
    rec = dict(estimates=estimates([T, T2], [st, st2]), **counters(ctx, device_work, profiling == 2))
    ctx.close()
    return rec


def batch(hip, b, p, options=None, profiling=0, device_work=True):
    n = b["images"].shape[0] // 2
    ctx = make(hip, b, p, n, options or {}, profiling)
    poses, stats = ctx.batch_run(b["images"], b["disparities"])      # (one lane: the estimate starts behind a deferred normalisation)
    rec = dict(estimates=estimates(poses, stats), **counters(ctx, device_work, profiling == 2))
    ctx.close()
    return rec


def rig_scene():
    X = [np.ascontiguousarray(synth.twist_to_matrix(t), np.float32) for t in RIG_TWISTS]
    return X, synth.make_rig_sequence(ROWS, COLS, 4, [x.astype(np.float64) for x in X], index=3)


def rigs_stateless(hip, X, sc):
    """bpvo_hip_estimate_pose_rigs: a rig of two members and a rig of one, from perturbed starts, at profiling 2"""
    ctx = hip.create(sc["K"][0], sc["b"][0], ROWS, COLS, params(hip), device=0, n_frames=6, n_pairs=3)
    ctx.profiling(2)
    for i in range(3):
        ctx.frame_set_data(2 * i, *sc["frames"][0][i])
        ctx.frame_set_template(2 * i)
        ctx.frame_set_data(2 * i + 1, *sc["frames"][2][i])
    T0 = np.stack([synth.twist_to_matrix(np.array([0.004, -0.003, 0.002, 0.02, -0.015, 0.03]) * s).astype(np.float32) for s in (1.0, 0.5)])
    T, stats = ctx.estimate_pose_rigs([[0, 1], [2]], [[0, 2], [4]], [[1, 3], [5]], [np.stack(X[:2]), np.stack(X[2:])], T0)
    rec = dict(estimates=estimates(T, stats), **counters(ctx, True, True))
    ctx.close()
    return rec


def rigs_unequal_limits(hip, X, sc):
    """the same two rigs through bpvo_hip_add_frames_rigs with parameters of their own: iteration limits 3 and 50, at profiling 2"""
    kf = dict(minTranslationMagToKeyFrame=0.02, minRotationMagToKeyFrame=2.5, maxFractionOfGoodPointsToKeyFrame=0.0, goodPointThreshold=0.8)
    cams = [(sc["K"][e], sc["b"][e], ROWS, COLS) for e in range(3)]
    ctx = hip.create_sequences(cams, params(hip, **kf))
    ctx.rigs_set([np.stack(X[:2]), np.stack(X[2:])], seqs=[[0, 1], [2]])
    ctx.rigs_set_params(0, params(hip, maxIterations=3, **kf))
    ctx.rigs_set_params(1, params(hip, maxIterations=50, **kf))
    ctx.profiling(2)
    frames = []
    for k in range(4):
        out = ctx.add_frames_rigs([[sc["frames"][k][0][0], sc["frames"][k][1][0]], [sc["frames"][k][2][0]]],
                                  [[sc["frames"][k][0][1], sc["frames"][k][1][1]], [sc["frames"][k][2][1]]])
        frames.append(estimates([r["pose"] for r in out], [r["stats"] for r in out]))
    rec = dict(frames=frames, **counters(ctx, True, True))
    ctx.close()
    return rec


def add_frames_two_losses(hip):
    """four bpvo_hip_add_frames calls of three sequences whose parameters name two different losses"""
    kf = dict(minTranslationMagToKeyFrame=0.05, minRotationMagToKeyFrame=2.5, maxFractionOfGoodPointsToKeyFrame=0.0, goodPointThreshold=0.8)
    seq = synth.make_sequence(ROWS, COLS, 4, index=5, step_rot=0.01, step_trans=0.06)
    ctx = hip.create(seq["K"], seq["b"], ROWS, COLS, params(hip, **kf), device=0, n_frames=9, n_pairs=3)
    own = [params(hip, loss="tukey", maxIterations=3, **kf), params(hip, loss="huber", maxIterations=50, **kf), params(hip, loss="tukey", **kf)]
    for s in range(3):
        ctx.seq_set_params(s, own[s])
    frames = []
    for img, disp in seq["frames"]:
        out = ctx.add_frames(np.stack([img] * 3), np.stack([disp] * 3))
        frames.append(estimates([r["pose"] for r in out], [r["stats"] for r in out]))
    rec = dict(frames=frames, **counters(ctx))
    ctx.close()
    return rec


def ledger(hip):
    pair = synth.make_pair(ROWS, COLS, 0)
    four = synth.make_batch(ROWS, COLS, 4, first_index=11)
    out = {}
    for desc, loss in (("bitplanes", "tukey"), ("intensity", "huber")):
        p = params(hip, desc, loss)
        tag = desc + "-" + loss
        out["one pair, defaults, " + tag] = single(hip, pair, p)
        out["one pair, persistent=0, profiling 2, " + tag] = single(hip, pair, p, dict(persistent=0), 2)
        for split in (0, 4):
            out[f"four pairs, defaults, team_split_max_pairs={split}, {tag}"] = batch(hip, four, p, dict(team_split_max_pairs=split))
        for sir in (0, 128):
            for fuse in (0, 1):
                out[f"four pairs, chain, profiling 2, step_in_reduce_max_pairs={sir}, fuse_frozen={fuse}, {tag}"] = \
                    batch(hip, four, p, dict(step_in_reduce_max_pairs=sir, fuse_frozen=fuse), 2)
        out["four pairs, reference_reduction=1, profiling 2, " + tag] = batch(hip, four, p, dict(reference_reduction=1), 2)
    p = params(hip)
    out["one pair, central difference of 80 channels, profiling 2"] = single(hip, pair, params(hip, "centraldiff", centralDifferenceRadius=4), None, 2)
    X, sc = rig_scene()
    out["estimate_pose_rigs, rigs of two members and of one, profiling 2"] = rigs_stateless(hip, X, sc)
    out["add_frames_rigs, the same rigs with maxIterations 3 and 50, profiling 2"] = rigs_unequal_limits(hip, X, sc)
    out["add_frames, three sequences, two losses"] = add_frames_two_losses(hip)
    out["one pair, persist_timeout_ticks=1"] = single(hip, pair, p, dict(persist_timeout_ticks=1), device_work=False)
    out["four pairs, persist_timeout_ticks=1, team_split_max_pairs=0"] = batch(hip, four, p, dict(persist_timeout_ticks=1, team_split_max_pairs=0), device_work=False)
    out["four pairs, persist_timeout_ticks=1, team_split_max_pairs=4"] = batch(hip, four, p, dict(persist_timeout_ticks=1, team_split_max_pairs=4), device_work=False)
    return out


if __name__ == "__main__":
    import bpvo_amd
    text = json.dumps(ledger(bpvo_amd.load()), indent=1, sort_keys=True)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")
    else:
        print(text)
