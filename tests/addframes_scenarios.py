"""Two scenarios of the batched addFrame driver (vo.hip: add_frames_run), shared by tests/test_gpu_multi_sequence.py and
tests/tools/addframes_record.py, on tests/test_gpu_rigs.py's scene, sizes, thresholds and snapshot.
ONE CALL: four sequences of one context, option "pose_covariance" on, advanced so that call 4 — the one call — takes every branch of the driver:
    sequence 0  "first"  120x160, the context's parameters: it enters at call 4, its first frame
    sequence 1  "none"   120x160, parameters of its own: KF_NEVER and the Tukey loss — no key frame
    sequence 2  "swap"   96x128 (the camera of the other size), the context's parameters (KF): every frame a key frame, none with re-estimation
    sequence 3  "again"  120x160, parameters of its own: KF_RE (Huber, the context's loss) — frames 1 - 3 no key frame, frame 4 a key frame WITH
                         re-estimation
The context runs intensity / Huber (PLANNED), where the ground truth plans the key frames of KF and KF_RE; KF_NEVER's thresholds no motion
reaches whatever the loss.  A key frame re-estimates exactly when the frame before it was none (only then the previous slot holds data).
RIGS OUT OF STEP: test_rigs_out_of_step's two rigs and schedule with option "pose_covariance" on."""
import numpy as np

from bpvo_amd import synth
from test_gpu_rigs import (INDEX, KF, KF_NEVER, KF_RE, LARGE, LEVELS, N_FRAMES, PLANNED, SMALL, advance, rig_spec, snapshot, stats_array,
                           together_context)
from util import make_params

ROLES = ("first", "none", "swap", "again")
ONE_CALL = 4                                    # the call that takes every branch
CALL_ORDER = [3, 0, 2, 1]                       # its entries: the sequences interleaved, not in id order
COVARIANCE = (("pose_covariance", 1),)


def one_call_setup(hip):
    """per sequence: its camera (K, b, rows, cols), its frames, its parameters; and the context's parameters"""
    sc = {size: synth.make_sequence(size[0], size[1], N_FRAMES, index=INDEX) for size in (LARGE, SMALL)}
    base = make_params(hip, levels=LEVELS, **dict(KF, **PLANNED))
    own = {1: make_params(hip, levels=LEVELS, **dict(KF_NEVER, descriptor="intensity", loss="tukey")),
           3: make_params(hip, levels=LEVELS, **dict(KF_RE, **PLANNED))}
    sizes = [LARGE, LARGE, SMALL, LARGE]
    cams = [(sc[z]["K"], sc[z]["b"], z[0], z[1]) for z in sizes]
    frames = [sc[z]["frames"] for z in sizes]
    return cams, frames, [own.get(s, base) for s in range(4)], base, own


def run_one_call(hip):
    """recs[s]: a snapshot per frame of sequence s; trajs[s]"""
    cams, frames, _, base, own = one_call_setup(hip)
    ctx = hip.create_sequences(cams, base)
    for k, v in COVARIANCE:
        ctx.set_option(k, v)
    for s, p in own.items():
        ctx.seq_set_params(s, p)
    recs = [[] for _ in cams]
    for call in range(ONE_CALL + 1):
        ids = CALL_ORDER if call == ONE_CALL else [1, 2, 3]
        fed = [frames[s][len(recs[s])] for s in ids]
        out = ctx.add_frames([f[0] for f in fed], [f[1] for f in fed], seq=ids)
        for s, res in zip(ids, out):
            recs[s].append(snapshot(ctx, res, [s], ctx.seq_pose_covariance(s)))
    trajs = [ctx.seq_trajectory(s) for s in range(len(cams))]
    ctx.close()
    return recs, trajs


def run_alone(hip, cam, frames, params):
    """the same frames through bpvo_hip_add_frame in a context of the sequence's own camera and parameters; snapshots of snapshot()'s shape"""
    K, b, rows, cols = cam
    ctx = hip.create(K, b, rows, cols, params, n_frames=3, n_pairs=1)
    for k, v in COVARIANCE:
        ctx.set_option(k, v)
    recs = []
    for img, disp in frames:
        res = ctx.add_frame(img, disp)
        recs.append(dict(res=res, cov=ctx.vo_pose_covariance(), counts=[[ctx.vo_num_points_at_level(l) for l in range(ctx.L)]],
                         clouds=[ctx.get_point_cloud()] if res["hasPointCloud"] else None))
    traj = ctx.trajectory()
    ctx.close()
    return recs, traj


def run_rigs_out_of_step(hip, scenes):
    specs = [rig_spec(scenes, (0, 1), **dict(KF_RE, **PLANNED)), rig_spec(scenes, (2, 0), **dict(KF_NEVER, **PLANNED))]
    seq_ids = [[0, 2], [3, 1]]
    ctx = together_context(hip, specs, seq_ids, dict(KF, **PLANNED), COVARIANCE)
    recs, done = [[], []], [0, 0]
    for call in [[0], [0], [1, 0], [0, 1], [1], [0, 1], [0]]:
        advance(ctx, specs, seq_ids, call, done, recs)
    trajs = [ctx.rigs_trajectory(r) for r in range(2)]
    ctx.close()
    return recs, trajs


def flatten(name, recs, trajs):
    """every array of a scenario's snapshots and trajectories under a key of its own (the .npz of tests/tools/addframes_record.py)"""
    out = {}
    for e, (frames, traj) in enumerate(zip(recs, trajs)):
        out[f"{name}/{e}/trajectory"] = np.ascontiguousarray(traj, np.float32)
        for k, x in enumerate(frames):
            at, res, cov = f"{name}/{e}/{k}/", x["res"], x["cov"]
            ints, floats = stats_array(res["stats"])
            out.update({at + "pose": res["pose"], at + "covariance": res["covariance"], at + "stats_int": ints, at + "stats_f32": floats,
                        at + "flags": np.array([res["isKeyFrame"], res["keyFramingReason"], res["hasPointCloud"]], np.int32),
                        at + "counts": np.array(x["counts"], np.int32), at + "cov_T": cov["T"], at + "cov_covariance": cov["covariance"],
                        at + "cov_sigma": np.float32(cov["sigma"]), at + "cov_ints": np.array([cov[f] for f in ("num_valid", "level", "status")], np.int64)})
            for p, (pts, T) in enumerate(x["clouds"] or []):
                out[at + f"cloud{p}"] = np.ascontiguousarray(pts).view(np.uint8)
                out[at + f"cloud{p}_pose"] = T
    return out
