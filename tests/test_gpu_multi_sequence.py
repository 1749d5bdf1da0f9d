"""bpvo_hip_add_frames: many independent VisualOdometry sequences advanced by one context.  Every sequence is compared, bit for bit, with a
context of its own driven by bpvo_hip_add_frame on the same frames: poses, per-level statistics, the key-frame decisions, every point cloud
(fetched right after its key frame), the point counts and the trajectory."""
import ctypes

import numpy as np
import pytest

from bpvo_amd import capi, synth
from util import ROT_TOL, bits_equal, make_params, pose_error, trans_tol

pytestmark = pytest.mark.gpu

ERR_INVALID_ARG, ERR_NO_TEMPLATE = -1, -4      # c_api.h BPVO_ERR_*

# test_gpu_parity.py::test_visual_odometry_add_frame_sequence's key-framing thresholds
KF = dict(minTranslationMagToKeyFrame=0.1, minRotationMagToKeyFrame=2.5, maxFractionOfGoodPointsToKeyFrame=0.7, goodPointThreshold=0.8)


def _sequences(rows, cols, n_frames, specs):
    """specs: (index, step_rot, step_trans) per sequence -> list of lists of (img, disp), and K, b (the same for every index)"""
    seqs = [synth.make_sequence(rows, cols, n_frames, index=i, step_rot=r, step_trans=t) for i, r, t in specs]
    return [s["frames"] for s in seqs], seqs[0]["K"], seqs[0]["b"]


def _snapshot_single(ctx, res):
    cloud = ctx.get_point_cloud() if res["hasPointCloud"] else None
    return dict(res=res, cloud=cloud, npts=ctx.vo_num_points_at_level())


def run_single(b, K, base, rows, cols, params, frames, options=None):
    """the frames of one sequence through add_frame on a context of its own (restarts: None entries start a fresh context)"""
    out, trajs = [], []
    ctx = None
    for f in frames:
        if f is None:
            if ctx is not None:
                trajs.append(ctx.trajectory())
                ctx.close()
            ctx = None
            continue
        if ctx is None:
            ctx = b.create(K, base, rows, cols, params, n_frames=3, n_pairs=1)
            for k, v in (options or {}).items():
                ctx.set_option(k, v)
        out.append(_snapshot_single(ctx, ctx.add_frame(*f)))
    trajs.append(ctx.trajectory())
    ctx.close()
    return out, trajs


def assert_same_result(a, b, what):
    ra, rb = a["res"], b["res"]
    assert bits_equal(ra["pose"], rb["pose"]), (what, "pose", ra["pose"], rb["pose"])
    assert bits_equal(ra["covariance"], rb["covariance"]), (what, "covariance")
    assert len(ra["stats"]) == len(rb["stats"])
    for l, (sa, sb) in enumerate(zip(ra["stats"], rb["stats"])):
        assert sa["numIterations"] == sb["numIterations"] and sa["status"] == sb["status"], (what, "level", l, sa, sb)
        assert np.float32(sa["finalError"]).tobytes() == np.float32(sb["finalError"]).tobytes(), (what, "finalError", l, sa, sb)
        assert np.float32(sa["firstOrderOptimality"]).tobytes() == np.float32(sb["firstOrderOptimality"]).tobytes(), (what, "optimality", l, sa, sb)
    for k in ("isKeyFrame", "keyFramingReason", "hasPointCloud"):
        assert ra[k] == rb[k], (what, k, ra[k], rb[k])
    assert a["npts"] == b["npts"], (what, "num_points_at_level", a["npts"], b["npts"])
    assert (a["cloud"] is None) == (b["cloud"] is None), (what, "cloud")
    if a["cloud"] is not None:
        (pa, Pa), (pb, Pb) = a["cloud"], b["cloud"]
        assert len(pa) > 0 and np.array_equal(pa.view(np.uint8), pb.view(np.uint8)), (what, "point cloud bytes")
        assert bits_equal(Pa, Pb), (what, "point cloud pose")


class Multi:
    """one context serving S sequences; records per sequence what the single path's snapshots record"""

    def __init__(self, b, K, base, rows, cols, params, S, options=None):
        self.ctx = b.create(K, base, rows, cols, params, n_frames=3 * S, n_pairs=S)
        for k, v in (options or {}).items():
            self.ctx.set_option(k, v)
        assert self.ctx.seq_capacity() == S
        self.out = [[] for _ in range(S)]
        self.trajs = [[] for _ in range(S)]

    def call(self, ids, frames, device=False):
        imgs = np.stack([f[0] for f in frames])
        disps = np.stack([f[1] for f in frames])
        if device:
            import torch
            ti = torch.from_numpy(imgs).cuda()
            td = torch.from_numpy(disps).cuda()
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


def assert_sequence_equal(multi, s, single_out, single_trajs):
    assert len(multi.out[s]) == len(single_out), (s, len(multi.out[s]), len(single_out))
    for k, (a, b) in enumerate(zip(multi.out[s], single_out)):
        assert_same_result(a, b, f"sequence {s} frame {k}")
    assert len(multi.trajs[s]) == len(single_trajs)
    for ta, tb in zip(multi.trajs[s], single_trajs):
        assert bits_equal(ta, tb), (s, "trajectory")


def lockstep(hip, K, base, rows, cols, params, seqs, options=None, device=False):
    """every sequence advanced in every call (sequence s = entry s of the call, in order)"""
    S = len(seqs)
    m = Multi(hip, K, base, rows, cols, params, S, options)
    for k in range(len(seqs[0])):
        m.call(list(range(S)), [seqs[s][k] for s in range(S)], device=device)
    m.finish()
    singles = [run_single(hip, K, base, rows, cols, params, seqs[s], options) for s in range(S)]
    for s in range(S):
        assert_sequence_equal(m, s, *singles[s])
    return m, singles


# six sequences; the last one moves fast enough that its second frame key-frames (the branch without a previous frame, vo.cc:161-173)
SMALL_SPECS = [(5, 0.01, 0.06), (1, 0.01, 0.06), (2, 0.004, 0.03), (3, 0.01, 0.08), (7, 0.006, 0.05), (11, 0.002, 0.16)]


def test_small_mixed_keyframing_equals_add_frame_and_the_oracle(hip, orc):
    rows, cols, levels = 120, 160, 3
    seqs, K, base = _sequences(rows, cols, 7, SMALL_SPECS)
    p = make_params(hip, descriptor="intensity", loss="huber", levels=levels, **KF)
    m, singles = lockstep(hip, K, base, rows, cols, p, seqs)
    kf_frames = [tuple(k for k, o in enumerate(m.out[s]) if o["res"]["isKeyFrame"] and k > 0) for s in range(len(seqs))]
    assert any(kf_frames), "the sequences should key-frame"
    assert len(set(kf_frames)) > 1, f"the sequences should key-frame on different frames: {kf_frames}"
    assert any(m.out[s][1]["res"]["isKeyFrame"] for s in range(len(seqs))), "a sequence whose second frame key-frames"
    # ... and the oracle's add_frame, within test_visual_odometry_add_frame_sequence's tolerances
    po = make_params(orc, descriptor="intensity", loss="huber", levels=levels, **KF)
    for s in range(len(seqs)):
        oo, (tro,) = run_single(orc, K, base, rows, cols, po, seqs[s])
        oh = [o["res"] for o in m.out[s]]
        assert [r["keyFramingReason"] for r in oh] == [o["res"]["keyFramingReason"] for o in oo], s
        for a, o in zip(oh, oo):
            rot, trans = pose_error(a["pose"], o["res"]["pose"])
            assert rot <= ROT_TOL and trans <= trans_tol(K), (s, rot, trans)
        assert np.abs(m.trajs[s][0] - tro).max() < 5e-3


def test_reference_order_equals_add_frame_and_the_oracle(hip, orc):
    rows, cols, levels = 120, 160, 3
    seqs, K, base = _sequences(rows, cols, 7, SMALL_SPECS)
    p = make_params(hip, descriptor="intensity", loss="huber", levels=levels, **KF)
    m, _ = lockstep(hip, K, base, rows, cols, p, seqs, options={"reference_reduction": 1})
    po = make_params(orc, descriptor="intensity", loss="huber", levels=levels, **KF)
    for s in range(len(seqs)):
        oo, _ = run_single(orc, K, base, rows, cols, po, seqs[s])
        for k, (a, o) in enumerate(zip(m.out[s], oo)):
            ra, ro = a["res"], o["res"]
            assert bits_equal(ra["pose"], ro["pose"]), (s, k, "pose")
            assert [x["numIterations"] for x in ra["stats"]] == [x["numIterations"] for x in ro["stats"]], (s, k)
            assert [x["status"] for x in ra["stats"]] == [x["status"] for x in ro["stats"]], (s, k)
            assert ra["keyFramingReason"] == ro["keyFramingReason"], (s, k)


def test_full_size_bitplanes(hip):
    """640x480 bit-planes / Tukey, 16 sequences of 6 frames: more frames than levels_in_one_launch_max_frames, the team / chain paths of the
    estimate against the single pair's persistent kernel."""
    rows, cols = 480, 640
    specs = [(i, 0.004 + 0.0005 * (i % 5), 0.03 + 0.01 * (i % 4)) for i in range(16)]
    seqs, K, base = _sequences(rows, cols, 6, specs)
    p = make_params(hip, descriptor="bitplanes", loss="tukey", levels=4, **KF)
    m, _ = lockstep(hip, K, base, rows, cols, p, seqs)
    assert any(o["res"]["isKeyFrame"] for s in range(16) for o in m.out[s][1:])


def test_ragged_calls_permutations_and_reset(hip):
    rows, cols, levels = 120, 160, 3
    S = 5
    seqs, K, base = _sequences(rows, cols, 8, SMALL_SPECS[:S])
    p = make_params(hip, descriptor="intensity", loss="huber", levels=levels, **KF)
    m = Multi(hip, K, base, rows, cols, p, S)
    nxt = [0] * S
    single_frames = [[] for _ in range(S)]
    # (ids of the call; "R<s>": reset sequence s before the call)
    plan = [[0, 1], [2, 1, 0], [4], [3, 0, 4, 2], "R1", [1, 3], [0, 2, 4, 1], [4, 3, 1], "R4", [2, 4, 0, 3], [1, 4], [4, 1, 3], [0, 1, 2, 3, 4]]
    for step in plan:
        if isinstance(step, str):
            s = int(step[1:])
            m.reset(s)
            single_frames[s].append(None)
            continue
        frames = []
        for s in step:
            f = seqs[s][nxt[s] % len(seqs[s])]
            nxt[s] += 1
            frames.append(f)
            single_frames[s].append(f)
        res = m.call(step, frames)
        for s, r in zip(step, res):
            if single_frames[s][-2:-1] == [None] or len(single_frames[s]) == 1:
                assert r["keyFramingReason"] == capi.KF_FIRST_FRAME, (step, s)
    m.finish()
    for s in range(S):
        fr = single_frames[s]
        while fr and fr[0] is None:
            fr.pop(0)
            m.trajs[s].pop(0)
        out, trajs = run_single(hip, K, base, rows, cols, p, fr)
        assert_sequence_equal(m, s, out, trajs)


@pytest.mark.parametrize("descriptor,kw", [("intensity", {}), ("gradient", {}), ("centraldiff", dict(centralDifferenceRadius=4))])
def test_descriptors(hip, descriptor, kw):
    rows, cols, levels = 120, 160, 3
    seqs, K, base = _sequences(rows, cols, 5, [SMALL_SPECS[0], SMALL_SPECS[3], SMALL_SPECS[5]])
    p = make_params(hip, descriptor=descriptor, loss="tukey", levels=levels, **KF, **kw)
    m, _ = lockstep(hip, K, base, rows, cols, p, seqs)
    if descriptor == "centraldiff":
        assert m.ctx.Cn > 48
    else:
        assert m.ctx.Cn == {"intensity": 1, "gradient": 3}[descriptor]


def test_device_inputs_equal_host_inputs(hip):
    rows, cols, levels = 120, 160, 3
    seqs, K, base = _sequences(rows, cols, 5, SMALL_SPECS[:4])
    p = make_params(hip, descriptor="intensity", loss="huber", levels=levels, **KF)
    lockstep(hip, K, base, rows, cols, p, seqs, device=True)


def test_one_sequence_equals_add_frame(hip):
    rows, cols, levels = 120, 160, 3
    seqs, K, base = _sequences(rows, cols, 7, SMALL_SPECS[:1])
    p = make_params(hip, descriptor="bitplanes", loss="tukey", levels=levels, **KF)
    lockstep(hip, K, base, rows, cols, p, seqs)


def test_every_branch_of_the_driver_in_one_call(hip):
    """addframes_scenarios.py's one call: a first frame, no key frame, a key frame without and a key frame with re-estimation, two sequences
    with parameters of their own and different losses (two estimates in the call), one camera of the other size, option "pose_covariance" on.
    Every sequence, over all its frames, against bpvo_hip_add_frame in a context of its own camera and parameters, no tolerance: pose,
    covariance and its record, every level's statistics, the key-frame flags, the point counts of every level, the point clouds' bytes and
    poses, the trajectory."""
    import addframes_scenarios as sc
    from test_gpu_rigs import assert_same_frames
    cams, frames, params, _, own = sc.one_call_setup(hip)
    assert own[1].lossFunction != own[3].lossFunction and (cams[2][2], cams[2][3]) != (cams[0][2], cams[0][3])
    recs, trajs = sc.run_one_call(hip)
    last = [r[-1]["res"] for r in recs]
    before = [r[-2]["res"] if len(r) > 1 else None for r in recs]
    first, none, swap, again = (sc.ROLES.index(x) for x in sc.ROLES)
    assert len(recs[first]) == 1 and last[first]["keyFramingReason"] == capi.KF_FIRST_FRAME, "no first frame in the call"
    assert not last[none]["isKeyFrame"], "the sequence that should take no key frame took one"
    assert last[swap]["isKeyFrame"] and before[swap]["isKeyFrame"] and last[swap]["hasPointCloud"], "no key frame without re-estimation in the call"
    assert last[again]["isKeyFrame"] and not before[again]["isKeyFrame"] and last[again]["hasPointCloud"], "no key frame with re-estimation in the call"
    assert all(len(recs[s]) == sc.ONE_CALL + 1 for s in (none, swap, again))
    for s in range(4):
        want, traj = sc.run_alone(hip, cams[s], frames[s][:len(recs[s])], params[s])
        assert_same_frames(recs[s], want, f"sequence {s} ({sc.ROLES[s]})")
        for k, (a, b) in enumerate(zip(recs[s], want)):
            for (pa, _), (pb, _) in zip(a["clouds"] or [], b["clouds"] or []):
                assert np.array_equal(pa.view(np.uint8), pb.view(np.uint8)), (s, k, "point cloud bytes")
        assert bits_equal(trajs[s], traj), (s, "trajectory")
        assert all(x["cov"]["status"] != capi.COV_NONE for x in recs[s][1:]), (s, "no covariance record")


def test_errors_change_no_sequence(hip):
    rows, cols, levels = 120, 160, 3
    S = 4
    seqs, K, base = _sequences(rows, cols, 4, SMALL_SPECS[:S])
    p = make_params(hip, descriptor="intensity", loss="huber", levels=levels, **KF)
    clean = Multi(hip, K, base, rows, cols, p, S)
    m = Multi(hip, K, base, rows, cols, p, S)
    empty = (seqs[3][0][0], np.zeros_like(seqs[3][0][1]))       # every disparity invalid: an empty template
    for mm in (clean, m):
        mm.call([0, 1, 2], [seqs[s][0] for s in range(3)])
    m.call([3], [empty])                                        # a first frame with an empty template is no error (vo.cc:133-139) ...
    sizes = [len(m.ctx.seq_trajectory(s)) for s in range(S)]
    frames = [seqs[s][1] for s in range(S)]
    imgs, disps = np.stack([f[0] for f in frames]), np.stack([f[1] for f in frames])
    res = (capi.Result * S)()
    fn = hip.fn("add_frames")

    def rc(n, ids, im, di, out):
        p_ids = None if ids is None else np.ascontiguousarray(ids, np.int32).ctypes.data_as(ctypes.c_void_p)
        return fn(m.ctx.h, n, p_ids, im, di, 0, out)

    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    assert rc(2, [0, S], ptr(imgs), ptr(disps), res) == ERR_INVALID_ARG          # an id out of capacity
    assert rc(3, [0, 1, 0], ptr(imgs), ptr(disps), res) == ERR_INVALID_ARG       # a duplicate id
    assert rc(S + 1, None, ptr(imgs), ptr(disps), res) == ERR_INVALID_ARG        # more frames than sequences
    assert rc(2, [0, 1], None, ptr(disps), res) == ERR_INVALID_ARG               # null pointers
    assert rc(2, [0, 1], ptr(imgs), None, res) == ERR_INVALID_ARG
    assert rc(2, [0, 1], ptr(imgs), ptr(disps), None) == ERR_INVALID_ARG
    assert rc(4, [0, 1, 2, 3], ptr(imgs), ptr(disps), res) == ERR_NO_TEMPLATE   # ... the estimate against it is (template_data.cc:177)
    err = hip.fn("last_error", ctypes.c_char_p)(m.ctx.h).decode()
    assert "sequence 3" in err, err
    assert [len(m.ctx.seq_trajectory(s)) for s in range(S)] == sizes                  # no sequence advanced
    with pytest.raises(capi.BpvoError):
        m.ctx.add_frame(*seqs[0][1])                                                  # one mode per context
    assert [len(m.ctx.seq_trajectory(s)) for s in range(S)] == sizes
    # the same call without the bad sequence: what a context that never saw the errors computes
    for mm in (clean, m):
        mm.call([2, 0, 1], [seqs[2][1], seqs[0][1], seqs[1][1]])
        mm.call([0, 1, 2], [seqs[s][2] for s in range(3)])
    for s in range(3):
        assert len(m.out[s]) == len(clean.out[s])
        for k, (a, b) in enumerate(zip(m.out[s], clean.out[s])):
            assert_same_result(a, b, f"sequence {s} frame {k}")
        assert bits_equal(m.ctx.seq_trajectory(s), clean.ctx.seq_trajectory(s))
    # ... and the other way round: a context that ran add_frame refuses add_frames
    single = hip.create(K, base, rows, cols, p, n_frames=3, n_pairs=1)
    single.add_frame(*seqs[0][0])
    with pytest.raises(capi.BpvoError):
        single.add_frames(np.stack([seqs[0][1][0]]), np.stack([seqs[0][1][1]]))
    assert len(single.trajectory()) == 1
