"""Per-sequence algorithm parameters in bpvo_hip_add_frames (bpvo_hip_seq_set_params): a parameter sweep over one dataset in one context.  Every
sequence is compared, bit for bit, with a bpvo_hip_create context of its camera AND its parameters driven by bpvo_hip_add_frame on the same
frames: poses, per-level statistics, key-frame decisions and reasons, point clouds (weights included), point counts and trajectories.  No
tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest

from bpvo_amd import capi, synth
from test_gpu_multi_sequence import KF, Multi, assert_same_result, assert_sequence_equal, run_single
from test_gpu_seq_cameras import KITTI, K_of, MultiCam, drive, frames_for, rc_and_error
from test_gpu_stereo_sequences import StereoMulti, stereo_frames_for, stereo_params
from util import bits_equal, make_params

pytestmark = pytest.mark.gpu

ERR_INVALID_ARG, ERR_UNSUPPORTED, ERR_NO_TEMPLATE = -1, -2, -4      # c_api.h BPVO_ERR_*
ROWS, COLS = 480, 640
LOSS = {"tukey": capi.LOSS_TUKEY, "huber": capi.LOSS_HUBER, "l2": capi.LOSS_L2}
# a second set of key-framing thresholds next to test_gpu_multi_sequence.KF: a larger translation, a smaller fraction at a lower weight
KF2 = dict(minTranslationMagToKeyFrame=0.25, minRotationMagToKeyFrame=2.5, maxFractionOfGoodPointsToKeyFrame=0.5, goodPointThreshold=0.6)
# a disparity gate at the median of the first frame's disparities: as maxValidDisparity the nearer half of the scene leaves the template, as
# minValidDisparity the farther half
GATE = "gate"
# the third minSaliency.  2.5 is what conf/kitti_bitplanes.cfg and conf/kitti_eval.cfg set; the intensity sweep runs it.  The bit-planes saliency
# is |dx| + |dy| of channel 0, a value in [0, 1]: it cannot exceed 2, so 2.5 leaves an EMPTY template on any frame (measured on
# these: 0 points at every level) and the own-context run answers BPVO_ERR_NO_TEMPLATE.  Such a set belongs in a case of its own —
# test_an_empty_template_names_its_sequence_and_leaves_the_others and test_reference_configurations_together, which run 2.5 on bit-planes —
# and the bit-planes sweep takes 1.0 in its place.
HIGH = "high"
HIGH_SALIENCY = {"intensity": 2.5, "bitplanes": 1.0}

# The sweep: between them all three losses, maxIterations 3 / 50 / 200, two settings of each tolerance (the defaults 1e-7 / 1e-6 / 1e-8 and a
# second one), two key-frame threshold sets, minSaliency 0.01 / 0.1 / HIGH and the disparity gate from either side
SWEEP = [
    dict(lossFunction="tukey", maxIterations=50, minSaliency=0.1, **KF),
    dict(lossFunction="huber", maxIterations=200, minSaliency=0.01, parameterTolerance=1e-6, functionTolerance=1e-4, **KF),
    dict(lossFunction="l2", maxIterations=3, minSaliency=0.1, **KF2),
    dict(lossFunction="tukey", maxIterations=3, minSaliency=HIGH, functionTolerance=5e-4, **KF),
    dict(lossFunction="huber", maxIterations=50, minSaliency=0.1, maxValidDisparity=GATE, gradientTolerance=1e-6, **KF),
    dict(lossFunction="l2", maxIterations=200, minSaliency=0.01, parameterTolerance=1e-5, gradientTolerance=1e-4, **KF2),
    dict(lossFunction="tukey", maxIterations=200, minSaliency=0.01, minValidDisparity=GATE, **KF2),
    dict(lossFunction="huber", maxIterations=3, minSaliency=HIGH, **KF2),
]


def sweep_frames(rows=ROWS, cols=COLS, n_frames=6):
    """one dataset for every sequence of a sweep: six frames whose motion key-frames under KF"""
    seq = synth.make_sequence(rows, cols, n_frames, index=5, step_rot=0.01, step_trans=0.06)
    return seq["frames"], seq["K"], seq["b"]


def params_of(hip, base, spec, frames):
    p = capi.Params.from_buffer_copy(base)
    for k, v in (spec or {}).items():
        if k == "lossFunction":
            v = LOSS[v]
        elif v == HIGH:
            v = HIGH_SALIENCY["bitplanes" if base.descriptor == capi.DESC_BITPLANES else "intensity"]
        elif v == GATE:
            d = frames[0][1]
            v = float(np.median(d[d > 0]))
        setattr(p, k, v)
    return p


def sweep_params(hip, desc, frames, specs=SWEEP, levels=4):
    base = make_params(hip, descriptor=desc, loss="tukey", levels=levels, **KF)
    return base, [params_of(hip, base, s, frames) for s in specs]


def params_bytes(p):
    return bytes(memoryview(p))


def make_sweep_ctx(hip, K, b, rows, cols, base, params, options=None):
    S = len(params)
    m = Multi(hip, K, b, rows, cols, base, S, options)
    for s, p in enumerate(params):
        m.ctx.seq_set_params(s, p)
        assert params_bytes(m.ctx.seq_get_params(s)) == params_bytes(p), s
    return m


def run_sweep(hip, K, b, rows, cols, base, params, frames, schedule="lockstep", device=False, options=None, ids=None):
    """sequence s = params[s] over `frames`; ids: the sequences that run (default all)"""
    m = make_sweep_ctx(hip, K, b, rows, cols, base, params, options)
    S = len(params)
    run = list(range(S)) if ids is None else list(ids)
    seqs = [frames if s in run else [] for s in range(S)]
    drive(m, seqs, schedule, device=device)
    return m


def singles_of(hip, K, b, rows, cols, params, frames, options=None):
    """one own-context run per DISTINCT parameter set (sequences that share one share its single)"""
    cache, out = {}, []
    for p in params:
        key = params_bytes(p)
        if key not in cache:
            cache[key] = run_single(hip, K, b, rows, cols, p, frames, options)
        out.append(cache[key])
    return out


def check(m, singles, ids=None):
    for s in (range(len(singles)) if ids is None else ids):
        assert_sequence_equal(m, s, *singles[s])


def assert_not_vacuous(singles, finest=0):
    npts = [o[0][-1]["npts"] for o in singles]
    iters = [tuple(tuple(st["numIterations"] for st in f["res"]["stats"]) for f in o[0]) for o in singles]
    kfs = [tuple(f["res"]["keyFramingReason"] for f in o[0]) for o in singles]
    print("finest-level point counts:", npts)
    print("iterations per frame and level:", iters)
    print("key-framing reasons:", kfs)
    assert len(set(npts)) >= 3, ("the finest-level point counts should take at least three values", npts)
    assert len(set(iters)) >= 2, ("the iteration counts should differ", iters)
    assert len(set(kfs)) >= 2, ("a key-frame decision should differ", kfs)


# ---- 1. a sweep equals contexts of its own -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("desc", ["bitplanes", "intensity"])
@pytest.mark.parametrize("mode", ["default", "reference_reduction"])
def test_a_sweep_equals_contexts_of_its_own(hip, desc, mode):
    frames, K, b = sweep_frames()
    base, params = sweep_params(hip, desc, frames)
    options = {"reference_reduction": 1} if mode == "reference_reduction" else None
    singles = singles_of(hip, K, b, ROWS, COLS, params, frames, options)      # (a set with an empty template level would raise here)
    assert_not_vacuous(singles)
    for device, schedule in ((False, "lockstep"), (True, "subsets")):
        m = run_sweep(hip, K, b, ROWS, COLS, base, params, frames, schedule, device, options)
        check(m, singles)
        for s in range(len(params)):
            for l in range(m.ctx.L):
                assert m.ctx.seq_num_points_at_level(s, l) > 0, (s, l)
        m.ctx.close()


# The good-point count of a table of jobs and the point clouds for the plain layouts besides C = 1 and for wide descriptors, each sequence with a
# loss and a threshold of its own: the sweeps above run bit-planes (tiles, C = 8) and intensity (C = 1) only.  Small frames, three levels.
COUNT_FORMS = {"gradient": {}, "fields2": {}, "centraldiff": dict(centralDifferenceRadius=4)}      # C = 3 and 10 (plain), 80 (wide)
COUNT_SETS = [
    dict(lossFunction="tukey", **KF),
    dict(lossFunction="huber", minTranslationMagToKeyFrame=10, minRotationMagToKeyFrame=2.5, maxFractionOfGoodPointsToKeyFrame=0.9, goodPointThreshold=0.9),
    dict(lossFunction="l2", **KF2),
]


@pytest.mark.parametrize("desc", sorted(COUNT_FORMS))
def test_count_and_cloud_forms_with_parameters_of_their_own(hip, desc):
    """The CPU oracle on these inputs, for all three descriptors: set 1 key-frames by translation at frames 3 and 5 (frame 3: a key frame with
    a second estimate), set 2 by the fraction of good points at every frame (frame 1: a key frame without a previous frame; Huber weights
    against 0.9), set 3 (L2: every weight is 1) never after the first frame."""
    rows, cols = 120, 160
    frames, K, b = sweep_frames(rows, cols, 6)
    base = make_params(hip, descriptor=desc, loss="tukey", levels=3, **KF, **COUNT_FORMS[desc])
    params = [params_of(hip, base, s, frames) for s in COUNT_SETS]
    singles = singles_of(hip, K, b, rows, cols, params, frames)
    kfs = [[f["res"]["keyFramingReason"] for f in o[0]] for o in singles]
    print("key-framing reasons:", kfs)
    assert all(k[0] == capi.KF_FIRST_FRAME for k in kfs), kfs
    assert capi.KF_LARGE_TRANSLATION in kfs[0] and capi.KF_SMALL_FRAC_GOOD in kfs[1], kfs
    assert all(r == capi.KF_NO_KEYFRAMING for r in kfs[2][1:]), kfs
    m = run_sweep(hip, K, b, rows, cols, base, params, frames)
    check(m, singles)
    m.ctx.close()


def test_an_empty_template_names_its_sequence_and_leaves_the_others(hip):
    """bit-planes with conf/kitti_bitplanes.cfg's minSaliency of 2.5, which no bit-planes saliency reaches: the first frame is accepted
    (vo.cc:133-139), the estimate against its empty template is refused before any sequence changes, and the others go on as if it had never
    been there"""
    frames, K, b = sweep_frames(120, 160, 4)
    base, params = sweep_params(hip, "bitplanes", frames, SWEEP[:3], levels=3)
    params[1].minSaliency = 2.5
    m = make_sweep_ctx(hip, K, b, 120, 160, base, params)
    m.call([0, 1, 2], [frames[0]] * 3)
    imgs, disps = np.stack([frames[1][0]] * 3), np.stack([frames[1][1]] * 3)
    res = (capi.Result * 3)()
    rc, msg = rc_and_error(m.ctx, "add_frames", 3, None, imgs.ctypes.data_as(C.c_void_p), disps.ctypes.data_as(C.c_void_p), 0, res)
    assert rc == ERR_NO_TEMPLATE and "sequence 1" in msg, (rc, msg)
    for k in (1, 2, 3):
        m.call([0, 2], [frames[k]] * 2)
    m.finish()
    for s in (0, 2):
        assert_sequence_equal(m, s, *run_single(hip, K, b, 120, 160, params[s], frames))
    with pytest.raises(capi.BpvoError):      # ... and a context of the refused sequence's own fails the same way
        run_single(hip, K, b, 120, 160, params[1], frames[:2])


# ---- 2. every estimate path ------------------------------------------------------------------------------------------------------------------
CHAIN = {"team": 0, "persistent": 0}
PATHS = {
    "persistent_one_per_call": (None, "one"),
    "team_fixed": ({"team_join": 0}, 6),
    "team_growing": ({"team_join": 2, "team_join_from_pairs": 2}, 6),
    "chain_step_in_reduce": (dict(CHAIN, step_in_reduce_max_pairs=128, fuse_frozen=1), 8),
    "chain_four_kernels": (dict(CHAIN, step_in_reduce_max_pairs=0, fuse_frozen=1), 8),
    "chain_unfused": (dict(CHAIN, step_in_reduce_max_pairs=0, fuse_frozen=0), 8),
    "chain_unfused_step_in_reduce": (dict(CHAIN, step_in_reduce_max_pairs=128, fuse_frozen=0), 8),
}


@pytest.mark.parametrize("path", sorted(PATHS))
def test_every_estimate_path(hip, path):
    options, count = PATHS[path]
    frames, K, b = sweep_frames()
    base, params = sweep_params(hip, "bitplanes", frames)
    singles = singles_of(hip, K, b, ROWS, COLS, params, frames)
    if count == "one":      # one sequence per call: the single pair's persistent kernel, with each sequence's parameters in turn
        m = make_sweep_ctx(hip, K, b, ROWS, COLS, base, params)
        for k in range(len(frames)):
            for s in range(len(params)):
                m.call([s], [frames[k]])
        m.finish()
        levels, gave_up = m.ctx.persistent_counts()
        assert levels > 0 and not gave_up
        check(m, singles)
        return
    m = run_sweep(hip, K, b, ROWS, COLS, base, params[:count], frames, options=options)
    check(m, singles[:count])
    if path.startswith("team"):
        assert m.ctx.team_counts() > 0, "the team kernel should have run"


def test_a_batch_above_team_max_pairs(hip):
    """136 sequences of 160x120 with ONE loss (so that one estimate holds them all: the chain with active lists) and everything else swept —
    then with the losses mixed as well (three estimates of about 45)"""
    rows, cols = 120, 160
    frames, K, b = sweep_frames(rows, cols, 4)
    for one_loss in (True, False):
        specs = [dict(s, lossFunction="tukey") if one_loss else s for s in SWEEP]
        base, eight = sweep_params(hip, "bitplanes", frames, specs, levels=3)
        eight[3].minSaliency = eight[7].minSaliency = 0.5
        params = [eight[s % 8] for s in range(136)]
        singles = singles_of(hip, K, b, rows, cols, params, frames)
        m = run_sweep(hip, K, b, rows, cols, base, params, frames)
        check(m, singles)
        m.ctx.close()


# ---- 3. unequal iteration limits ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("options", [None, CHAIN], ids=["team", "chain"])
def test_unequal_iteration_limits(hip, options):
    frames, K, b = sweep_frames()
    base = make_params(hip, descriptor="bitplanes", loss="tukey", levels=4, **KF)
    params = []
    for it in (1, 200, 1, 200, 5, 50):
        p = capi.Params.from_buffer_copy(base)
        p.maxIterations = it
        params.append(p)
    singles = singles_of(hip, K, b, ROWS, COLS, params, frames)
    m = run_sweep(hip, K, b, ROWS, COLS, base, params, frames, options=options)
    check(m, singles)
    s1, s200 = m.out[0], m.out[1]
    print("maxIterations 1:", [[(st["numIterations"], st["status"]) for st in f["res"]["stats"]] for f in s1[1:]])
    print("maxIterations 200:", [[(st["numIterations"], st["status"]) for st in f["res"]["stats"]] for f in s200[1:]])
    for k in range(1, len(frames)):
        for l in range(m.ctx.L):
            a, w = s1[k]["res"]["stats"][l], singles[0][0][k]["res"]["stats"][l]
            assert (a["numIterations"], a["status"]) == (w["numIterations"], w["status"]), (k, l, a, w)
            a, w = s200[k]["res"]["stats"][l], singles[1][0][k]["res"]["stats"][l]
            assert (a["numIterations"], a["status"]) == (w["numIterations"], w["status"]), (k, l, a, w)
    st1 = [st for f in s1[1:] for st in f["res"]["stats"]]
    st200 = [st for f in s200[1:] for st in f["res"]["stats"]]
    assert any(st["status"] == capi.STATUS_MAX_ITERATIONS for st in st1), "the limit of 1 should be what ends a level"
    assert max(st["numIterations"] for st in st1) < max(st["numIterations"] for st in st200), "the neighbour's limit must not show in the statistics"


# ---- 4. with the other per-sequence features ---------------------------------------------------------------------------------------------------
def test_mixed_cameras_and_mixed_parameters(hip):
    cams = [(K_of(fx, fx, cx, cy), bl, r, c) for r, c, fx, cx, cy, bl in KITTI for _ in range(2)]
    seqs = frames_for(cams, 6)
    base = make_params(hip, descriptor="bitplanes", loss="tukey", levels=4, **KF)
    params = [params_of(hip, base, SWEEP[s], seqs[s]) for s in range(len(cams))]
    singles = [run_single(hip, K, bl, r, c, params[s], seqs[s]) for s, (K, bl, r, c) in enumerate(cams)]
    for device, schedule in ((False, "subsets"), (True, "lockstep")):
        ctx = hip.create_sequences(cams, base)
        for s, p in enumerate(params):
            ctx.seq_set_params(s, p)
        m = MultiCam(ctx, len(cams))
        drive(m, seqs, schedule, device=device)
        check(m, singles)
        ctx.close()


def test_stereo_with_mixed_parameters(hip):
    from test_gpu_stereo_sequences import cameras, run_single_stereo
    cams = cameras()
    which, n_frames = [0, 1, 3, 4], 5
    base = make_params(hip, levels=4, **KF)
    seqs = stereo_frames_for(cams, n_frames, which)
    specs = {0: SWEEP[1], 1: SWEEP[2], 3: SWEEP[5], 4: SWEEP[0]}
    params = {s: params_of(hip, base, {k: v for k, v in specs[s].items() if v != GATE}, None) for s in which}
    singles = {s: run_single_stereo(hip, cams[s], params[s], seqs[s], "bm") for s in which}
    for device in (False, True):
        ctx = hip.create_sequences(cams, base)
        for s in which:
            ctx.seq_set_params(s, params[s])
        m = StereoMulti(ctx, len(cams), stereo_params(ctx, "bm"))
        for k in range(n_frames):
            m.call(which, [seqs[s][k] for s in which], device=device)
        m.finish(which)
        for s in which:
            assert_sequence_equal(m, s, *singles[s])
        ctx.close()


# ---- 5. reference configurations together ----------------------------------------------------------------------------------------------------
# what a sequence may own of four of the reference's conf/*.cfg files that run bit-planes, brought to one pyramid (four levels) and to the
# context's descriptor parameters: kitti_bitplanes, perf_bitplanes, tsukuba_eval, tunnel
REFERENCE_CONFIGS = [
    dict(lossFunction="huber", maxIterations=100, parameterTolerance=1e-6, functionTolerance=1e-4, minSaliency=2.5, minTranslationMagToKeyFrame=1.0,
         minRotationMagToKeyFrame=2.5, maxFractionOfGoodPointsToKeyFrame=0.6, relaxTolerancesForCoarseLevels=1),
    dict(lossFunction="l2", maxIterations=50, parameterTolerance=1e-6, functionTolerance=1e-4, minTranslationMagToKeyFrame=0.1,
         minRotationMagToKeyFrame=5.0, relaxTolerancesForCoarseLevels=1),
    dict(lossFunction="huber", maxIterations=100, parameterTolerance=1e-6, functionTolerance=1e-6, gradientTolerance=1e-6, minSaliency=0.005,
         minTranslationMagToKeyFrame=0.1, minRotationMagToKeyFrame=5.0, maxFractionOfGoodPointsToKeyFrame=0.75, goodPointThreshold=0.75,
         relaxTolerancesForCoarseLevels=0),
    dict(lossFunction="huber", maxIterations=100, parameterTolerance=1e-6, functionTolerance=5e-4, minTranslationMagToKeyFrame=0.0,
         minRotationMagToKeyFrame=2.5, minSaliency=0.05),
]


def test_reference_configurations_together(hip):
    """Four sequences of one context.  kitti_bitplanes' minSaliency of 2.5 leaves an empty bit-planes template (see HIGH above): its own context
    accepts the first frame and refuses the second with BPVO_ERR_NO_TEMPLATE, and so does the call that holds its sequence, naming it and
    changing nothing; the other three run on beside it and equal their own contexts."""
    frames, K, b = sweep_frames()
    base = make_params(hip, descriptor="bitplanes", loss="tukey", levels=4)
    params = [params_of(hip, base, s, frames) for s in REFERENCE_CONFIGS]
    with pytest.raises(capi.BpvoError, match="status -4"):
        run_single(hip, K, b, ROWS, COLS, params[0], frames[:2])
    singles = [None] + singles_of(hip, K, b, ROWS, COLS, params[1:], frames)
    m = make_sweep_ctx(hip, K, b, ROWS, COLS, base, params)
    m.call([0, 1, 2, 3], [frames[0]] * 4)
    assert [m.ctx.seq_num_points_at_level(s, 0) > 0 for s in range(4)] == [False, True, True, True]
    imgs, disps = np.stack([frames[1][0]] * 4), np.stack([frames[1][1]] * 4)
    res = (capi.Result * 4)()
    rc, msg = rc_and_error(m.ctx, "add_frames", 4, None, imgs.ctypes.data_as(C.c_void_p), disps.ctypes.data_as(C.c_void_p), 0, res)
    assert rc == ERR_NO_TEMPLATE and "sequence 0" in msg, (rc, msg)
    for k in range(1, len(frames)):
        m.call([1, 2, 3], [frames[k]] * 3)
    m.finish()
    check(m, singles, ids=(1, 2, 3))
    assert m.ctx.seq_get_params(2).relaxTolerancesForCoarseLevels == 0      # (a field the library never reads: returned as set)


# ---- 6. nothing changes for uniform parameters ---------------------------------------------------------------------------------------------
def test_uniform_parameters_change_nothing(hip):
    frames, K, b = sweep_frames()
    base = make_params(hip, descriptor="bitplanes", loss="tukey", levels=4, **KF)
    S = 6
    runs = []
    for given in (False, True):
        m = Multi(hip, K, b, ROWS, COLS, base, S)
        if given:
            for s in range(S):
                m.ctx.seq_set_params(s, m.ctx.seq_get_params(s))
        m.ctx.profiling(2)
        drive(m, [frames] * S, "lockstep")
        stats = {k["name"]: k["launches"] for k in m.ctx.kernel_stats()}
        runs.append((m, stats))
    (plain, launches_plain), (given, launches_given) = runs
    print("launches:", launches_plain)
    assert launches_plain == launches_given and sum(launches_plain.values()) > 0
    for s in range(S):
        for k, (x, y) in enumerate(zip(given.out[s], plain.out[s])):
            assert_same_result(x, y, f"sequence {s} frame {k}")
        assert bits_equal(given.trajs[s][0], plain.trajs[s][0])


# ---- 7. errors ------------------------------------------------------------------------------------------------------------------------------------
STRUCTURAL = dict(numPyramidLevels=2, minImageDimensionForPyramid=50, descriptor=capi.DESC_INTENSITY, sigmaPriorToCensusTransform=0.9,
                  sigmaBitPlanes=1.1, dfSigma1=0.6, dfSigma2=1.9, latchNumBytes=2, latchRotationInvariance=1, latchHalfSsdSize=2,
                  centralDifferenceRadius=2, centralDifferenceSigmaBefore=0.5, centralDifferenceSigmaAfter=1.5, laplacianKernelSize=3,
                  gradientEstimation=capi.GRAD_CD5, interp=capi.INTERP_CUBIC, withNormalization=0, nonMaxSuppRadius=2,
                  minNumPixelsForNonMaximaSuppression=1000, maxTestLevel=1)


def test_errors(hip):
    rows, cols = 120, 160
    frames, K, b = sweep_frames(rows, cols, 4)
    base, params = sweep_params(hip, "bitplanes", frames, SWEEP[:3], levels=3)
    m = make_sweep_ctx(hip, K, b, rows, cols, base, params)
    ctx = m.ctx
    before = [params_bytes(ctx.seq_get_params(s)) for s in range(3)]
    unchanged = lambda: [params_bytes(ctx.seq_get_params(s)) for s in range(3)] == before
    fields = {f[0] for f in capi.Params._fields_}
    for name, value in STRUCTURAL.items():
        assert name in fields, name
        q = capi.Params.from_buffer_copy(params[1])
        assert getattr(q, name) != value, name
        setattr(q, name, value)
        rc, msg = rc_and_error(ctx, "seq_set_params", 1, C.byref(q))
        assert rc == ERR_UNSUPPORTED and name in msg and "sequence 1" in msg, (name, rc, msg)
        assert unchanged(), name
    q = capi.Params.from_buffer_copy(params[1])
    q.lossFunction = 77
    rc, msg = rc_and_error(ctx, "seq_set_params", 1, C.byref(q))
    assert rc == ERR_UNSUPPORTED and "lossFunction" in msg and unchanged(), (rc, msg)      # bpvo_hip_create's code for it
    with pytest.raises(capi.BpvoError):
        bad = capi.Params.from_buffer_copy(base)
        bad.lossFunction = 77
        hip.create(K, b, rows, cols, bad)
    q = capi.Params.from_buffer_copy(params[1])
    q.numPyramidLevels = -1      # automatic: 1 + round(log2(120 / 40)) = 3 levels for this size, the context's count — accepted
    q.maxIterations = 7
    assert rc_and_error(ctx, "seq_set_params", 1, C.byref(q))[0] == 0 and ctx.seq_get_params(1).maxIterations == 7
    ctx.seq_set_params(1, params[1])
    for seq in (-1, 3):
        rc, msg = rc_and_error(ctx, "seq_set_params", seq, C.byref(params[0]))
        assert rc == ERR_INVALID_ARG and unchanged(), (seq, rc, msg)
        assert ctx.b.fn("seq_get_params")(ctx.h, seq, C.byref(capi.Params())) == ERR_INVALID_ARG
    rc, msg = rc_and_error(ctx, "seq_set_params", 0, None)
    assert rc == ERR_INVALID_ARG and unchanged(), (rc, msg)
    assert ctx.b.fn("seq_get_params")(ctx.h, 0, None) == ERR_INVALID_ARG
    # refused once the sequence holds a frame, accepted again after a reset
    m.call([0, 1, 2], [frames[0]] * 3)
    rc, msg = rc_and_error(ctx, "seq_set_params", 2, C.byref(params[0]))
    assert rc == ERR_INVALID_ARG and "sequence 2" in msg and unchanged(), (rc, msg)
    # ... and what follows still equals the singles
    for k in (1, 2, 3):
        m.call([0, 1, 2], [frames[k]] * 3)
    m.finish()
    check(m, singles_of(hip, K, b, rows, cols, params, frames))
    ctx.seq_reset(2)
    assert params_bytes(ctx.seq_get_params(2)) == before[2]      # a reset keeps the parameters
    ctx.seq_set_params(2, params[1])
    assert params_bytes(ctx.seq_get_params(2)) == before[1]
    m2 = Multi.__new__(Multi)
    m2.ctx, m2.out, m2.trajs = ctx, [[] for _ in range(3)], [[] for _ in range(3)]
    for k in range(4):
        m2.call([2], [frames[k]])
    m2.trajs[2].append(ctx.seq_trajectory(2))
    assert_sequence_equal(m2, 2, *run_single(hip, K, b, rows, cols, params[1], frames))
    # a context that runs add_frame refuses the setter; one that took the setter refuses add_frame
    single = hip.create(K, b, rows, cols, base, n_frames=3, n_pairs=1)
    single.add_frame(*frames[0])
    rc, msg = rc_and_error(single, "seq_set_params", 0, C.byref(params[1]))
    assert rc == ERR_INVALID_ARG and "add_frame" in msg, (rc, msg)
    assert params_bytes(single.seq_get_params(0)) == params_bytes(base)
    fresh = hip.create(K, b, rows, cols, base, n_frames=3, n_pairs=1)
    assert params_bytes(fresh.seq_get_params(0)) == params_bytes(base)      # never given parameters: the context's
    fresh.seq_set_params(0, params[1])
    with pytest.raises(capi.BpvoError):
        fresh.add_frame(*frames[0])
