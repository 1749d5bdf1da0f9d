"""Pose scoring on the device (c_api.h bpvo_hip_score_poses / _pairs / bpvo_hip_estimate_pose_best_start; kernels_score.hip) against the
numpy statement of the score (tests/pose_score_ref.py) evaluated on the ORACLE's residuals and valid flags and on the library's own
bpvo_hip_linearize: counts exact, cost_sum within the bound of an f64 sum of non-negative terms in any order, score by the formula; template
sizes that break indexing; bit determinism and independence of the launch's shape; no trace in any workspace; the refusals; and the starts the
score rescues (the identity start's failure on those scenes is asserted on the oracle: tests/test_pose_score_cpu.py)."""
import ctypes as C

import numpy as np
import pytest

import hostile_poses as hp
import pose_score_ref as ref
from bpvo_amd import capi, synth
from util import bits_equal, make_params, perturbed_pose, pose_error, setup_pair

pytestmark = pytest.mark.gpu

# descriptor: (channels, tau in its units)
DESCRIPTORS = {"intensity": (1, 30.0), "bitplanes": (8, 0.5), "gradient": (3, 15.0), "fields2": (10, 1.0)}
FORMULATIONS = {"f64": 0, "project_points": 1, "dspace": 2}


def pair_context(binding, descriptor, formulation=0, rows=96, cols=128, levels=3, **kw):
    ctx, d, _ = setup_pair(binding, rows, cols, descriptor=descriptor, levels=levels, **kw)
    X = ctx.get_points(0, 0)      # RigidBodyWarp's points: the hostile poses are built from them whatever the formulation
    if formulation:
        ctx.set_warp_formulation(formulation)
        ctx.frame_set_template(0)
    return ctx, d, X


def same_records(a, b):
    return a.shape == b.shape and a.dtype == b.dtype == capi.POSE_SCORE and a.tobytes() == b.tobytes()


def assert_record(got, want, C, N, tau, at):
    """One device record against the reference record of the same pose."""
    assert int(got["n_valid"]) == int(want["n_valid"]) and int(got["n_below"]) == int(want["n_below"]), (at, got, want)
    assert abs(float(got["cost_sum"]) - float(want["cost_sum"])) <= ref.cost_sum_bound(want, C), (at, got["cost_sum"], want["cost_sum"])
    assert float(got["score"]) == ref.score_from_formula(got["cost_sum"], got["n_valid"], N, C, tau), (at, got)


def many_poses(n):
    return np.stack([perturbed_pose(s) for s in np.linspace(-40.0, 40.0, n)])


# ---- 1. parity ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("formulation", list(FORMULATIONS))
@pytest.mark.parametrize("descriptor", list(DESCRIPTORS))
def test_scores_are_the_definition_on_the_oracles_and_the_librarys_residuals(hip, orc, descriptor, formulation):
    Cn, tau = DESCRIPTORS[descriptor]
    ch, d, X = pair_context(hip, descriptor, FORMULATIONS[formulation])
    co, _, _ = pair_context(orc, descriptor, FORMULATIONS[formulation])
    assert ch.Cn == co.Cn == Cn
    poses = {"identity": np.eye(4, dtype=np.float32), "T_gt": d["T_gt"].astype(np.float32), "perturbed_1": perturbed_pose(1), "perturbed_30": perturbed_pose(30)}
    poses.update({"hostile_" + k: v for k, v in hp.poses(d["K"], X, 96, 128).items()})
    names = list(poses)
    stack = np.stack([poses[k] for k in names])
    truncated = False
    for level in range(ch.L):
        N = ch.num_points(0, level)
        assert N == co.num_points(0, level) and N > 0
        got = ch.score_poses(0, 1, level, stack, tau)      # no hostile pose raises
        for k, name in enumerate(names):
            at = (descriptor, formulation, "level", level, name)
            with np.errstate(all="ignore"):
                want_o = ref.score_by_linearize(co, 0, 1, level, poses[name], tau)
                want_h = ref.score_by_linearize(ch, 0, 1, level, poses[name], tau)
            assert_record(got[k], want_o, Cn, N, tau, at + ("oracle",))
            assert_record(got[k], want_h, Cn, N, tau, at + ("bpvo_hip_linearize",))
            if name in ("hostile_nan", "hostile_inf", "hostile_overflow"):
                assert (got[k]["n_valid"], got[k]["n_below"], got[k]["cost_sum"], got[k]["score"]) == (0, 0, 0.0, float(np.float32(tau))), at
            truncated = truncated or 0 < got[k]["n_below"] < got[k]["n_valid"] * Cn
        assert got[names.index("identity")]["n_valid"] > 0
    assert truncated, "no pose had terms on both sides of tau: the truncation was not exercised"
    ch.close(); co.close()


# ---- 2. shapes that break indexing ----------------------------------------------------------------------------------------------------------
SHAPES = {"intensity": dict(levels=4), "bitplanes": dict(levels=3, minSaliency=1.0)}


@pytest.mark.parametrize("descriptor", list(SHAPES))
def test_template_sizes_below_and_across_chunks_and_pose_counts(hip, descriptor):
    """96x128 gives templates of fewer than 256 points, of a count that is no multiple of 256 and of many chunks; P in {1, 7, 17, 65, 1000} poses in
    a call (every pose-tile size the host picks); the records of a pose do not depend on P, on its place in the list or on its neighbours."""
    Cn, tau = DESCRIPTORS[descriptor]
    ch, d, _ = pair_context(hip, descriptor, **SHAPES[descriptor])
    sizes = [ch.num_points(0, l) for l in range(ch.L)]
    print(descriptor, "template sizes", sizes)
    assert any(0 < n < 256 for n in sizes) and any(n > 256 and n % 256 for n in sizes) and any(n > 2048 for n in sizes), sizes
    poses = many_poses(1000)
    rng = np.random.RandomState(7)
    perm = rng.permutation(len(poses))
    for level, N in enumerate(sizes):
        full = ch.score_poses(0, 1, level, poses, tau)
        assert same_records(full, ch.score_poses(0, 1, level, poses, tau)), (level, "two calls differ")
        for P in (1, 7, 17, 65):
            assert same_records(ch.score_poses(0, 1, level, poses[:P], tau), full[:P]), (level, P)
        assert same_records(ch.score_poses(0, 1, level, poses[perm], tau), full[perm]), (level, "permuted list")
        for k in (0, 6, 16, 64, 500, 999):
            assert_record(full[k], ref.score_by_linearize(ch, 0, 1, level, poses[k], tau), Cn, N, tau, (descriptor, level, k))
        equal = ch.score_poses(0, 1, level, np.repeat(poses[421:422], 65, axis=0), tau)
        assert all(equal[k].tobytes() == full[421].tobytes() for k in range(65)), level
    ch.close()


def test_an_empty_level_scores_tau(hip):
    """minSaliency raised until a level of the template is empty: cost_sum 0, both counts 0, score = tau for every pose, the hostile ones included."""
    poses = np.stack([np.eye(4, dtype=np.float32), perturbed_pose(5), np.full((4, 4), np.nan, np.float32)])
    for min_saliency in (10.0, 20.0, 30.0, 40.0, 60.0, 80.0, 100.0, 1000.0, 1e6):
        ch, _, _ = pair_context(hip, "intensity", levels=4, minSaliency=min_saliency)
        sizes = [ch.num_points(0, l) for l in range(ch.L)]
        if 0 in sizes:
            break
        ch.close()
    else:
        raise AssertionError("no minSaliency up to 1e6 empties a level")
    print("minSaliency", min_saliency, "template sizes", sizes)
    for level, N in enumerate(sizes):
        got = ch.score_poses(0, 1, level, poses, 30.0)
        if N == 0:
            assert all((r["cost_sum"], r["score"], r["n_valid"], r["n_below"]) == (0.0, 30.0, 0, 0) for r in got), (level, got)
        else:
            assert got[0]["n_valid"] > 0 and got[2]["n_valid"] == 0 and got[2]["score"] == 30.0, (level, got)
    ch.close()


def test_at_least_4096_poses_in_one_call(hip):
    ch, _, _ = pair_context(hip, "bitplanes")
    poses = many_poses(4099)
    got = ch.score_poses(0, 1, 2, poses, 0.5)
    for k in (0, 2048, 4098):
        assert got[k].tobytes() == ch.score_poses(0, 1, 2, poses[k:k + 1], 0.5)[0].tobytes(), k
    ch.close()


# ---- 3. determinism and independence --------------------------------------------------------------------------------------------------------
def test_pairs_of_two_image_sizes_in_one_launch_equal_each_pair_alone(hip):
    """Three pairs, two image sizes, in one bpvo_hip_create_sequences context (pair s on the slots 3s, 3s + 1 of sequence s): every pair's
    records of the one launch are those of bpvo_hip_score_poses on it alone, bit for bit, and one of each size is checked against the definition."""
    shapes = [(96, 128, 3), (120, 160, 4), (96, 128, 5)]
    pairs = [synth.make_pair(r, c, i) for r, c, i in shapes]
    p = make_params(hip, descriptor="bitplanes", levels=3)
    ch = hip.create_sequences([capi.camera(d["K"], d["b"], r, c) for d, (r, c, _) in zip(pairs, shapes)], p)
    for s, d in enumerate(pairs):
        for slot, img, disp in ((3 * s, d["imgA"], d["dispA"]), (3 * s + 1, d["imgB"], d["dispB"])):
            img, disp = np.ascontiguousarray(img, np.uint8), np.ascontiguousarray(disp, np.float32)
            ch.call("frame_set_data", slot, img.ctypes.data_as(C.c_void_p), disp.ctypes.data_as(C.c_void_p))
        ch.frame_set_template(3 * s)
    refs, curs = [0, 3, 6], [1, 4, 7]
    P = 23
    poses = np.stack([np.roll(many_poses(P), s, axis=0) for s in range(3)])      # [3, P, 4, 4], every pair its own list
    for level in range(3):
        sizes = [ch.num_points(r, level) for r in refs]
        assert sizes[0] != sizes[1], sizes
        together = ch.score_poses_pairs(refs, curs, level, poses, 0.5)
        assert same_records(together, ch.score_poses_pairs(refs, curs, level, poses, 0.5))
        for s in range(3):
            alone = ch.score_poses(refs[s], curs[s], level, poses[s], 0.5)
            assert same_records(together[s], alone), (level, s)
        back = ch.score_poses_pairs(refs[::-1], curs[::-1], level, poses[::-1], 0.5)
        assert same_records(back[::-1].copy(), together), (level, "pairs in another order")
        for s in (0, 1):
            for k in (0, P - 1):
                assert_record(together[s, k], ref.score_by_linearize(ch, refs[s], curs[s], level, poses[s, k], 0.5, ws=s), 8, sizes[s], 0.5, (level, s, k))
    ch.close()


# ---- 4. no interference ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("descriptor", ["bitplanes", "intensity"])
def test_scoring_leaves_no_trace_in_the_workspace(hip, descriptor):
    Cn, tau = DESCRIPTORS[descriptor]
    ch, d, _ = pair_context(hip, descriptor)
    ch.linearize(0, 0, 1, 0, perturbed_pose(2), reset_scale=True)
    before = (ch.get_residuals(0), ch.get_valid(0), ch.get_weights(0))
    lin_before = ch.total_linearizations()
    for level in range(ch.L):
        ch.score_poses(0, 1, level, many_poses(40), tau)
    assert ch.total_linearizations() == lin_before
    after = (ch.get_residuals(0), ch.get_valid(0), ch.get_weights(0))
    assert all(bits_equal(a, b) for a, b in zip(before, after))
    ch.close()
    # ... and an estimate behind scoring calls is the estimate of a context that never scored
    scored, _, _ = pair_context(hip, descriptor)
    for level in range(scored.L):
        scored.score_poses(0, 1, level, many_poses(40), tau)
    T_after, st_after = scored.estimate_pose(0, 0, 1)
    assert scored.total_linearizations() > 0
    scored.close()
    fresh, _, _ = pair_context(hip, descriptor)
    T_fresh, st_fresh = fresh.estimate_pose(0, 0, 1)
    fresh.close()
    assert bits_equal(T_after, T_fresh)
    assert [(s["numIterations"], s["status"], np.float32(s["finalError"]).tobytes(), np.float32(s["firstOrderOptimality"]).tobytes()) for s in st_after] == \
           [(s["numIterations"], s["status"], np.float32(s["finalError"]).tobytes(), np.float32(s["firstOrderOptimality"]).tobytes()) for s in st_fresh]


# ---- 5. refusals ----------------------------------------------------------------------------------------------------------------------------
def refused(ctx, status, call, *args, **kw):
    with pytest.raises(capi.BpvoError) as e:
        call(*args, **kw)
    text = str(e.value)
    assert text.startswith("status %d: " % status) and len(text) > len("status %d: " % status), text
    msg = ctx.b.fn("last_error", C.c_char_p)(ctx.h)
    assert msg and msg.decode() in text
    return text


def test_refusals(hip):
    INVALID, UNSUPPORTED, NO_DATA, NO_TEMPLATE = -1, -2, -3, -4
    eye = np.eye(4, dtype=np.float32)[None]
    d = synth.make_pair(96, 128, 0)
    p = make_params(hip, descriptor="bitplanes", levels=3)
    ch = hip.create(d["K"], d["b"], 96, 128, p, n_frames=3, n_pairs=1)
    ch.frame_set_data(0, d["imgA"], d["dispA"])
    ch.frame_set_data(1, d["imgB"], d["dispB"])
    refused(ch, NO_TEMPLATE, ch.score_poses, 0, 1, 2, eye, 0.5)
    ch.frame_set_template(0)
    refused(ch, NO_DATA, ch.score_poses, 0, 2, 2, eye, 0.5)
    assert ch.score_poses(0, 1, 2, eye, 0.5)[0]["n_valid"] > 0
    for level in (-1, 3, 99):
        refused(ch, INVALID, ch.score_poses, 0, 1, level, eye, 0.5)
    refused(ch, INVALID, ch.score_poses, 0, 1, 2, np.zeros((0, 4, 4), np.float32), 0.5)
    out = np.zeros(1, capi.POSE_SCORE)
    refused(ch, INVALID, ch.call, "score_poses", 0, 1, 2, -1, eye.ctypes.data_as(C.c_void_p), C.c_float(0.5), out.ctypes.data_as(C.c_void_p))
    for tau in (0.0, -1.0, float("nan"), float("inf")):
        refused(ch, INVALID, ch.score_poses, 0, 1, 2, eye, tau)
        refused(ch, INVALID, ch.score_poses_pairs, [0], [1], 2, eye[None], tau)
        refused(ch, INVALID, ch.estimate_pose_best_start, 0, 0, 1, eye, tau)
    refused(ch, INVALID, ch.call, "score_poses", 0, 1, 2, 1, None, C.c_float(0.5), out.ctypes.data_as(C.c_void_p))
    refused(ch, INVALID, ch.call, "score_poses", 0, 1, 2, 1, eye.ctypes.data_as(C.c_void_p), C.c_float(0.5), None)
    refused(ch, INVALID, ch.score_poses, 7, 1, 2, eye, 0.5)
    slots = np.array([0, 1], np.int32)
    refused(ch, INVALID, ch.call, "score_poses_pairs", 0, slots.ctypes.data_as(C.c_void_p), slots[1:].ctypes.data_as(C.c_void_p), 2, 1,
            eye.ctypes.data_as(C.c_void_p), C.c_float(0.5), out.ctypes.data_as(C.c_void_p))
    refused(ch, INVALID, ch.estimate_pose_best_start, 0, 0, 1, eye, 0.5, score_level=3)
    ch.close()
    ch, _, _ = pair_context(hip, "bitplanes", interp=capi.INTERP_CUBIC)
    assert "kCubic" in refused(ch, UNSUPPORTED, ch.score_poses, 0, 1, 2, eye, 0.5)
    ch.close()
    ch, _, _ = pair_context(hip, "latch", rows=120, cols=160, levels=2, latchNumBytes=16)
    assert ch.Cn == 128 and "128" in refused(ch, UNSUPPORTED, ch.score_poses, 0, 1, 1, eye, 0.5)
    ch.close()


# ---- 6. best start --------------------------------------------------------------------------------------------------------------------------
def stats_key(st):
    return [(s["numIterations"], s["status"], np.float32(s["finalError"]).tobytes(), np.float32(s["firstOrderOptimality"]).tobytes()) for s in st]


@pytest.mark.parametrize("descriptor,rows,cols,index,max_trans", [f for f in ref.FIXTURES if f[1:3] == (120, 160)])
def test_the_estimate_starts_at_the_best_candidate(hip, orc, descriptor, rows, cols, index, max_trans):
    assert (rows, cols) == (120, 160)
    d = ref.fixture_pair(rows, cols, index, max_trans)
    cands = ref.candidates(d)
    tau = ref.TAU[descriptor]

    def context(binding):
        ctx = binding.create(d["K"], d["b"], rows, cols, make_params(binding, descriptor=descriptor, levels=3), n_frames=2, n_pairs=1)
        ctx.frame_set_data(0, d["imgA"], d["dispA"])
        ctx.frame_set_template(0)
        ctx.frame_set_data(1, d["imgB"], d["dispB"])
        return ctx
    ch, co = context(hip), context(orc)
    for reference in (0, 1):
        ch.set_option("reference_reduction", reference)
        T, st, chosen, scores = ch.estimate_pose_best_start(0, 0, 1, cands, tau, score_level=ref.SCORE_LEVEL)
        print(descriptor, index, max_trans, "scores", scores["score"].tolist(), "chosen", chosen, "error", pose_error(T, d["T_gt"]))
        assert chosen == ref.WINNER == int(np.argmin(scores["score"])), scores
        assert same_records(scores, ch.score_poses(0, 1, ref.SCORE_LEVEL, cands, tau))
        T_plain, st_plain = ch.estimate_pose(0, 0, 1, cands[chosen])
        assert bits_equal(T, T_plain) and stats_key(st) == stats_key(st_plain)
        if reference:
            T_orc, st_orc = co.estimate_pose(0, 0, 1, cands[chosen])
            assert bits_equal(T, T_orc) and stats_key(st) == stats_key(st_orc), (T, T_orc, st, st_orc)
        assert pose_error(T, d["T_gt"])[1] < 0.05
    # the coarsest level is the default score level; ties go to the lowest index
    T2, _, chosen2, _ = ch.estimate_pose_best_start(0, 0, 1, cands, tau)
    assert chosen2 == ref.WINNER
    twice = np.concatenate([cands[ref.WINNER:ref.WINNER + 1], cands, cands[ref.WINNER:ref.WINNER + 1]])
    assert ch.estimate_pose_best_start(0, 0, 1, twice, tau)[2] == 0
    ch.close(); co.close()
