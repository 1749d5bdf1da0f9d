"""BPVO_LOSS_STUDENT_T on the device (include/bpvo_hip/c_api.h states the definition; tests/student_t_ref.py evaluates it in numpy): the scale
stage (gn_tscale.h) at the operator seam against the f64 definition, its freeze decisions against a numpy mirror, weights bit for bit, the normal
equations at the bar of test_gpu_parity.py, then every driver — trace replay, batches, both launch shapes, sequences, rigs, the pose covariance —
and what the loss is for: an occluded pair where L2 fails.  Every estimate with the loss stays on the four-kernel chain."""
import numpy as np
import pytest

import hostile_poses as hp
import pose_covariance_ref as cov_ref
import student_t_ref as ref
from bpvo_amd import capi, synth
from test_gpu_multi_sequence import KF as SEQ_KF
from test_gpu_rigs import KF_LOW, assert_rigs_equal_their_own_contexts, rig_spec, scenes      # noqa: F401  (scenes: a fixture)
from test_gpu_seq_params import check, params_of, run_sweep, singles_of, sweep_frames
from util import bits_equal, make_params, normal_equations_f64, perturbed_pose, pose_error, set_options, setup_pair

pytestmark = pytest.mark.gpu

TL = capi.LOSS_STUDENT_T
SIZES = [(96, 128), (120, 160)]
LEVELS = 3
CONVERGED = (capi.STATUS_PARAMETER_TOL, capi.STATUS_FUNCTION_TOL, capi.STATUS_GRADIENT_TOL)


def t_pair(hip, rows, cols, descriptor, scene="plane", levels=LEVELS, **kw):
    """setup_pair with the Student-t loss (util.make_params knows the reference's three by name; any field goes through as a keyword)"""
    return setup_pair(hip, rows, cols, scene=scene, descriptor=descriptor, levels=levels, lossFunction=TL, **kw)


def valid_residuals(ctx):
    r = ctx.get_residuals(0).reshape(ctx.Cn, -1)
    return r[:, ctx.get_valid(0) != 0]


def f32_bits(a, b):
    return np.float32(a).tobytes() == np.float32(b).tobytes()


class Mirror:
    """The state machine around the stage, in numpy: a level holds (sigma, delta); a frozen scale (delta <= 1e-6) is not estimated again.  The fit
    starts from the DEVICE's previous sigma (f32), so that the two sides decide about the same start."""

    def __init__(self):
        self.sigma, self.delta, self.have = np.float32(1.0), 1e10, False

    def step(self, R):
        if not self.delta > 1e-6:
            return None
        f = ref.fit(R, sigma_prev=self.sigma if self.have else None)
        self.delta, self.have = f["delta"], True
        return f


# ---- 1. the operator seam ---------------------------------------------------------------------------------------------------------------------
WALK = [8.0, 2.0, 1.0, 1.0, 1.0, 4.0]      # perturbed_pose scales: the third visit of 1.0 at the latest starts at its own fixed point


@pytest.mark.parametrize("rows,cols", SIZES)
@pytest.mark.parametrize("scene", ["plane", "layered"])
@pytest.mark.parametrize("descriptor", ["bitplanes", "intensity", "gradient"])      # C = 8 tiled, C = 1, generic C (IntensityAndGradient)
def test_operator_seam(hip, descriptor, scene, rows, cols):
    ctx, d, p = t_pair(hip, rows, cols, descriptor, scene)
    C, thr = ctx.Cn, p.goodPointThreshold
    froze = 0
    for level in range(LEVELS):
        J = ctx.get_jacobians(0, level)
        mirror, prev = Mirror(), None
        for k, scale in enumerate(WALK):
            at = (descriptor, scene, rows, cols, "level", level, "linearisation", k)
            a = ctx.linearize(0, 0, 1, level, perturbed_pose(scale), reset_scale=(k == 0))
            sigma = np.float32(a["sigma"])
            r, v = ctx.get_residuals(0), ctx.get_valid(0)
            R = r.reshape(C, -1)[:, v != 0]
            assert a["num_valid"] == int(np.count_nonzero(v)) and R.size > 0, at
            f = mirror.step(R)
            if f is None:      # frozen earlier in the level: the stage did not run
                assert f32_bits(sigma, prev), (at, sigma, prev)
            else:
                assert f["exists"] and f["passes"] < ref.MAX_PASSES, (at, f)
                print(at, "sigma", sigma, "numpy", f["sigma"], "passes", f["passes"], "frozen", f["frozen"])
                if f["frozen"]:
                    assert f32_bits(sigma, prev), (at, "the mirror froze; the device moved", sigma, prev)
                    froze += 1
                else:
                    assert abs(float(sigma) - float(f["sigma"])) <= 2e-4 * float(f["sigma"]), (at, sigma, f)
                    assert prev is None or not f32_bits(sigma, prev) or k == 0, (at, "the mirror moved; the device froze")
                # the returned sigma is the fixed point, whatever the start: the stop rule plus 10 % for f32 terms summed in f64
                s = float(sigma)
                assert abs(np.sqrt(ref.T(s * s, R)) - s) <= 1.1e-4 * s, (at, s, np.sqrt(ref.T(s * s, R)))
                mirror.sigma = sigma
            prev = sigma
            w = ctx.get_weights(0)
            assert bits_equal(w, ref.weights_f32(r, sigma)), at
            H64, G64, f64 = normal_equations_f64(J, r, w, v, C)
            hs = np.abs(H64).max()
            assert np.abs(a["H"] - H64).max() <= 4e-6 * hs, at      # the bar of test_gpu_parity.test_linearize_parity
            assert np.abs(a["G"] - G64).max() <= 4e-6 * max(np.abs(G64).max(), 1e-3 * hs), at
            assert abs(a["f_norm"] - f64) <= 4e-6 * max(f64, 1e-6), at
            good = np.float32(np.count_nonzero(w > np.float32(thr))) / np.float32(w.size)
            assert f32_bits(ctx.fraction_good(0, thr), good), at
    assert froze >= LEVELS, "every level's walk should freeze once"
    # no valid point: sigma = 1, H = 0
    far = np.eye(4, dtype=np.float32)
    far[0, 3] = 1e6
    a = ctx.linearize(0, 0, 1, 0, far, reset_scale=True)
    assert a["num_valid"] == 0 and a["sigma"] == 1.0 and not a["H"].any() and not a["G"].any() and a["f_norm"] == 0.0, a
    ctx.close()


def test_the_start_does_not_move_the_fixed_point(hip):
    """A level that holds another pose's scale (warm) and a reset one (cold) end at the same fixed point of the same residuals."""
    ctx, d, p = t_pair(hip, 120, 160, "intensity", "layered")
    T = perturbed_pose(1.0)
    cold = ctx.linearize(0, 0, 1, 0, T, reset_scale=True)["sigma"]
    ctx.linearize(0, 0, 1, 0, perturbed_pose(8.0), reset_scale=True)
    warm = ctx.linearize(0, 0, 1, 0, T, reset_scale=False)["sigma"]
    R = valid_residuals(ctx)
    for s in (cold, warm):
        assert abs(np.sqrt(ref.T(s * s, R)) - s) <= 1.1e-4 * s, (cold, warm)
    assert abs(cold - warm) <= 2e-4 * cold and cold != 1.0
    ctx.close()


def test_an_unknown_loss_is_still_refused(hip):
    K, b = synth.calibration(120, 160)
    p = make_params(hip, levels=3)
    p.lossFunction = 0x14
    with pytest.raises(capi.BpvoError, match=r"\(-2\).*unknown lossFunction"):
        hip.create(K, b, 120, 160, p)
    p.lossFunction = TL
    hip.create(K, b, 120, 160, p).close()


# ---- 2. the estimate's trace, replayed through the seam ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,cols", SIZES)
@pytest.mark.parametrize("descriptor,scene", [("bitplanes", "plane"), ("intensity", "layered"), ("gradient", "plane")])
def test_trace_replays_through_the_seam(hip, descriptor, scene, rows, cols):
    ctx, d, p = t_pair(hip, rows, cols, descriptor, scene)
    before = ctx.tscale_counts()
    T, stats, rec = ctx.estimate_pose_trace(0, 0, 1)
    stages, passes = (a - b for a, b in zip(ctx.tscale_counts(), before))
    assert len(rec) > LEVELS
    assert 0 < stages <= len(rec) and passes >= stages, (stages, passes, len(rec))
    assert ctx.median_path_counts() == (0, 0)
    level = None
    for i, q in enumerate(rec):
        first = int(q[67]) != level
        level = int(q[67])
        a = ctx.linearize(0, 0, 1, level, q[:16].reshape(4, 4), reset_scale=first)
        at = (descriptor, scene, rows, cols, "linearisation", i, "level", level)
        assert f32_bits(a["sigma"], q[59]) and a["num_valid"] == int(q[60]) and f32_bits(a["f_norm"], q[58]), (at, a["sigma"], q[59], a["f_norm"], q[58])
    rot, trans = pose_error(T, d["T_gt"])
    print(descriptor, scene, rows, cols, "iterations", [s["numIterations"] for s in stats], "stage runs", stages, "passes", passes, "error", rot, trans)
    ctx.close()


# ---- 3. paths -------------------------------------------------------------------------------------------------------------------------------------
def batch_of_copies(hip, d, p, n, T0=None, lanes=None):
    rows, cols = d["imgA"].shape
    ctx = hip.create(d["K"], d["b"], rows, cols, p, n_frames=2 * n, n_pairs=n)
    if lanes:
        ctx.set_max_lanes(lanes)
    ctx.frames_set_data(0, 1, np.stack([d["imgA"], d["imgB"]] * n), np.stack([d["dispA"], d["dispB"]] * n))
    ctx.frames_set_template(0, 2, n)
    poses, stats = ctx.batch_estimate(n, T0)
    out = dict(poses=poses, stats=stats, pk=ctx.persistent_counts(), team=ctx.team_counts(), med=ctx.median_path_counts(), ts=ctx.tscale_counts())
    ctx.close()
    return out


@pytest.mark.parametrize("descriptor", ["bitplanes", "intensity"])
def test_the_loss_stays_on_the_chain(hip, descriptor, monkeypatch):
    monkeypatch.delenv("BPVO_HIP_OPTIONS", raising=False)
    set_options(monkeypatch, team="1")
    d = synth.make_pair(120, 160, 0)
    for n in (1, 8):
        t = batch_of_copies(hip, d, make_params(hip, descriptor=descriptor, levels=LEVELS, lossFunction=TL), n)
        k = batch_of_copies(hip, d, make_params(hip, descriptor=descriptor, loss="tukey", levels=LEVELS), n)
        assert t["pk"] == (0, 0) and t["team"] == 0 and t["med"] == (0, 0) and t["ts"][0] > 0, (n, t)
        assert (k["pk"][0] > 0 if n == 1 else k["team"] > 0) and k["ts"] == (0, 0), (n, k["pk"], k["team"])      # the same kind of context leaves the chain
        assert all(s in CONVERGED or s == capi.STATUS_MAX_ITERATIONS for s in t["stats"]["status"].reshape(-1))


@pytest.mark.parametrize("descriptor", ["bitplanes", "intensity", "gradient"])
def test_reference_reduction_keeps_sigma_and_weights(hip, descriptor):
    ctx, d, p = t_pair(hip, 120, 160, descriptor)
    out = {}
    for mode in (0, 1):
        ctx.set_option("reference_reduction", mode)
        rows = []
        for k, scale in enumerate((8.0, 1.0, 1.0, 2.0)):
            a = ctx.linearize(0, 0, 1, 0, perturbed_pose(scale), reset_scale=(k == 0))
            rows.append((np.float32(a["sigma"]), ctx.get_weights(0), a))
        out[mode] = rows
        T, stats = ctx.estimate_pose(0, 0, 1)      # ... and an estimate in the mode runs
        assert np.isfinite(T).all()
    for (s0, w0, a0), (s1, w1, a1) in zip(out[0], out[1]):
        assert f32_bits(s0, s1) and bits_equal(w0, w1) and a0["num_valid"] == a1["num_valid"]
        assert np.abs(a0["H"] - a1["H"]).max() <= 2e-4 * np.abs(a0["H"]).max()      # (the reference order's serial f32 sums: test_linearize_parity's bar for them)
    ctx.close()


# ---- 4. batches -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("descriptor", ["bitplanes", "intensity"])
def test_batch_copies_equal_the_single_estimate(hip, descriptor):
    d = synth.make_pair(96, 128, 3)
    p = make_params(hip, descriptor=descriptor, levels=LEVELS, lossFunction=TL)
    one = batch_of_copies(hip, d, p, 1)
    five = batch_of_copies(hip, d, p, 5)
    for k in range(5):
        assert bits_equal(five["poses"][k], one["poses"][0]) and five["stats"][k].tobytes() == one["stats"][0].tobytes(), k
    assert five["ts"] == (5 * one["ts"][0], 5 * one["ts"][1])


@pytest.mark.parametrize("descriptor", ["bitplanes", "intensity"])
def test_a_pair_that_finishes_early_changes_nothing(hip, descriptor):
    """pair 0 starts at the truth and leaves the active set first; the others, from the Identity, end where a single estimate ends"""
    d = synth.make_pair(120, 160, 1)
    p = make_params(hip, descriptor=descriptor, levels=LEVELS, lossFunction=TL)
    n = 4
    T0 = np.stack([d["T_gt"].astype(np.float32)] + [np.eye(4, dtype=np.float32)] * (n - 1))
    got = batch_of_copies(hip, d, p, n, T0, lanes=1)
    at_truth = batch_of_copies(hip, d, p, 1, T0[:1])
    at_identity = batch_of_copies(hip, d, p, 1)
    its = got["stats"]["numIterations"]
    print(descriptor, "iterations per pair and level", its.tolist())
    # the premise: at some level pair 0 and the others leave the active set at different iterations (whoever is first, the launches of the
    # rest of that level run over a compacted list)
    assert any(its[0][l] != its[1][l] for l in range(its.shape[1])), "the pairs finish every level together: the active set is not exercised"
    assert bits_equal(got["poses"][0], at_truth["poses"][0]) and got["stats"][0].tobytes() == at_truth["stats"][0].tobytes()
    for k in range(1, n):
        assert bits_equal(got["poses"][k], at_identity["poses"][0]) and got["stats"][k].tobytes() == at_identity["stats"][0].tobytes(), k


@pytest.mark.parametrize("descriptor", ["bitplanes", "intensity"])
def test_both_launch_shapes_give_the_same_bits(hip, descriptor):
    """264 tiny pairs in one launch (more than 256 workgroups: the 512-thread shape of tscale_kernel) against the same pairs in launches of 66
    (the 1024-thread shape)."""
    rows, cols, levels, n, sub, distinct = 48, 64, 2, 264, 66, 6
    batch = synth.make_batch(rows, cols, distinct, first_index=40, workers=1)
    pick = np.arange(n) % distinct
    imgs = np.stack([batch["images"][2 * k + e] for k in pick for e in (0, 1)])
    disps = np.stack([batch["disparities"][2 * k + e] for k in pick for e in (0, 1)])
    p = make_params(hip, descriptor=descriptor, levels=levels, lossFunction=TL, maxIterations=12)
    outs = []
    for width in (n, sub):
        ctx = hip.create(batch["K"], batch["b"], rows, cols, p, n_frames=2 * width, n_pairs=width)
        ctx.set_max_lanes(1)
        poses, stats = [], []
        for k in range(0, n, width):
            ctx.frames_set_data(0, 1, imgs[2 * k: 2 * (k + width)], disps[2 * k: 2 * (k + width)])
            ctx.frames_set_template(0, 2, width)
            ps, ss = ctx.batch_estimate(width)
            poses.append(ps); stats.append(ss)
        outs.append((np.concatenate(poses), np.concatenate(stats), ctx.tscale_counts(), ctx.total_linearizations()))
        assert ctx.team_counts() == 0 and ctx.persistent_counts() == (0, 0)
        ctx.close()
    (pw, sw, tw, lw), (pn, sn, tn, ln) = outs
    print(descriptor, "stage runs / passes", tw, "linearisations", lw)
    assert bits_equal(pw, pn) and sw.tobytes() == sn.tobytes() and tw == tn and lw == ln and tw[0] > 0
    assert len({pw[k].tobytes() for k in range(distinct)}) == distinct      # (the pairs differ: equal bits are not one pair's)


# ---- 5. sequences, 6. rigs ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("desc", ["bitplanes", "intensity"])
def test_four_losses_in_one_add_frames_context(hip, desc):
    rows, cols = 120, 160
    frames, K, b = sweep_frames(rows, cols, n_frames=4)
    base = make_params(hip, descriptor=desc, loss="tukey", levels=LEVELS, **SEQ_KF)
    params = [params_of(hip, base, dict(lossFunction=l), frames) for l in ("huber", "tukey", "l2")] + [params_of(hip, base, None, frames)]
    params[3].lossFunction = TL
    singles = singles_of(hip, K, b, rows, cols, params, frames)
    m = run_sweep(hip, K, b, rows, cols, base, params, frames)
    check(m, singles)
    poses = [np.asarray(o[0][-1]["res"]["pose"]) for o in singles]
    assert not bits_equal(poses[3], poses[1]) and not bits_equal(poses[3], poses[2]), "the Student-t sequence should not be another loss's"
    m.ctx.close()


def test_a_student_t_rig_beside_a_tukey_rig(hip, scenes):
    base = dict(KF_LOW, descriptor="intensity", loss="tukey")
    specs = [rig_spec(scenes, (0, 1), **dict(base, lossFunction=TL)), rig_spec(scenes, (0, 1), **base)]
    recs = assert_rigs_equal_their_own_contexts(hip, specs, [[0, 1], [2, 3]], base=base)
    assert not bits_equal(recs[0][-1]["res"]["pose"], recs[1][-1]["res"]["pose"]), "the two rigs should not run the same loss"


# ---- 7. covariance ------------------------------------------------------------------------------------------------------------------------------------
def covariance_f64(ctx, level, T, sigma):
    """c_api.h's definition with d(u) = 6 (5 - u^2) / (5 + u^2)^2, the sums in f64 (w and d per residual in the device's f32 operations, as
    pose_covariance_ref takes the other losses')"""
    ctx.linearize_at_scale(0, 0, 1, level, T, sigma)
    r, valid, J = ctx.get_residuals(0), ctx.get_valid(0), np.asarray(ctx.get_jacobians(0, level), np.float64)
    C, N = J.shape[0], J.shape[1]
    r32 = np.asarray(r, np.float32).reshape(C, N)
    x = r32 * (np.float32(1.0) / np.float32(sigma))
    x2 = x * x
    den = np.float32(5.0) + x2
    d = (np.float32(6.0) * (np.float32(5.0) - x2)) / (den * den)
    w = ref.weights_f32(r32, sigma)
    assert np.allclose(d, ref.curvature(x.astype(np.float64)), rtol=1e-5, atol=1e-6)
    v = (valid.reshape(N) != 0).astype(np.float64)
    M = np.einsum("cn,cni,cnj->ij", d.astype(np.float64) * v, J, J)
    g = np.einsum("cn,cni->ni", w.astype(np.float64) * v * r32.astype(np.float64), J)
    Q = g.T @ g
    A = cov_ref.normalization_map(ctx.get_normalization(0, level))
    st = cov_ref.status_of(M, Q, int(v.sum()))
    return dict(M=M, Q=Q, A=A, status=st, num_valid=int(v.sum()), negative=int(np.count_nonzero((d < 0) & (v[None, :] > 0))))


@pytest.mark.parametrize("descriptor", ["bitplanes", "intensity", "gradient"])
def test_pose_covariance_against_f64(hip, descriptor):
    ctx, d, p = t_pair(hip, 96, 128, descriptor, levels=2)
    ok = 0
    for level in (1, 0):
        for scale in (0.25, 1.0):
            T = perturbed_pose(scale)
            sigma = ctx.linearize(0, 0, 1, level, T, reset_scale=True)["sigma"]
            e = covariance_f64(ctx, level, T, sigma)
            rec = ctx.pose_covariances([0], [0], [1], level, T=[T], sigma=[sigma])[0]
            M, Q = ctx.debug_pose_covariance_sums(0)
            what = (descriptor, level, scale)
            eM = np.abs(M.astype(np.float64) - e["M"]).max() / np.abs(e["M"]).max()
            eQ = np.abs(Q.astype(np.float64) - e["Q"]).max() / np.abs(e["Q"]).max()
            print(what, "relative error of M %.2e, Q %.2e; residuals with d < 0: %d; status %d" % (eM, eQ, e["negative"], rec["status"]))
            assert eM <= 4e-6 and eQ <= 4e-6, (what, eM, eQ)      # test_gpu_pose_covariance's bar for Tukey
            assert e["negative"] > 0, "no residual beyond sqrt(5) sigma: the negative branch of d is not exercised"
            assert rec["status"] == e["status"] and rec["num_valid"] == e["num_valid"], (what, rec["status"], e["status"])
            if rec["status"] == capi.COV_OK:
                ok += 1
                S = e["A"] @ cov_ref.sandwich(M.astype(np.float64), Q.astype(np.float64)) @ e["A"].T
                sd = np.sqrt(np.diag(S))
                assert (np.abs(rec["covariance"].astype(np.float64) - S) / np.outer(sd, sd)).max() <= 1e-6, what
    assert ok > 0
    ctx.close()


# ---- 8. robustness ------------------------------------------------------------------------------------------------------------------------------------
OCCLUDER = (30, 90, 40, 120)      # rows 30 .. 89, columns 40 .. 119 of the 120 x 160 frame: a quarter of its pixels


def occluded_pair():
    d = synth.make_pair(120, 160, 0)
    foreign = synth.make_pair(120, 160, 11)["imgB"]
    y0, y1, x0, x1 = OCCLUDER
    imgB = d["imgB"].copy()
    imgB[y0:y1, x0:x1] = foreign[y0:y1, x0:x1]
    return dict(d, imgB=imgB)


def final_error(binding, d, **pk):
    p = make_params(binding, descriptor="intensity", levels=LEVELS, **pk)
    ctx = binding.create(d["K"], d["b"], 120, 160, p, n_frames=2, n_pairs=1)
    ctx.frame_set_data(0, d["imgA"], d["dispA"])
    ctx.frame_set_template(0)
    ctx.frame_set_data(1, d["imgB"], d["dispB"])
    T, stats = ctx.estimate_pose(0, 0, 1)
    ctx.close()
    return pose_error(T, d["T_gt"])[1], stats


def test_an_occluder_that_breaks_l2(hip, orc):
    """No margin is invented: Student-t must converge and end nearer the truth than L2.  Measured on an MI355X (translation error to T_gt):
    Huber 1.75 mm, Tukey 1.73 mm, L2 42.7 mm, Student-t 3.82 mm; the oracle's L2 / Tukey: 42.7 / 1.73 mm."""
    d = occluded_pair()
    # the condition that makes the scene discriminate, on the oracle: L2 ends at least 5 times farther from the truth than Tukey
    o_l2, o_tukey = final_error(orc, d, loss="l2")[0], final_error(orc, d, loss="tukey")[0]
    print("oracle: L2 %.5f m, Tukey %.5f m" % (o_l2, o_tukey))
    assert o_l2 >= 5.0 * o_tukey, (o_l2, o_tukey)
    err = {name: final_error(hip, d, **pk) for name, pk in (("huber", dict(loss="huber")), ("tukey", dict(loss="tukey")), ("l2", dict(loss="l2")),
                                                            ("student_t", dict(lossFunction=TL)))}
    print("device, translation error to T_gt (m):", {k: round(v[0], 5) for k, v in err.items()})
    assert err["student_t"][1][0]["status"] in CONVERGED, err["student_t"][1]
    assert err["student_t"][0] < err["l2"][0], err


# ---- 9. hostile starts ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("descriptor", ["bitplanes", "intensity", "fields2"])
def test_hostile_starts_do_not_raise(hip, descriptor):
    rows, cols, levels = hp.SIZES["96x128"]
    ctx, d, p = t_pair(hip, rows, cols, descriptor, levels=levels)
    X = ctx.get_points(0, 0)
    for name, T in hp.poses(d["K"], X, rows, cols).items():
        Te, stats = ctx.estimate_pose(0, 0, 1, T)
        a = ctx.linearize(0, 0, 1, 0, T, reset_scale=True)
        print(descriptor, name, "status", [s["status"] for s in stats], "sigma at the start", a["sigma"], "valid", a["num_valid"])
        assert a["sigma"] > 0 and np.isfinite(a["sigma"]), (name, a["sigma"])
        if name in hp.NON_FINITE:
            assert a["num_valid"] == 0 and a["sigma"] == 1.0, (name, a)
    ctx.close()
