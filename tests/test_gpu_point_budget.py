"""Point budget (bpvo_hip_set_point_budget, an extension): at most K template points per level, the most salient first, ties at the threshold in
raster order.  Two references, no tolerance anywhere:
  * tie cut — the kept indices are the numpy rule's (tests/point_budget_ref.py, pinned to the oracle's selection by tests/test_point_budget_cpu.py)
    on the oracle's saliency map, the points the unbudgeted oracle template's rows at those indices;
  * clean cut — when #{S >= t} == K the budgeted template is the oracle's with minSaliency = max(minSaliency, t), bit for bit, down to the
    Gauss-Newton trajectory in reference_reduction mode.
Then every selection path, sequences with budgets of their own, "off means off" and the refusals."""
import ctypes as C

import numpy as np
import pytest

import point_budget_ref as pb
from bpvo_amd import capi, synth
from util import bits_equal, make_params

pytestmark = pytest.mark.gpu

ERR_INVALID_ARG = -1      # c_api.h BPVO_ERR_INVALID_ARG
SIZES = [(96, 128), (100, 150), (120, 160)]      # 100x150: a word tail, rows no multiple of the tile height
KF = dict(minTranslationMagToKeyFrame=0.1, minRotationMagToKeyFrame=2.5, maxFractionOfGoodPointsToKeyFrame=0.7, goodPointThreshold=0.8)


def _nms_level0(rows, cols):
    """non-maximum suppression at level 0 only: level 1 is dense"""
    return dict(minNumPixelsForNonMaximaSuppression=rows * cols)


def _template_ctx(b, d, rows, cols, p, n_frames=2):
    ctx = b.create(d["K"], d["b"], rows, cols, p, device=0, n_frames=n_frames, n_pairs=1)
    ctx.frame_set_data(0, d["imgA"], d["dispA"])
    ctx.frame_set_template(0)
    return ctx


def _level_radius(ctx, p, level):
    r, c = ctx.level_size(level)
    return p.nonMaxSuppRadius if (r * c >= p.minNumPixelsForNonMaximaSuppression and p.nonMaxSuppRadius > 0) else -1


def _oracle_levels(orc, d, rows, cols, p):
    """per level of the unbudgeted oracle template: saliency map, candidates and their saliencies, template indices and points"""
    co = _template_ctx(orc, d, rows, cols, p)
    out = []
    for l in range(p.maxTestLevel, co.L):
        S = co.get_saliency(0, l)
        radius = _level_radius(co, p, l)
        cand = pb.candidates(S, d["dispA"], l, radius, p.minSaliency, p.minValidDisparity, p.maxValidDisparity, nms_param_radius=p.nonMaxSuppRadius)
        inds = co.get_point_indices(0, l)
        assert np.array_equal(cand[:len(cand) & ~15], inds), l      # (the numpy candidate rule is the oracle's)
        out.append(dict(level=l, S=S, radius=radius, cand=cand, s=S.reshape(-1)[cand], inds=inds, pts=co.get_points(0, l)))
    co.close()
    return out


def _budget_cases(s):
    """the budgets a (frame, level) with candidate saliencies s is tried with"""
    n = len(s)
    vals, counts = np.unique(s, return_counts=True)
    cases = {"16": 16, "count": n, "count-1": n - 1, "above": n + 5}
    # a cut inside a tie group: the most salient group of at least two whose middle lies at 16 points or more
    for v, c in sorted(zip(vals, counts), key=lambda vc: -vc[0]):
        k = int((s > v).sum()) + int(c) // 2
        if c >= 2 and 16 <= k < n:
            cases["inside-ties"] = k
            break
    cases["half-odd"] = (n // 2) | 1      # no multiple of 16
    return {k: v for k, v in cases.items() if v >= 16}


def _assert_level_follows_rule(ch, ref, d, p, K, what):
    l = ref["level"]
    want = pb.kept_indices(ref["S"], d["dispA"], l, ref["radius"], p.minSaliency, p.minValidDisparity, p.maxValidDisparity, K,
                           nms_param_radius=p.nonMaxSuppRadius)
    assert np.array_equal(want["cand"], ref["cand"])
    inds = ch.get_point_indices(0, l)
    assert np.array_equal(inds, want["kept"]), (what, l, K, len(inds), len(want["kept"]))
    assert ch.num_points(0, l) == len(inds) == (min(K, len(ref["cand"])) & ~15 if K else len(ref["cand"]) & ~15)
    # the points: the rows of the unbudgeted oracle template at those indices (its last count mod 16 candidates are in no template)
    row = np.searchsorted(ref["inds"], inds)
    have = (row < len(ref["inds"])) & (ref["inds"][np.minimum(row, len(ref["inds"]) - 1)] == inds)
    assert have.sum() >= len(inds) - 15
    assert bits_equal(ch.get_points(0, l)[have], ref["pts"][row[have]]), (what, l, K)
    info = ch.selection_info(0, l)
    assert info["n_candidates"] == len(ref["cand"]), (what, l, K, info)
    t = want["t"] if want["bound"] else np.float32(p.minSaliency)
    assert bits_equal(np.float32(info["threshold"]), np.float32(t)) and info["n_ties_kept"] == want["quota"], (what, l, K, info, want["t"], want["quota"])
    return want


# ---- tie cut ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,cols", SIZES)
@pytest.mark.parametrize("descriptor,kw", [("bitplanes", dict(sigmaBitPlanes=-1.0)), ("intensity", {})], ids=["binary-bitplanes", "intensity"])
def test_tie_cut_follows_the_numpy_rule(hip, orc, rows, cols, descriptor, kw):
    """sigmaBitPlanes <= 0: binary channels, saliencies from a handful of values, massive ties"""
    d = synth.make_pair(rows, cols, 2)
    p = make_params(hip, descriptor=descriptor, levels=2, **_nms_level0(rows, cols), **kw)
    refs = _oracle_levels(orc, d, rows, cols, p)
    cases = [_budget_cases(r["s"]) for r in refs]
    assert all("inside-ties" in c for c in cases) or descriptor == "intensity", cases
    ch = _template_ctx(hip, d, rows, cols, p)
    # (the binary planes' strict maxima all have one saliency at these two sizes: there EVERY candidate ties, and the first K in raster order stay)
    all_tie = [len(np.unique(r["s"])) == 1 for r in refs]
    assert any(all_tie) == (descriptor == "bitplanes" and (rows, cols) != (100, 150)), [np.unique(r["s"]) for r in refs]
    bound_with_ties = 0
    for name in sorted(set().union(*cases)):
        budget = [c.get(name, 0) for c in cases]
        ch.set_point_budget(budget)
        assert ch.get_point_budget() == budget
        ch.frame_set_template(0)
        for r, K in zip(refs, budget):
            want = _assert_level_follows_rule(ch, r, d, p, K, (descriptor, name))
            bound_with_ties += bool(want["bound"] and want["quota"] < int((r["s"] == want["t"]).sum()))
            if all_tie[r["level"]] and want["bound"]:
                assert want["quota"] == K and np.array_equal(want["kept"], r["cand"][:K & ~15])
    assert bound_with_ties >= 1      # (a cut through a tie group was among them)
    ch.close()


# ---- clean cut -------------------------------------------------------------------------------------------------------------------------------
def _clean_cut(s):
    """t among the distinct candidate saliencies with about half the candidates at or above it; K = #{S >= t}"""
    vals = np.unique(s)
    at_or_above = np.array([(s >= v).sum() for v in vals])
    t = vals[np.argmin(np.abs(at_or_above - len(s) / 2.0))]
    return np.float32(t), int((s >= t).sum())


def _everything(ctx, level, T, st, rec):
    Tn, Tni = ctx.get_normalization(0, level)
    return dict(inds=ctx.get_point_indices(0, level), pts=ctx.get_points(0, level), pix=ctx.get_pixels(0, level), jac=ctx.get_jacobians(0, level),
                Tn=Tn, Tni=Tni, T=T, trace=rec, its=np.array([s["numIterations"] for s in st]), status=np.array([s["status"] for s in st]))


@pytest.mark.parametrize("rows,cols", [(96, 128), (120, 160)])
@pytest.mark.parametrize("level", [0, 1])
@pytest.mark.parametrize("descriptor,loss", [("intensity", "huber"), ("bitplanes", "tukey")])
def test_clean_cut_is_the_oracle_with_a_raised_min_saliency(hip, orc, rows, cols, level, descriptor, loss):
    d = synth.make_pair(rows, cols, 1)
    kw = dict(descriptor=descriptor, loss=loss, levels=level + 1, maxTestLevel=level, **_nms_level0(rows, cols))
    p = make_params(hip, **kw)
    ref = _oracle_levels(orc, d, rows, cols, p)[0]
    assert ref["level"] == level
    t, K = _clean_cut(ref["s"])
    assert 16 <= K < len(ref["s"]) and t > p.minSaliency, (t, K, len(ref["s"]))
    # the oracle with minSaliency' = t and no budget
    po = make_params(orc, **dict(kw, minSaliency=float(t)))
    co = _template_ctx(orc, d, rows, cols, po)
    co.frame_set_data(1, d["imgB"], d["dispB"])
    want = _everything(co, level, *co.estimate_pose_trace(0, 0, 1))
    co.close()
    assert len(want["inds"]) == K & ~15
    ch = hip.create(d["K"], d["b"], rows, cols, p, device=0, n_frames=2, n_pairs=1)
    ch.set_option("reference_reduction", 1)
    ch.set_point_budget([0] * level + [K])
    ch.frame_set_data(0, d["imgA"], d["dispA"])
    ch.frame_set_template(0)
    ch.frame_set_data(1, d["imgB"], d["dispB"])
    got = _everything(ch, level, *ch.estimate_pose_trace(0, 0, 1))
    info = ch.selection_info(0, level)
    ch.close()
    assert np.array_equal(got["inds"], want["inds"])
    for k in ("pts", "pix", "jac", "Tn", "Tni", "trace", "T"):
        assert bits_equal(got[k], want[k]), k
    assert np.array_equal(got["its"], want["its"]) and np.array_equal(got["status"], want["status"])
    assert info["n_candidates"] == len(ref["s"]) and bits_equal(np.float32(info["threshold"]), t) and info["n_ties_kept"] == int((ref["s"] == t).sum())


# ---- every path ------------------------------------------------------------------------------------------------------------------------------
PATHS = [
    pytest.param("intensity", dict(nonMaxSuppRadius=2, minNumPixelsForNonMaximaSuppression=1), id="nms-radius-2-flag-path"),
    pytest.param("bitplanes", dict(minNumPixelsForNonMaximaSuppression=1 << 30), id="dense-levels-without-nms"),
    pytest.param("fields1", dict(minNumPixelsForNonMaximaSuppression=100 * 150), id="descriptor-fields-generic-channels"),
]


@pytest.mark.parametrize("descriptor,kw", PATHS)
@pytest.mark.parametrize("rows,cols", [(100, 150), (96, 128)])
def test_every_selection_path_follows_the_rule(hip, orc, rows, cols, descriptor, kw):
    d = synth.make_pair(rows, cols, 3)
    p = make_params(hip, descriptor=descriptor, levels=2, **kw)
    refs = _oracle_levels(orc, d, rows, cols, p)
    ch = _template_ctx(hip, d, rows, cols, p)
    for name in ("half-odd", "inside-ties", "16", "above"):
        budget = [_budget_cases(r["s"]).get(name, 0) for r in refs]
        ch.set_point_budget(budget)
        ch.frame_set_template(0)
        for r, K in zip(refs, budget):
            _assert_level_follows_rule(ch, r, d, p, K, (descriptor, name))
    ch.close()


LEVELS = 3


def _batch_params(hip, rows, cols):
    # NMS (radius 1) at levels 0 and 1 — the lazy levels of a pair batch's template frames —, none at level 2
    return make_params(hip, levels=LEVELS, minNumPixelsForNonMaximaSuppression=(rows // 2) * (cols // 2))


def _pair_record(ctx, slot, T, its):
    rec = dict(T=T, its=np.asarray(its, np.int32))
    for l in range(LEVELS):
        rec["inds", l] = ctx.get_point_indices(slot, l)
        rec["pts", l] = ctx.get_points(slot, l)
        rec["pix", l] = ctx.get_pixels(slot, l)
    return rec


def _assert_records_equal(a, z, what):
    assert a.keys() == z.keys()
    for k in a:
        assert bits_equal(a[k], z[k]), (what, k)


def test_pair_batch_with_lazy_template_levels_equals_the_frame_api(hip):
    """4 pairs through batch_run — template frames on the lazy levels, with and without their saliency map, team kernel and chain — against the same
    pairs through frame_set_data / frame_set_template / estimate_pose (persistent kernel and chain), all with the same budget"""
    rows, cols, n = 100, 150, 4
    b = synth.make_batch(rows, cols, n, first_index=20)
    p = _batch_params(hip, rows, cols)
    # budgets that bind: half the unbudgeted count of pair 0's template per level
    probe = hip.create(b["K"], b["b"], rows, cols, p, n_frames=2, n_pairs=1)
    probe.frame_set_data(0, b["images"][0], b["disparities"][0])
    probe.frame_set_template(0)
    budget = [max(16, (probe.selection_info(0, l)["n_candidates"] // 2) | 1) for l in range(LEVELS)]
    singles = {}
    for persistent in (1, 0):
        probe.set_option("persistent", persistent)
        probe.set_point_budget(budget)
        for k in range(n):
            probe.frame_set_data(0, b["images"][2 * k], b["disparities"][2 * k])
            probe.frame_set_template(0)
            probe.frame_set_data(1, b["images"][2 * k + 1], b["disparities"][2 * k + 1])
            T, st = probe.estimate_pose(0, 0, 1)
            rec = _pair_record(probe, 0, T, [s["numIterations"] for s in st])
            assert all(probe.selection_info(0, l)["n_candidates"] > budget[l] for l in range(LEVELS)), k      # (the budget binds)
            assert [probe.num_points(0, l) for l in range(LEVELS)] == [K & ~15 for K in budget]
            if persistent:
                singles[k] = rec
            else:
                _assert_records_equal(rec, singles[k], ("chain against persistent", k))
    probe.close()
    for lazy_saliency in (0, 1):
        for team in (1, 0):
            ctx = hip.create(b["K"], b["b"], rows, cols, p, n_frames=2 * n, n_pairs=n)
            ctx.set_option("lazy_template_saliency", lazy_saliency)
            ctx.set_option("team", team)
            ctx.set_point_budget(budget)
            poses, stats = ctx.batch_run(b["images"], b["disparities"])
            for k in range(n):
                rec = _pair_record(ctx, 2 * k, poses[k], stats["numIterations"][k][:LEVELS])
                _assert_records_equal(rec, singles[k], (lazy_saliency, team, k))
            ctx.close()


# ---- sequences -------------------------------------------------------------------------------------------------------------------------------
SEQ_CAMS = [(96, 128), (100, 150), (96, 128)]
SEQ_BUDGETS = [[304, 1008], [], [208, 512]]      # sequence 1: none of its own


def _seq_cameras(baseline=None):
    cams = []
    for r, c in SEQ_CAMS:
        K, b = synth.calibration(r, c)
        cams.append((np.asarray(K, np.float32).reshape(3, 3), b if baseline is None else baseline, r, c))
    return cams


def _result_key(res, npts):
    return dict(pose=res["pose"], its=np.array([s["numIterations"] for s in res["stats"]]), err=np.array([s["finalError"] for s in res["stats"]], np.float32),
                kf=np.array([res["isKeyFrame"], res["keyFramingReason"]]), npts=np.array(npts))


def _seq_params(hip):
    return make_params(hip, descriptor="bitplanes", levels=2, minNumPixelsForNonMaximaSuppression=96 * 128, **KF)


def test_sequences_with_budgets_of_their_own_equal_contexts_of_their_own(hip):
    p = _seq_params(hip)
    cams = _seq_cameras()
    seqs = [synth.make_sequence(r, c, 4, index=30 + s, step_rot=0.01, step_trans=0.08, camera=(K, b))["frames"] for s, (K, b, r, c) in enumerate(cams)]
    m = hip.create_sequences(cams, p)
    for s, bud in enumerate(SEQ_BUDGETS):
        if bud:
            m.seq_set_point_budget(s, bud)
        assert m.seq_get_point_budget(s) == ((bud if bud else [0, 0]), bool(bud))
    multi = {s: [] for s in range(3)}
    for k in range(4):
        res = m.add_frames([seqs[s][k][0] for s in range(3)], [seqs[s][k][1] for s in range(3)])
        for s in range(3):
            multi[s].append(_result_key(res[s], [m.seq_num_points_at_level(s, l) for l in range(2)]))
    m.seq_reset(0)
    assert m.seq_get_point_budget(0) == (SEQ_BUDGETS[0], True)      # the budget outlives a reset
    m.close()
    kfs, bound = 0, 0
    for s, (K, b, r, c) in enumerate(cams):
        one = hip.create(K, b, r, c, p, n_frames=3, n_pairs=1)
        if SEQ_BUDGETS[s]:
            one.set_point_budget(SEQ_BUDGETS[s])
        for k in range(4):
            res = one.add_frame(*seqs[s][k])
            _assert_records_equal(_result_key(res, [one.vo_num_points_at_level(l) for l in range(2)]), multi[s][k], (s, k))
            kfs += res["isKeyFrame"]
            if SEQ_BUDGETS[s]:
                assert all(one.vo_num_points_at_level(l) <= SEQ_BUDGETS[s][l] for l in range(2))
                bound += all(one.vo_num_points_at_level(l) == SEQ_BUDGETS[s][l] & ~15 for l in range(2))
        one.close()
    assert kfs >= 3 and bound >= 2      # a key frame was forced somewhere, and the budgets bound


def test_stereo_sequences_with_budgets_equal_contexts_of_their_own(hip):
    p = _seq_params(hip)
    cams = _seq_cameras(baseline=1.0)      # (disparities of a dozen pixels for the block matcher)
    seqs = [synth.make_stereo_sequence(r, c, 4, index=40 + s, step_rot=0.01, step_trans=0.08, camera=(K, b))["frames"] for s, (K, b, r, c) in enumerate(cams)]
    m = hip.create_sequences(cams, p)
    sp = m.default_stereo_params(32)
    for s, bud in enumerate(SEQ_BUDGETS):
        if bud:
            m.seq_set_point_budget(s, [bud[0] // 2 & ~15, bud[1] // 2 & ~15])
    multi = {s: [] for s in range(3)}
    for k in range(4):
        res = m.add_frames_stereo([seqs[s][k][0] for s in range(3)], [seqs[s][k][1] for s in range(3)], sp)
        for s in range(3):
            multi[s].append(_result_key(res[s], [m.seq_num_points_at_level(s, l) for l in range(2)]))
    m.close()
    for s, (K, b, r, c) in enumerate(cams):
        one = hip.create(K, b, r, c, p, n_frames=3, n_pairs=1)
        if SEQ_BUDGETS[s]:
            one.set_point_budget([SEQ_BUDGETS[s][0] // 2 & ~15, SEQ_BUDGETS[s][1] // 2 & ~15])
        for k in range(4):
            res = one.add_frame_stereo(seqs[s][k][0], seqs[s][k][1], one.default_stereo_params(32))
            _assert_records_equal(_result_key(res, [one.vo_num_points_at_level(l) for l in range(2)]), multi[s][k], (s, k))
        one.close()


def test_rig_members_with_their_own_budgets_equal_the_context_wide_budget(hip):
    rows, cols = 96, 128
    p = _seq_params(hip)
    X = [np.eye(4, dtype=np.float32), np.ascontiguousarray(synth.twist_to_matrix((0, 0.14, 0.02, 0.3, 0.02, 0.1)), np.float32)]
    seq = synth.make_rig_sequence(rows, cols, 4, [x.astype(np.float64) for x in X], index=3, step_rot=0.01, step_trans=0.08)
    cams = [(np.asarray(seq["K"][q], np.float32).reshape(3, 3), seq["b"][q], rows, cols) for q in range(2)]
    budget = [304, 1008]
    out = {}
    for how in ("per-sequence", "context-wide", "none"):
        ctx = hip.create_sequences(cams, p)
        ctx.rig_set(np.stack(X))
        if how == "per-sequence":
            for s in range(2):
                ctx.seq_set_point_budget(s, budget)
        elif how == "context-wide":
            ctx.set_point_budget(budget)
        out[how] = []
        for k in range(4):
            res = ctx.add_frames_rig([seq["frames"][k][q][0] for q in range(2)], [seq["frames"][k][q][1] for q in range(2)])
            out[how].append(_result_key(res, [ctx.seq_num_points_at_level(s, l) for s in range(2) for l in range(2)]))
        ctx.close()
    for k in range(4):
        _assert_records_equal(out["per-sequence"][k], out["context-wide"][k], k)
    assert out["context-wide"][0]["npts"][0] == budget[0] & ~15 and out["none"][0]["npts"][0] > budget[0]      # (the budget binds)


# ---- off means off ---------------------------------------------------------------------------------------------------------------------------
def _launches(ctx):
    return {k["name"]: k["launches"] for k in ctx.kernel_stats()}


def test_off_means_off(hip, orc):
    rows, cols = 100, 150
    d = synth.make_pair(rows, cols, 5)
    p = make_params(hip, descriptor="bitplanes", levels=2, **_nms_level0(rows, cols))
    refs = _oracle_levels(orc, d, rows, cols, p)
    out = {}
    for how in ("never-set", "zero", "above-every-count"):
        ch = hip.create(d["K"], d["b"], rows, cols, p, device=0, n_frames=2, n_pairs=1)
        ch.profiling(1)
        if how == "zero":
            ch.set_point_budget([0, 0])
        elif how == "above-every-count":
            ch.set_point_budget([len(r["cand"]) + 1 for r in refs])
        ch.frame_set_data(0, d["imgA"], d["dispA"])
        ch.frame_set_template(0)
        ch.frame_set_data(1, d["imgB"], d["dispB"])
        T, st = ch.estimate_pose(0, 0, 1)
        launches = _launches(ch)
        assert launches["saliency_select"] > 0
        assert (launches["point_budget"] > 0) == (how == "above-every-count"), (how, launches)      # no budget: the kernel is not launched
        out[how] = dict(T=T, its=np.array([s["numIterations"] for s in st]))
        for r in refs:
            l = r["level"]
            assert np.array_equal(ch.get_point_indices(0, l), r["inds"]) and bits_equal(ch.get_points(0, l), r["pts"]), (how, l)      # the oracle's template
            info = ch.selection_info(0, l)
            assert info["n_candidates"] == len(r["cand"]) and info["n_ties_kept"] == 0 and bits_equal(np.float32(info["threshold"]), np.float32(p.minSaliency))
            out[how]["pix", l] = ch.get_pixels(0, l)
        ch.close()
    for how in ("zero", "above-every-count"):
        _assert_records_equal(out[how], out["never-set"], how)


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_setting_in_place(hip):
    rows, cols = 96, 128
    cams = _seq_cameras()[:1] * 2
    p = _seq_params(hip)
    ctx = hip.create_sequences(cams, p)
    ctx.set_point_budget([512, 64])
    ctx.seq_set_point_budget(1, [256, 32])

    def rc(fn, *args):
        return ctx.b.fn(fn)(ctx.h, *args)

    def ints(*v):
        return (C.c_int * len(v))(*v)

    bad = [(ints(15, 64), 2), (ints(512, 1), 2), (ints(-1, 64), 2), (ints(512, -16), 2), (ints(512, 64, 32), 3), (None, 1)]
    for arr, n in bad:
        assert rc("set_point_budget", arr, n) == ERR_INVALID_ARG, (list(arr or []), n)
        assert rc("seq_set_point_budget", 1, arr, n) == ERR_INVALID_ARG, (list(arr or []), n)
    assert rc("seq_set_point_budget", 2, ints(512, 64), 2) == ERR_INVALID_ARG      # an unknown sequence
    assert rc("seq_set_point_budget", -1, ints(512, 64), 2) == ERR_INVALID_ARG
    out = ints(*([0] * capi.MAX_LEVELS))
    assert rc("seq_get_point_budget", 2, out, None) == ERR_INVALID_ARG
    assert ctx.get_point_budget() == [512, 64]
    assert ctx.seq_get_point_budget(1) == ([256, 32], True) and ctx.seq_get_point_budget(0) == ([512, 64], False)
    ctx.set_point_budget([512])                                                    # the levels beyond n_levels: no budget
    assert ctx.get_point_budget() == [512, 0]
    ctx.seq_set_point_budget(1, [])                                                # back to the context's
    assert ctx.seq_get_point_budget(1) == ([512, 0], False)
    ctx.close()
