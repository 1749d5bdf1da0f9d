"""K7, the exact median of |r| and the robust scale (bpvo_amd/csrc/gn_median.h, bracket_chunk in gn_common.h), on residual multisets the
synthetic scenes never produce: heavy ties, bulk zeros, two-valued keys, a handful of valid points (tests/robust_scale_cases.py; that every
case has the property it is built for is checked on the oracle in tests/test_robust_scale_inputs_cpu.py).

No tolerance anywhere: residuals, valid flags, sigma and weights are the oracle's bit for bit, sigma is also the plain numpy rule's
(np.partition + the utils.h / mestimator.cc rules) evaluated on what the GPU context hands back, and bpvo_hip_median_path_counts moves by
what the numpy mirror of the path decisions predicts.  Then every instantiation of the code (dense-run form, persistent kernel, team kernel,
512-thread shape) against the plain four-kernel chain, and two cases against the oracle in reference order."""
import numpy as np
import pytest

import robust_scale_cases as rsc
from util import assert_same_run, bits_equal, set_options

pytestmark = pytest.mark.gpu

CHAIN = dict(lanes="1", team="0", persistent="0", dense_candidates_from=str(1 << 30))      # the four-kernel chain, one segment per chunk


def same_weights(a, b):
    """bit-equal, NaNs (sigma = inf: 0 x inf) compared by position"""
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and bits_equal(a[~na], b[~nb])


@pytest.mark.parametrize("name", rsc.CASES)
def test_linearize_sequences(hip, orc, name, monkeypatch):
    set_options(monkeypatch, **CHAIN)
    cs = rsc.case(name)
    ch, co = cs.create(hip), cs.create(orc)
    before = ch.median_path_counts()
    wh, wo = rsc.walk(ch, cs), rsc.walk(co, cs)
    after = ch.median_path_counts()
    analysis = rsc.analyse(cs, wh)                 # the plain reference, from the arrays of the GPU context
    print(rsc.check_property(cs, analysis))        # (the oracle's arrays have it: the GPU's are about to be shown equal)
    for k, (sh, so, rows) in enumerate(zip(wh, wo, analysis)):
        for i, (a, b, r) in enumerate(zip(sh, so, rows)):
            at = (name, "run", k, "linearisation", i, r["multiset"], r["path"])
            print(at, "sigma", a["sigma"])
            assert np.array_equal(a["valid"], b["valid"]) and a["num_valid"] == b["num_valid"], at
            assert bits_equal(a["r"], b["r"]), at
            assert bits_equal(a["sigma"], b["sigma"]), (at, a["sigma"], b["sigma"])
            assert bits_equal(a["sigma"], np.float32(r["sigma"])), (at, a["sigma"], r["sigma"])
            assert same_weights(a["w"], b["w"]), at
    predicted = rsc.predicted_counts(analysis)
    got = (after[0] - before[0], after[1] - before[1])
    print(name, "median_path_counts (bracketed, full):", got)
    assert got == predicted, (name, got, predicted)


# ---- every instantiation against the plain chain ---------------------------------------------------------------------------------------------
def estimate_copies(hip, cs, start, n, **kw):
    """n copies of one start of the case (template, current image, starting pose) through bpvo_hip_batch_estimate."""
    ctx = hip.create(cs.K, cs.b, cs.rows, cs.cols, cs.make_params(hip, **kw), n_frames=2 * n, n_pairs=n)
    if cs.formulation:
        ctx.set_warp_formulation(cs.formulation)
    ctx.frames_set_data(0, 1, np.stack([cs.imgA, start.cur] * n), np.stack([cs.disp] * (2 * n)))
    ctx.frames_set_template(0, 2, n)
    poses, stats = ctx.batch_estimate(n, np.stack([start.T0] * n))
    out = dict(poses=poses, stats=stats, med=ctx.median_path_counts(), lin=ctx.total_linearizations(), team=ctx.team_counts(), pk=ctx.persistent_counts())
    ctx.close()
    return out


def replay(hip, cs, start, **kw):
    """What the selection meets during the chain's estimate of one start: the estimate's trace (the pose of every linearisation), then every one
    of them again through bpvo_hip_linearize, the estimator reset at the first of a level, and the downloaded residuals and flags through the plain
    scale rule and the numpy path model.  -> [dict(level, keys, sigma, recomputed, path, multiset)]; sigma and the valid count of every
    linearisation are asserted to be the trace's."""
    ctx = cs.create(hip, **kw)
    ctx.frame_set_data(1, start.cur, cs.disp)
    _, _, rec = ctx.estimate_pose_trace(0, 0, 1, start.T0)
    rows, level, tracker, model = [], None, None, None
    for q in rec:
        l = int(q[67])
        if l != level:
            level, tracker, model = l, rsc.ScaleTracker(), rsc.PathModel()
            first = True
        a = ctx.linearize(0, 0, 1, l, q[:16].reshape(4, 4), reset_scale=first)
        first = False
        valid = ctx.get_valid(0)
        keys = rsc.keys_of(ctx.get_residuals(0), valid, cs.C)
        sigma, recomputed = tracker.step(keys)
        same = lambda x: np.float32(x).tobytes() == np.float32(q[59]).tobytes()
        assert a["num_valid"] == int(q[60]) and same(a["sigma"]) and same(sigma), (cs.name, start.label, l, a["sigma"], sigma, q[59])
        rows.append(dict(level=l, keys=keys, sigma=sigma, recomputed=recomputed, path=model.step(keys, valid.size) if recomputed else None, multiset=rsc.multiset(keys)))
    ctx.close()
    return rows


def evidence(rows):
    """The branches of a replay, for the log and for assertions: key counts per level, the paths, and what the selections met."""
    paths = [r["path"] for r in rows if r["recomputed"]]
    br, fu = [p for p in paths if p["path"] == "bracketed"], [p for p in paths if p["path"] == "full"]
    return dict(n=[(r["level"], r["multiset"]["n"]) for r in rows], counts=(len(br), len(fu)),
                ties=[(r["multiset"]["distinct"], r["multiset"]["tie"]) for r in rows if r["recomputed"]],
                largest_bracket=max([p["m"] for p in br], default=0), fullest_bin=max([p["bin"] for p in br], default=0),
                most_shared=max([p.get("shared", 0) for p in fu], default=0), split=any(p.get("split") for p in paths),
                sigma_inf=any(np.isinf(r["sigma"]) for r in rows))


STARTS = [(name, st.label) for name in rsc.CASES for st in rsc.case(name).starts()]
_chain = {}


def chain_result(hip, cs, start, monkeypatch):
    """The four-kernel chain's estimate of a start (once per session), with the path counts the numpy model predicts from its replay."""
    key = (cs.name, start.label)
    if key not in _chain:
        set_options(monkeypatch, **CHAIN)
        ref = estimate_copies(hip, cs, start, 1)
        assert ref["team"] == 0 and ref["pk"] == (0, 0)
        ref["evidence"] = evidence(replay(hip, cs, start))
        print(key, "chain:", ref["evidence"])
        assert ref["med"] == ref["evidence"]["counts"], (key, ref["med"], ref["evidence"])
        assert ref["lin"] == len(ref["evidence"]["n"])
        if start.reach_n is not None:
            assert (0, start.reach_n) in ref["evidence"]["n"] and ref["evidence"]["sigma_inf"] == (start.reach_n == 6), (key, ref["evidence"])
        _chain[key] = ref
    return _chain[key]


def assert_copies_of(ref, got, n, what):
    for k in range(n):
        assert bits_equal(got["poses"][k], ref["poses"][0]), (what, k, got["poses"][k], ref["poses"][0])
        assert got["stats"][k].tobytes() == ref["stats"][0].tobytes(), (what, k, got["stats"][k], ref["stats"][0])      # numIterations, finalError, optimality, status
    assert got["med"] == (n * ref["med"][0], n * ref["med"][1]), (what, got["med"], ref["med"])
    assert got["lin"] == n * ref["lin"], (what, got["lin"], ref["lin"])


# (the persistent and team kernels serve the default warp formulation only: all-zero, in disparity space, would compare the chain with itself there)
@pytest.mark.parametrize("name,label,variant", [(n, l, v) for n, l in STARTS for v in ("dense-run", "persistent", "team")
                                                if v == "dense-run" or not rsc.case(n).formulation])
def test_instantiations_equal_the_chain(hip, name, label, variant, monkeypatch):
    """Every start of every case (each run's image and first pose; tiny-n: one start per valid count 7, 6, 5, 3, 2, 1, which the first level-0
    linearisation of the estimate sees) through the dense-run form, the persistent kernel and the team kernel (8 copies): poses, per-level
    statistics, median_path_counts and total_linearizations of the chain, whose own path counts are what the numpy model predicts."""
    cs = rsc.case(name)
    start = {st.label: st for st in cs.starts()}[label]
    ref = chain_result(hip, cs, start, monkeypatch)
    if variant == "dense-run":
        set_options(monkeypatch, **dict(CHAIN, dense_candidates_from="0"))
        got, n = estimate_copies(hip, cs, start, 1), 1
    elif variant == "persistent":
        monkeypatch.delenv("BPVO_HIP_OPTIONS", raising=False)      # one pair, default options
        got, n = estimate_copies(hip, cs, start, 1), 1
        assert got["pk"][0] > 0 and got["pk"][1] == 0, got["pk"]
    else:
        monkeypatch.delenv("BPVO_HIP_OPTIONS", raising=False)
        set_options(monkeypatch, team="1")
        got, n = estimate_copies(hip, cs, start, 8), 8
        assert got["team"] > 0, "the team kernel should have run"
    print(name, label, variant, "median_path_counts", got["med"], "linearisations", got["lin"], "iterations", got["stats"]["numIterations"][0])
    assert_copies_of(ref, got, n, (name, label, variant))


WIDE = {"intensity": [("bracket-miss", "run0"), ("tiny-n", "n7"), ("tiny-n", "n6"), ("tiny-n", "n5"), ("tiny-n", "n3"), ("tiny-n", "n2"), ("tiny-n", "n1"),
                      ("bracket-miss", "run0")],
        "bitplanes": [("two-valued", "run0"), ("two-valued", "run1"), ("two-valued-straddle", "run0"), ("two-valued-straddle", "run1")]}


@pytest.mark.parametrize("group", ["intensity", "bitplanes"])
def test_wide_launch_shape_equals_the_chain(hip, group, monkeypatch):
    """264 workspaces in one launch (more than 256: median_finish_kernel's 512-thread / 2-copy / 7168-word shape), cycling through the starts of
    the 160 x 120 cases of one descriptor, against the same pairs in launches of 66 (the 1024-thread shape): poses, statistics, path counts,
    linearisations.  The path counts are also the numpy model's, from a replay of every start; the replays show what the selections of the
    wide launch met — bitplanes: a pass-3 rescan (more than 7168 keys share the median's top bits), a bracket of more than 6144 keys, split
    cursors; intensity: n = 7, 6 (sigma inf), 5, 3, 2, 1 and bracket misses.  (all-zero runs the other warp formulation, a context setting: it
    is in no group.)"""
    set_options(monkeypatch, lanes="1", team="0", persistent="0")
    picks = [(rsc.case(c), {st.label: st for st in rsc.case(c).starts()}[l]) for c, l in WIDE[group]]
    n, sub, iters = 264, 66, 5
    assert n % len(picks) == 0
    cs0 = picks[0][0]
    ev = [evidence(replay(hip, cs, st, maxIterations=iters)) for cs, st in picks]
    for (cs, st), e in zip(picks, ev):
        print(group, cs.name, st.label, e)
    predicted = tuple(n // len(picks) * sum(e["counts"][i] for e in ev) for i in (0, 1))
    if group == "bitplanes":
        assert max(e["most_shared"] for e in ev) > rsc.SHAPES[512]["CACHE"] and max(e["largest_bracket"] for e in ev) > rsc.lds_room(512)
        assert any(e["split"] for e in ev)
    else:
        assert {1, 2, 3, 5, 6, 7} <= {k for e in ev for l, k in e["n"] if l == 0} and any(e["sigma_inf"] for e in ev)
    imgs = np.empty((2 * n, cs0.rows, cs0.cols), np.uint8)
    T0 = np.empty((n, 4, 4), np.float32)
    for k in range(n):
        cs, st = picks[k % len(picks)]
        imgs[2 * k], imgs[2 * k + 1], T0[k] = cs.imgA, st.cur, st.T0
    disps = np.stack([cs0.disp] * (2 * n))
    outs = []
    for width in (n, sub):
        ctx = hip.create(cs0.K, cs0.b, cs0.rows, cs0.cols, cs0.make_params(hip, maxIterations=iters), n_frames=2 * width, n_pairs=width)
        poses, stats = [], []
        for k in range(0, n, width):
            ctx.frames_set_data(0, 1, imgs[2 * k: 2 * (k + width)], disps[2 * k: 2 * (k + width)])
            ctx.frames_set_template(0, 2, width)
            p, s = ctx.batch_estimate(width, T0[k: k + width])
            poses.append(p); stats.append(s)
        outs.append((np.concatenate(poses), np.concatenate(stats), ctx.median_path_counts(), ctx.total_linearizations()))
        ctx.close()
    (pw, sw, mw, lw), (pn, sn, mn, ln) = outs
    print(group, "median_path_counts", mw, "predicted", predicted, "linearisations", lw)
    assert bits_equal(pw, pn) and sw.tobytes() == sn.tobytes()
    assert mw == mn == predicted and lw == ln == n // len(picks) * sum(len(e["n"]) for e in ev)


@pytest.mark.parametrize("name", ["ties-large", "two-valued-straddle"])
def test_reference_order_estimate_is_the_oracles(hip, orc, name, monkeypatch):
    """estimate_pose in the validation mode reference_reduction against the oracle: every linearisation's pose, H, G, f, sigma, valid count and
    step, every level's iterations, status and final error, and the pose, bit for bit."""
    set_options(monkeypatch, persistent="0")
    cs = rsc.case(name)
    ch, co = cs.create(hip), cs.create(orc)
    ch.set_option("reference_reduction", 1)
    Th, sh, rh = ch.estimate_pose_trace(0, 0, 1, cs.runs[0].poses[0])
    To, so, ro = co.estimate_pose_trace(0, 0, 1, cs.runs[0].poses[0])
    assert_same_run(Th, sh, rh, To, so, ro, name)
    ch.close(); co.close()
