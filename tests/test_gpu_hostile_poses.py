"""The warp's validity rule on the device at the hostile poses of tests/hostile_poses.py: points behind the camera (valid: the rule has no
z > 0 test), zero and tiny depths, integer coordinates, x or y in (-1, 0), the image's last column, and NaN / Inf / coordinates beyond the
int range, where the explicit range test of the device code stands in for x86's cvttsd2si -> INT_MIN.  The rule exists in four hand-written
copies (gn_warp.h warp_point f64 and f32 forms, gn_irls.h the fused frozen-scale path, kernels_gn_team.hip the staged warp phase of the
persistent / team kernels, kernels_gn.hip the cosine / cubic / Hermite kernel); every one is driven here:

 (a) bpvo_hip_linearize at every case against the oracle and, for the f64 form, against numpy directly;
 (b) estimates that start from every case against the oracle's trace, bit for bit (validation mode reference_reduction);
 (c) the persistent kernel, the team kernel and the fused path against the plain four-kernel chain, one pair and a batch of 16 in which every
     case is one pair's start, with the path counters asserted so that no comparison is the chain against itself.

No start raises on either side (RAISES): the oracle, like the reference, has no check of the pose, and neither has the library.

A NaN is compared as a NaN: its sign and payload are the hardware's (0 * inf is the negative "real indefinite" on x86 and a positive quiet NaN
on the GPU), not the algorithm's.  Everything else, infinities included, is compared by bit pattern."""
import numpy as np
import pytest

import hostile_poses as hp
from bpvo_amd import capi
from util import assert_same_run, bits_equal, normal_equations_f64, set_options, setup_pair

pytestmark = pytest.mark.gpu

CONFIGS = {
    "intensity-huber": dict(descriptor="intensity", loss="huber"),                                     # C = 1, speculative tap loads
    "bitplanes-tukey": dict(descriptor="bitplanes", loss="tukey"),                                     # C = 8, tap cache, tiled records
    "fields2-huber": dict(descriptor="fields2", loss="huber"),                                         # generic-C path (pitch)
    "centraldiff80-tukey": dict(descriptor="centraldiff", loss="tukey", centralDifferenceRadius=4),    # channel groups of a wide descriptor
}
# (warp formulation, interpolation)
MODES = {"f64": (0, capi.INTERP_LINEAR), "project_points": (1, capi.INTERP_LINEAR), "dspace": (2, capi.INTERP_LINEAR),
         "cosine": (0, capi.INTERP_COSINE), "cubic": (0, capi.INTERP_CUBIC), "cubic_hermite": (0, capi.INTERP_CUBIC_HERMITE)}
BORDERS = {"f64": (0, 1), "cosine": (0, 1), "cubic": (1, 3), "cubic_hermite": (1, 3)}
LINEARIZE = [(c, s, m) for s in hp.SIZES for c in CONFIGS for m in MODES
             if (c != "centraldiff80-tukey" or s == "96x128") and (m in ("f64", "project_points", "dspace") or c in ("intensity-huber", "bitplanes-tukey"))]
ESTIMATES = ["bitplanes-tukey", "intensity-huber"]
RAISES = ()      # the starts at which estimate_pose raises on both sides: none


def canon(a):
    """NaNs replaced by one NaN (module docstring); dtype and every other bit pattern kept."""
    a = np.array(a, copy=True)
    if a.dtype.kind == "f":
        a[np.isnan(a)] = np.nan
    return a


def same(a, b):
    return bits_equal(canon(np.asarray(a, np.float32)), canon(np.asarray(b, np.float32)))


def canon_stats(st):
    return [dict(s, finalError=float(canon(np.float32(s["finalError"]))), firstOrderOptimality=float(canon(np.float32(s["firstOrderOptimality"])))) for s in st]


def make_pair_contexts(binding, size, config, formulation=0, **kw):
    rows, cols, levels = hp.SIZES[size]
    ctx, d, _ = setup_pair(binding, rows, cols, **dict(dict(CONFIGS[config], levels=levels), **kw))
    X = ctx.get_points(0, 0)      # RigidBodyWarp's points: the poses are built from them whatever the formulation
    if formulation:
        ctx.set_warp_formulation(formulation)
        ctx.frame_set_template(0)
    return ctx, d, X


def within_bar(got, want64, scale):
    """The project's bar for the default mode's sums (test_linearize_parity): 4e-6 of the scale against an f64 evaluation; an entry that is
    not finite there is not finite here."""
    got, want64 = np.atleast_1d(np.asarray(got, np.float64)), np.atleast_1d(np.asarray(want64, np.float64))
    fin = np.isfinite(want64)
    return np.array_equal(np.isfinite(got), fin) and bool(np.all(np.abs(got[fin] - want64[fin]) <= 4e-6 * scale))


@pytest.mark.parametrize("config,size,mode", LINEARIZE)
def test_linearize_at_every_case(hip, orc, config, size, mode):
    """One context, bpvo_hip_linearize(reset_scale) through hostile, identity, hostile, ... and back: every call meets the residual, valid and
    tap-cache buffers of the case before it (the oracle has no cache; linearize itself resets the level's cache keys, so what a stale buffer
    could leak is content, which (b) and (c) complement with real hits).  Per call: valid mask, count, residuals, sigma and weights are the
    oracle's; in reference order H, G, f_norm too, bit for bit; in the default mode they are within 4e-6 of the f64 evaluation of the oracle's
    J, r, w, valid.  The f64 form's masks are also np_valid's, which does not depend on the oracle."""
    rows, cols, _ = hp.SIZES[size]
    formulation, interp = MODES[mode]
    ch, d, _ = make_pair_contexts(hip, size, config, formulation, interp=interp)
    co, _, X = make_pair_contexts(orc, size, config, formulation, interp=interp)
    poses = hp.poses(d["K"], X, rows, cols)
    C = co.Cn
    J = co.get_jacobians(0, 0)
    want = {}
    for name, T in poses.items():
        b = co.linearize(0, 0, 1, 0, T, reset_scale=True)
        o = dict(lin=b, v=co.get_valid(0), r=co.get_residuals(0), w=co.get_weights(0))
        with np.errstate(all="ignore"):
            o["H64"], o["G64"], o["f64"] = normal_equations_f64(J, o["r"], o["w"], o["v"], C)
        if mode in BORDERS:
            x, y = hp.np_project(d["K"], T, X)
            o["np_valid"] = hp.np_valid(x, y, rows, cols, *BORDERS[mode])
        if name in hp.NON_FINITE:
            assert b["num_valid"] == 0 and b["sigma"] == 1.0 and b["f_norm"] == 0.0, (name, b)
        want[name] = o
    for reference in (1, 0):
        ch.set_option("reference_reduction", reference)
        for k, name in enumerate(hp.interleaved()):
            at = (config, size, mode, "reference order" if reference else "default mode", "call", k, name)
            o = want[name]
            a = ch.linearize(0, 0, 1, 0, poses[name], reset_scale=True)
            v = ch.get_valid(0)
            assert np.array_equal(v, o["v"]), (at, int(v.sum()), int(o["v"].sum()), np.flatnonzero(v != o["v"])[:8])
            if "np_valid" in o:
                assert np.array_equal(v.astype(bool), o["np_valid"]), (at, "against numpy")
            assert a["num_valid"] == o["lin"]["num_valid"] == int(o["v"].sum()), at
            assert same(ch.get_residuals(0), o["r"]), at
            assert same(a["sigma"], o["lin"]["sigma"]), (at, a["sigma"], o["lin"]["sigma"])
            assert same(ch.get_weights(0), o["w"]), at
            if reference:
                assert same(a["H"], o["lin"]["H"]) and same(a["G"], o["lin"]["G"]) and same(a["f_norm"], o["lin"]["f_norm"]), (at, a["f_norm"], o["lin"]["f_norm"])
            else:
                fin = np.isfinite(o["H64"])
                scale = np.abs(o["H64"][fin]).max() if fin.any() else 0.0
                gfin = np.isfinite(o["G64"])
                gscale = max(np.abs(o["G64"][gfin]).max() if gfin.any() else 0.0, 1e-3 * scale)
                assert within_bar(a["H"], o["H64"], scale), (at, "H", np.abs(a["H"] - o["H64"]).max(), scale)
                assert within_bar(a["G"], o["G64"], gscale), (at, "G", np.abs(a["G"] - o["G64"]).max(), gscale)
                assert within_bar(a["f_norm"], o["f64"], max(o["f64"], 1e-6) if np.isfinite(o["f64"]) else 0.0), (at, "f_norm", a["f_norm"], o["f64"])
    ch.close(); co.close()


def traces(ctx, T0):
    try:
        T, st, rec = ctx.estimate_pose_trace(0, 0, 1, T0)
    except capi.BpvoError as e:
        return e
    return canon(T), canon_stats(st), canon(rec)


def assert_same_estimates(ch, co, poses, names, what):
    raised = []
    for name in names:
        h, o = traces(ch, poses[name]), traces(co, poses[name])
        if isinstance(o, Exception) or isinstance(h, Exception):
            assert isinstance(o, Exception) and isinstance(h, Exception), (what, name, "one side raises, the other does not", h if isinstance(h, Exception) else o)
            raised.append(name)
            continue
        print(what, name, "iterations", [s["numIterations"] for s in o[1]], "valid", o[2][:, 60].astype(int).tolist(), "sigma", o[2][:, 59].tolist())
        assert_same_run(*h, *o, what=(what, name))
    return raised


@pytest.mark.parametrize("config", ESTIMATES)
def test_estimates_from_hostile_starts_are_the_oracles(hip, orc, config, monkeypatch):
    """96x128, 2 levels, maxIterations 3: estimate_pose from every case, the non-finite ones included, in reference order against the oracle —
    every linearisation's pose, H, G, f_norm, sigma, valid count and step, every level's statistics and the pose.  Same run, or both raise."""
    set_options(monkeypatch, persistent="0")
    ch, d, X = make_pair_contexts(hip, "96x128", config, levels=2, maxIterations=3)
    co, _, _ = make_pair_contexts(orc, "96x128", config, levels=2, maxIterations=3)
    ch.set_option("reference_reduction", 1)
    raised = assert_same_estimates(ch, co, hp.poses(d["K"], X, 96, 128), hp.CASES, config)
    print(config, "starts that raise on both sides:", raised)
    assert tuple(raised) == RAISES
    ch.close(); co.close()


def estimates(hip, config, names, monkeypatch, interp=capi.INTERP_LINEAR, **options):
    """estimate_pose from the named starts on a fresh context created under `options`; poses, statistics and the path counters."""
    monkeypatch.delenv("BPVO_HIP_OPTIONS", raising=False)
    if options:
        set_options(monkeypatch, **options)
    ctx, d, X = make_pair_contexts(hip, "96x128", config, levels=2, maxIterations=3, interp=interp)
    poses = hp.poses(d["K"], X, 96, 128)
    out = {name: ctx.estimate_pose(0, 0, 1, poses[name]) for name in names}
    rec = dict(out=out, fused=ctx.fused_point_counts(), pk=ctx.persistent_counts(), team=ctx.team_counts(), taps=ctx.tap_cache_counts())
    ctx.close()
    return rec


def assert_same_poses(a, b, what):
    for name in a["out"]:
        (Ta, sa), (Tb, sb) = a["out"][name], b["out"][name]
        assert same(Ta, Tb), (what, name, Ta, Tb)
        for key in ("numIterations", "status"):
            assert [s[key] for s in sa] == [s[key] for s in sb], (what, name, key, sa, sb)
        for key in ("finalError", "firstOrderOptimality"):
            assert same([s[key] for s in sa], [s[key] for s in sb]), (what, name, key, sa, sb)


@pytest.mark.parametrize("config", ESTIMATES)
def test_single_pair_kernels_equal_the_chain(hip, config, monkeypatch):
    """One pair from every start: the four-kernel chain against the persistent kernel (the default: kernels_gn_team.hip's staged warp phase and,
    for C = 8, its fused reduction) and against the chain without the fused frozen-scale path (gn_irls.h) — poses and statistics bit for bit,
    and the counters show that each run took the path it is meant to."""
    chain = estimates(hip, config, hp.CASES, monkeypatch, persistent="0")
    default = estimates(hip, config, hp.CASES, monkeypatch)
    unfused = estimates(hip, config, hp.CASES, monkeypatch, persistent="0", fuse_frozen="0")
    print(config, "chain", chain["fused"], chain["pk"], "default", default["fused"], default["pk"], "unfused", unfused["fused"], "taps", chain["taps"])
    assert chain["pk"] == (0, 0) and unfused["pk"] == (0, 0)
    assert default["pk"][0] >= 2 * len(hp.CASES) and default["pk"][1] == 0, default["pk"]      # every level of every estimate, never gave up
    if CONFIGS[config]["descriptor"] == "bitplanes":      # (the fused path is C = 8's)
        assert chain["fused"][0] > 0 and default["fused"] == chain["fused"], (chain["fused"], default["fused"])
    assert unfused["fused"][0] == 0, unfused["fused"]
    assert chain["taps"][0] > 0      # the tap cache was hit: keys written at one pose were looked up at the next
    assert_same_poses(chain, default, (config, "persistent kernel"))
    assert_same_poses(chain, unfused, (config, "fuse_frozen = 0"))


def batch(hip, config, T0, monkeypatch, **options):
    """len(T0) copies of the pair through bpvo_hip_batch_estimate, pair k from T0[k]."""
    monkeypatch.delenv("BPVO_HIP_OPTIONS", raising=False)
    if options:
        set_options(monkeypatch, **options)
    n = len(T0)
    rows, cols, _ = hp.SIZES["96x128"]
    ctx, d, _ = setup_pair(hip, rows, cols, levels=2, maxIterations=3, n_frames=2 * n, n_pairs=n, **CONFIGS[config])
    ctx.frames_set_data(0, 1, np.stack([d["imgA"], d["imgB"]] * n), np.stack([d["dispA"], d["dispB"]] * n))
    ctx.frames_set_template(0, 2, n)
    poses, stats = ctx.batch_estimate(n, np.stack(T0))
    rec = dict(poses=poses, stats=stats, fused=ctx.fused_point_counts(), team=ctx.team_counts(), pk=ctx.persistent_counts())
    ctx.close()
    return rec


def same_pairs(a, b, pairs):
    return all(same(a["poses"][k], b["poses"][k]) and same(a["stats"][k]["finalError"], b["stats"][k]["finalError"]) and
               same(a["stats"][k]["firstOrderOptimality"], b["stats"][k]["firstOrderOptimality"]) and
               np.array_equal(a["stats"][k]["numIterations"], b["stats"][k]["numIterations"]) and np.array_equal(a["stats"][k]["status"], b["stats"][k]["status"])
               for k in pairs)


@pytest.mark.parametrize("config", ESTIMATES)
def test_batch_with_one_hostile_start_per_pair(hip, config, monkeypatch):
    """16 pairs through bpvo_hip_batch_estimate, every case (the non-finite ones too) the start of one pair and the rest at identity: the team
    kernel (the default), the chain and the chain without the fused path agree pair by pair, bit for bit; every pair equals the single-pair
    chain from the same start; and the identity pairs equal the same pairs of a batch that starts at identity throughout — a hostile neighbour
    does not change a healthy pair."""
    ctx, d, X = make_pair_contexts(hip, "96x128", config, levels=2, maxIterations=3)
    ctx.close()
    poses = hp.poses(d["K"], X, 96, 128)
    n = 16
    names = hp.CASES + ["identity"] * (n - len(hp.CASES))
    T0 = [poses[name] for name in names]
    team = batch(hip, config, T0, monkeypatch)
    chain = batch(hip, config, T0, monkeypatch, team="0", persistent="0")
    unfused = batch(hip, config, T0, monkeypatch, team="0", persistent="0", fuse_frozen="0")
    healthy = batch(hip, config, [poses["identity"]] * n, monkeypatch)
    single = estimates(hip, config, hp.CASES, monkeypatch, persistent="0")
    print(config, "team", team["team"], team["pk"], team["fused"], "chain", chain["team"], chain["fused"], "unfused", unfused["fused"])
    assert team["team"] > 0 and team["pk"][1] == 0 and healthy["team"] > 0, (team["team"], team["pk"])
    assert chain["team"] == 0 and unfused["team"] == 0 and chain["pk"] == (0, 0)
    if CONFIGS[config]["descriptor"] == "bitplanes":
        assert chain["fused"][0] > 0 and team["fused"][0] > 0, (chain["fused"], team["fused"])
    assert unfused["fused"][0] == 0
    everyone = range(n)
    assert same_pairs(team, chain, everyone), [k for k in everyone if not same_pairs(team, chain, [k])]
    assert same_pairs(chain, unfused, everyone), [k for k in everyone if not same_pairs(chain, unfused, [k])]
    at_identity = [k for k, name in enumerate(names) if name == "identity"]
    assert len(at_identity) == 3
    assert same_pairs(team, healthy, at_identity), "a hostile neighbour changed a healthy pair"
    assert same_pairs(healthy, healthy, everyone) and all(same(healthy["poses"][k], healthy["poses"][0]) for k in everyone)
    for k, name in enumerate(hp.CASES):
        T, st = single["out"][name]
        assert same(chain["poses"][k], T), (name, chain["poses"][k], T)
        assert [s["numIterations"] for s in st] == chain["stats"][k]["numIterations"].tolist() and [s["status"] for s in st] == chain["stats"][k]["status"].tolist(), name


@pytest.mark.parametrize("config", ESTIMATES)
@pytest.mark.parametrize("interp", ["cosine", "cubic_hermite"])
def test_interpolation_kernel_inside_an_estimate(hip, orc, interp, config, monkeypatch):
    """kernels_gn.hip's own copy of the rule (the (0, 1) and (1, 3) borders) inside an estimate, from the "all behind", "zero depth" and "camera
    in the plane" starts: in reference order the oracle's run bit for bit; and persistent = 0 against the default.  (The persistent kernel is
    kLinear's: both of those take warp_residual_interp_kernel, which the counter confirms — the oracle is the comparison that can fail.)"""
    names = ["all_behind", "zero_depth", "camera_in_plane"]
    it = MODES[interp][1]
    chain = estimates(hip, config, names, monkeypatch, interp=it, persistent="0")
    default = estimates(hip, config, names, monkeypatch, interp=it)
    assert chain["pk"] == (0, 0) and default["pk"] == (0, 0)
    assert_same_poses(chain, default, (config, interp))
    set_options(monkeypatch, persistent="0")
    ch, d, X = make_pair_contexts(hip, "96x128", config, levels=2, maxIterations=3, interp=it)
    co, _, _ = make_pair_contexts(orc, "96x128", config, levels=2, maxIterations=3, interp=it)
    ch.set_option("reference_reduction", 1)
    assert assert_same_estimates(ch, co, hp.poses(d["K"], X, 96, 128), names, (config, interp)) == []
    ch.close(); co.close()
