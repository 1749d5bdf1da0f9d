"""The measurement variance on the device (c_api.h "measurement variance") against the numpy statement of the rule (tests/disparity_variance_ref.py),
bit for bit: the kernel through bpvo_hip_disparity_variance_frames on every path it has; the filter with a caller's variances; the stereo drivers as
"the rule plus today's drivers"; off is off; refusals; the C++ facade.

The library serves cameras of at least 8 x 8 pixels, so the smallest shape here is 9 x 11 where the CPU test runs 1 x 1 and 5 x 7."""
import os
import subprocess

import numpy as np
import pytest

import disparity_fusion_ref as fref
import disparity_variance_ref as ref
from bpvo_amd import capi, synth
from util import bits_equal, make_params

pytestmark = pytest.mark.gpu
F32 = np.float32

FUSION = dict(mode=1, measurement_sigma=0.5, process_sigma=0.1, gate=3.0, max_fill_sigma=2.0)
FPRM = fref.rule(0.5, 0.1, 3.0, 2.0)
VARIANCE = ref.setting(ref.RULE)      # radius 2, noise 2 grey levels, clamp 0.02 .. 2 px
SHAPES = [(9, 11), (33, 65), (61, 131)]
GATES = ((0.001, 64.0), (-1.0e4, float(ref.F32_MAX)))


@pytest.fixture(scope="module")
def plain(hip):
    """A context that serves the stand-alone calls: nothing of it depends on its camera."""
    K = np.array([[100, 0, 64], [0, 100, 32], [0, 0, 1]], F32)
    ctx = hip.create(K, 0.1, 64, 128, make_params(hip, levels=1), n_frames=3, n_pairs=1)
    yield ctx
    ctx.close()


def _assert_maps(got, want, what):
    (maps, counts), (rmaps, rcounts) = got, want
    for k, (a, b) in enumerate(zip(maps, rmaps)):
        assert ref.same_bits(a, b), (what, k, np.argwhere(ref.bits(a) != ref.bits(b))[:5], a[ref.bits(a) != ref.bits(b)][:5], b[ref.bits(a) != ref.bits(b)][:5])
    assert counts == rcounts, (what, counts, rcounts)


def _want(prm, Ls, Rs, Ms, lo, hi):
    out = [ref.variance(prm, L, R, M, lo, hi) for L, R, M in zip(Ls, Rs, Ms)]
    return [o[0] for o in out], [o[1] for o in out]


# ---- 1. the rule -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", [1, 3, 7])
def test_rule_three_unlike_cameras_in_one_call(plain, radius):
    prm = ref.rule(radius, 2.0, 0.02, 2.0)
    pairs = [ref.random_pair(r, c, seed=c + radius) for r, c in SHAPES]
    Ls, Rs = [p[0] for p in pairs], [p[1] for p in pairs]
    Ms = [ref.hostile_disparities(r, c, radius, seed=r, hi=64.0) for r, c in SHAPES]
    seen = {k: 0 for k in ref.CLASSES}
    for lo, hi in GATES:
        launches0, pixels0, _ = plain.measurement_variance_counts()
        got = plain.disparity_variance_frames(Ls, Rs, Ms, lo, hi, ref.setting(prm))
        launches, pixels, _ = plain.measurement_variance_counts()
        assert launches == launches0 + 1 and pixels == pixels0 + sum(r * c for r, c in SHAPES)      # one launch for the three cameras
        want = _want(prm, Ls, Rs, Ms, lo, hi)
        _assert_maps(got, want, (radius, lo))
        for c in want[1]:
            assert sum(c.values()) in [r * w for r, w in SHAPES]
            for k in ref.CLASSES:
                seen[k] += c[k]
    assert seen["invalid"] > 0 and seen["border"] > 0 and seen["model"] + seen["floor"] + seen["ceiling"] + seen["flat"] > 0, seen


# ---- 2. every path of the kernel -------------------------------------------------------------------------------------------------------------
def test_staged_and_direct_tiles_give_the_same_integers(plain):
    """The kernel stages the right strip of a tile in LDS where the disparities of the tile spread little, and reads the right image where it lies
    otherwise (kernels_disparity_variance.hip: a strip of at most 160 columns).  A smooth map takes the first path in every tile that needs sums;
    independent disparities in [1, 280] spread over more than 160 columns wherever the tile lies far enough right to hold them."""
    rows, cols, radius = 48, 300, 3
    prm = ref.rule(radius, 2.0, 0.02, 2.0)
    L, R = ref.random_pair(rows, cols, seed=5)
    smooth = ref.smooth_disparities(rows, cols, 3.0, 40.0)
    rng = np.random.default_rng(11)
    wild = rng.integers(1, 281, (rows, cols)).astype(F32)
    tiles = ((rows + 7) // 8) * ((cols + 31) // 32)
    for name, M in (("smooth", smooth), ("wild", wild)):
        t0 = plain.measurement_variance_counts()[2]
        got = plain.disparity_variance_frames([L], [R], [M], 0.001, 512.0, ref.setting(prm))
        t1 = plain.measurement_variance_counts()[2]
        staged, direct, idle = (b - a for a, b in zip(t0, t1))
        want = _want(prm, [L], [R], [M], 0.001, 512.0)
        _assert_maps(got, want, name)
        assert want[1][0]["invalid"] == 0 and want[1][0]["model"] + want[1][0]["floor"] + want[1][0]["ceiling"] + want[1][0]["flat"] > 1000, want[1]
        assert staged + direct + idle == tiles, (name, staged, direct, idle)
        if name == "smooth":
            assert direct == 0 and staged > tiles // 2, (staged, direct, idle)
        else:
            assert direct >= tiles // 4, (staged, direct, idle)


# ---- 3. overflow and the flat class ----------------------------------------------------------------------------------------------------------
def test_checkerboard_against_its_inverse_and_a_constant_image(plain):
    rows, cols, radius = 33, 65, 7
    prm = ref.rule(radius, 2.0, 0.02, 2.0)
    M = np.full((rows, cols), 2.0, F32)      # an even shift: S_0 = 225 * 65025, the largest sum; an odd one: S_-1 = S_+1 = 225 * 65025
    M[::2, ::3] = 3.0
    Lc, Rc = ref.checkerboard_pair(rows, cols)
    Lk, Rk = ref.constant_pair(rows, cols)
    got = plain.disparity_variance_frames([Lc, Lk], [Rc, Rk], [M, M], 0.001, 64.0, ref.setting(prm))
    want = _want(prm, [Lc, Lk], [Rc, Rk], [M, M], 0.001, 64.0)
    _assert_maps(got, want, "checkerboard / constant")
    assert want[1][0]["flat"] > 0 and want[1][0]["floor"] > 0 and want[1][0]["model"] + want[1][0]["ceiling"] == 0
    assert want[1][1]["flat"] + want[1][1]["border"] == rows * cols and want[1][1]["flat"] > 0


# ---- 4. no state -----------------------------------------------------------------------------------------------------------------------------
def test_a_pair_alone_and_among_five_others_and_the_same_call_twice(plain):
    shapes = [(33, 65), (61, 131), (9, 11), (48, 300), (33, 65), (20, 40)]
    pairs = [ref.random_pair(r, c, seed=30 + i) for i, (r, c) in enumerate(shapes)]
    Ls, Rs = [p[0] for p in pairs], [p[1] for p in pairs]
    Ms = [ref.hostile_disparities(r, c, 2, seed=40 + i) for i, (r, c) in enumerate(shapes)]
    s = ref.setting(ref.RULE)
    a = plain.disparity_variance_frames(Ls, Rs, Ms, 0.001, 64.0, s)
    b = plain.disparity_variance_frames(Ls, Rs, Ms, 0.001, 64.0, s)
    _assert_maps(b, a, "twice")
    alone = plain.disparity_variance_frames([Ls[3]], [Rs[3]], [Ms[3]], 0.001, 64.0, s)
    assert ref.same_bits(alone[0][0], a[0][3]) and alone[1][0] == a[1][3]
    _assert_maps(a, _want(ref.RULE, Ls, Rs, Ms, 0.001, 64.0), "six")


# ---- 5. the filter with a caller's variances -------------------------------------------------------------------------------------------------
def _K(cam):
    return np.array([[cam["fx"], 0, cam["cx"]], [0, cam["fy"], cam["cy"]], [0, 0, 1]], F32)


def _fusion_ctx(hip, cams):
    p = make_params(hip, levels=1, minValidDisparity=float(cams[0]["lo"]), maxValidDisparity=float(cams[0]["hi"]))
    ctx = hip.create_sequences([(_K(c), float(c["b"]), c["rows"], c["cols"]) for c in cams], p)
    ctx.set_disparity_fusion(FUSION)
    return ctx


def _fusion_state(ctx, s, cam):
    D, V = ctx.seq_get_fused_disparity(s)
    info = ctx.seq_disparity_fusion_info(s)
    return D, V, info, ctx.get_disparity(info["slot"], (cam["rows"], cam["cols"]))


def _assert_step(got, want, what):
    D, V, info, slot = got
    rD, rV, rcounts = want
    assert ref.same_bits(D, rD), (what, "D", np.argwhere(ref.bits(D) != ref.bits(rD))[:5])
    assert ref.same_bits(V, rV), (what, "V", np.argwhere(ref.bits(V) != ref.bits(rV))[:5])
    assert ref.same_bits(slot, rD), (what, "slot")
    assert {k: info[k] for k in fref.CLASSES} == rcounts, (what, info, rcounts)


def _variance_maps(shape, seed):
    """Variances between 0.01 and 4 among entries that take the constant: 0, -0, negative, NaN, +-Inf."""
    rng = np.random.default_rng(seed)
    R2 = rng.uniform(0.01, 4.0, shape).astype(F32)
    special = np.array([0.0, -0.0, -1.0, np.nan, np.inf, -np.inf, ref.F32_MAX, np.finfo(F32).tiny], F32)
    flat = R2.reshape(-1)
    at = rng.permutation(flat.size)[:flat.size // 4]
    flat[at] = special[np.arange(at.size) % special.size]
    return R2


def test_fuse_disparities_var_three_chained_steps_and_the_constant_form_is_unchanged(hip):
    cases = [fref.chain_case(r, c, seed=c) for r, c in SHAPES]
    cams = [c[0] for c in cases]
    a, b = _fusion_ctx(hip, cams), _fusion_ctx(hip, cams)
    carried_a = [(None, None)] * 3
    carried_b = [(None, None)] * 3
    for k in range(3):
        Ms, Ps = [c[1][k] for c in cases], [c[2][k] for c in cases]
        R2s = [_variance_maps(M.shape, 100 + 10 * k + i) for i, M in enumerate(Ms)]
        a.fuse_disparities_var(Ms, R2s, Ps)
        b.fuse_disparities(Ms, Ps)
        for s in range(3):
            P = None if k == 0 else Ps[s]
            want = ref.step_var(cams[s], FPRM, Ms[s], R2s[s], carried_a[s][0], carried_a[s][1], P)
            _assert_step(_fusion_state(a, s, cams[s]), want, ("var", k, s))
            carried_a[s] = want[:2]
            old = fref.step(cams[s], FPRM, Ms[s], carried_b[s][0], carried_b[s][1], P)
            _assert_step(_fusion_state(b, s, cams[s]), old, ("constant", k, s))
            carried_b[s] = old[:2]
            if k == 2:
                assert not ref.same_bits(want[1], old[1])      # (the maps do change the filter)
    a.close(); b.close()


# ---- 6. the drivers are the rule plus today's drivers ------------------------------------------------------------------------------------------
VO_KW = dict(loss="huber", levels=3, minTranslationMagToKeyFrame=0.035, minRotationMagToKeyFrame=100.0, maxFractionOfGoodPointsToKeyFrame=0.0)


def _cam_of(seq, rows, cols, p):
    K = np.asarray(seq["K"], F32)
    return fref.camera(rows, cols, fx=K[0, 0], fy=K[1, 1], cx=K[0, 2], cy=K[1, 2], b=seq["b"], lo=p.minValidDisparity, hi=p.maxValidDisparity)


def _same_results(ra, rb, what):
    assert bits_equal(ra["pose"], rb["pose"]) and ra["stats"] == rb["stats"], (what, ra["stats"], rb["stats"])
    assert ra["isKeyFrame"] == rb["isKeyFrame"] and ra["keyFramingReason"] == rb["keyFramingReason"] and ra["hasPointCloud"] == rb["hasPointCloud"], what


class _Chain:
    """The numpy side of a sequence: the variance map of every frame and the fusion chain with it."""

    def __init__(self, cam):
        self.cam, self.D, self.V, self.frames = cam, None, None, 0
        self.seen = {k: 0 for k in ref.CLASSES}
        self.fused = 0

    def step(self, left, right, M, pose, variance=True):
        R2, vcounts = ref.variance(ref.RULE, left, right, M, self.cam["lo"], self.cam["hi"]) if variance else (None, None)
        want = ref.step_var(self.cam, FPRM, M, R2, self.D, self.V, None if self.frames == 0 else pose)
        self.D, self.V = want[:2]
        self.frames += 1
        self.fused += want[2]["fused"]
        for k in ref.CLASSES:
            self.seen[k] += vcounts[k] if variance else 0
        return want, R2, vcounts


def test_add_frames_stereo_is_the_rule_plus_todays_driver(hip):
    sizes = [(120, 160), (96, 128)]
    n_frames = 5
    seqs = [synth.make_stereo_sequence(r, c, n_frames, index=i) for i, (r, c) in enumerate(sizes)]
    p = make_params(hip, descriptor="bitplanes", **VO_KW)
    cameras = [(s["K"], s["b"], r, c) for s, (r, c) in zip(seqs, sizes)]
    A = hip.create_sequences(cameras, p)
    B = hip.create_sequences(cameras, p)      # fusion and variance off: the front-end alone, and today's add_frames
    A.set_disparity_fusion(FUSION)
    A.set_measurement_variance(VARIANCE)
    with pytest.raises(capi.BpvoError, match="status -3:"):      # BPVO_ERR_NO_DATA before the first stereo call
        A.seq_measurement_variance_info(0)
    sp = A.default_stereo_params(ndisp=32)
    chains = [_Chain(_cam_of(s, r, c, p)) for s, (r, c) in zip(seqs, sizes)]
    for f in range(n_frames):
        lefts = [s["frames"][f][0] for s in seqs]
        rights = [s["frames"][f][1] for s in seqs]
        Ms = B.stereo_frames(sizes, lefts, rights, sp)
        launches0 = A.measurement_variance_counts()[0]
        ra = A.add_frames_stereo(lefts, rights, sp)
        assert A.measurement_variance_counts()[0] == launches0 + 1      # once per call, for both sequences
        fusedD = []
        for s in range(2):
            want, R2, vcounts = chains[s].step(lefts[s], rights[s], Ms[s], ra[s]["pose"])
            _assert_step(_fusion_state(A, s, chains[s].cam), want, (f, s))
            assert ref.same_bits(A.seq_get_measurement_variance_map(s), R2), (f, s)
            assert A.seq_measurement_variance_info(s) == vcounts, (f, s)
            fusedD.append(want[0])
        rb = B.add_frames(lefts, fusedD)
        for s in range(2):
            _same_results(ra[s], rb[s], (f, s))
            for level in range(A.L):
                assert A.seq_num_points_at_level(s, level) == B.seq_num_points_at_level(s, level), (f, s, level)
    for s in range(2):
        assert bits_equal(A.seq_trajectory(s), B.seq_trajectory(s))
        assert chains[s].fused > 0 and chains[s].seen["model"] + chains[s].seen["floor"] > 0 and chains[s].seen["invalid"] > 0, chains[s].seen
    assert B.measurement_variance_counts()[:2] == (0, 0) and B.disparity_fusion_counts() == (0, 0)
    A.seq_reset(1)
    with pytest.raises(capi.BpvoError):
        A.seq_measurement_variance_info(1)      # the record does not outlive the reset
    assert A.seq_get_measurement_variance(1)[0]["mode"] == 1      # the setting does
    A.close(); B.close()


def test_add_frame_stereo_is_the_rule_plus_todays_driver(hip):
    rows, cols, n_frames = 120, 160, 5
    seq = synth.make_stereo_sequence(rows, cols, n_frames, index=0)
    p = make_params(hip, descriptor="bitplanes", **VO_KW)
    A = hip.create(seq["K"], seq["b"], rows, cols, p, n_frames=3, n_pairs=1)
    B = hip.create(seq["K"], seq["b"], rows, cols, p, n_frames=3, n_pairs=1)
    A.set_disparity_fusion(FUSION)
    A.set_measurement_variance(VARIANCE)
    sp = A.default_stereo_params(ndisp=32)
    chain = _Chain(_cam_of(seq, rows, cols, p))
    keyframes = 0
    for f, (left, right) in enumerate(seq["frames"]):
        M = B.stereo_frames([(rows, cols)], [left], [right], sp)[0]
        ra = A.add_frame_stereo(left, right, sp)
        want, R2, vcounts = chain.step(left, right, M, ra["pose"])
        Da, Va = A.vo_get_fused_disparity()
        info = A.vo_disparity_fusion_info()
        _assert_step((Da, Va, info, A.get_disparity(info["slot"])), want, f)
        assert ref.same_bits(A.vo_get_measurement_variance(), R2) and A.vo_measurement_variance_info() == vcounts, f
        rb = B.add_frame(left, want[0])
        _same_results(ra, rb, f)
        keyframes += int(f > 0 and ra["isKeyFrame"])
    assert bits_equal(A.trajectory(), B.trajectory()) and chain.fused > 0 and keyframes > 0
    A.close(); B.close()


def test_add_frames_stereo_raw_with_identity_maps_is_the_rule_plus_todays_driver(hip):
    rows, cols, n_frames = 96, 128, 3
    seq = synth.make_stereo_sequence(rows, cols, n_frames, index=1)
    p = make_params(hip, descriptor="bitplanes", **VO_KW)
    A = hip.create(seq["K"], seq["b"], rows, cols, p, n_frames=3, n_pairs=1)
    B = hip.create(seq["K"], seq["b"], rows, cols, p, n_frames=3, n_pairs=1)
    yy, xx = np.mgrid[0:rows, 0:cols]
    for ctx in (A, B):
        for side in (0, 1):
            ctx.set_rectification_maps(side, rows, cols, xx.astype(F32), yy.astype(F32), seq=0)
    A.set_disparity_fusion(FUSION)
    A.seq_set_measurement_variance(0, VARIANCE)
    sp = A.default_stereo_params(ndisp=32)
    chain = _Chain(_cam_of(seq, rows, cols, p))
    for f, (left, right) in enumerate(seq["frames"]):
        rl, rr = B.rectify_frames([left], 0, seq=[0])[0], B.rectify_frames([right], 1, seq=[0])[0]      # the pair the front-end sees
        M = B.stereo_frames([(rows, cols)], [rl], [rr], sp)[0]
        ra = A.add_frames_stereo_raw([left], [right], sp)[0]
        want, R2, vcounts = chain.step(rl, rr, M, ra["pose"])
        _assert_step(_fusion_state(A, 0, chain.cam), want, f)
        assert ref.same_bits(A.seq_get_measurement_variance_map(0), R2) and A.seq_measurement_variance_info(0) == vcounts, f
        _same_results(ra, B.add_frames([left], [want[0]])[0], f)
    assert chain.fused > 0
    A.close(); B.close()


# ---- 7. off is off ---------------------------------------------------------------------------------------------------------------------------
def _run_stereo(ctx, seq, sp, n=None):
    return [ctx.add_frames_stereo([l], [r], sp)[0] for l, r in seq["frames"][:n]]


def test_off_is_a_context_that_never_heard_of_the_feature(hip):
    rows, cols, n_frames = 96, 128, 5
    seq = synth.make_stereo_sequence(rows, cols, n_frames, index=2)
    p = make_params(hip, descriptor="bitplanes", **VO_KW)
    mk = lambda: hip.create(seq["K"], seq["b"], rows, cols, p, n_frames=3, n_pairs=1)
    live0 = hip.debug_live_resources()
    never = mk()
    sp = never.default_stereo_params(ndisp=32)
    want = _run_stereo(never, seq, sp)
    live_one = hip.debug_live_resources()
    off = mk()
    off.set_measurement_variance(dict(VARIANCE, mode=0))
    off.seq_set_measurement_variance(0, dict(mode=0))
    for ra, rb in zip(want, _run_stereo(off, seq, sp)):
        _same_results(ra, rb, "mode 0")
    live_two = hip.debug_live_resources()
    unfused = mk()
    unfused.set_measurement_variance(VARIANCE)      # on, but the sequence does not fuse: nothing to do
    for ra, rb in zip(want, _run_stereo(unfused, seq, sp)):
        _same_results(ra, rb, "fusion off")
    live_three = hip.debug_live_resources()
    per_ctx = tuple(b - a for a, b in zip(live0, live_one))
    assert tuple(b - a for a, b in zip(live_one, live_two)) == per_ctx and tuple(b - a for a, b in zip(live_two, live_three)) == per_ctx
    for ctx in (never, off, unfused):
        assert bits_equal(ctx.seq_trajectory(0), never.seq_trajectory(0))
        assert ctx.measurement_variance_counts() == (0, 0, (0, 0, 0)) and ctx.disparity_fusion_counts() == (0, 0)
        with pytest.raises(capi.BpvoError):
            ctx.seq_get_measurement_variance_map(0)
    # with fusion on: a context never told of the variance and one told mode 0 carry the same maps
    fa, fb = mk(), mk()
    for ctx in (fa, fb):
        ctx.set_disparity_fusion(FUSION)
    fb.set_measurement_variance(dict(VARIANCE, mode=0))
    for ra, rb in zip(_run_stereo(fa, seq, sp), _run_stereo(fb, seq, sp)):
        _same_results(ra, rb, "fusion on, variance mode 0")
    (Da, Va), (Db, Vb) = fa.seq_get_fused_disparity(0), fb.seq_get_fused_disparity(0)
    assert ref.same_bits(Da, Db) and ref.same_bits(Va, Vb) and fb.measurement_variance_counts()[0] == 0
    for ctx in (never, off, unfused, fa, fb):
        ctx.close()
    assert hip.debug_live_resources() == live0


def test_a_mixed_call_equals_each_sequences_own_context(hip):
    rows, cols, n_frames = 96, 128, 4
    seqs = [synth.make_stereo_sequence(rows, cols, n_frames, index=3 + i) for i in range(3)]
    p = make_params(hip, descriptor="bitplanes", **VO_KW)
    K, b = seqs[0]["K"], seqs[0]["b"]
    mixed = hip.create(K, b, rows, cols, p, n_frames=9, n_pairs=3)
    sp = mixed.default_stereo_params(ndisp=32)

    def configure(ctx, s, role):
        if role != "unfused":
            ctx.seq_set_disparity_fusion(s, FUSION)
        if role != "constant":
            ctx.seq_set_measurement_variance(s, VARIANCE)

    roles = ("variance", "constant", "unfused")
    for s, role in enumerate(roles):
        configure(mixed, s, role)
    singles = []
    for s, role in enumerate(roles):
        one = hip.create(K, b, rows, cols, p, n_frames=3, n_pairs=1)
        configure(one, 0, role)
        singles.append(one)
    for f in range(n_frames):
        res = mixed.add_frames_stereo([q["frames"][f][0] for q in seqs], [q["frames"][f][1] for q in seqs], sp)
        for s, one in enumerate(singles):
            _same_results(res[s], one.add_frames_stereo([seqs[s]["frames"][f][0]], [seqs[s]["frames"][f][1]], sp)[0], (f, s))
    for s, (role, one) in enumerate(zip(roles, singles)):
        assert bits_equal(mixed.seq_trajectory(s), one.seq_trajectory(0)), role
        if role != "unfused":
            (Da, Va), (Db, Vb) = mixed.seq_get_fused_disparity(s), one.seq_get_fused_disparity(0)
            assert ref.same_bits(Da, Db) and ref.same_bits(Va, Vb), role
        if role == "variance":
            assert ref.same_bits(mixed.seq_get_measurement_variance_map(s), one.seq_get_measurement_variance_map(0))
            assert mixed.seq_measurement_variance_info(s) == one.seq_measurement_variance_info(0)
        else:
            with pytest.raises(capi.BpvoError):
                mixed.seq_measurement_variance_info(s)
    assert mixed.measurement_variance_counts()[:2] == (n_frames, n_frames * rows * cols)      # one job per call: sequence 0's
    (_, Vv), (_, Vc) = mixed.seq_get_fused_disparity(0), singles[1].seq_get_fused_disparity(0)
    assert np.any(Vv != FPRM["r2"]) and Vv.shape == Vc.shape
    mixed.close()
    for one in singles:
        one.close()


# ---- 8. refusals -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bad", [dict(radius=0), dict(radius=8), dict(noise_sigma=0.0), dict(noise_sigma=np.nan), dict(min_sigma=0.0),
                                 dict(min_sigma=3.0), dict(max_sigma=np.inf), dict(mode=2)])
def test_invalid_settings_are_refused_and_nothing_changes(hip, bad):
    cam = fref.camera(9, 11)
    ctx = hip.create_sequences([(_K(cam), 0.1, 9, 11)] * 2, make_params(hip, levels=1))
    ctx.seq_set_measurement_variance(1, VARIANCE)
    before = ctx.get_measurement_variance(), ctx.seq_get_measurement_variance(0), ctx.seq_get_measurement_variance(1)
    for call in (lambda: ctx.set_measurement_variance(dict(VARIANCE, **bad)), lambda: ctx.seq_set_measurement_variance(1, dict(VARIANCE, **bad))):
        with pytest.raises(capi.BpvoError, match="status -1:"):      # BPVO_ERR_INVALID_ARG
            call()
    assert (ctx.get_measurement_variance(), ctx.seq_get_measurement_variance(0), ctx.seq_get_measurement_variance(1)) == before
    assert before[0]["mode"] == 0 and before[1] == (before[0], False) and before[2][1] and before[2][0]["mode"] == 1
    ctx.seq_set_measurement_variance(1, None)
    assert ctx.seq_get_measurement_variance(1) == (before[0], False)
    ctx.close()


# ---- 9. the C++ facade -----------------------------------------------------------------------------------------------------------------------
def test_set_measurement_variance_through_the_facade(hip, tmp_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, "bpvo_amd", "csrc")
    exe = str(tmp_path / "disparity_variance_facade")
    r = subprocess.run(["g++", "-std=c++11", "-O2", "-I", os.path.join(root, "include"), os.path.join(root, "tests", "cpp", "disparity_variance_facade.cc"),
                        "-o", exe, "-L", csrc, "-lbpvo_hip", f"-Wl,-rpath,{csrc}"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    rows, cols, n_frames = 96, 128, 3
    seq = synth.make_stereo_sequence(rows, cols, n_frames, index=0)
    for k, (left, right) in enumerate(seq["frames"]):
        left.tofile(tmp_path / f"left_{k}.u8")
        right.tofile(tmp_path / f"right_{k}.u8")
    K = seq["K"]
    r = subprocess.run([exe, str(tmp_path), str(rows), str(cols), repr(float(K[0, 0])), repr(float(K[1, 1])), repr(float(K[0, 2])), repr(float(K[1, 2])),
                        repr(float(seq["b"])), str(n_frames), "32", "0.5", "0.1", "3.0", "2.0", "2", "2.0", "0.02", "2.0"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    poses = np.fromfile(tmp_path / "poses.bin", F32).reshape(n_frames, 4, 4)
    poses_seq = np.fromfile(tmp_path / "poses_seq.bin", F32).reshape(n_frames, 2, 4, 4)
    lines = [[int(v) for v in line.split()] for line in r.stdout.strip().splitlines()]
    # the same through the ctypes binding, with the facade's parameters (the defaults but three levels, bit-planes, Huber)
    p = make_params(hip, descriptor="bitplanes", loss="huber", levels=3)
    one = hip.create(K, seq["b"], rows, cols, p, n_frames=3, n_pairs=1)
    one.set_disparity_fusion(FUSION)
    one.set_measurement_variance(VARIANCE)
    two = hip.create(K, seq["b"], rows, cols, p, n_frames=6, n_pairs=2)
    two.set_disparity_fusion(FUSION)
    two.seq_set_measurement_variance(1, VARIANCE)
    sp = one.default_stereo_params(ndisp=32)
    for k, (left, right) in enumerate(seq["frames"]):
        assert bits_equal(one.add_frame_stereo(left, right, sp)["pose"], poses[k]), k
        info = one.vo_measurement_variance_info()
        assert lines[k] == [info[c] for c in ref.CLASSES], k
        res = two.add_frames_stereo([left, left], [right, right], sp)
        assert bits_equal(res[0]["pose"], poses_seq[k, 0]) and bits_equal(res[1]["pose"], poses_seq[k, 1]), k
    for var, fused, name in ((one.vo_get_measurement_variance(), one.vo_get_fused_disparity(), "var.bin"),
                             (two.seq_get_measurement_variance_map(1), two.seq_get_fused_disparity(1), "var_seq1.bin")):
        got = np.fromfile(tmp_path / name, F32).reshape(3, rows, cols)
        assert ref.same_bits(got[0], var) and ref.same_bits(got[1], fused[0]) and ref.same_bits(got[2], fused[1]), name
    one.close(); two.close()
