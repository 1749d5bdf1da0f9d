"""GPU parity tests: the HIP path (through the C ABI) against the CPU oracle on the same seeded inputs.

Bars (BASELINE.json north_star): bit-exact for integer / byte / index work (pyramid, census, selection, valid masks)
and for every float stage whose operation order is pinned on both sides (descriptor, saliency, points,
normalisation, pixels, Jacobians, residuals, sigma, weights); tolerance only where the summation order differs by
design (H, G, f_norm: deterministic tree on the GPU vs serial loop in the reference) and for the final
pose (1e-4 rad / 1e-3 m).
"""
import numpy as np
import pytest

from bpvo_amd import capi, synth
from util import ROT_TOL, assert_trace_reproduced, both, bits_equal, make_params, normal_equations_f64, perturbed_pose as _perturbed_pose, pose_error, setup_pair, trans_tol, set_options

pytestmark = pytest.mark.gpu

SIZES = [
    pytest.param(120, 160, 3, id="160x120-L3"),
    pytest.param(376, 1241, 4, id="kitti-1241x376-L4"),
    pytest.param(480, 640, 4, id="640x480-L4"),
]


@pytest.mark.parametrize("rows,cols,levels", SIZES)
@pytest.mark.parametrize("descriptor", ["intensity", "bitplanes"])
def test_pyramid_and_descriptor_bit_exact(hip, orc, rows, cols, levels, descriptor):
    ch, co, _ = both(hip, orc, rows, cols, levels, descriptor=descriptor)
    for l in range(levels):
        assert np.array_equal(ch.get_image(0, l), co.get_image(0, l)), f"pyrDown level {l}"
        for c in range(ch.Cn):
            a, b = ch.get_descriptor_channel(1, l, c), co.get_descriptor_channel(1, l, c)
            assert bits_equal(a, b), f"descriptor level {l} channel {c}: max |d| = {np.abs(a - b).max()}"


@pytest.mark.parametrize("rows,cols,levels", SIZES)
@pytest.mark.parametrize("descriptor", ["intensity", "bitplanes"])
def test_template_bit_exact(hip, orc, rows, cols, levels, descriptor):
    ch, co, _ = both(hip, orc, rows, cols, levels, descriptor=descriptor)
    for l in range(levels):
        assert bits_equal(ch.get_saliency(0, l), co.get_saliency(0, l)), f"saliency level {l}"
        assert ch.num_points(0, l) == co.num_points(0, l), f"N level {l}"
        assert ch.num_points(0, l) % 16 == 0
        assert np.array_equal(ch.get_point_indices(0, l), co.get_point_indices(0, l)), f"selected pixels level {l}"
        assert bits_equal(ch.get_points(0, l), co.get_points(0, l)), f"points level {l}"
        Th, Tih = ch.get_normalization(0, l)
        To, Tio = co.get_normalization(0, l)
        assert bits_equal(Th, To) and bits_equal(Tih, Tio), f"normalisation level {l}"
        assert bits_equal(ch.get_pixels(0, l), co.get_pixels(0, l)), f"pixels level {l}"
        Jh, Jo = ch.get_jacobians(0, l), co.get_jacobians(0, l)
        assert bits_equal(Jh, Jo), f"jacobians level {l}: max |d| = {np.abs(Jh - Jo).max()}"


@pytest.mark.parametrize("rows,cols,levels", SIZES)
@pytest.mark.parametrize("descriptor,loss", [("intensity", "huber"), ("bitplanes", "tukey"), ("intensity", "l2")])
def test_linearize_parity(hip, orc, rows, cols, levels, descriptor, loss):
    ch, co, _ = both(hip, orc, rows, cols, levels, descriptor=descriptor, loss=loss)
    for l in range(levels):
        for T in (np.eye(4, dtype=np.float32), _perturbed_pose(1.0), _perturbed_pose(8.0)):
            a = ch.linearize(0, 0, 1, l, T)
            b = co.linearize(0, 0, 1, l, T)
            vh, vo = ch.get_valid(0), co.get_valid(0)
            assert np.array_equal(vh, vo), f"valid mask level {l}"                      # bit-exact masks
            assert a["num_valid"] == b["num_valid"] == int(vo.sum())
            assert bits_equal(ch.get_residuals(0), co.get_residuals(0)), f"residuals level {l}"
            assert a["sigma"] == b["sigma"], f"sigma level {l}: {a['sigma']} vs {b['sigma']}"   # exact median
            assert bits_equal(ch.get_weights(0), co.get_weights(0)), f"weights level {l}"
            # H, G, f_norm: the reference sums serially in f32 (rounding error grows with N*C), the GPU sums a tree and
            # combines block partials in f64.  Both are checked against an f64 evaluation of the same (bit-identical)
            # J, r, w, valid arrays: the GPU tightly, the oracle within its own serial-summation error.
            H64, G64, f64 = normal_equations_f64(co.get_jacobians(0, l), co.get_residuals(0), co.get_weights(0), vo, ch.Cn)
            scale = np.abs(H64).max()
            gscale = max(np.abs(G64).max(), 1e-3 * scale)
            assert np.abs(a["H"] - H64).max() <= 4e-6 * scale, f"H level {l} (hip vs f64)"
            assert np.abs(a["G"] - G64).max() <= 4e-6 * gscale, f"G level {l} (hip vs f64)"
            assert abs(a["f_norm"] - f64) <= 4e-6 * max(f64, 1e-6)
            assert np.abs(b["H"] - H64).max() <= 2e-4 * scale and np.abs(b["G"] - G64).max() <= 2e-4 * gscale
            assert np.allclose(a["H"], a["H"].T)
            assert abs(ch.fraction_good(0, 0.85) - co.fraction_good(0, 0.85)) < 1e-6


@pytest.mark.parametrize("rows,cols,levels", SIZES)
@pytest.mark.parametrize("descriptor,loss", [("intensity", "huber"), ("bitplanes", "tukey")])
def test_scale_freeze_sequence(hip, orc, rows, cols, levels, descriptor, loss):
    """AutoScaleEstimator keeps state across linearisations of a level (Q6): same sequence, same sigmas."""
    ch, co, _ = both(hip, orc, rows, cols, levels, descriptor=descriptor, loss=loss)
    l = levels - 1
    poses = [np.eye(4, dtype=np.float32), _perturbed_pose(1.0), _perturbed_pose(1.0), _perturbed_pose(1.0), _perturbed_pose(2.0)]
    for k, T in enumerate(poses):
        a = ch.linearize(0, 0, 1, l, T, reset_scale=(k == 0))
        b = co.linearize(0, 0, 1, l, T, reset_scale=(k == 0))
        assert a["sigma"] == b["sigma"], (k, a["sigma"], b["sigma"])


@pytest.mark.parametrize("rows,cols,levels", SIZES)
@pytest.mark.parametrize("descriptor,loss", [("intensity", "huber"), ("bitplanes", "tukey"), ("intensity", "l2")])
def test_estimate_pose_parity(hip, orc, rows, cols, levels, descriptor, loss):
    """Configs 2-4 of BASELINE.json: final SE(3) pose within 1e-4 rad / 1e-3 m of the CPU path, and the per-iteration
    trace of the oracle reproduced when the HIP path is linearised at the oracle's poses."""
    ch, co, d = both(hip, orc, rows, cols, levels, descriptor=descriptor, loss=loss)
    Th, sh = ch.estimate_pose(0, 0, 1)
    To, so, trace = co.estimate_pose_trace(0, 0, 1)
    rot, trans = pose_error(Th, To)
    assert rot <= ROT_TOL and trans <= trans_tol(d["K"]), (rot, trans, sh, so)
    # against ground truth both must be reasonable (sanity of the synthetic scene, not a parity bar)
    rg, tg = pose_error(Th, d["T_gt"])
    assert rg < 1e-2 and tg < 1e-1, (rg, tg)
    assert_trace_reproduced(ch, trace)


def test_estimate_pose_nonzero_workspace_and_init(hip, orc):
    rows, cols, levels = 120, 160, 3
    d = synth.make_pair(rows, cols, 3)
    outs = []
    for b in (hip, orc):
        p = make_params(b, descriptor="bitplanes", loss="tukey", levels=levels)
        ctx = b.create(d["K"], d["b"], rows, cols, p, n_frames=4, n_pairs=3)
        ctx.frame_set_data(2, d["imgA"], d["dispA"])
        ctx.frame_set_template(2)
        ctx.frame_set_data(3, d["imgB"], d["dispB"])
        T0 = synth.twist_to_matrix([0.001, 0.0, -0.001, 0.005, 0.0, 0.002]).astype(np.float32)
        outs.append(ctx.estimate_pose(2, 2, 3, T0))
        assert ctx.frame_state(2) == (True, True) and ctx.frame_state(3) == (True, False) and ctx.frame_state(0) == (False, False)
    (Th, sh), (To, so) = outs
    rot, trans = pose_error(Th, To)
    assert rot <= ROT_TOL and trans <= trans_tol(d["K"]), (rot, trans)


def test_fixed_iteration_mode_counts(hip, orc):
    """Throughput mode: tolerances 0, maxIterations = K -> exactly K+2 linearisations per level."""
    rows, cols, levels, K = 120, 160, 3, 5
    kw = dict(descriptor="bitplanes", loss="tukey", levels=levels, maxIterations=K, parameterTolerance=0.0,
              functionTolerance=0.0, gradientTolerance=0.0)
    ch, co, _ = both(hip, orc, rows, cols, levels, **{k: v for k, v in kw.items() if k != "levels"})
    Th, sh = ch.estimate_pose(0, 0, 1)
    To, so = co.estimate_pose(0, 0, 1)
    assert [s["numIterations"] for s in sh] == [s["numIterations"] for s in so] == [K] * levels
    assert all(s["status"] == capi.STATUS_MAX_ITERATIONS for s in sh)
    assert ch.total_linearizations() == levels * (K + 2)
    rot, trans = pose_error(Th, To)
    assert rot <= ROT_TOL and trans <= trans_tol(synth.calibration(rows, cols)[0])


@pytest.mark.parametrize("formulation", [pytest.param(0, id="rigid-body-warp"), pytest.param(2, id="disparity-space-warp")])
def test_visual_odometry_add_frame_sequence(hip, orc, formulation):
    """VisualOdometry::addFrame state machine (bpvo/vo.cc:125-224) on a short synthetic trajectory; also with
    DisparitySpaceWarp as the warp (its getImagePoint colours the point cloud, bpvo/disparity_space_warp.h:73-76)."""
    rows, cols, levels = 120, 160, 3
    seq = synth.make_sequence(rows, cols, 7, index=5, step_rot=0.01, step_trans=0.06)
    res = []
    for b in (hip, orc):
        p = make_params(b, descriptor="intensity", loss="huber", levels=levels, minTranslationMagToKeyFrame=0.1,
                        minRotationMagToKeyFrame=2.5, maxFractionOfGoodPointsToKeyFrame=0.7, goodPointThreshold=0.8)
        ctx = b.create(seq["K"], seq["b"], rows, cols, p, n_frames=3, n_pairs=1)
        if formulation:
            ctx.set_warp_formulation(formulation)
        out, clouds = [], []
        for img, disp in seq["frames"]:
            out.append(ctx.add_frame(img, disp))
            if out[-1]["hasPointCloud"]:          # a Result owns its point cloud (bpvo/types.h:549-563): fetch it now
                clouds.append(ctx.get_point_cloud())
        res.append((out, ctx.trajectory(), ctx.vo_num_points_at_level(), ctx.get_point_cloud(), clouds))
        assert ctx.add_frame_null() != 0        # THROW_ERROR_IF(nullptr) -> error status
    (oh, trh, nh, (pch, pph), clh), (oo, tro, no_, (pco, ppo), clo) = res
    assert len(clh) == len(clo) and len(clh) >= 1
    for (ph, Ph), (po, Po) in zip(clh, clo):
        assert len(ph) == len(po) and len(ph) > 0
        assert np.array_equal(ph["xyzw"], po["xyzw"]) and np.array_equal(ph["rgba"], po["rgba"])
        assert len(np.unique(ph["rgba"][:, 0])) > 8               # colours were looked up, not defaulted
        assert np.abs(ph["weight"] - po["weight"]).max() < 1e-3
        assert np.abs(Ph - Po).max() < 5e-3
    assert nh == no_
    assert [r["keyFramingReason"] for r in oh] == [r["keyFramingReason"] for r in oo]
    assert [r["isKeyFrame"] for r in oh] == [r["isKeyFrame"] for r in oo]
    assert oh[0]["keyFramingReason"] == capi.KF_FIRST_FRAME
    assert any(r["isKeyFrame"] for r in oh[1:]), "sequence should trigger key-framing"
    for a, b in zip(oh, oo):
        rot, trans = pose_error(a["pose"], b["pose"])
        assert rot <= ROT_TOL and trans <= trans_tol(seq["K"])
        assert np.array_equal(a["covariance"], np.eye(6, dtype=np.float32))            # Q16
    assert trh.shape == tro.shape
    assert np.abs(trh - tro).max() < 5e-3
    assert pch.shape == pco.shape
    if len(pch):
        assert np.array_equal(pch["xyzw"], pco["xyzw"]) and np.array_equal(pch["rgba"], pco["rgba"])
        assert np.abs(pch["weight"] - pco["weight"]).max() < 1e-3


def test_edge_cases(hip, orc):
    rows, cols, levels = 120, 160, 3
    d = synth.make_pair(rows, cols, 1)
    for b in (hip, orc):
        p = make_params(b, levels=levels)
        ctx = b.create(d["K"], d["b"], rows, cols, p, n_frames=2, n_pairs=1)
        with pytest.raises(capi.BpvoError):
            ctx.frame_set_template(0)                       # "no data in frame" (bpvo/vo_frame.cc:63)
        ctx.frame_set_data(0, d["imgA"], np.zeros_like(d["dispA"]))   # all disparities invalid -> no points
        ctx.frame_set_template(0)
        assert all(ctx.num_points(0, l) == 0 for l in range(levels))
        ctx.frame_set_data(1, d["imgB"], d["dispB"])
        with pytest.raises(capi.BpvoError):
            ctx.linearize(0, 0, 1, 0, np.eye(4, dtype=np.float32))    # computeResiduals on an empty template throws
        with pytest.raises(capi.BpvoError):
            ctx.get_image(5, 0)
        ctx.frame_clear(0)
        assert ctx.frame_state(0) == (False, False)
    # ragged selection: disparity valid only on a band -> N truncated to a multiple of 16, same on both sides
    disp = d["dispA"].copy()
    disp[:, : cols // 3] = 0.0
    disp[::7, :] = 600.0     # above maxValidDisparity
    ns = []
    for b in (hip, orc):
        p = make_params(b, levels=levels)
        ctx = b.create(d["K"], d["b"], rows, cols, p, n_frames=2, n_pairs=1)
        ctx.frame_set_data(0, d["imgA"], disp)
        ctx.frame_set_template(0)
        ns.append([ctx.num_points(0, l) for l in range(levels)])
        ns.append([ctx.get_point_indices(0, l).tobytes() for l in range(levels)])
    assert ns[0] == ns[2] and ns[1] == ns[3]
    assert all(n % 16 == 0 for n in ns[0])
    # a pose that throws every point out of the image: all invalid, residuals 0, sigma -> 1
    T = np.eye(4, dtype=np.float32)
    T[0, 3] = 1e4
    ch, co, _ = both(hip, orc, rows, cols, levels)
    a, b = ch.linearize(0, 0, 1, 0, T), co.linearize(0, 0, 1, 0, T)
    assert a["num_valid"] == b["num_valid"] == 0 and a["sigma"] == b["sigma"] == 1.0 and a["f_norm"] == b["f_norm"] == 0.0


def test_unsupported_and_invalid_create(hip):
    K, b = synth.calibration(120, 160)
    p = make_params(hip, levels=3)
    p.interp = 7
    with pytest.raises(capi.BpvoError):
        hip.create(K, b, 120, 160, p)
    p = make_params(hip, levels=3)
    p.descriptor = 0x38      # past the last DescriptorType (bpvo/types.h:142-152): DenseDescriptor::Create throws
    with pytest.raises(capi.BpvoError):
        hip.create(K, b, 120, 160, p)
    for nbytes in (3, 128):    # kLatch: sizes LATCHDescriptorExtractorImpl rejects (bpvo/latch_descriptor.cc:104)
        p = make_params(hip, levels=3, descriptor="latch", latchNumBytes=nbytes)
        with pytest.raises(capi.BpvoError):
            hip.create(K, b, 120, 160, p)
    p = make_params(hip, levels=3)
    p.maxTestLevel = 7
    with pytest.raises(capi.BpvoError):
        hip.create(K, b, 120, 160, p)
    p = make_params(hip, levels=-1)
    ctx = hip.create(K, b, 480, 640, p)
    assert ctx.L == 1 + round(np.log2(480 / 40.0))      # auto pyramid levels (bpvo/vo.cc:101-105)


@pytest.mark.parametrize("descriptor,loss", [("bitplanes", "tukey"), ("intensity", "huber")])
def test_estimation_lanes_are_bit_identical(hip, descriptor, loss, monkeypatch):
    """Option "lanes" (bpvo_hip_set_option; here through BPVO_HIP_OPTIONS): a batch split over 2 or 3 estimation streams driven by host threads gives,
    pair for pair, the bits of the single-lane run — the lanes only change what overlaps in time."""
    import os
    rows, cols, levels, n = 120, 160, 3, 40
    batch = synth.make_batch(rows, cols, n, first_index=60, workers=1)
    out = {}
    for lanes in (1, 2, 3, "team"):
        # (a batch of this size would take the team-persistent kernel, which runs on one lane: switched off for the lane runs, and
        # run last as a fourth variant — same bits again)
        set_options(monkeypatch, team="1" if lanes == "team" else "0")
        set_options(monkeypatch, lanes="2" if lanes == "team" else str(lanes))
        ctx = hip.create(batch["K"], batch["b"], rows, cols, make_params(hip, descriptor=descriptor, loss=loss, levels=levels),
                         n_frames=2 * n, n_pairs=n)
        out[lanes] = ctx.batch_run(batch["images"], batch["disparities"])
        assert ctx.team_counts() == (1 if lanes == "team" else 0)
        ctx.close()
    for lanes in (2, 3, "team"):
        assert bits_equal(out[lanes][0], out[1][0]), lanes
        assert np.array_equal(out[lanes][1]["numIterations"], out[1][1]["numIterations"])
        assert np.array_equal(out[lanes][1]["status"], out[1][1]["status"])


def test_wide_launches_take_the_second_median_shape_and_change_nothing(hip):
    """Launches of more than 256 workspaces run median_finish in its 512-thread / 53 KB shape (three workgroups per CU), smaller ones
    in the 1024-thread shape (kernels_gn.hip): the selection is exact in either, so a 288-pair batch on ONE lane (one launch covers
    all 288) equals, pair for pair, the same pairs run as batches of 48."""
    rows, cols, levels, n, sub = 96, 128, 2, 288, 48
    batch = synth.make_batch(rows, cols, n, first_index=300, workers=8)
    p = make_params(hip, descriptor="bitplanes", loss="tukey", levels=levels)
    ctx = hip.create(batch["K"], batch["b"], rows, cols, p, n_frames=2 * n, n_pairs=n)
    ctx.set_max_lanes(1)
    poses, stats = ctx.batch_run(batch["images"], batch["disparities"])
    ctx.close()
    small = hip.create(batch["K"], batch["b"], rows, cols, p, n_frames=2 * sub, n_pairs=sub)
    small.set_max_lanes(1)
    for k in range(0, n, sub):
        ps, ss = small.batch_run(batch["images"][2 * k: 2 * (k + sub)], batch["disparities"][2 * k: 2 * (k + sub)])
        assert bits_equal(ps, poses[k: k + sub]), k
        assert np.array_equal(ss["numIterations"], stats["numIterations"][k: k + sub])
        assert np.array_equal(ss["status"], stats["status"][k: k + sub])
    small.close()


@pytest.mark.parametrize("descriptor,loss", [("bitplanes", "tukey"), ("intensity", "huber")])
def test_dense_levels_without_tap_cache_leave_no_stale_entries(hip, monkeypatch, descriptor, loss):
    """Batches run their dense pyramid levels without the per-point tap cache (PairJob::tapcache_on).  Calls that do use it afterwards
    on the same workspace — the on-demand refresh behind get_residuals / get_weights — must not find entries an EARLIER cached run left
    there: the keys are reset at the start of every level whether the cache is used or not.  160 x 120: no level reaches
    minNumPixelsForNonMaximaSuppression, every level is dense."""
    rows, cols, levels, n = 120, 160, 3, 3
    b1 = synth.make_batch(rows, cols, n, first_index=40)
    b2 = synth.make_batch(rows, cols, n, first_index=50)
    p = make_params(hip, descriptor=descriptor, loss=loss, levels=levels)
    ctx = hip.create(b1["K"], b1["b"], rows, cols, p, n_frames=2 * n, n_pairs=n)
    # a cached single-pair estimate on OTHER images fills the tap cache of workspace 2 (same geometry: the same footprints recur)
    ctx.frames_set_data(0, 1, b2["images"], b2["disparities"])
    ctx.frame_set_template(4)
    ctx.estimate_pose(2, 4, 5)
    poses, stats = ctx.batch_run(b1["images"], b1["disparities"])
    r, w, v = ctx.get_residuals(2), ctx.get_weights(2), ctx.get_valid(2)
    ctx.close()
    set_options(monkeypatch, tapcache_max_density="2.0")        # the cache at every level, as before
    ref = hip.create(b1["K"], b1["b"], rows, cols, p, n_frames=2 * n, n_pairs=n)
    poses_ref, stats_ref = ref.batch_run(b1["images"], b1["disparities"])
    assert bits_equal(poses, poses_ref) and stats.tobytes() == stats_ref.tobytes()
    assert np.array_equal(v, ref.get_valid(2)) and bits_equal(r, ref.get_residuals(2)) and bits_equal(w, ref.get_weights(2))
    ref.close()


@pytest.mark.parametrize("interp", ["cosine", "cubic", "cubic_hermite"])
@pytest.mark.parametrize("descriptor,loss,rows,cols,levels", [("bitplanes", "tukey", 376, 1241, 3), ("intensity", "huber", 240, 320, 3)])
def test_tap_cache_of_the_other_interpolations_changes_nothing(hip, orc, monkeypatch, interp, descriptor, loss, rows, cols, levels):
    """kCosine / kCubic / kCubicHermite (bpvo/photo_error.cc:391-444) keep a point's 2 x 2 / 4 x 4 footprint in the per-point tap cache (C = 8 and 1):
    a batch with the cache at every level, a batch with the cache at no level (every tap gathered from the descriptor at every iteration) and the
    same pairs one at a time give the same poses and statistics bit for bit — and the oracle's within the bar.  NMS on at the finest level
    (1241 x 376: sparse points, where the cache hits) and off at the coarser ones."""
    n = 3
    b = synth.make_batch(rows, cols, n, first_index=70)
    kw = dict(descriptor=descriptor, loss=loss, levels=levels, interp={"cosine": 1, "cubic": 2, "cubic_hermite": 3}[interp])
    outs = []
    for density in ("1e9", "0"):      # tapcache_max_density: levels denser than this gather straight from the descriptor
        set_options(monkeypatch, tapcache_max_density=density, lanes="1")
        ctx = hip.create(b["K"], b["b"], rows, cols, make_params(hip, **kw), n_frames=2 * n, n_pairs=n)
        outs.append(ctx.batch_run(b["images"], b["disparities"]))
        if density == "1e9":
            hits, lookups, _, _ = ctx.tap_cache_counts()
            assert lookups > 0 and hits > 0.5 * lookups, (hits, lookups)      # the cache is in use, and most lookups of a run hit
        ctx.close()
    assert bits_equal(outs[0][0], outs[1][0]) and outs[0][1].tobytes() == outs[1][1].tobytes()
    monkeypatch.delenv("BPVO_HIP_OPTIONS", raising=False)
    for k in range(n):
        one = hip.create(b["K"], b["b"], rows, cols, make_params(hip, **kw), n_frames=2, n_pairs=1)
        one.frame_set_data(0, b["images"][2 * k], b["disparities"][2 * k]); one.frame_set_template(0)
        one.frame_set_data(1, b["images"][2 * k + 1], b["disparities"][2 * k + 1])
        T, st = one.estimate_pose(0, 0, 1)
        assert bits_equal(T, outs[0][0][k]) and [s_["numIterations"] for s_ in st] == [int(v) for v in outs[0][1]["numIterations"][k]], k
        one.close()
    co = orc.create(b["K"], b["b"], rows, cols, make_params(orc, **kw), n_frames=2, n_pairs=1)
    co.frame_set_data(0, b["images"][0], b["disparities"][0]); co.frame_set_template(0)
    co.frame_set_data(1, b["images"][1], b["disparities"][1])
    To, _ = co.estimate_pose(0, 0, 1)
    rot, trans = pose_error(outs[0][0][0], To)
    assert rot <= ROT_TOL and trans <= trans_tol(b["K"]), (rot, trans)


@pytest.mark.parametrize("case", ["kitti-bitplanes", "vga-dense-intensity-hermite", "vga-dense-bitplanes"])
def test_dense_candidate_run_of_the_median_changes_nothing(hip, orc, monkeypatch, case):
    """The exact median's candidates (keys inside the bracket around the previous median: bpvo/mestimator.cc:452-490, utils.h:224-252) as ONE
    contiguous run per workspace with four totals (option dense_candidates_from; the chunks' leaders take their place with a returning add, so
    the run's order differs from launch to launch) against one segment and one counter record per 256-point chunk: the same poses, statistics
    and per-linearisation records (pose, H, G, f, sigma, valid count, step) bit for bit, for a batch on the chain and for a single pair, with
    the bracketed selection in use — and the oracle's trajectory bit for bit in reference order.  Dense templates (NMS off, conf/tsukuba.cfg)
    are what the run is for: a 640 x 480 level has 1172 chunks."""
    kw, rows, cols, n = {"kitti-bitplanes": (dict(descriptor="bitplanes", loss="tukey", levels=3), 376, 1241, 3),
                         "vga-dense-intensity-hermite": (dict(descriptor="intensity", loss="huber", levels=3, interp=3, nonMaxSuppRadius=0, minSaliency=0.001), 480, 640, 2),
                         "vga-dense-bitplanes": (dict(descriptor="bitplanes", loss="tukey", levels=2, nonMaxSuppRadius=0), 480, 640, 2)}[case]
    b = synth.make_batch(rows, cols, n, first_index=90)
    outs, traces = [], []
    for dense_from in ("0", "1073741824"):
        set_options(monkeypatch, dense_candidates_from=dense_from, lanes="1", team="0", persistent="0")      # the four-kernel chain
        ctx = hip.create(b["K"], b["b"], rows, cols, make_params(hip, **kw), n_frames=2 * n, n_pairs=n)
        outs.append(ctx.batch_run(b["images"], b["disparities"]))
        bracketed, full = ctx.median_path_counts()
        assert bracketed > full > 0, (bracketed, full)
        ctx.close()
        one = hip.create(b["K"], b["b"], rows, cols, make_params(hip, **kw), n_frames=2, n_pairs=1)
        one.frame_set_data(0, b["images"][0], b["disparities"][0]); one.frame_set_template(0)
        one.frame_set_data(1, b["images"][1], b["disparities"][1])
        traces.append(one.estimate_pose_trace(0, 0, 1, max_records=4096))
        one.close()
    assert bits_equal(outs[0][0], outs[1][0]) and outs[0][1].tobytes() == outs[1][1].tobytes()
    assert bits_equal(traces[0][0], traces[1][0]) and bits_equal(traces[0][2], traces[1][2])
    assert bits_equal(traces[0][0], outs[0][0][0])
    # reference order, dense run: the oracle's records
    set_options(monkeypatch, dense_candidates_from="0", persistent="0")
    ref = hip.create(b["K"], b["b"], rows, cols, make_params(hip, **kw), n_frames=2, n_pairs=1)
    ref.set_option("reference_reduction", 1)
    co = orc.create(b["K"], b["b"], rows, cols, make_params(orc, **kw), n_frames=2, n_pairs=1)
    for c in (ref, co):
        c.frame_set_data(0, b["images"][0], b["disparities"][0]); c.frame_set_template(0)
        c.frame_set_data(1, b["images"][1], b["disparities"][1])
    Th, sh, th = ref.estimate_pose_trace(0, 0, 1, max_records=4096)
    To, so, to = co.estimate_pose_trace(0, 0, 1, max_records=4096)
    assert bits_equal(Th, To) and bits_equal(th, to) and [s_["numIterations"] for s_ in sh] == [s_["numIterations"] for s_ in so]
    ref.close(); co.close()


def test_batch_matches_single_and_records(hip, orc):
    """Config 5 shape: a batch of independent pairs equals the pairs run one by one, and equals the oracle."""
    rows, cols, levels, n = 120, 160, 3, 6
    batch = synth.make_batch(rows, cols, n, first_index=10)
    p = make_params(hip, descriptor="bitplanes", loss="tukey", levels=levels)
    ctx = hip.create(batch["K"], batch["b"], rows, cols, p, n_frames=2 * n, n_pairs=n)
    poses, stats = ctx.batch_run(batch["images"], batch["disparities"])
    # one by one on a second context
    ctx1 = hip.create(batch["K"], batch["b"], rows, cols, p, n_frames=2, n_pairs=1)
    po = make_params(orc, descriptor="bitplanes", loss="tukey", levels=levels)
    cto = orc.create(batch["K"], batch["b"], rows, cols, po, n_frames=2, n_pairs=1)
    for i in range(n):
        for c in (ctx1, cto):
            c.frame_set_data(0, batch["images"][2 * i], batch["disparities"][2 * i])
            c.frame_set_template(0)
            c.frame_set_data(1, batch["images"][2 * i + 1], batch["disparities"][2 * i + 1])
        T1, s1 = ctx1.estimate_pose(0, 0, 1)
        assert np.array_equal(T1, poses[i]), f"pair {i}: batched result differs from the single-pair run"
        assert [s["numIterations"] for s in s1] == list(stats[i]["numIterations"])
        To, _ = cto.estimate_pose(0, 0, 1)
        rot, trans = pose_error(poses[i], To)
        assert rot <= ROT_TOL and trans <= trans_tol(batch["K"]), (i, rot, trans)
    # packed records that the RCCL gather moves
    ptr, nf = ctx.batch_result_records_device()
    assert nf == 32 and ptr


def test_config1_vo_perf_plumbing_two_frames(hip, orc):
    """BASELINE.json configs[0]: 640x480, Intensity, 1 pyramid level, L2 loss, two addFrame calls (apps/vo_perf.cc loop)."""
    rows, cols = 480, 640
    d = synth.make_pair(rows, cols, 0)
    out = []
    for b in (hip, orc):
        p = make_params(b, descriptor="intensity", loss="l2", levels=1)
        ctx = b.create(d["K"], d["b"], rows, cols, p, n_frames=3, n_pairs=1)
        r0 = ctx.add_frame(d["imgA"], d["dispA"])
        r1 = ctx.add_frame(d["imgB"], d["dispB"])
        out.append((r0, r1, ctx.vo_num_points_at_level(0)))
    (h0, h1, nh), (o0, o1, no_) = out
    assert nh == no_ and nh > 0
    assert h0["keyFramingReason"] == o0["keyFramingReason"] == capi.KF_FIRST_FRAME
    assert h1["keyFramingReason"] == o1["keyFramingReason"]
    assert h1["stats"][0]["numIterations"] == o1["stats"][0]["numIterations"]
    rot, trans = pose_error(h1["pose"], o1["pose"])
    assert rot <= ROT_TOL and trans <= trans_tol(d["K"]), (rot, trans)


@pytest.mark.parametrize("descriptor", ["intensity", "bitplanes"])
def test_cd5_gradients_bit_exact(hip, orc, descriptor):
    """kCentralDifference_5 (bpvo/template_data.cc:123-130): Jacobians bit-exact, pose within the bar."""
    rows, cols, levels = 120, 160, 3
    ch, co, d = both(hip, orc, rows, cols, levels, descriptor=descriptor, gradientEstimation=capi.GRAD_CD5)
    for l in range(levels):
        assert bits_equal(ch.get_jacobians(0, l), co.get_jacobians(0, l)), f"CD5 jacobians level {l}"
    Th, _ = ch.estimate_pose(0, 0, 1)
    To, _ = co.estimate_pose(0, 0, 1)
    rot, trans = pose_error(Th, To)
    assert rot <= ROT_TOL and trans <= trans_tol(d["K"])


def test_no_nms_and_no_normalization_variants(hip, orc):
    rows, cols, levels = 120, 160, 2
    for kw in (dict(nonMaxSuppRadius=0), dict(withNormalization=0), dict(nonMaxSuppRadius=2, minNumPixelsForNonMaximaSuppression=100),
               dict(maxTestLevel=1), dict(minSaliency=0.6)):
        ch, co, d = both(hip, orc, rows, cols, levels, descriptor="bitplanes", **kw)
        first = kw.get("maxTestLevel", 0)
        for l in range(first, levels):
            assert np.array_equal(ch.get_point_indices(0, l), co.get_point_indices(0, l)), (kw, l)
            assert bits_equal(ch.get_jacobians(0, l), co.get_jacobians(0, l)), (kw, l)
        Th, sh = ch.estimate_pose(0, 0, 1)
        To, so = co.estimate_pose(0, 0, 1)
        rot, trans = pose_error(Th, To)
        assert rot <= ROT_TOL and trans <= trans_tol(d["K"]), (kw, rot, trans)
        assert [s["status"] for s in sh][:first] == [capi.STATUS_SOLVER_ERROR] * first      # untouched levels keep the default stats


def test_empty_template_errors_like_the_reference(hip, orc):
    """No pixel passes the saliency gate -> N = 0 -> computeResiduals throws (bpvo/template_data.cc:177)."""
    for b in (hip, orc):
        ctx, d, _ = setup_pair(b, 120, 160, levels=2, descriptor="bitplanes", minSaliency=50.0)
        assert ctx.num_points(0, 0) == 0 and ctx.num_points(0, 1) == 0
        with pytest.raises(capi.BpvoError):
            ctx.estimate_pose(0, 0, 1)
    # the batch entry point keeps going: the affected pair reports kSolverError and an unchanged pose
    batch = synth.make_batch(120, 160, 2, first_index=3)
    p = make_params(hip, levels=2, descriptor="bitplanes", minSaliency=50.0)
    ctx = hip.create(batch["K"], batch["b"], 120, 160, p, n_frames=4, n_pairs=2)
    poses, stats = ctx.batch_run(batch["images"], batch["disparities"])
    assert np.array_equal(poses[0], np.eye(4, dtype=np.float32)) and (stats["status"] == capi.STATUS_SOLVER_ERROR).all()


def test_full_size_batch_properties(hip):
    """Config 5 shape at full image size (a 24-pair shard of the 1024-pair KITTI batch): size-independent properties —
    determinism, independence of the pairs from batch composition / order, result records = poses, sane accuracy."""
    rows, cols, levels, n = 376, 1241, 4, 24
    batch = synth.make_batch(rows, cols, n, first_index=100, workers=8)
    p = make_params(hip, descriptor="bitplanes", loss="tukey", levels=levels)
    ctx = hip.create(batch["K"], batch["b"], rows, cols, p, n_frames=2 * n, n_pairs=n)
    poses, stats = ctx.batch_run(batch["images"], batch["disparities"])
    poses2, stats2 = ctx.batch_run(batch["images"], batch["disparities"])
    assert np.array_equal(poses, poses2) and np.array_equal(stats["numIterations"], stats2["numIterations"])   # deterministic
    # batch_run runs every estimation lane's pairs end to end on the lane's stream (staggered frame stages); the three stages called
    # one after the other over all pairs give the same results bit for bit
    ctx.frames_set_data(0, 1, batch["images"], batch["disparities"])
    ctx.frames_set_template(0, 2, n)
    poses3, stats3 = ctx.batch_estimate(n)
    assert np.array_equal(poses3, poses) and np.array_equal(stats3["numIterations"], stats["numIterations"])
    # reversed pair order in a second context: every pair's result is unchanged bit for bit
    perm = np.arange(n)[::-1]
    idx = np.stack([2 * perm, 2 * perm + 1], axis=1).reshape(-1)
    ctx_r = hip.create(batch["K"], batch["b"], rows, cols, p, n_frames=2 * n, n_pairs=n)
    poses_r, stats_r = ctx_r.batch_run(batch["images"][idx], batch["disparities"][idx])
    assert np.array_equal(poses_r[::-1], poses)
    assert np.array_equal(stats_r["numIterations"][::-1], stats["numIterations"])
    # a sub-batch gives the same results as the same pairs inside the big batch
    ctx_s = hip.create(batch["K"], batch["b"], rows, cols, p, n_frames=8, n_pairs=4)
    poses_s, _ = ctx_s.batch_run(batch["images"][:8], batch["disparities"][:8])
    assert np.array_equal(poses_s, poses[:4])
    # rigid transforms, bounded iterations, accuracy against the scene's ground truth
    R = poses[:, :3, :3].astype(np.float64)
    assert np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max() < 1e-4
    assert np.array_equal(poses[:, 3], np.tile(np.array([0, 0, 0, 1], np.float32), (n, 1)))
    assert stats["numIterations"].max() <= 50 and stats["numIterations"].min() >= 0
    dt = np.linalg.norm(poses[:, :3, 3] - batch["T_gt"][:, :3, 3], axis=1)
    assert np.median(dt) < 5e-3 and dt.max() < 5e-2, (np.median(dt), dt.max())
    # the packed records on the device are the poses
    import torch
    from bpvo_amd.distributed import records_to_poses
    rec = torch.zeros((n, 32), dtype=torch.float32, device="cuda:0")
    ctx.batch_copy_records_device(rec.data_ptr(), n)
    rp, it, _ = records_to_poses(rec)
    assert np.array_equal(rp[:, :3, :], poses[:, :3, :]) and np.array_equal(it[:, :levels], stats["numIterations"])
    # measurement counters: every valid template point of every linearisation looks up the tap cache once; the first linearisation
    # of a level starts with an empty cache, later ones mostly hit
    hits, lookups, hits8, lookups8 = ctx.tap_cache_counts()
    assert 0 < hits < lookups and 0 < hits8 < lookups8 < lookups and hits8 <= hits
    assert hits / lookups > 0.9 and hits8 / lookups8 < hits / lookups
    med = ctx.median_path_counts()
    assert med[1] >= 2 * n * levels and med[0] > med[1]           # >= one full selection per level, pair and run; the rest bracketed


@pytest.mark.parametrize("rows,cols,levels", [pytest.param(120, 160, 3, id="160x120-L3"), pytest.param(376, 1241, 4, id="kitti-1241x376-L4")])
@pytest.mark.parametrize("descriptor,loss", [("intensity", "huber"), ("bitplanes", "tukey")])
def test_project_points_f32_formulation_parity(hip, orc, rows, cols, levels, descriptor, loss):
    """The reference's inactive all-float warp (projectPoints + interpolation coefficients + dot product,
    bpvo/project_points.cc:180-214, bpvo/photo_error.cc:82-214) as an optional mode: bit-exact against its restatement."""
    ch, co, d = both(hip, orc, rows, cols, levels, descriptor=descriptor, loss=loss)
    ch.set_warp_formulation(1)
    co.set_warp_formulation(1)
    for l in range(levels):
        for T in (np.eye(4, dtype=np.float32), _perturbed_pose(1.0), _perturbed_pose(8.0)):
            a = ch.linearize(0, 0, 1, l, T)
            b = co.linearize(0, 0, 1, l, T)
            vo = co.get_valid(0)
            assert np.array_equal(ch.get_valid(0), vo)
            assert bits_equal(ch.get_residuals(0), co.get_residuals(0)), f"residuals level {l}"
            assert a["sigma"] == b["sigma"] and a["num_valid"] == b["num_valid"]
            assert bits_equal(ch.get_weights(0), co.get_weights(0))
            H64, G64, f64 = normal_equations_f64(co.get_jacobians(0, l), co.get_residuals(0), co.get_weights(0), vo, ch.Cn)
            assert np.abs(a["H"] - H64).max() <= 4e-6 * np.abs(H64).max()
    r = co.get_residuals(0).reshape(ch.Cn, -1)
    inv = co.get_valid(0) == 0
    if inv.any():   # invalid points carry r = -I0 in this formulation
        assert np.array_equal(r[:, inv], -co.get_pixels(0, levels - 1)[:, inv])
    Th, _ = ch.estimate_pose(0, 0, 1)
    To, _ = co.estimate_pose(0, 0, 1)
    rot, trans = pose_error(Th, To)
    assert rot <= ROT_TOL and trans <= trans_tol(d["K"]), (rot, trans)
    # and it agrees with the active f64 formulation up to float rounding
    ch.set_warp_formulation(0)
    T0, _ = ch.estimate_pose(0, 0, 1)
    rot, trans = pose_error(Th, T0)
    assert rot <= 5e-4 and trans <= 5 * trans_tol(d["K"]), (rot, trans)


@pytest.mark.parametrize("rows,cols,levels", [pytest.param(120, 160, 3, id="160x120-L3"), pytest.param(376, 1241, 4, id="kitti-1241x376-L4")])
@pytest.mark.parametrize("descriptor,loss", [("intensity", "huber"), ("bitplanes", "tukey"), ("gradient", "l2")])
def test_disparity_space_warp_parity(hip, orc, rows, cols, levels, descriptor, loss):
    """DisparitySpaceWarp in the place of RigidBodyWarp (bpvo/disparity_space_warp.{h,cc}; named by the north star, never
    instantiated by the reference): points (x - cx, y - cy, d, 1), H = G T G^-1, operator() in f32, its jacobian(), no
    normalisation, paramsToPose = TwistToMatrix.  Points, Jacobians, valid masks, residuals, sigma, weights bit-exact
    against the restatement; H / G against an f64 evaluation; the pose within the bar of the oracle's and of the rigid warp's."""
    ch, co, d = both(hip, orc, rows, cols, levels, descriptor=descriptor, loss=loss)
    T_rigid, _ = ch.estimate_pose(0, 0, 1)
    for ctx in (ch, co):
        ctx.set_warp_formulation(2)
        if ctx is ch:
            assert not ctx.frame_state(0)[1]           # the rigid-warp template was dropped
            with pytest.raises(capi.BpvoError):
                ctx.estimate_pose(0, 0, 1)
        ctx.frame_set_template(0)
    K = np.asarray(d["K"], np.float32)
    for l in range(levels):
        ph, po = ch.get_points(0, l), co.get_points(0, l)
        assert bits_equal(ph, po), f"points level {l}"
        assert np.array_equal(ch.get_point_indices(0, l), co.get_point_indices(0, l))
        # makePoint: pixel coordinates relative to the principal point of the level, raw disparity
        lr, lc = ch.level_size(l)
        inds = co.get_point_indices(0, l)
        cx, cy = np.float32(K[0, 2] * 0.5 ** l), np.float32(K[1, 2] * 0.5 ** l)
        assert np.array_equal(po[:, 0], (inds % lc).astype(np.float32) - cx) and np.array_equal(po[:, 1], (inds // lc).astype(np.float32) - cy)
        assert np.array_equal(po[:, 2], d["dispA"].ravel()[(1 << l) * ((inds // lc) * cols + inds % lc)])
        assert bits_equal(ch.get_pixels(0, l), co.get_pixels(0, l))
        assert bits_equal(ch.get_jacobians(0, l), co.get_jacobians(0, l)), f"jacobians level {l}"
        for T in (np.eye(4, dtype=np.float32), _perturbed_pose(1.0), _perturbed_pose(8.0)):
            a = ch.linearize(0, 0, 1, l, T)
            b = co.linearize(0, 0, 1, l, T)
            vo = co.get_valid(0)
            assert np.array_equal(ch.get_valid(0), vo), f"valid level {l}"
            assert bits_equal(ch.get_residuals(0), co.get_residuals(0)), f"residuals level {l}"
            assert a["sigma"] == b["sigma"] and a["num_valid"] == b["num_valid"]
            assert bits_equal(ch.get_weights(0), co.get_weights(0))
            H64, G64, f64 = normal_equations_f64(co.get_jacobians(0, l), co.get_residuals(0), co.get_weights(0), vo, ch.Cn)
            assert np.abs(a["H"] - H64).max() <= 4e-6 * np.abs(H64).max()
            assert np.abs(a["G"] - G64).max() <= 2e-5 * max(np.abs(G64).max(), 1e-3 * np.sqrt(np.abs(H64).max()))
    Th, sh = ch.estimate_pose(0, 0, 1)
    To, so = co.estimate_pose(0, 0, 1)
    rot, trans = pose_error(Th, To)
    assert rot <= ROT_TOL and trans <= trans_tol(d["K"]), (rot, trans, sh, so)
    # the same motion as the rigid-body warp finds (different parametrisation of the same problem)
    rot, trans = pose_error(Th, T_rigid)
    assert rot <= 1e-3 and trans <= 10 * trans_tol(d["K"]), (rot, trans)
    # a batch in this mode equals the pair run alone
    if rows <= 120:
        n = 3
        b = synth.make_batch(rows, cols, n, first_index=0)
        bc = hip.create(b["K"], b["b"], rows, cols, make_params(hip, descriptor=descriptor, loss=loss, levels=levels), n_frames=2 * n, n_pairs=n)
        bc.set_warp_formulation(2)
        poses, _ = bc.batch_run(b["images"], b["disparities"])
        assert bits_equal(poses[0], Th)


@pytest.mark.parametrize("rows,cols,levels", [pytest.param(120, 160, 3, id="160x120-L3"), pytest.param(376, 1241, 4, id="kitti-1241x376-L4")])
@pytest.mark.parametrize("interp", ["cosine", "cubic", "cubic_hermite"])
@pytest.mark.parametrize("descriptor,loss", [("intensity", "huber"), ("bitplanes", "tukey")])
def test_interpolation_variants_parity(hip, orc, rows, cols, levels, interp, descriptor, loss):
    """kCosine / kCubic / kCubicHermite of PhotoError::Impl::run (bpvo/photo_error.cc:391-444): masks with the
    (1, 3) borders bit-exact, f32 interpolation bit-exact for the polynomial forms; kCosine goes through a double
    cos() whose last bit may differ between libm and the device library, so its residuals get a 1-ulp-of-a-coefficient bar."""
    it = {"cosine": capi.INTERP_COSINE, "cubic": capi.INTERP_CUBIC, "cubic_hermite": capi.INTERP_CUBIC_HERMITE}[interp]
    ch, co, d = both(hip, orc, rows, cols, levels, descriptor=descriptor, loss=loss, interp=it)
    for l in range(levels):
        for T in (np.eye(4, dtype=np.float32), _perturbed_pose(1.0), _perturbed_pose(8.0)):
            a = ch.linearize(0, 0, 1, l, T)
            b = co.linearize(0, 0, 1, l, T)
            vo = co.get_valid(0)
            assert np.array_equal(ch.get_valid(0), vo), f"valid level {l}"
            assert a["num_valid"] == b["num_valid"]
            rh, ro = ch.get_residuals(0), co.get_residuals(0)
            if interp == "cosine":
                assert np.abs(rh - ro).max() <= 4e-7 * max(1.0, np.abs(ro).max()), f"residuals level {l}"
                assert abs(a["sigma"] - b["sigma"]) <= 1e-6 * b["sigma"]
            else:
                assert bits_equal(rh, ro), f"residuals level {l}"
                assert a["sigma"] == b["sigma"]
                assert bits_equal(ch.get_weights(0), co.get_weights(0))
            H64, G64, f64 = normal_equations_f64(co.get_jacobians(0, l), ro, co.get_weights(0), vo, ch.Cn)
            assert np.abs(a["H"] - H64).max() <= 1e-5 * np.abs(H64).max()
    Th, sh = ch.estimate_pose(0, 0, 1)
    To, so = co.estimate_pose(0, 0, 1)
    rot, trans = pose_error(Th, To)
    assert rot <= ROT_TOL and trans <= trans_tol(d["K"]), (rot, trans, sh, so)
    # the projectPoints f32 formulation exists for kLinear only
    with pytest.raises(capi.BpvoError):
        ch.set_warp_formulation(1)


@pytest.mark.parametrize("rows,cols,levels", [pytest.param(120, 160, 3, id="160x120-L3"), pytest.param(376, 1241, 4, id="kitti-1241x376-L4")])
@pytest.mark.parametrize("sigma_ct,sigma_bp", [(0.75, 0.5), (1.5, -1.0)])
def test_census_of_smoothed_image_bit_exact(hip, orc, rows, cols, levels, sigma_ct, sigma_bp):
    """sigmaPriorToCensusTransform > 0: cv::GaussianBlur(u8, 3x3) in fixed point before the census (bpvo/census.cc:63-66),
    fused into the census kernel.  Descriptor, selection and pose all follow bit-exactly / within the pose bar."""
    kw = dict(descriptor="bitplanes", loss="tukey", sigmaPriorToCensusTransform=sigma_ct, sigmaBitPlanes=sigma_bp)
    ch, co, d = both(hip, orc, rows, cols, levels, **kw)
    plain, _, _ = setup_pair(hip, rows, cols, levels=levels, descriptor="bitplanes", loss="tukey", sigmaBitPlanes=sigma_bp)
    differs = False
    for l in range(levels):
        for c in range(8):
            a, b = ch.get_descriptor_channel(1, l, c), co.get_descriptor_channel(1, l, c)
            assert bits_equal(a, b), f"descriptor level {l} channel {c}"
            differs |= not np.array_equal(a, plain.get_descriptor_channel(1, l, c))
            if sigma_bp <= 0:
                assert set(np.unique(a)) <= {0.0, 1.0}
        assert np.array_equal(ch.get_point_indices(0, l), co.get_point_indices(0, l))
    assert differs            # the smoothing is really applied
    Th, _ = ch.estimate_pose(0, 0, 1)
    To, _ = co.estimate_pose(0, 0, 1)
    rot, trans = pose_error(Th, To)
    assert rot <= ROT_TOL and trans <= trans_tol(d["K"]), (rot, trans)


@pytest.mark.parametrize("rows,cols,levels", [pytest.param(120, 160, 3, id="160x120-L3"), pytest.param(376, 1241, 4, id="kitti-1241x376-L4")])
@pytest.mark.parametrize("loss", ["tukey", "huber"])
def test_fused_frozen_scale_path_is_bit_identical(hip, rows, cols, levels, loss, monkeypatch):
    """Once a workspace's robust scale is frozen for a level (mestimator.cc:467-490), irls_reduce recomputes the residuals
    itself and warp_residual skips the workspace; the residual / valid buffers are refreshed on demand from the pose of the
    last linearisation.  Everything observable must equal the two-kernel form bit for bit."""
    out = []
    for fuse in ("0", "1"):
        set_options(monkeypatch, fuse_frozen=fuse)
        ctx, d, _ = setup_pair(hip, rows, cols, levels=levels, descriptor="bitplanes", loss=loss)
        T, st = ctx.estimate_pose(0, 0, 1)
        rec = dict(T=T, st=st, frac=ctx.fraction_good(0, 0.85), r=ctx.get_residuals(0), v=ctx.get_valid(0), w=ctx.get_weights(0),
                   fused=ctx.fused_point_counts())
        # and again through the batch entry point
        b = synth.make_batch(rows, cols, 3, first_index=5)
        bctx = hip.create(b["K"], b["b"], rows, cols, make_params(hip, descriptor="bitplanes", loss=loss, levels=levels), n_frames=6, n_pairs=3)
        poses, stats = bctx.batch_run(b["images"], b["disparities"])
        rec["bposes"] = poses
        rec["bstats"] = stats
        rec["br"] = bctx.get_residuals(2)
        rec["bw"] = bctx.get_weights(2)
        out.append(rec)
    a = out[0]
    assert a["fused"][0] == 0
    for b in out[1:]:
        assert b["fused"][0] > 0 and a["fused"][1] == b["fused"][1]
        assert bits_equal(a["T"], b["T"]) and bits_equal(a["bposes"], b["bposes"])
        assert a["st"] == b["st"]
        assert a["bstats"].tobytes() == b["bstats"].tobytes()
        assert a["frac"] == b["frac"]
        assert np.array_equal(a["v"], b["v"]) and bits_equal(a["r"], b["r"]) and bits_equal(a["w"], b["w"])
        assert bits_equal(a["br"], b["br"]) and bits_equal(a["bw"], b["bw"])


@pytest.mark.parametrize("seed", range(6))
def test_random_odd_sizes_and_parameters_pipeline_parity(hip, orc, seed):
    """Ragged shapes: image sizes that are not multiples of the 64 x 4 / 64 x 8 / 256-pixel tiles of the frame kernels
    (odd widths make every pyramid level ragged too), random noise images with constant, ramp or random disparities,
    NMS on / off, CD3 / CD5, with / without blur and normalisation.  Every stage must stay bit-exact, the pose within the bar."""
    rng = np.random.default_rng(4242 + seed)
    rows = int(rng.integers(49, 150))
    cols = int(rng.integers(70, 260))
    levels = int(rng.integers(1, 4))
    while min(rows, cols) >> (levels - 1) < 24:
        levels -= 1
    descriptor = ["bitplanes", "intensity"][seed % 2]
    kw = dict(descriptor=descriptor, loss=["tukey", "huber", "l2"][seed % 3], levels=levels,
              gradientEstimation=int(rng.integers(0, 2)), withNormalization=int(rng.integers(0, 2)),
              minNumPixelsForNonMaximaSuppression=int(rng.choice([1, 10**9])), minSaliency=float(rng.choice([0.05, 0.1, 1.0])),
              sigmaBitPlanes=float(rng.choice([-1.0, 0.5, 1.2])), sigmaPriorToCensusTransform=float(rng.choice([-1.0, 0.8])))
    base = synth.make_pair(160, 256, 30 + seed)
    yy, xx = np.mgrid[0:rows, 0:cols]
    img = base["imgA"][yy % 160, xx % 256].copy()
    img[rng.random((rows, cols)) < 0.02] = 255                      # salt
    img2 = np.roll(img, 1, axis=1)
    mode = seed % 3
    if mode == 0:
        disp = np.full((rows, cols), 7.5, np.float32)
    elif mode == 1:
        disp = (1.0 + 0.05 * xx + 0.02 * yy).astype(np.float32)
    else:
        disp = rng.uniform(-1.0, 40.0, (rows, cols)).astype(np.float32)   # negative -> rejected by the disparity gate
    K = np.array([[200.0, 0, cols / 2.0], [0, 200.0, rows / 2.0], [0, 0, 1]], np.float32)
    ctxs = []
    for b in (hip, orc):
        ctx = b.create(K, 0.2, rows, cols, make_params(b, **kw), n_frames=2, n_pairs=1)
        ctx.frame_set_data(0, img, disp)
        ctx.frame_set_template(0)
        ctx.frame_set_data(1, img2, disp)
        ctxs.append(ctx)
    ch, co = ctxs
    total = 0
    for l in range(levels):
        assert np.array_equal(ch.get_image(0, l), co.get_image(0, l)), (rows, cols, l)
        for c in range(ch.Cn):
            assert bits_equal(ch.get_descriptor_channel(1, l, c), co.get_descriptor_channel(1, l, c)), (rows, cols, l, c)
        assert bits_equal(ch.get_saliency(0, l), co.get_saliency(0, l)), (rows, cols, l)
        assert np.array_equal(ch.get_point_indices(0, l), co.get_point_indices(0, l)), (rows, cols, l)
        assert bits_equal(ch.get_points(0, l), co.get_points(0, l))
        assert bits_equal(ch.get_pixels(0, l), co.get_pixels(0, l))
        assert bits_equal(ch.get_jacobians(0, l), co.get_jacobians(0, l))
        n = ch.num_points(0, l)
        total += n
        if n == 0:
            continue
        T = _perturbed_pose(1.0)
        a, b = ch.linearize(0, 0, 1, l, T), co.linearize(0, 0, 1, l, T)
        assert np.array_equal(ch.get_valid(0), co.get_valid(0)) and bits_equal(ch.get_residuals(0), co.get_residuals(0))
        assert a["sigma"] == b["sigma"] and bits_equal(ch.get_weights(0), co.get_weights(0))
    if total and all(ch.num_points(0, l) > 0 for l in range(levels)):
        Th, sh = ch.estimate_pose(0, 0, 1)
        To, so = co.estimate_pose(0, 0, 1)
        rot, trans = pose_error(Th, To)
        # random textures can leave the problem ill-conditioned: the bar scales with the conditioning seen by both sides
        assert rot <= 20 * ROT_TOL and trans <= 20 * trans_tol(K), (rows, cols, kw, rot, trans, sh, so)


def test_full_hd_auto_pyramid_parity(hip, orc):
    """1920x1080, numPyramidLevels = -1 (auto: 1 + round(log2(1080 / 40)) = 6 levels, bpvo/vo.cc:101-105), bit-planes / Tukey:
    the largest size in the tests — selection lists, robust scales and the final pose against the CPU path."""
    rows, cols = 1080, 1920
    ch, co, d = both(hip, orc, rows, cols, -1, descriptor="bitplanes", loss="tukey")
    assert ch.L == co.L == 6
    for l in range(ch.L):
        assert np.array_equal(ch.get_point_indices(0, l), co.get_point_indices(0, l)), l
    T = _perturbed_pose(1.0)
    for l in (0, 3, 5):
        a, b = ch.linearize(0, 0, 1, l, T), co.linearize(0, 0, 1, l, T)
        assert np.array_equal(ch.get_valid(0), co.get_valid(0)) and bits_equal(ch.get_residuals(0), co.get_residuals(0))
        assert a["sigma"] == b["sigma"] and a["num_valid"] == b["num_valid"]
    Th, _ = ch.estimate_pose(0, 0, 1)
    To, _ = co.estimate_pose(0, 0, 1)
    rot, trans = pose_error(Th, To)
    assert rot <= ROT_TOL and trans <= trans_tol(d["K"]), (rot, trans)


@pytest.mark.parametrize("which", ["perf_bitplanes", "perf_intensity"])
def test_reference_timing_configurations_sequence(hip, orc, which):
    """The reference's own timing set-ups (conf/perf_bitplanes.cfg, conf/perf_intensity.cfg: the runs behind the figures quoted
    in BASELINE.md §1) as AlgorithmParameters(filename) builds them — file defaults included (CD5 gradients, gradientTolerance
    1e-6, minValidDisparity 1, goodPointThreshold 0.75; bpvo/types.cc:68-107) — on a 640x480 sequence through addFrame:
    sigma_ct 0.75 + sigma_bp 1.6 + L2 for bit-planes, NMS radius 2 + minSaliency 2.5 + Huber for intensity."""
    rows, cols = 480, 640
    common = dict(levels=3, parameterTolerance=1e-6, functionTolerance=1e-4, gradientTolerance=1e-6, maxIterations=50,
                  relaxTolerancesForCoarseLevels=1, gradientEstimation=capi.GRAD_CD5, minValidDisparity=1.0, goodPointThreshold=0.75)
    if which == "perf_bitplanes":
        kw = dict(common, descriptor="bitplanes", loss="l2", minTranslationMagToKeyFrame=0.1, minRotationMagToKeyFrame=5.0,
                  sigmaPriorToCensusTransform=0.75, sigmaBitPlanes=1.6)
    else:
        kw = dict(common, descriptor="intensity", loss="huber", minSaliency=2.5, nonMaxSuppRadius=2,
                  minTranslationMagToKeyFrame=1000.0, minRotationMagToKeyFrame=1000.0, maxFractionOfGoodPointsToKeyFrame=0.75)
    seq = synth.make_sequence(rows, cols, 5, index=11, step_rot=0.006, step_trans=0.04)
    res = []
    for b in (hip, orc):
        ctx = b.create(seq["K"], seq["b"], rows, cols, make_params(b, **kw), n_frames=3, n_pairs=1)
        out = [ctx.add_frame(img, disp) for img, disp in seq["frames"]]
        res.append((out, [ctx.vo_num_points_at_level(l) for l in range(3)]))
    (oh, nh), (oo, no_) = res
    assert nh == no_ and all(n > 0 for n in nh)
    assert [r["isKeyFrame"] for r in oh] == [r["isKeyFrame"] for r in oo]
    assert [r["keyFramingReason"] for r in oh] == [r["keyFramingReason"] for r in oo]
    for a, b in zip(oh, oo):
        rot, trans = pose_error(a["pose"], b["pose"])
        assert rot <= ROT_TOL and trans <= trans_tol(seq["K"]), (which, rot, trans)


@pytest.mark.parametrize("rows,cols,levels", [pytest.param(120, 160, 3, id="160x120-L3"), pytest.param(480, 640, 4, id="640x480-L4")])
@pytest.mark.parametrize("ksize", [1, 3, 5, 7])
def test_laplacian_descriptor_parity(hip, orc, rows, cols, levels, ksize):
    """kLaplacian (bpvo/gradient_descriptor.cc:64-67, cv::Laplacian with kernel size 1, 3, 5 or 7): one integer-valued f32 channel,
    then the same single-channel pipeline as Intensity — every stage bit-exact, poses within the bar."""
    ch, co, d = both(hip, orc, rows, cols, levels, descriptor="laplacian", loss="huber", laplacianKernelSize=ksize)
    assert ch.Cn == co.Cn == 1
    for l in range(levels):
        a, b = ch.get_descriptor_channel(1, l, 0), co.get_descriptor_channel(1, l, 0)
        assert bits_equal(a, b) and np.array_equal(a, np.round(a)) and np.abs(a).max() <= {1: 4, 3: 8, 5: 64, 7: 768}[ksize] * 255
        assert bits_equal(ch.get_saliency(0, l), co.get_saliency(0, l))
        assert np.array_equal(ch.get_point_indices(0, l), co.get_point_indices(0, l))
        assert bits_equal(ch.get_pixels(0, l), co.get_pixels(0, l)) and bits_equal(ch.get_jacobians(0, l), co.get_jacobians(0, l))
        T = _perturbed_pose(1.0)
        x, y = ch.linearize(0, 0, 1, l, T), co.linearize(0, 0, 1, l, T)
        assert np.array_equal(ch.get_valid(0), co.get_valid(0)) and bits_equal(ch.get_residuals(0), co.get_residuals(0))
        assert x["sigma"] == y["sigma"] and bits_equal(ch.get_weights(0), co.get_weights(0))
    Th, _ = ch.estimate_pose(0, 0, 1)
    To, _ = co.estimate_pose(0, 0, 1)
    rot, trans = pose_error(Th, To)
    assert rot <= ROT_TOL and trans <= trans_tol(d["K"]), (rot, trans)
    p = make_params(hip, descriptor="laplacian", levels=2, laplacianKernelSize=9)
    with pytest.raises(capi.BpvoError):
        hip.create(d["K"], d["b"], rows, cols, p)


@pytest.mark.parametrize("rows,cols,levels", [pytest.param(120, 160, 3, id="160x120-L3"), pytest.param(121, 163, 2, id="163x121-L2"),
                                              pytest.param(480, 640, 4, id="640x480-L4")])
@pytest.mark.parametrize("loss", ["huber", "tukey"])
def test_intensity_and_gradient_descriptor_parity(hip, orc, rows, cols, levels, loss):
    """kIntensityAndGradient (GradientDescriptor, bpvo/gradient_descriptor.cc:42-63 with sigma <= 0): three channels
    (I, Ix, Iy) through the generic-C forms of every kernel (point-major records) — all stages bit-exact, poses within the bar."""
    ch, co, d = both(hip, orc, rows, cols, levels, descriptor="gradient", loss=loss)
    assert ch.Cn == co.Cn == 3
    for l in range(levels):
        for c in range(3):
            assert bits_equal(ch.get_descriptor_channel(1, l, c), co.get_descriptor_channel(1, l, c)), (l, c)
        assert bits_equal(ch.get_saliency(0, l), co.get_saliency(0, l)), l
        assert np.array_equal(ch.get_point_indices(0, l), co.get_point_indices(0, l))
        assert bits_equal(ch.get_pixels(0, l), co.get_pixels(0, l)) and bits_equal(ch.get_jacobians(0, l), co.get_jacobians(0, l))
        for T in (np.eye(4, dtype=np.float32), _perturbed_pose(2.0)):
            a, b = ch.linearize(0, 0, 1, l, T), co.linearize(0, 0, 1, l, T)
            vo = co.get_valid(0)
            assert np.array_equal(ch.get_valid(0), vo) and bits_equal(ch.get_residuals(0), co.get_residuals(0))
            assert a["sigma"] == b["sigma"] and bits_equal(ch.get_weights(0), co.get_weights(0))
            H64, G64, f64 = normal_equations_f64(co.get_jacobians(0, l), co.get_residuals(0), co.get_weights(0), vo, 3)
            assert np.abs(a["H"] - H64).max() <= 1e-5 * np.abs(H64).max()
            assert abs(ch.fraction_good(0, 0.85) - co.fraction_good(0, 0.85)) < 1e-6
    Th, _ = ch.estimate_pose(0, 0, 1)
    To, _ = co.estimate_pose(0, 0, 1)
    rot, trans = pose_error(Th, To)
    assert rot <= ROT_TOL and trans <= trans_tol(d["K"]), (rot, trans)
    # batch entry point
    b3 = synth.make_batch(rows, cols, 3, first_index=40)
    outs = []
    for bind in (hip, orc):
        bc = bind.create(b3["K"], b3["b"], rows, cols, make_params(bind, descriptor="gradient", loss=loss, levels=levels), n_frames=6, n_pairs=3)
        outs.append(bc.batch_run(b3["images"], b3["disparities"])[0])
    for k in range(3):
        rot, trans = pose_error(outs[0][k], outs[1][k])
        assert rot <= ROT_TOL and trans <= trans_tol(b3["K"]), (k, rot, trans)
    # the optional pre-smoothing of the gradient channels (cv::GaussianBlur with OpenCV's automatic kernel size: 5 taps for
    # sigma 0.5 — the small-kernel filter forms — and 9 taps for sigma 1.0, the generic ones); channel 0 stays unsmoothed
    for sg in (0.5, 1.0):
        sh, so, _ = both(hip, orc, rows, cols, levels, descriptor="gradient", loss=loss, sigmaPriorToCensusTransform=sg)
        for l in range(levels):
            assert np.array_equal(sh.get_descriptor_channel(1, l, 0), sh.get_image(1, l).astype(np.float32))
            for c in range(3):
                assert bits_equal(sh.get_descriptor_channel(1, l, c), so.get_descriptor_channel(1, l, c)), (sg, l, c)
            assert not np.array_equal(sh.get_descriptor_channel(1, l, 1), ch.get_descriptor_channel(1, l, 1))
        Ts, _ = sh.estimate_pose(0, 0, 1)
        To2, _ = so.estimate_pose(0, 0, 1)
        rot, trans = pose_error(Ts, To2)
        assert rot <= ROT_TOL and trans <= trans_tol(d["K"]), (sg, rot, trans)
    for sg in (0.3, 4.0):     # 3 taps (another filter form) and more than 31 taps are refused
        with pytest.raises(capi.BpvoError):
            hip.create(d["K"], d["b"], rows, cols, make_params(hip, descriptor="gradient", levels=2, sigmaPriorToCensusTransform=sg))


@pytest.mark.parametrize("rows,cols,levels", [pytest.param(120, 160, 3, id="160x120-L3"), pytest.param(121, 163, 2, id="163x121-L2"),
                                              pytest.param(480, 640, 4, id="640x480-L4")])
@pytest.mark.parametrize("descriptor,C", [("fields1", 5), ("fields2", 10)])
def test_descriptor_fields_parity(hip, orc, rows, cols, levels, descriptor, C):
    """kDescriptorFieldsFirstOrder / SecondOrder (bpvo/gradient_descriptor.cc:100-160): 5 / 10 channels of smoothed positive and
    negative gradient parts, through the generic-C kernels — every stage bit-exact, poses within the bar.  Includes the
    reference's quirk that the second-order "Ixy" channels repeat the Ixx ones."""
    ch, co, d = both(hip, orc, rows, cols, levels, descriptor=descriptor, loss="huber")
    assert ch.Cn == co.Cn == C
    for l in range(levels):
        for c in range(C):
            assert bits_equal(ch.get_descriptor_channel(1, l, c), co.get_descriptor_channel(1, l, c)), (l, c)
        if C == 10:
            assert bits_equal(ch.get_descriptor_channel(1, l, 4), ch.get_descriptor_channel(1, l, 2))
        assert bits_equal(ch.get_saliency(0, l), co.get_saliency(0, l)), l
        assert np.array_equal(ch.get_point_indices(0, l), co.get_point_indices(0, l))
        assert bits_equal(ch.get_pixels(0, l), co.get_pixels(0, l)) and bits_equal(ch.get_jacobians(0, l), co.get_jacobians(0, l))
        for T in (np.eye(4, dtype=np.float32), _perturbed_pose(2.0)):
            a, b = ch.linearize(0, 0, 1, l, T), co.linearize(0, 0, 1, l, T)
            vo = co.get_valid(0)
            assert np.array_equal(ch.get_valid(0), vo) and bits_equal(ch.get_residuals(0), co.get_residuals(0))
            assert a["sigma"] == b["sigma"] and bits_equal(ch.get_weights(0), co.get_weights(0))
            H64, G64, f64 = normal_equations_f64(co.get_jacobians(0, l), co.get_residuals(0), co.get_weights(0), vo, C)
            assert np.abs(a["H"] - H64).max() <= 1e-5 * np.abs(H64).max()
            assert abs(ch.fraction_good(0, 0.85) - co.fraction_good(0, 0.85)) < 1e-6
    Th, _ = ch.estimate_pose(0, 0, 1)
    To, _ = co.estimate_pose(0, 0, 1)
    rot, trans = pose_error(Th, To)
    assert rot <= ROT_TOL and trans <= trans_tol(d["K"]), (rot, trans)


@pytest.mark.parametrize("descriptor", ["fields1", "fields2"])
def test_descriptor_fields_sigma_variants(hip, orc, descriptor):
    """dfSigma1 / dfSigma2 <= 0 switch the smoothing steps off (gradient_descriptor.cc:93,107); sigmas >= 2.5 make imsmooth
    pick kernels wider than 5 taps (7 for 2.6, 9 for 3.6: the generic filter forms); beyond 31 taps is refused.  Batch entry
    point with Tukey weights."""
    rows, cols, levels = 96, 128, 2
    for s1, s2 in ((-1.0, -1.0), (1.2, -1.0), (-1.0, 2.4), (2.6, 0.8), (0.75, 3.6)):
        ch, co, d = both(hip, orc, rows, cols, levels, descriptor=descriptor, loss="tukey", dfSigma1=s1, dfSigma2=s2)
        for l in range(levels):
            for c in range(ch.Cn):
                assert bits_equal(ch.get_descriptor_channel(1, l, c), co.get_descriptor_channel(1, l, c)), (s1, s2, l, c)
            assert np.array_equal(ch.get_point_indices(0, l), co.get_point_indices(0, l))
        Th, _ = ch.estimate_pose(0, 0, 1)
        To, _ = co.estimate_pose(0, 0, 1)
        rot, trans = pose_error(Th, To)
        assert rot <= ROT_TOL and trans <= trans_tol(d["K"]), (s1, s2, rot, trans)
    b3 = synth.make_batch(rows, cols, 3, first_index=50)
    outs = []
    for bind in (hip, orc):
        bc = bind.create(b3["K"], b3["b"], rows, cols, make_params(bind, descriptor=descriptor, loss="tukey", levels=levels), n_frames=6, n_pairs=3)
        outs.append(bc.batch_run(b3["images"], b3["disparities"])[0])
    for k in range(3):
        rot, trans = pose_error(outs[0][k], outs[1][k])
        assert rot <= ROT_TOL and trans <= trans_tol(b3["K"]), (k, rot, trans)
    with pytest.raises(capi.BpvoError):
        hip.create(b3["K"], b3["b"], rows, cols, make_params(hip, descriptor=descriptor, levels=2, dfSigma2=15.6))


@pytest.mark.parametrize("radius,rows,cols,levels,loss", [pytest.param(1, 120, 160, 3, "tukey", id="r1-8ch-160x120"),
                                                          pytest.param(2, 121, 163, 2, "huber", id="r2-24ch-163x121"),
                                                          pytest.param(3, 120, 160, 3, "huber", id="r3-48ch-160x120"),
                                                          pytest.param(1, 480, 640, 4, "huber", id="r1-8ch-640x480"),
                                                          pytest.param(4, 120, 160, 3, "huber", id="r4-80ch-160x120-5-groups-of-16"),
                                                          pytest.param(5, 121, 163, 2, "tukey", id="r5-120ch-163x121-5-groups-of-24"),
                                                          pytest.param(9, 96, 128, 2, "huber", id="r9-360ch-128x96-15-groups-of-24")])
def test_central_difference_descriptor_parity(hip, orc, radius, rows, cols, levels, loss):
    """kCentralDifference (bpvo/central_difference_descriptor.cc:36-131): the smoothed u8 image minus its shifts over a
    (2r+1)^2 window, each channel smoothed — 8 / 24 / 48 channels.  Radius 1 runs through the tuned 8-channel kernels (tiled
    records, tap cache), radius 2 / 3 through the generic-C forms, radii 4 .. 9 (80 .. 360 channels) through the same forms one channel
    GROUP at a time (types.h PairJob::pitch).  Every stage bit-exact, poses within the bar — and, in reference order, equal."""
    C = (2 * radius + 1) ** 2 - 1
    ch, co, d = both(hip, orc, rows, cols, levels, descriptor="centraldiff", loss=loss, centralDifferenceRadius=radius)
    assert ch.Cn == co.Cn == C
    for l in range(levels):
        for c in range(C):
            assert bits_equal(ch.get_descriptor_channel(1, l, c), co.get_descriptor_channel(1, l, c)), (l, c)
        assert bits_equal(ch.get_saliency(0, l), co.get_saliency(0, l)), l
        assert np.array_equal(ch.get_point_indices(0, l), co.get_point_indices(0, l))
        assert bits_equal(ch.get_pixels(0, l), co.get_pixels(0, l)) and bits_equal(ch.get_jacobians(0, l), co.get_jacobians(0, l))
        for T in (np.eye(4, dtype=np.float32), _perturbed_pose(2.0)):
            a, b = ch.linearize(0, 0, 1, l, T), co.linearize(0, 0, 1, l, T)
            vo = co.get_valid(0)
            assert np.array_equal(ch.get_valid(0), vo) and bits_equal(ch.get_residuals(0), co.get_residuals(0))
            assert a["sigma"] == b["sigma"] and bits_equal(ch.get_weights(0), co.get_weights(0))
            H64, G64, f64 = normal_equations_f64(co.get_jacobians(0, l), co.get_residuals(0), co.get_weights(0), vo, C)
            assert np.abs(a["H"] - H64).max() <= 1e-5 * np.abs(H64).max()
    Th, _ = ch.estimate_pose(0, 0, 1)
    To, so = co.estimate_pose(0, 0, 1)
    rot, trans = pose_error(Th, To)
    assert rot <= ROT_TOL and trans <= trans_tol(d["K"]), (rot, trans)
    if C > 48:      # the groups change nothing but the summation order: in the reference's own order the run is the oracle's, bit for bit
        ch.set_option("reference_reduction", 1)
        Tr, sr = ch.estimate_pose(0, 0, 1)
        assert bits_equal(Tr, To) and [s["numIterations"] for s in sr] == [s["numIterations"] for s in so] and [s["status"] for s in sr] == [s["status"] for s in so]
        a, b = ch.linearize(0, 0, 1, 0, _perturbed_pose(1.0)), co.linearize(0, 0, 1, 0, _perturbed_pose(1.0))
        assert bits_equal(a["H"], b["H"]) and bits_equal(a["G"], b["G"]) and a["f_norm"] == b["f_norm"] and a["num_valid"] == b["num_valid"]


def test_central_difference_variants(hip, orc):
    """Smoothing steps switched off (sigma <= 0: the raw u8 differences), the batch entry point, and the refused settings."""
    rows, cols, levels = 96, 128, 2
    # (2.7, 3.4): imsmooth picks 7 taps for the u8 blur before and 7 for the f32 blur after — the generic filter forms
    for sb, sa in ((-1.0, -1.0), (1.1, -1.0), (-1.0, 0.9), (2.7, 3.4), (0.75, 4.6)):
        ch, co, d = both(hip, orc, rows, cols, levels, descriptor="centraldiff", loss="tukey", centralDifferenceRadius=1,
                         centralDifferenceSigmaBefore=sb, centralDifferenceSigmaAfter=sa)
        for l in range(levels):
            for c in range(8):
                assert bits_equal(ch.get_descriptor_channel(1, l, c), co.get_descriptor_channel(1, l, c)), (sb, sa, l, c)
            assert np.array_equal(ch.get_point_indices(0, l), co.get_point_indices(0, l))
        Th, _ = ch.estimate_pose(0, 0, 1)
        To, _ = co.estimate_pose(0, 0, 1)
        rot, trans = pose_error(Th, To)
        assert rot <= ROT_TOL and trans <= trans_tol(d["K"]), (sb, sa, rot, trans)
    b3 = synth.make_batch(rows, cols, 3, first_index=60)
    outs = []
    for bind in (hip, orc):
        bc = bind.create(b3["K"], b3["b"], rows, cols, make_params(bind, descriptor="centraldiff", loss="huber", levels=levels,
                                                                     centralDifferenceRadius=2), n_frames=6, n_pairs=3)
        outs.append(bc.batch_run(b3["images"], b3["disparities"])[0])
    for k in range(3):
        rot, trans = pose_error(outs[0][k], outs[1][k])
        assert rot <= ROT_TOL and trans <= trans_tol(b3["K"]), (k, rot, trans)
    for kw in (dict(centralDifferenceRadius=10), dict(centralDifferenceRadius=0), dict(centralDifferenceSigmaAfter=16.0)):
        with pytest.raises(capi.BpvoError):
            hip.create(b3["K"], b3["b"], rows, cols, make_params(hip, descriptor="centraldiff", levels=2, **kw))


@pytest.mark.parametrize("descriptor,kw", [("gradient", {}), ("fields1", {}), ("fields2", {}),
                                           ("centraldiff", dict(centralDifferenceRadius=1)),
                                           ("centraldiff", dict(centralDifferenceRadius=2)),
                                           ("centraldiff", dict(centralDifferenceRadius=3, centralDifferenceSigmaAfter=-1.0))])
def test_scale_sequence_every_channel_count(hip, orc, descriptor, kw):
    """The bracketed median (second and later linearisations of a level: bracket_block + median_finish) for every channel
    count the kernels are instantiated for — found by tests/tools/fuzz_parity.py: a 32-bit channel mask broke it for 48 channels.
    Same pose sequence on both sides, same sigma / weights every time, and the bracketed path must actually be taken."""
    rows, cols = 50, 265
    ch, co, d = both(hip, orc, rows, cols, 1, descriptor=descriptor, loss="huber", **kw)
    To, so, trace = co.estimate_pose_trace(0, 0, 1)
    before = ch.median_path_counts()
    for k, rec in enumerate(trace[:12]):
        T = rec[:16].reshape(4, 4)
        a = ch.linearize(0, 0, 1, 0, T, reset_scale=(k == 0))
        b = co.linearize(0, 0, 1, 0, T, reset_scale=(k == 0))
        assert a["sigma"] == b["sigma"] and np.isfinite(a["sigma"]), (k, a["sigma"], b["sigma"])
        assert a["sigma"] == rec[59], (k, a["sigma"], rec[59])
        assert bits_equal(ch.get_weights(0), co.get_weights(0)), k
    after = ch.median_path_counts()
    assert after[0] - before[0] >= 1, (before, after)       # bracketed selections happened
    Th, sh = ch.estimate_pose(0, 0, 1)
    rot, trans = pose_error(Th, To)
    assert rot <= ROT_TOL and trans <= trans_tol(d["K"]), (rot, trans, sh, so)


@pytest.mark.parametrize("n,lanes,team", [(70, "2", "0"), (40, "2", "1"), (33, "1", "0"), (530, "2", "0")])
def test_host_buffer_batches_go_through_the_upload_pipeline_unchanged(hip, n, lanes, team, monkeypatch):
    """bpvo_hip_batch_run handed HOST buffers: batches of at least 32 pairs are staged in pinned chunks of 16 pairs by worker threads
    and uploaded on streams of their own while the lanes work on the chunks that have landed (B's disparity never crosses the bus).
    Same poses and statistics, bit for bit, as the batch with its inputs resident on the device and as the plain copies
    (option upload_workers = 0) — with ragged chunk and lane boundaries, one lane, the team kernel behind it, and (530 pairs) the
    three-group upload plan of large batches with the lanes' job tables copied by a kernel."""
    import torch
    rows, cols, levels = 120, 160, 3
    batch = synth.make_batch(rows, cols, n, first_index=400, workers=8)
    set_options(monkeypatch, lanes=lanes)
    set_options(monkeypatch, team=team)
    out = {}
    for workers in ("6", "0", "dev"):
        set_options(monkeypatch, upload_workers="6" if workers == "dev" else workers)
        ctx = hip.create(batch["K"], batch["b"], rows, cols, make_params(hip, descriptor="bitplanes", loss="tukey", levels=levels), n_frames=2 * n, n_pairs=n)
        if workers == "dev":
            di = torch.from_numpy(batch["images"]).cuda(); dd = torch.from_numpy(batch["disparities"]).cuda()
            out[workers] = ctx.batch_run_device(n, di.data_ptr(), dd.data_ptr())
        else:
            out[workers] = ctx.batch_run(batch["images"], batch["disparities"])
            secs, nbytes = ctx.upload_stats()
            assert (nbytes == n * rows * cols * 6 and secs > 0) if workers == "6" else nbytes == 0
            # the B slots of a batch hold no disparity: they cannot become templates
            with pytest.raises(capi.BpvoError):
                ctx.frame_set_template(1)
        ctx.close()
    for k in ("0", "dev"):
        assert bits_equal(out["6"][0], out[k][0]), k
        assert out["6"][1].tobytes() == out[k][1].tobytes(), k


def test_current_frames_of_a_batch_keep_a_complete_descriptor(hip, orc):
    """The current frames of a pair batch get neither their disparity (never read) nor the compact channel-0 plane of their descriptor
    (it serves the saliency map of template frames only).  The descriptor records themselves are complete, and set_template on such a
    frame is refused — there is no disparity to select by — until setData hands the frame over again."""
    rows, cols, n = 120, 160, 3
    batch = synth.make_batch(rows, cols, n, first_index=90)
    p = make_params(hip, levels=3)
    ctx = hip.create(batch["K"], batch["b"], rows, cols, p, n_frames=2 * n, n_pairs=n)
    ctx.batch_run(batch["images"], batch["disparities"])
    oc = orc.create(batch["K"], batch["b"], rows, cols, make_params(orc, levels=3), n_frames=2, n_pairs=1)
    oc.frame_set_data(0, batch["images"][1], batch["disparities"][1])
    oc.frame_set_template(0)
    for l in range(3):
        for ch in range(ctx.Cn):
            assert bits_equal(ctx.get_descriptor_channel(1, l, ch), oc.get_descriptor_channel(0, l, ch))
    with pytest.raises(capi.BpvoError):
        ctx.frame_set_template(1)
    ctx.frame_set_data(1, batch["images"][1], batch["disparities"][1])
    ctx.frame_set_template(1)
    for l in range(3):
        assert np.array_equal(ctx.get_point_indices(1, l), oc.get_point_indices(0, l))
        assert bits_equal(ctx.get_pixels(1, l), oc.get_pixels(0, l)) and bits_equal(ctx.get_saliency(1, l), oc.get_saliency(0, l))
    ctx.close(); oc.close()


@pytest.mark.parametrize("rows,cols", [(33, 70), (64, 64), (65, 129), (200, 37), (97, 301), (16, 64), (24, 40)])
@pytest.mark.parametrize("radius,nms_from", [(1, 1), (1, 10 ** 9), (2, 1)])
def test_selection_on_odd_shapes(hip, orc, rows, cols, radius, nms_from):
    """The tiled saliency + selection pass (NMS radius <= 1: 64 x 32 tiles, candidate bit words, word scan, full-wave compaction) and the
    three-pass form it leaves to larger radii, on images narrower than a tile, one pixel wider than one, taller than wide: saliency,
    point order, points and template pixels equal the oracle's at every level."""
    d = synth.make_pair(rows, cols, 5)
    kw = dict(levels=2, nonMaxSuppRadius=radius, minNumPixelsForNonMaximaSuppression=nms_from, minSaliency=0.05)
    ch = hip.create(d["K"], d["b"], rows, cols, make_params(hip, **kw), n_frames=2, n_pairs=1)
    co = orc.create(d["K"], d["b"], rows, cols, make_params(orc, **kw), n_frames=2, n_pairs=1)
    for c in (ch, co):
        c.frame_set_data(0, d["imgA"], d["dispA"])
        c.frame_set_template(0)
    for l in range(2):
        assert bits_equal(ch.get_saliency(0, l), co.get_saliency(0, l)), l
        assert ch.num_points(0, l) == co.num_points(0, l), (l, ch.num_points(0, l), co.num_points(0, l))
        assert np.array_equal(ch.get_point_indices(0, l), co.get_point_indices(0, l)), l
        assert bits_equal(ch.get_points(0, l), co.get_points(0, l)) and bits_equal(ch.get_pixels(0, l), co.get_pixels(0, l)), l
    ch.close(); co.close()


@pytest.mark.parametrize("rows,cols,levels,nbytes,K,rotation", [
    pytest.param(120, 160, 3, 1, 1, 0, id="160x120-1byte"), pytest.param(120, 160, 3, 4, 1, 0, id="160x120-4bytes"),
    pytest.param(480, 640, 4, 1, 1, 0, id="640x480-1byte"), pytest.param(480, 640, 4, 4, 1, 0, id="640x480-4bytes"),
    pytest.param(121, 163, 2, 2, 3, 1, id="163x121-2bytes-K3-rotation"), pytest.param(120, 160, 2, 1, 0, 1, id="160x120-1byte-K0-rotation"),
    pytest.param(120, 160, 2, 8, 1, 0, id="160x120-8bytes-2-groups-of-32"), pytest.param(121, 163, 2, 16, 2, 1, id="163x121-16bytes-K2-rotation-4-groups-of-32"),
    pytest.param(120, 160, 2, 64, 1, 0, id="160x120-64bytes-16-groups-of-32")])
def test_latch_descriptor_parity(hip, orc, rows, cols, levels, nbytes, K, rotation):
    """kLatch (LatchDescriptor, bpvo/latch_descriptor.cc:83-165,1041-1086; factory bpvo/dense_descriptor.cc:69-72; parameters of
    conf/tsukuba_eval.cfg:49-52 in the first cases): 8 * latchNumBytes channels of +-128-valued bit planes of the densely evaluated LATCH
    bytes, each smoothed with imsmooth(1.75) — integer sums of squared differences over u8 patches, so the planes must equal the oracle's
    BIT FOR BIT, as must everything built from them; poses within the bar.  Levels too small for a key point (border 24 + K on every side)
    give a zero descriptor and an empty template on both sides."""
    ch, co, d = both(hip, orc, rows, cols, levels, descriptor="latch", loss="tukey", latchNumBytes=nbytes, latchHalfSsdSize=K,
                     latchRotationInvariance=rotation)
    C = 8 * nbytes
    assert ch.Cn == co.Cn == C
    some_points = False
    for l in range(levels):
        for c in range(C):
            a = ch.get_descriptor_channel(1, l, c)
            assert bits_equal(a, co.get_descriptor_channel(1, l, c)), (l, c)
        assert bits_equal(ch.get_saliency(0, l), co.get_saliency(0, l)), l
        assert np.array_equal(ch.get_point_indices(0, l), co.get_point_indices(0, l))
        if ch.num_points(0, l) == 0:
            continue
        some_points = True
        assert bits_equal(ch.get_pixels(0, l), co.get_pixels(0, l)) and bits_equal(ch.get_jacobians(0, l), co.get_jacobians(0, l))
        for T in (np.eye(4, dtype=np.float32), _perturbed_pose(1.0)):
            a, b = ch.linearize(0, 0, 1, l, T), co.linearize(0, 0, 1, l, T)
            vo = co.get_valid(0)
            assert np.array_equal(ch.get_valid(0), vo) and bits_equal(ch.get_residuals(0), co.get_residuals(0))
            assert a["sigma"] == b["sigma"] and bits_equal(ch.get_weights(0), co.get_weights(0))
            H64, G64, f64 = normal_equations_f64(co.get_jacobians(0, l), co.get_residuals(0), co.get_weights(0), vo, C)
            assert np.abs(a["H"] - H64).max() <= 1e-5 * np.abs(H64).max()
    assert some_points
    hip_err = orc_err = None
    try:
        Th, _ = ch.estimate_pose(0, 0, 1)
    except capi.BpvoError as e:
        hip_err = str(e)
    try:
        To, _ = co.estimate_pose(0, 0, 1)
    except capi.BpvoError as e:
        orc_err = str(e)
    assert (hip_err is None) == (orc_err is None), (hip_err, orc_err)
    if hip_err is None:
        rot, trans = pose_error(Th, To)
        assert rot <= ROT_TOL and trans <= trans_tol(d["K"]), (rot, trans)
        if C > 48:      # channel groups: in the reference's summation order the run is the oracle's, bit for bit
            ch.set_option("reference_reduction", 1)
            assert bits_equal(ch.estimate_pose(0, 0, 1)[0], To)


@pytest.mark.parametrize("rows,cols,levels", [pytest.param(120, 160, 3, id="160x120-L3"), pytest.param(376, 1241, 4, id="kitti-1241x376-L4"),
                                              pytest.param(243, 651, 3, id="651x243-L3-ragged")])
def test_normalisation_sums_hand_scheduled_against_the_compilers_form(hip, rows, cols, levels):
    """The Hartley sums (bpvo/warps.cc:27-48) are sequential f32 additions.  Option "normalization_form": 1 (the default) back-to-back DPP adds without
    the wait states the compiler's hazard table inserts (kernels_frame.hip nrm_add_batch), 0 the compiler's form of those chains, 2 broadcast LDS
    reads + plain adds (no cross-lane traffic, no asm), 3 the same reads with the adds as blocks of back-to-back plain v_add_f32 on a wave that does nothing else:
    T_n / T_n^-1 of every level, and every pose built on them, must be the same bits in all four — a toolchain
    or hardware change that invalidates the hand-scheduled form fails here (and the default against the oracle in test_template_bit_exact)."""
    outs = []
    for asm in (2, 1, 0, 3):
        ch, d, _ = setup_pair(hip, rows, cols, levels=levels, descriptor="bitplanes", loss="tukey")
        ch.set_option("normalization_form", asm)
        ch.frame_set_template(0)
        outs.append(([np.stack(ch.get_normalization(0, l)) for l in range(levels)], ch.estimate_pose(0, 0, 1)[0]))
        ch.close()
    for o in outs[1:]:
        for l in range(levels):
            assert bits_equal(outs[0][0][l], o[0][l]), l
        assert bits_equal(outs[0][1], o[1])


def test_current_frames_of_a_pair_batch_keep_no_disparity_unless_asked(hip):
    """bpvo_hip_batch_run neither uploads nor stores the disparity of the CURRENT frame (B) of a pair — nothing on the path reads it (the
    reference's setData copies whatever it is handed, bpvo/vo_frame.cc:48-55; the difference is stated in c_api.h).  Making such a slot a
    template therefore fails with BPVO_ERR_NO_DATA; with the option keep_current_disparity = 1 it works, and the poses are the same."""
    rows, cols, n = 96, 128, 4
    b = synth.make_batch(rows, cols, n, first_index=3)
    outs = []
    for keep in (0, 1):
        ctx = hip.create(b["K"], b["b"], rows, cols, make_params(hip, levels=2), n_frames=2 * n, n_pairs=n)
        assert ctx.get_option("keep_current_disparity") == 0.0
        ctx.set_option("keep_current_disparity", keep)
        poses, _ = ctx.batch_run(b["images"], b["disparities"])
        outs.append(poses)
        if keep:
            ctx.frame_set_template(1)                                   # B of pair 0 becomes the template of a later estimate
            T, _ = ctx.estimate_pose(0, 1, 2)
            assert np.isfinite(T).all()
        else:
            with pytest.raises(capi.BpvoError, match="status -3"):      # BPVO_ERR_NO_DATA
                ctx.frame_set_template(1)
        ctx.close()
    assert bits_equal(outs[0], outs[1])
    with pytest.raises(capi.BpvoError):
        ctx = hip.create(b["K"], b["b"], rows, cols, make_params(hip, levels=2), n_frames=2, n_pairs=1)
        ctx.set_option("no_such_option", 1)


@pytest.mark.parametrize("rows,cols,levels", [pytest.param(376, 1241, 4, id="kitti-1241x376-L4"), pytest.param(243, 651, 3, id="651x243-L3-ragged"),
                                              pytest.param(112, 144, 1, id="144x112-L1-width-multiple-of-4"), pytest.param(480, 640, 4, id="640x480-L4")])
def test_lazy_template_descriptor_is_bit_identical(hip, rows, cols, levels):
    """Pair batches keep, for their TEMPLATE frames, census bytes + channel 0 instead of descriptor records at the levels with non-maximum
    suppression (option lazy_template_descriptor, default on); template_build forms the records of its stencils from the census bytes.
    Against the dense form: template pixels and Jacobians of every level, poses and statistics, bit for bit; the accessor rebuilds the
    records of a lazy level on demand (= the descriptor of the same image set through the frame API).  Every context first runs a batch
    of OTHER images with dense records, so that a record the lazy form does not write but something reads — the saliency of column 3 reads
    the record of column 0 of the next row when the width is a multiple of 4 (the reference's read past the row, Q7) — is a stale one."""
    n = 3
    b = synth.make_batch(rows, cols, n, first_index=40)
    other = synth.make_batch(rows, cols, n, first_index=77)
    out = {}
    for lazy in (0, 1):
        ctx = hip.create(b["K"], b["b"], rows, cols, make_params(hip, levels=levels, minNumPixelsForNonMaximaSuppression=100 * 100 if levels > 1 else 1),
                         n_frames=2 * n, n_pairs=n)
        ctx.set_option("lazy_template_descriptor", 0)
        ctx.batch_run(other["images"], other["disparities"])
        ctx.set_option("lazy_template_descriptor", lazy)
        poses, stats = ctx.batch_run(b["images"], b["disparities"])
        rec = dict(poses=poses, stats=stats, pix=[ctx.get_pixels(2, l) for l in range(levels)], jac=[ctx.get_jacobians(2, l) for l in range(levels)],
                   npts=[ctx.num_points(2, l) for l in range(levels)], sal=[ctx.get_saliency(2, l) for l in range(levels)])
        rec["desc"] = [np.stack([ctx.get_descriptor_channel(2, l, c) for c in range(8)]) for l in range(levels)]      # (lazy: rebuilt on demand)
        rec["desc_b"] = ctx.get_descriptor_channel(3, 0, 5)
        out[lazy] = rec
        ctx.close()
    a, z = out[0], out[1]
    assert a["npts"] == z["npts"] and min(a["npts"]) > 0
    assert bits_equal(a["poses"], z["poses"]) and a["stats"].tobytes() == z["stats"].tobytes()
    for l in range(levels):
        assert bits_equal(a["sal"][l], z["sal"][l]), l
        assert bits_equal(a["pix"][l], z["pix"][l]), l
        assert bits_equal(a["jac"][l], z["jac"][l]), l
        assert bits_equal(a["desc"][l], z["desc"][l]), l
    assert bits_equal(a["desc_b"], z["desc_b"])


@pytest.mark.parametrize("kw", [pytest.param(dict(descriptor="bitplanes", loss="tukey"), id="bitplanes-tukey"),
                                pytest.param(dict(descriptor="bitplanes", loss="l2"), id="bitplanes-l2"),
                                pytest.param(dict(descriptor="intensity", loss="huber"), id="intensity-huber"),
                                pytest.param(dict(descriptor="bitplanes", loss="tukey", interp=capi.INTERP_CUBIC), id="bitplanes-cubic"),
                                pytest.param(dict(descriptor="gradient", loss="tukey"), id="gradient-tukey"),
                                pytest.param(dict(descriptor="bitplanes", loss="huber", fuse_frozen=0), id="bitplanes-unfused")])
def test_step_taken_by_the_last_reduction_tile_is_bit_identical(hip, kw):
    """Option step_in_reduce_max_pairs (groups of up to 128 pairs by default): the four-kernel chain of a batch runs as three — the tile of a pair that stores its partial sums
    last in an irls_reduce launch sums them (in tile order, as gn_step_kernel does) and takes the Gauss-Newton step.  Poses, statistics,
    residuals and weights against the four-kernel form, bit for bit; the batch holds a pair whose template is empty at every level (its
    tile 0 takes the step: solver error, like the separate kernel) and is run twice on the same context (the tickets are back at zero)."""
    kw = dict(kw)
    fuse = kw.pop("fuse_frozen", 1)
    rows, cols, levels, n = 120, 160, 3, 6
    b = synth.make_batch(rows, cols, n, first_index=11)
    disp = b["disparities"].copy()
    disp[2 * 4] = 0.0                      # pair 4: no valid disparity in its template frame -> no points
    out = {}
    for step in (0, 1):
        ctx = hip.create(b["K"], b["b"], rows, cols, make_params(hip, levels=levels, **kw), n_frames=2 * n, n_pairs=n)
        ctx.set_option("team", 0)           # the chain, not the team kernel of small batches
        ctx.set_option("fuse_frozen", fuse)
        ctx.set_option("step_in_reduce_max_pairs", 1000 * step)
        assert ctx.get_option("step_in_reduce_max_pairs") == 1000.0 * step
        for _ in range(2):
            poses, stats = ctx.batch_run(b["images"], disp)
        out[step] = dict(poses=poses, stats=stats, r=ctx.get_residuals(1), w=ctx.get_weights(1), n4=ctx.num_points(2 * 4, 0))
        ctx.close()
    a, z = out[0], out[1]
    assert a["n4"] == 0 and z["n4"] == 0
    assert bits_equal(a["poses"], z["poses"])
    assert a["stats"].tobytes() == z["stats"].tobytes()
    assert bits_equal(a["r"], z["r"]) and bits_equal(a["w"], z["w"])
    assert np.isfinite(z["poses"][[0, 1, 2, 3, 5]]).all()
