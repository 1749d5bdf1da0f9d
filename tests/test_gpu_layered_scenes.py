"""The pipeline on layered scenes (synth scene="layered"): a slanted background behind three or four planar patches at their own depths,
disparity holes in value-noise blobs and along every depth edge (0, -1, 600), sensor noise on frame B, occlusions, front-surface
disparities over 3-30 px (640x480) and 15-96 px (1241x376).  Every other full-size parity test renders one textured plane, where every
disparity is valid, nothing is occluded and Tukey's zero-weight region stays almost empty.

The bars are the plane tests' own: bit-exact stages (test_gpu_parity.py), bit-exact trajectories in reference order
(test_gpu_reference_order.py), poses within 1e-4 rad / 1e-3 m in the default mode, bit-identity across scheduling options.
"""
import gc
import json
import os

import numpy as np
import pytest

from bpvo_amd import capi, synth
from util import (ROT_TOL, TRANS_TOL, assert_same_run, assert_trace_reproduced, bits_equal, both, make_params, normal_equations_f64,
                  oracle_pairs, perturbed_pose, pose_error)

pytestmark = pytest.mark.gpu

SIZES = [pytest.param(480, 640, 4, id="640x480-L4"), pytest.param(376, 1241, 4, id="kitti-1241x376-L4")]
CONFIGS = [("intensity", "huber"), ("bitplanes", "tukey")]
INDEX = 3          # the layered pair of the single-pair tests (seed 1003)


def _stage_cases():
    for rows, cols, levels in (p.values for p in SIZES):
        for desc, loss in CONFIGS:
            yield pytest.param(rows, cols, levels, desc, loss, id=f"{cols}x{rows}-{desc}-{loss}")
    yield pytest.param(480, 640, 4, "intensity", "l2", id="640x480-intensity-l2")


@pytest.mark.parametrize("rows,cols,levels,descriptor,loss", list(_stage_cases()))
def test_layered_stages_bit_exact(hip, orc, rows, cols, levels, descriptor, loss):
    """pyramid, every descriptor channel, saliency, N, point indices, points, normalisation, pixels, Jacobians; at identity and the 1x / 8x
    perturbed poses the valid mask, residuals, sigma and weights bit for bit, H / G / f against the f64 evaluation."""
    ch, co, d = both(hip, orc, rows, cols, levels, scene="layered", index=INDEX, descriptor=descriptor, loss=loss)
    for l in range(levels):
        assert np.array_equal(ch.get_image(0, l), co.get_image(0, l)), f"pyrDown A level {l}"
        assert np.array_equal(ch.get_image(1, l), co.get_image(1, l)), f"pyrDown B level {l}"
        for c in range(ch.Cn):
            a, b = ch.get_descriptor_channel(1, l, c), co.get_descriptor_channel(1, l, c)
            assert bits_equal(a, b), f"descriptor level {l} channel {c}"
        assert bits_equal(ch.get_saliency(0, l), co.get_saliency(0, l)), f"saliency level {l}"
        n = ch.num_points(0, l)
        assert n == co.num_points(0, l) and n % 16 == 0 and n > 0, f"N level {l}"
        assert np.array_equal(ch.get_point_indices(0, l), co.get_point_indices(0, l)), f"selected pixels level {l}"
        assert bits_equal(ch.get_points(0, l), co.get_points(0, l)), f"points level {l}"
        Th, Tih = ch.get_normalization(0, l)
        To, Tio = co.get_normalization(0, l)
        assert bits_equal(Th, To) and bits_equal(Tih, Tio), f"normalisation level {l}"
        assert bits_equal(ch.get_pixels(0, l), co.get_pixels(0, l)), f"pixels level {l}"
        assert bits_equal(ch.get_jacobians(0, l), co.get_jacobians(0, l)), f"jacobians level {l}"
    # the selection never takes a hole: every selected pixel's disparity passes the gate
    idx = ch.get_point_indices(0, 0)
    dsel = d["dispA"].reshape(-1)[idx]
    assert ((dsel >= np.float32(0.001)) & (dsel <= 512)).all()
    zero_weight = []
    for l in range(levels):
        for k, T in enumerate((np.eye(4, dtype=np.float32), perturbed_pose(1.0), perturbed_pose(8.0))):
            a = ch.linearize(0, 0, 1, l, T)
            b = co.linearize(0, 0, 1, l, T)
            vh, vo = ch.get_valid(0), co.get_valid(0)
            assert np.array_equal(vh, vo), f"valid mask level {l} pose {k}"
            assert a["num_valid"] == b["num_valid"] == int(vo.sum())
            assert bits_equal(ch.get_residuals(0), co.get_residuals(0)), f"residuals level {l} pose {k}"
            assert a["sigma"] == b["sigma"], f"sigma level {l} pose {k}: {a['sigma']} vs {b['sigma']}"
            w = co.get_weights(0)
            assert bits_equal(ch.get_weights(0), w), f"weights level {l} pose {k}"
            H64, G64, f64 = normal_equations_f64(co.get_jacobians(0, l), co.get_residuals(0), w, vo, ch.Cn)
            scale = np.abs(H64).max()
            gscale = max(np.abs(G64).max(), 1e-3 * scale)
            assert np.abs(a["H"] - H64).max() <= 4e-6 * scale, f"H level {l} pose {k} (hip vs f64)"
            assert np.abs(a["G"] - G64).max() <= 4e-6 * gscale, f"G level {l} pose {k} (hip vs f64)"
            assert abs(a["f_norm"] - f64) <= 4e-6 * max(f64, 1e-6)
            # the oracle's serial f32 sums: 2.6e-4 of max |H| from the f64 value at 1241x376 bit-planes level 0 on this pair (more terms of large
            # magnitude than on the plane, where 2e-4 holds); the GPU's own bar above stays 4e-6
            assert np.abs(b["H"] - H64).max() <= 5e-4 * scale and np.abs(b["G"] - G64).max() <= 5e-4 * gscale
            wv = np.asarray(w).reshape(ch.Cn, -1)[:, vo.astype(bool)]
            zero_weight.append(int((wv == 0).sum()))
    if loss == "tukey":
        # points of weight zero were compared: bit-plane residuals lie in [-1, 1], so Tukey's cut-off 4.685 sigma is crossed where sigma is
        # small — at identity on these pairs; at the 1x / 8x perturbed poses sigma grows past 0.2 and the zero-weight region empties
        assert sum(zero_weight) > 0, zero_weight
    ch.close()
    co.close()


REF_CONFIGS = [pytest.param(480, 640, 4, dict(descriptor="intensity", loss="huber"), id="config2-640x480-intensity-huber"),
               pytest.param(480, 640, 4, dict(descriptor="bitplanes", loss="tukey"), id="config3-640x480-bitplanes-tukey"),
               pytest.param(376, 1241, 4, dict(descriptor="bitplanes", loss="tukey"), id="config4-1241x376-bitplanes-tukey")]


@pytest.mark.parametrize("rows,cols,levels,kw", REF_CONFIGS)
def test_layered_reference_order_bit_exact(hip, orc, rows, cols, levels, kw):
    """reference_reduction = 1: every linearisation, the pose and the statistics of every level are the oracle's, from identity and from
    a perturbed start, on two layered pairs.  Around these runs the median and tap-cache counters show that the compared runs went through
    full median selections after bracketed ones and through tap-cache misses."""
    mb, mf, lin_starts = 0, 0, 0
    hits = lookups = 0
    for index in (INDEX, 9):
        ch, co, _ = both(hip, orc, rows, cols, levels, reference=True, scene="layered", index=index, **kw)
        b0, f0 = ch.median_path_counts()
        t0 = ch.tap_cache_counts()
        for T0 in (None, perturbed_pose(2.0)):
            Th, sh, rh = ch.estimate_pose_trace(0, 0, 1, T0)
            To, so, ro = co.estimate_pose_trace(0, 0, 1, T0)
            assert_same_run(Th, sh, rh, To, so, ro, f"{kw} index {index} start {'identity' if T0 is None else 'perturbed'}")
            lin_starts += levels
        b1, f1 = ch.median_path_counts()
        t1 = ch.tap_cache_counts()
        mb, mf = mb + b1 - b0, mf + f1 - f0
        hits, lookups = hits + t1[0] - t0[0], lookups + t1[1] - t0[1]
        ch.close()
        co.close()
    print(f"\n{kw}: median bracketed {mb} full {mf} (level starts {lin_starts}); tap cache {hits} / {lookups}")
    assert mb > 0 and mf > lin_starts, ("full median selections beyond the level starts", mb, mf, lin_starts)
    assert lookups > hits > 0, ("tap-cache misses and hits", hits, lookups)


@pytest.mark.parametrize("rows,cols,levels", SIZES)
@pytest.mark.parametrize("descriptor,loss", CONFIGS)
def test_layered_fast_mode_single_pair(hip, orc, rows, cols, levels, descriptor, loss):
    """default mode: pose within the bar of the oracle, its per-iteration trace reproduced; persistent 0 / 1 and fuse_frozen 0 / 1 give
    bit-identical poses and statistics."""
    ch, co, d = both(hip, orc, rows, cols, levels, scene="layered", index=INDEX, descriptor=descriptor, loss=loss)
    Th, sh = ch.estimate_pose(0, 0, 1)
    To, so, trace = co.estimate_pose_trace(0, 0, 1)
    rot, trans = pose_error(Th, To)
    assert rot <= ROT_TOL and trans <= TRANS_TOL, (rot, trans, sh, so)
    rg, tg = pose_error(Th, d["T_gt"])
    assert rg < 1e-2 and tg < 1e-1, (rg, tg)
    for key in ("persistent", "fuse_frozen"):
        v = ch.get_option(key)
        ch.set_option(key, 1 - int(v))
        T2, s2 = ch.estimate_pose(0, 0, 1)
        ch.set_option(key, int(v))
        assert bits_equal(T2, Th) and s2 == sh, (key, s2, sh)
    # H, G: the oracle's serial f32 sums deviate by up to ~3e-4 of max |H| on these pairs (test_layered_stages_bit_exact bounds the GPU's
    # own sums against f64 at 4e-6)
    assert_trace_reproduced(ch, trace, h_tol=1e-3)
    ch.close()
    co.close()


# ---- the layered config-5 shard ----------------------------------------------------------------------------------------------------
ROWS, COLS, LEVELS = 376, 1241, 4
SHARD, N_ORACLE = 128, 32


def _diagnostics(ctx):
    b, f = ctx.median_path_counts()
    t = ctx.tap_cache_counts()
    fu, tot = ctx.fused_point_counts()
    return dict(tap_hit_rate=round(t[0] / max(t[1], 1), 4), tap_hit_rate_first8=round(t[2] / max(t[3], 1), 4), median_bracketed=b, median_full=f,
                fused_share=round(fu / max(tot, 1), 4))


@pytest.fixture(scope="module")
def layered_shard(hip, orc):
    batch = synth.make_batch(ROWS, COLS, SHARD, first_index=0, workers=min(8, os.cpu_count() or 1), scene="layered")
    kw = dict(descriptor="bitplanes", loss="tukey", levels=LEVELS)
    gc.collect()           # the team kernel runs only while one context is live on the device: drop what earlier tests left
    ctx = hip.create(batch["K"], batch["b"], ROWS, COLS, make_params(hip, **kw), n_frames=2 * SHARD, n_pairs=SHARD)
    poses, stats = ctx.batch_run(batch["images"], batch["disparities"])
    diag = dict(_diagnostics(ctx), team_launches=ctx.team_counts())
    picks = list(range(0, SHARD, SHARD // N_ORACLE))
    ref = oracle_pairs(orc, batch, picks, kw, trace=True)
    yield dict(batch=batch, ctx=ctx, poses=poses, stats=stats, picks=picks, ref=ref, kw=kw, diag=diag)
    ctx.close()


def test_layered_shard_against_the_oracle(layered_shard):
    """32 of the 128 pairs: pose within the bar pair by pair; the first linearisation of every level (at the oracle's pose) gives the
    oracle's valid count and sigma; the iteration-count distributions agree as in the plane shard's test.  Prints the diagnostics."""
    sh = layered_shard
    ctx = sh["ctx"]
    worst = (0.0, 0.0)
    for k, r in zip(sh["picks"], sh["ref"]):
        rot, tr = pose_error(sh["poses"][k], r["T"])
        assert rot <= ROT_TOL and tr <= TRANS_TOL, (k, rot, tr, sh["stats"]["numIterations"][k].tolist(), r["its"])
        worst = (max(worst[0], rot), max(worst[1], tr))
        levels = r["trace"][:, 67].astype(int)
        for l in range(LEVELS - 1, -1, -1):
            i = int(np.flatnonzero(levels == l)[0])
            rec = r["trace"][i]
            a = ctx.linearize(k, 2 * k, 2 * k + 1, l, rec[:16].reshape(4, 4), reset_scale=True)
            assert a["num_valid"] == int(rec[60]) and a["sigma"] == rec[59], (k, l, a["num_valid"], rec[60], a["sigma"], rec[59])
    its_h = sh["stats"]["numIterations"][sh["picks"]]
    st_h = sh["stats"]["status"][sh["picks"]]
    its_o = np.array([r["its"] for r in sh["ref"]])
    st_o = np.array([r["status"] for r in sh["ref"]])
    mean_h, mean_o = its_h.mean(axis=0), its_o.mean(axis=0)
    for mh, mo in zip(mean_h, mean_o):
        assert abs(mh - mo) <= 0.25 * max(mh, mo) + 2.0, (mean_h, mean_o)
    assert abs((st_h == capi.STATUS_MAX_ITERATIONS).mean() - (st_o == capi.STATUS_MAX_ITERATIONS).mean()) <= 0.25
    assert its_h.min() >= 0 and its_h.max() <= 50
    print(f"\nlayered config-5 shard: worst pose disagreement over {len(sh['picks'])} pairs {worst[0]:.2e} rad {worst[1]:.2e} m; "
          f"mean iterations hip {mean_h.round(2).tolist()} oracle {mean_o.round(2).tolist()}; diagnostics", json.dumps(sh["diag"]))


def test_layered_shard_scheduling_is_bit_identical(hip, layered_shard):
    """the default (team kernel), team = 0 and persistent = 0 give the same poses and statistics over all 128 pairs"""
    sh = layered_shard
    batch = sh["batch"]
    for key in ("team", "persistent"):
        ctx = hip.create(batch["K"], batch["b"], ROWS, COLS, make_params(hip, **sh["kw"]), n_frames=2 * SHARD, n_pairs=SHARD)
        ctx.set_option(key, 0)
        poses, stats = ctx.batch_run(batch["images"], batch["disparities"])
        ctx.close()
        assert np.array_equal(poses.view(np.uint32), sh["poses"].view(np.uint32)), key
        assert np.array_equal(stats["numIterations"], sh["stats"]["numIterations"]) and np.array_equal(stats["status"], sh["stats"]["status"]), key
    assert sh["diag"]["team_launches"] >= 1, "the default run should take the team kernel"


def test_layered_shard_slice_in_reference_order(hip, orc, layered_shard):
    """reference_reduction = 1 on an 8-pair slice: every pair's pose, iterations and status are the oracle's"""
    sh = layered_shard
    n = 8
    sl = dict(K=sh["batch"]["K"], b=sh["batch"]["b"], images=sh["batch"]["images"][: 2 * n], disparities=sh["batch"]["disparities"][: 2 * n])
    ctx = hip.create(sl["K"], sl["b"], ROWS, COLS, make_params(hip, **sh["kw"]), n_frames=2 * n, n_pairs=n)
    ctx.set_option("reference_reduction", 1)
    poses, stats = ctx.batch_run(sl["images"], sl["disparities"])
    ctx.close()
    ref = oracle_pairs(orc, sl, list(range(n)), sh["kw"])
    for k, r in enumerate(ref):
        assert bits_equal(poses[k], r["T"]), (k, poses[k], r["T"])
        assert stats["numIterations"][k].tolist() == r["its"] and stats["status"][k].tolist() == r["status"], (k, stats["numIterations"][k], r["its"])


# ---- disparity edge values ----------------------------------------------------------------------------------------------------------
F32 = np.float32
EDGE_VALUES = [("0", F32(0.0)), ("-0", F32(-0.0)), ("-1", F32(-1.0)), ("nan", F32(np.nan)), ("+inf", F32(np.inf)), ("-inf", F32(-np.inf)),
               ("subnormal", F32(1e-40)), ("0.001f", F32(0.001)), ("below-0.001f", np.nextafter(F32(0.001), F32(0))),
               ("512", F32(512.0)), ("above-512", np.nextafter(F32(512.0), F32(np.inf))), ("1e30", F32(1e30))]


def test_layered_disparity_edge_values_select_like_the_oracle(hip, orc):
    """The holes of a layered 1241x376 dispA filled with each edge value in turn: the selection, N and the points equal the oracle's
    through the single-pair path, batch_run and add_frame."""
    rows, cols, levels = 376, 1241, 4
    d = synth.make_pair(rows, cols, INDEX, scene="layered")
    holes = ~((d["dispA"] >= F32(0.001)) & (d["dispA"] <= F32(512)))
    kw = dict(descriptor="bitplanes", loss="tukey", levels=levels)
    single = hip.create(d["K"], d["b"], rows, cols, make_params(hip, **kw), n_frames=2, n_pairs=1)
    batch = hip.create(d["K"], d["b"], rows, cols, make_params(hip, **kw), n_frames=4, n_pairs=2)
    oc = orc.create(d["K"], d["b"], rows, cols, make_params(orc, **kw), n_frames=2, n_pairs=1)
    counts = {}
    for name, val in EDGE_VALUES:
        disp = d["dispA"].copy()
        disp[holes] = val
        oc.frame_set_data(0, d["imgA"], disp)
        oc.frame_set_template(0)
        want = [(oc.num_points(0, l), oc.get_point_indices(0, l), oc.get_points(0, l)) for l in range(levels)]
        counts[name] = [w[0] for w in want]
        single.frame_set_data(0, d["imgA"], disp)
        single.frame_set_template(0)
        for l, (n, idx, pts) in enumerate(want):
            assert single.num_points(0, l) == n, (name, "single", l)
            assert np.array_equal(single.get_point_indices(0, l), idx) and bits_equal(single.get_points(0, l), pts), (name, "single", l)
        images = np.stack([d["imgA"], d["imgB"], d["imgA"], d["imgB"]])
        disps = np.stack([disp, d["dispB"], d["dispA"], d["dispB"]])
        batch.batch_run(images, disps)
        for l, (n, idx, pts) in enumerate(want):
            assert batch.num_points(0, l) == n, (name, "batch", l)
            assert np.array_equal(batch.get_point_indices(0, l), idx) and bits_equal(batch.get_points(0, l), pts), (name, "batch", l)
        vh = hip.create(d["K"], d["b"], rows, cols, make_params(hip, **kw), n_frames=3, n_pairs=1)
        vo = orc.create(d["K"], d["b"], rows, cols, make_params(orc, **kw), n_frames=3, n_pairs=1)
        vh.add_frame(d["imgA"], disp)
        vo.add_frame(d["imgA"], disp)
        assert vh.vo_num_points_at_level() == vo.vo_num_points_at_level(), name
        ph, po = vh.vo_points_at_level(), vo.vo_points_at_level()
        assert bits_equal(ph, po), (name, "add_frame")
        vh.close()
        vo.close()
    # the values outside [0.001f, 512] all select the same points; 0.001f and 512 themselves are valid and select more
    inside = {"0.001f", "512"}
    outside = [v for k, v in counts.items() if k not in inside]
    assert all(v == outside[0] for v in outside), counts
    assert counts["0.001f"][0] > outside[0][0] and counts["512"][0] > outside[0][0], counts
    single.close()
    batch.close()
    oc.close()


# ---- visual odometry on a layered sequence --------------------------------------------------------------------------------------------
VO_ROWS, VO_COLS, VO_FRAMES, VO_INDEX = 480, 640, 12, 1
VO_KW = dict(descriptor="intensity", loss="huber", levels=4, minTranslationMagToKeyFrame=10.0, minRotationMagToKeyFrame=100.0,
             maxFractionOfGoodPointsToKeyFrame=0.9, goodPointThreshold=0.8)     # key frames from the fraction of good points alone


def _vo_sequence(index=VO_INDEX):
    return synth.make_sequence(VO_ROWS, VO_COLS, VO_FRAMES, index=index, step_rot=0.006, step_trans=0.05, scene="layered")


def _run_vo(b, seq, mode=None, options=()):
    ctx = b.create(seq["K"], seq["b"], VO_ROWS, VO_COLS, make_params(b, **VO_KW), n_frames=3, n_pairs=1)
    if mode == "reference-order":
        ctx.set_option("reference_reduction", 1)
    for k, v in options:
        ctx.set_option(k, v)
    out, clouds, counts = [], [], []
    for img, disp in seq["frames"]:
        out.append(ctx.add_frame(img, disp))
        counts.append(ctx.vo_num_points_at_level())
        if out[-1]["hasPointCloud"]:
            clouds.append(ctx.get_point_cloud())
    traj = ctx.trajectory()
    ctx.close()
    return dict(out=out, clouds=clouds, counts=counts, traj=traj)


@pytest.fixture(scope="module")
def vo_oracle(orc):
    seq = _vo_sequence()
    return seq, _run_vo(orc, seq)


@pytest.mark.parametrize("mode", ["fast", "reference-order"])
def test_layered_vo_sequence(hip, vo_oracle, mode):
    """addFrame over a 12-frame layered sequence whose key frames come from the fraction of good points (occlusion): key-frame decisions
    and reasons equal; in reference order also the poses, statistics, point clouds, point counts and trajectory bit for bit; in the default
    mode poses within the bar."""
    seq, ro = vo_oracle
    rh = _run_vo(hip, seq, mode)
    oh, oo = rh["out"], ro["out"]
    assert [r["isKeyFrame"] for r in oh] == [r["isKeyFrame"] for r in oo]
    assert [r["keyFramingReason"] for r in oh] == [r["keyFramingReason"] for r in oo]
    assert any(r["isKeyFrame"] for r in oo[1:]) and all(r["keyFramingReason"] in (capi.KF_SMALL_FRAC_GOOD, capi.KF_NO_KEYFRAMING) for r in oo[1:])
    assert rh["counts"] == ro["counts"]
    for k, (a, b) in enumerate(zip(oh, oo)):
        rot, trans = pose_error(a["pose"], b["pose"])
        assert rot <= ROT_TOL and trans <= TRANS_TOL, (k, rot, trans)
        if mode == "reference-order":
            assert bits_equal(a["pose"], b["pose"]) and a["stats"] == b["stats"], (k, a["stats"], b["stats"])
    assert len(rh["clouds"]) == len(ro["clouds"]) >= 2
    for (ph, Ph), (po, Po) in zip(rh["clouds"], ro["clouds"]):
        assert np.array_equal(ph["xyzw"], po["xyzw"]) and np.array_equal(ph["rgba"], po["rgba"])
        if mode == "reference-order":
            assert bits_equal(ph["weight"], po["weight"]) and bits_equal(Ph, Po)
    if mode == "reference-order":
        assert bits_equal(rh["traj"], ro["traj"])
    else:
        assert np.abs(rh["traj"] - ro["traj"]).max() < 5e-3


def test_layered_vo_late_disparity_upload_and_add_frames(hip):
    """vo_disparity_late 0 / 1 give the same results bit for bit; add_frames over 4 layered sequences equals 4 single contexts"""
    seqs = [_vo_sequence(VO_INDEX + s) for s in range(4)]
    runs = {}
    for late in (0, 1):
        runs[late] = _run_vo(hip, seqs[0], options=[("vo_disparity_late", late)])
    a, b = runs[0], runs[1]
    for x, y in zip(a["out"], b["out"]):
        assert bits_equal(x["pose"], y["pose"]) and x["stats"] == y["stats"] and x["isKeyFrame"] == y["isKeyFrame"]
    assert a["counts"] == b["counts"] and bits_equal(a["traj"], b["traj"])
    singles = [runs[0]] + [_run_vo(hip, s) for s in seqs[1:]]
    ctx = hip.create(seqs[0]["K"], seqs[0]["b"], VO_ROWS, VO_COLS, make_params(hip, **VO_KW), n_frames=3 * 4, n_pairs=4)
    for f in range(VO_FRAMES):
        res = ctx.add_frames(np.stack([s["frames"][f][0] for s in seqs]), np.stack([s["frames"][f][1] for s in seqs]))
        for s in range(4):
            want = singles[s]["out"][f]
            assert bits_equal(res[s]["pose"], want["pose"]) and res[s]["stats"] == want["stats"], (s, f)
            assert res[s]["isKeyFrame"] == want["isKeyFrame"] and res[s]["keyFramingReason"] == want["keyFramingReason"], (s, f)
            assert ctx.seq_num_points_at_level(s) == singles[s]["counts"][f], (s, f)
    for s in range(4):
        assert bits_equal(ctx.seq_trajectory(s), singles[s]["traj"]), s
    ctx.close()


# ---- stereo front-ends --------------------------------------------------------------------------------------------------------------
def _hip_ctx(hip, d, rows, cols):
    p = hip.default_params(); p.numPyramidLevels = 2; p.verbosity = capi.VERB_SILENT
    return hip.create(d["K"], d["b"], rows, cols, p, n_frames=3, n_pairs=1)


@pytest.mark.parametrize("algo,rows,cols,ndisp", [pytest.param("bm", 376, 1241, 128, id="bm-1241x376-ndisp128"),
                                                  pytest.param("bm", 480, 640, 64, id="bm-640x480-ndisp64"),
                                                  pytest.param("sgm", 376, 1241, 128, id="sgm-1241x376-ndisp128"),
                                                  pytest.param("sgm", 480, 640, 64, id="sgm-640x480-ndisp64"),
                                                  pytest.param("sgbm", 376, 1241, 128, id="sgbm-kitti_seq_0-1241x376-ndisp128")])
def test_layered_stereo_bit_exact(hip, orc, algo, rows, cols, ndisp):
    """BM (wsz 15), SGM (its defaults) and SGBM (conf/kitti_seq_0.cfg: wsz 7) against the oracle on layered stereo pairs: depth
    discontinuities, occluded strips, noise on the right image, disparities up to 96 px (1241x376) / 30 px (640x480)."""
    import test_stereo as ts
    d = synth.make_stereo_pair(rows, cols, INDEX, scene="layered")
    assert d["disp"].max() < ndisp and d["occluded"].mean() > 0.005
    left, right = d["left"], d["right"]
    ctx = _hip_ctx(hip, d, rows, cols)
    if algo == "bm":
        sp = ctx.default_stereo_params(ndisp)
        sp.SADWindowSize = 15
        sp.minDisparity = 0
        want = ts.orc_bm(orc, left, right, wsz=15, ndisp=ndisp, mind=0)
    elif algo == "sgm":
        sp = ts._sgm_params(ctx, ndisp=ndisp)
        want = ts.orc_sgm(orc, left, right, ndisp=ndisp)
    else:
        sp = ts._hip_sgbm_params(ctx, ndisp=ndisp, wsz=7)
        want = ts.orc_sgbm(orc, left, right, ndisp=ndisp, wsz=7)
    got = ctx.stereo_bm(left, right, sp)
    ctx.close()
    assert want is not None
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (np.argwhere(got != want)[:8], got[got != want][:8], want[got != want][:8])
    inv = 0 if algo == "sgm" else -1
    assert (got == inv).any() and (got > max(inv, 0)).mean() > 0.3
