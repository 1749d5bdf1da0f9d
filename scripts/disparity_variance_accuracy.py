#!/usr/bin/env python3
"""What the per-pixel measurement variance does to the disparity filter (c_api.h "measurement variance"), on one GPU: the table of
scripts/disparity_fusion_accuracy.py with one more column.  Written to profiles/disparity_variance_accuracy.json and printed, every row, the ones
where the feature loses included; a record, not a bar.

  stereo   synth.make_stereo_sequence (plane) at 240x320 through block matching and SGM (bpvo_hip_add_frames_stereo), 8 frames, key frames from
           the translation (0.035 m); the truth is synth's map.  Settings: fusion off; fusion with the constant measurement_sigma = 1/16 (block
           matching's quantum), max_fill_sigma 0 and 2; the same two with the per-pixel variance on.
  noise    the variance needs the rectified pair, which only the stereo sequence of the plane scene has (the layered scene's sequences are
           rendered without a right image): synth.make_stereo_sequence at 120x160, 240x320 and 640x480, the true disparities plus seeded Gaussian
           noise of sigma = 0, 0.25, 0.5 and 1.0 px as the measured maps, the true frame-to-frame motions, through the filter alone:
           bpvo_hip_fuse_disparities (constant: max(sigma, 1/16)) against bpvo_hip_fuse_disparities_var with the maps of
           bpvo_hip_disparity_variance_frames.  No pose is estimated in these rows.
The variance setting: radius 2, noise_sigma 2 grey levels, min_sigma 0.02, max_sigma 2 px; process_sigma 0.1, gate 3.  Per row: the RMS error of the
gated fused disparities against the truth after every frame (px), and the shares of the six classes of the variance maps over the run."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OUT = os.path.join(ROOT, "profiles", "disparity_variance_accuracy.json")
SIZES = ((120, 160), (240, 320), (480, 640))
SIGMAS = (0.0, 0.25, 0.5, 1.0)
FRAMES = 8
VARIANCE = dict(mode=1, radius=2, noise_sigma=2.0, min_sigma=0.02, max_sigma=2.0)
CLASSES = ("invalid", "border", "flat", "floor", "ceiling", "model")
# (name, max_fill_sigma or None for fusion off, per-pixel variance)
SETTINGS = (("mode0", None, False), ("constant_nofill", 0.0, False), ("constant_fill2", 2.0, False), ("variance_nofill", 0.0, True),
            ("variance_fill2", 2.0, True))


def params(hip, capi):
    p = hip.default_params()
    p.numPyramidLevels = 3
    p.descriptor = capi.DESC_BITPLANES
    p.lossFunction = capi.LOSS_HUBER
    p.verbosity = capi.VERB_SILENT
    p.minTranslationMagToKeyFrame = 0.035
    p.minRotationMagToKeyFrame = 100.0
    p.maxFractionOfGoodPointsToKeyFrame = 0.0
    return p


def fusion(sigma_m, fill):
    return dict(mode=1, measurement_sigma=max(sigma_m, 1.0 / 16.0), process_sigma=0.1, gate=3.0, max_fill_sigma=fill)


def gated_rms(D, truth, p):
    with np.errstate(invalid="ignore"):
        ok = (D >= p.minValidDisparity) & (D <= p.maxValidDisparity) & (truth >= p.minValidDisparity) & (truth <= p.maxValidDisparity)
    if not ok.any():
        return None, 0
    return float(np.sqrt(np.mean((D[ok].astype(np.float64) - truth[ok]) ** 2))), int(ok.sum())


def shares(total):
    n = sum(total.values())
    return {k: round(total[k] / n, 4) for k in CLASSES} if n else None


def sigma_summary(maps):
    """The model's own values (the clamped classes left out): quartiles of sigma = sqrt(R2), px."""
    v = np.concatenate([m[(m > VARIANCE["min_sigma"] ** 2 * 1.0001) & (m < VARIANCE["max_sigma"] ** 2 * 0.9999)].reshape(-1) for m in maps]) if maps else np.zeros(0)
    if v.size == 0:
        return None
    q = np.sqrt(np.percentile(v.astype(np.float64), [10, 50, 90]))
    return dict(p10=round(float(q[0]), 4), median=round(float(q[1]), 4), p90=round(float(q[2]), 4))


def run_stereo(hip, seq, p, fill, variance, sp):
    rows, cols = seq["frames"][0][0].shape
    ctx = hip.create(seq["K"], seq["b"], rows, cols, p, n_frames=3, n_pairs=1)
    if fill is not None:
        ctx.set_disparity_fusion(fusion(1.0 / 16.0, fill))
    if variance:
        ctx.set_measurement_variance(VARIANCE)
    out, total, maps = [], {k: 0 for k in CLASSES}, []
    W = np.eye(4)
    for f, (left, right) in enumerate(seq["frames"]):
        r = ctx.add_frames_stereo([left], [right], sp)[0]
        if fill is not None:
            D = ctx.get_disparity(ctx.seq_disparity_fusion_info(0)["slot"])
        else:
            D = ctx.stereo_frames([(rows, cols)], [left], [right], sp)[0]
        if variance:
            info = ctx.seq_measurement_variance_info(0)
            for k in CLASSES:
                total[k] += info[k]
            maps.append(ctx.seq_get_measurement_variance_map(0))
        W = np.asarray(r["pose"], np.float64) @ W if f else W
        terr = float(np.linalg.norm(W[:3, 3] - np.asarray(seq["poses"][f], np.float64)[:3, 3]))
        rms, n = gated_rms(np.asarray(D, np.float32), np.asarray(seq["disps"][f], np.float32), p)
        out.append(dict(frame=f, key_frame=bool(r["isKeyFrame"]), translation_error_m=round(terr, 6), gated_rms_px=None if rms is None else round(rms, 4),
                        gated_pixels=n, points_finest=ctx.seq_num_points_at_level(0)))
    ctx.close()
    return out, shares(total), sigma_summary(maps)


def run_filter(hip, seq, p, sigma, measured, fill, variance):
    """The filter alone on the noisy maps with the true motions."""
    rows, cols = measured[0].shape
    ctx = hip.create(seq["K"], seq["b"], rows, cols, p, n_frames=3, n_pairs=1)
    ctx.set_disparity_fusion(fusion(sigma, fill))
    out, total, maps = [], {k: 0 for k in CLASSES}, []
    for f, (left, right) in enumerate(seq["frames"]):
        P = np.eye(4) if f == 0 else np.asarray(seq["poses"][f], np.float64) @ np.linalg.inv(np.asarray(seq["poses"][f - 1], np.float64))
        if variance:
            R2, counts = ctx.disparity_variance_frames([left], [right], [measured[f]], p.minValidDisparity, p.maxValidDisparity, VARIANCE)
            for k in CLASSES:
                total[k] += counts[0][k]
            maps.append(R2[0])
            ctx.fuse_disparities_var([measured[f]], [R2[0]], [P.astype(np.float32)], seq=[0])
        else:
            ctx.fuse_disparities([measured[f]], [P.astype(np.float32)], seq=[0])
        D, _ = ctx.seq_get_fused_disparity(0)
        rms, n = gated_rms(D, np.asarray(seq["disps"][f], np.float32), p)
        out.append(dict(frame=f, gated_rms_px=None if rms is None else round(rms, 4), gated_pixels=n))
    ctx.close()
    return out, shares(total), sigma_summary(maps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    import bpvo_amd
    from bpvo_amd import capi, synth
    hip = bpvo_amd.load()
    p = params(hip, capi)
    rows_out = []
    seq = synth.make_stereo_sequence(240, 320, FRAMES, index=2)
    for algo, algo_name in ((capi.STEREO_BM, "block_matching"), (capi.STEREO_SGM, "sgm")):
        ctx = hip.create(seq["K"], seq["b"], 240, 320, p, n_frames=3, n_pairs=1)
        sp = ctx.default_stereo_params(ndisp=64)
        sp.algorithm = algo
        ctx.close()
        for name, fill, variance in SETTINGS:
            try:
                frames, share, sig = run_stereo(hip, seq, p, fill, variance, sp)
            except capi.BpvoError as e:      # (kept in the record: a run that ended is a row, too)
                rows_out.append(dict(kind="stereo", matcher=algo_name, rows=240, cols=320, setting=name, error=str(e)))
                print("stereo", algo_name, name, "error", e, flush=True)
                continue
            rows_out.append(dict(kind="stereo", matcher=algo_name, rows=240, cols=320, setting=name, frames=frames, class_shares=share, model_sigma_px=sig))
            print("stereo", algo_name, name, "terr_last %.5f" % frames[-1]["translation_error_m"], "rms", [fr["gated_rms_px"] for fr in frames],
                  "shares", share, "sigma", sig, flush=True)
    for rows, cols in SIZES:
        seq = synth.make_stereo_sequence(rows, cols, FRAMES, index=2)
        for sigma in SIGMAS:
            rng = np.random.default_rng(77)
            measured = []
            for d in seq["disps"]:
                m = np.array(d, np.float32)
                with np.errstate(invalid="ignore"):
                    ok = (m >= p.minValidDisparity) & (m <= p.maxValidDisparity)
                m[ok] += rng.normal(0.0, sigma, int(ok.sum())).astype(np.float32) if sigma > 0 else 0.0
                measured.append(m)
            raw, _ = gated_rms(measured[-1], np.asarray(seq["disps"][-1], np.float32), p)
            for name, fill, variance in SETTINGS[1:]:
                frames, share, sig = run_filter(hip, seq, p, sigma, measured, fill, variance)
                rows_out.append(dict(kind="noise", scene="plane", rows=rows, cols=cols, sigma=sigma, setting=name, measured_rms_px=round(raw, 4), frames=frames,
                                     class_shares=share, model_sigma_px=sig))
                print("noise", rows, cols, sigma, name, "measured %.4f" % raw, "rms", [fr["gated_rms_px"] for fr in frames], "shares", share, "sigma", sig,
                      flush=True)
    with open(a.out, "w") as f:
        json.dump(dict(frames=FRAMES, settings=[s[0] for s in SETTINGS], variance=VARIANCE, process_sigma=0.1, gate=3.0,
                       measurement_sigma="max(sigma, 1/16); stereo rows: 1/16", rows=rows_out), f, indent=0)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
