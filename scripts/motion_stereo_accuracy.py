#!/usr/bin/env python3
"""What motion stereo does to the disparity filter and to the VO (c_api.h "motion stereo"), on one GPU.  Written to
profiles/motion_stereo_accuracy.json and printed, every row, the ones where the feature loses included; a record, not a bar.  The poses are the
library's own estimates in every row but the first.

  rule     the rule alone (bpvo_hip_motion_stereo_frames) on synth's plane pair at 48x64 under a sideways step of 0.2 m (a gain of 2 pixels per
           disparity pixel), exact motion, the prior the truth + 0.4 px with variance 0.25: the share of fused pixels and the RMS error of the
           prior and of the result over them — the case of tests/test_motion_stereo_cpu.py, on the device.
  noise    synth.make_sequence, plane and layered, 240x320, 8 frames, the true disparities plus seeded Gaussian noise of sigma 0.25 / 0.5 / 1 px
           as the measured maps, through bpvo_hip_add_frames: fusion alone against fusion with motion stereo, and no fusion for scale.  Two
           trajectories: synth's own steps (up to 0.03 m a frame: under a pixel of parallax per frame at this size, key frames at 0.035 m) and
           wide steps (up to 0.15 m a frame, key frames at 0.3 m).
  stereo   synth.make_stereo_sequence (plane) at 240x320 through block matching with filling (max_fill_sigma 2), both trajectories.
  mono     the wide plane trajectory, 12 frames: true disparities for the first two frames, all-invalid maps (-1) for the other ten, filling
           with max_fill_sigma 4 — per frame the template's point count, the carried variance's percentiles and the translation error.
Per frame: the RMS error of the gated fused disparities against the truth (px), the translation error of the composed poses against the truth
(m), and, with the feature on, the shares of its seven classes."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OUT = os.path.join(ROOT, "profiles", "motion_stereo_accuracy.json")
ROWS, COLS, FRAMES = 240, 320, 8
SIGMAS = (0.25, 0.5, 1.0)
MOTION_STEREO = dict(mode=1, radius=2, steps=2, min_gain=0.25, noise_sigma=2.0, min_sigma=0.02, max_sigma=2.0, gate=3.0)
CLASSES = ("no_prior", "low_parallax", "border", "edge", "flat", "rejected", "fused")
TRAJECTORIES = dict(synth=dict(step_trans=0.03, keyframe_m=0.035), wide=dict(step_trans=0.15, keyframe_m=0.3))
SETTINGS = ("mode0", "fusion", "fusion_motion_stereo")


def params(hip, capi, keyframe_m):
    p = hip.default_params()
    p.numPyramidLevels = 3
    p.descriptor = capi.DESC_BITPLANES
    p.lossFunction = capi.LOSS_HUBER
    p.verbosity = capi.VERB_SILENT
    p.minTranslationMagToKeyFrame = keyframe_m
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


def run(hip, seq, truths, p, setting, fuse, frames, stereo_params=None, measured=None, variance_percentiles=False):
    """One sequence through add_frames (measured[f] with the frames' images) or add_frames_stereo (stereo_params): the per-frame record."""
    rows, cols = seq["frames"][0][0].shape
    ctx = hip.create(seq["K"], seq["b"], rows, cols, p, n_frames=3, n_pairs=1)
    if setting != "mode0":
        ctx.set_disparity_fusion(fuse)
    if setting == "fusion_motion_stereo":
        ctx.set_motion_stereo(MOTION_STEREO)
    out, total = [], {k: 0 for k in CLASSES}
    W = np.eye(4)
    for f in range(frames):
        try:
            if stereo_params is not None:
                left, right = seq["frames"][f]
                r = ctx.add_frames_stereo([left], [right], stereo_params)[0]
            else:
                r = ctx.add_frames([seq["frames"][f][0]], [measured[f]])[0]
        except Exception as e:      # (kept in the record: a run that ended is a row, too)
            out.append(dict(frame=f, error=str(e)))
            break
        if setting != "mode0":
            D, V = ctx.seq_get_fused_disparity(0)
        elif stereo_params is not None:
            D, V = ctx.stereo_frames([(rows, cols)], [seq["frames"][f][0]], [seq["frames"][f][1]], stereo_params)[0], None
        else:
            D, V = measured[f], None
        W = np.asarray(r["pose"], np.float64) @ W if f else W
        terr = float(np.linalg.norm(W[:3, 3] - np.asarray(seq["poses"][f], np.float64)[:3, 3]))
        rms, n = gated_rms(np.asarray(D, np.float32), np.asarray(truths[f], np.float32), p)
        row = dict(frame=f, key_frame=bool(r["isKeyFrame"]), translation_error_m=round(terr, 6), gated_rms_px=None if rms is None else round(rms, 4),
                   gated_pixels=n, points_finest=ctx.seq_num_points_at_level(0, 0))
        if variance_percentiles and V is not None:
            v = V[V >= 0]
            row["carried_sigma_px_p10_p50_p90"] = [round(float(x), 4) for x in np.sqrt(np.percentile(v.astype(np.float64), [10, 50, 90]))] if v.size else None
            row["carried_pixels"] = int(v.size)
        if setting == "fusion_motion_stereo":
            info = ctx.seq_motion_stereo_info(0)
            for k in CLASSES:
                total[k] += info[k]
            row["fused_by_motion_stereo"] = info["fused"]
        out.append(row)
    ctx.close()
    return out, shares(total)


def rule_row(hip, capi, synth):
    rows, cols, tx = 48, 64, 0.2
    seq = synth.make_sequence_steps(rows, cols, [tx], (1.0, 0.0, 0.0), (0.0, 0.0, 0.0))
    (img0, _), (img1, d1) = seq["frames"]
    Q = np.linalg.inv(seq["poses"][1]).astype(np.float32)
    p = hip.default_params()
    p.numPyramidLevels = 1
    p.verbosity = capi.VERB_SILENT
    ctx = hip.create(seq["K"], seq["b"], rows, cols, p, n_frames=3, n_pairs=1)
    ctx.set_motion_stereo(MOTION_STEREO)
    pd = (np.asarray(d1, np.float32) + np.float32(0.4)).astype(np.float32)
    Ds, Vs, Cs = ctx.motion_stereo_frames([(seq["K"], seq["b"], rows, cols)], [img1], [img0], [Q], [pd], [np.full(pd.shape, 0.25, np.float32)])
    ctx.close()
    fused = Cs[0] == 6
    rms = lambda a: float(np.sqrt(np.mean((a[fused].astype(np.float64) - d1[fused]) ** 2)))
    before, after = rms(pd), rms(Ds[0])
    return dict(kind="rule", rows=rows, cols=cols, sideways_m=tx, fused_share=round(float(fused.mean()), 4), prior_rms_px=round(before, 4),
                result_rms_px=round(after, 4), ratio=round(after / before, 4),
                class_shares={k: round(float((Cs[0] == i).mean()), 4) for i, k in enumerate(CLASSES)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    import bpvo_amd
    from bpvo_amd import capi, synth
    hip = bpvo_amd.load()
    rows_out = [rule_row(hip, capi, synth)]
    print(json.dumps(rows_out[0]), flush=True)
    for tname, tr in TRAJECTORIES.items():
        p = params(hip, capi, tr["keyframe_m"])
        for scene in ("plane", "layered"):
            seq = synth.make_sequence(ROWS, COLS, FRAMES, index=2, scene=scene, step_trans=tr["step_trans"])
            truths = [fr[1] for fr in seq["frames"]]
            for sigma in SIGMAS:
                rng = np.random.default_rng(77)
                measured = []
                for d in truths:
                    m = np.array(d, np.float32)
                    with np.errstate(invalid="ignore"):
                        ok = (m >= p.minValidDisparity) & (m <= p.maxValidDisparity)
                    m[ok] += rng.normal(0.0, sigma, int(ok.sum())).astype(np.float32)
                    measured.append(m)
                for setting in SETTINGS:
                    frames, share = run(hip, seq, truths, p, setting, fusion(sigma, 2.0), FRAMES, measured=measured)
                    rows_out.append(dict(kind="noise", trajectory=tname, scene=scene, rows=ROWS, cols=COLS, sigma=sigma, setting=setting, frames=frames,
                                         class_shares=share))
                    print("noise", tname, scene, sigma, setting, "terr_last", frames[-1].get("translation_error_m"), "rms",
                          [fr.get("gated_rms_px") for fr in frames], "shares", share, flush=True)
        seq = synth.make_stereo_sequence(ROWS, COLS, FRAMES, index=2, step_trans=tr["step_trans"])
        ctx = hip.create(seq["K"], seq["b"], ROWS, COLS, p, n_frames=3, n_pairs=1)
        sp = ctx.default_stereo_params(ndisp=64)
        sp.algorithm = capi.STEREO_BM
        ctx.close()
        for setting in SETTINGS:
            frames, share = run(hip, seq, seq["disps"], p, setting, fusion(1.0 / 16.0, 2.0), FRAMES, stereo_params=sp)
            rows_out.append(dict(kind="stereo", matcher="block_matching", trajectory=tname, rows=ROWS, cols=COLS, setting=setting, frames=frames, class_shares=share))
            print("stereo", tname, setting, "terr_last", frames[-1].get("translation_error_m"), "rms", [fr.get("gated_rms_px") for fr in frames], "shares", share,
                  flush=True)
    tr = TRAJECTORIES["wide"]
    p = params(hip, capi, tr["keyframe_m"])
    n_mono = 12
    seq = synth.make_sequence(ROWS, COLS, n_mono, index=2, step_trans=tr["step_trans"])
    truths = [fr[1] for fr in seq["frames"]]
    measured = [np.asarray(truths[f], np.float32) if f < 2 else np.full((ROWS, COLS), -1.0, np.float32) for f in range(n_mono)]
    for setting in SETTINGS[1:]:
        frames, share = run(hip, seq, truths, p, setting, fusion(1.0 / 16.0, 4.0), n_mono, measured=measured, variance_percentiles=True)
        rows_out.append(dict(kind="mono", trajectory="wide", rows=ROWS, cols=COLS, setting=setting, frames=frames, class_shares=share))
        print("mono", setting, json.dumps(frames), "shares", share, flush=True)
    with open(a.out, "w") as f:
        json.dump(dict(frames=FRAMES, settings=list(SETTINGS), motion_stereo=MOTION_STEREO, trajectories=TRAJECTORIES, process_sigma=0.1, gate=3.0,
                       measurement_sigma="max(sigma, 1/16); stereo and mono rows: 1/16",
                       not_measured="real imagery; what a pose error does to the map beyond these runs (the feedback of the map into later estimates over long runs)",
                       rows=rows_out), f, indent=0)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
