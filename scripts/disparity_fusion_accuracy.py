#!/usr/bin/env python3
"""Where disparity fusion helps and where it does not (c_api.h "disparity fusion"), on one GPU.  Written to profiles/disparity_fusion_accuracy.json and
printed, every row, the ones where fusion loses included; a record, not a bar.

  noise    synth.make_sequence, plane and layered, at 120x160, 240x320 and 640x480, 8 frames, key frames from the translation (0.035 m); seeded
           Gaussian noise of sigma = 0, 0.25, 0.5 and 1.0 px on the valid measured disparities (the maps synth renders are the truth).
  stereo   synth.make_stereo_sequence (plane) at 240x320 through block matching and SGM (bpvo_hip_add_frames_stereo); the truth is synth's map.
Each against three settings: mode 0; mode 1 with max_fill_sigma = 0 (never fill); mode 1 with max_fill_sigma = 2.  measurement_sigma =
max(sigma, 1/16) (stereo: 1/16 — block matching's quantum), process_sigma 0.1, gate 3.  Per frame: the translation error of the accumulated pose to
the truth (m); the RMS error of the frame's gated disparities, as the template stage would read them (the slot's map), against the truth (px); the
template points at the finest level.  Expected losers: depth edges smeared by the nearest-pixel splat (layered), and a lost pose poisoning the
carried map."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OUT = os.path.join(ROOT, "profiles", "disparity_fusion_accuracy.json")
SIZES = ((120, 160), (240, 320), (480, 640))
SIGMAS = (0.0, 0.25, 0.5, 1.0)
FRAMES = 8
SETTINGS = (("mode0", None), ("mode1_nofill", 0.0), ("mode1_fill2", 2.0))


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


def gated_rms(D, truth, p):
    with np.errstate(invalid="ignore"):
        ok = (D >= p.minValidDisparity) & (D <= p.maxValidDisparity) & (truth >= p.minValidDisparity) & (truth <= p.maxValidDisparity)
    if not ok.any():
        return None, 0
    return float(np.sqrt(np.mean((D[ok].astype(np.float64) - truth[ok]) ** 2))), int(ok.sum())


def run(hip, capi, seq, p, sigma_m, fill, measured=None, stereo=None):
    """One sequence through add_frames (sequence 0 of a one-sequence context): the per-frame rows."""
    rows, cols = seq["frames"][0][0].shape
    ctx = hip.create(seq["K"], seq["b"], rows, cols, p, n_frames=3, n_pairs=1)
    if fill is not None:
        ctx.set_disparity_fusion(dict(mode=1, measurement_sigma=max(sigma_m, 1.0 / 16.0), process_sigma=0.1, gate=3.0, max_fill_sigma=fill))
    out = []
    W = np.eye(4)
    truth_maps = seq["disps"] if stereo is not None else [f[1] for f in seq["frames"]]
    for f in range(len(seq["frames"])):
        if stereo is not None:
            r = ctx.add_frames_stereo([seq["frames"][f][0]], [seq["frames"][f][1]], stereo)[0]
        else:
            r = ctx.add_frames([seq["frames"][f][0]], [measured[f]])[0]
        if fill is not None:
            D = ctx.get_disparity(ctx.seq_disparity_fusion_info(0)["slot"])
        elif stereo is not None:
            D = ctx.stereo_frames([(rows, cols)], [seq["frames"][f][0]], [seq["frames"][f][1]], stereo)[0]
        else:
            D = measured[f]
        W = np.asarray(r["pose"], np.float64) @ W if f else W
        terr = float(np.linalg.norm(W[:3, 3] - np.asarray(seq["poses"][f], np.float64)[:3, 3]))
        rms, n = gated_rms(np.asarray(D, np.float32), np.asarray(truth_maps[f], np.float32), p)
        out.append(dict(frame=f, key_frame=bool(r["isKeyFrame"]), translation_error_m=round(terr, 6), gated_rms_px=None if rms is None else round(rms, 4),
                        gated_pixels=n, points_finest=ctx.seq_num_points_at_level(0)))
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    import bpvo_amd
    from bpvo_amd import capi, synth
    hip = bpvo_amd.load()
    p = params(hip, capi)
    rows_out = []
    for scene in ("plane", "layered"):
        for rows, cols in SIZES:
            seq = synth.make_sequence(rows, cols, FRAMES, index=2, scene=scene)
            for sigma in SIGMAS:
                rng = np.random.default_rng(77)
                measured = []
                for _, d in seq["frames"]:
                    m = np.array(d, np.float32)
                    with np.errstate(invalid="ignore"):
                        ok = (m >= p.minValidDisparity) & (m <= p.maxValidDisparity)
                    m[ok] += rng.normal(0.0, sigma, int(ok.sum())).astype(np.float32) if sigma > 0 else 0.0
                    measured.append(m)
                for name, fill in SETTINGS:
                    frames = run(hip, capi, seq, p, sigma, fill, measured=measured)
                    row = dict(kind="noise", scene=scene, rows=rows, cols=cols, sigma=sigma, setting=name, frames=frames)
                    rows_out.append(row)
                    print(scene, rows, cols, sigma, name, "terr_last %.5f" % frames[-1]["translation_error_m"],
                          "rms", [fr["gated_rms_px"] for fr in frames], "pts", [fr["points_finest"] for fr in frames], flush=True)
    seq = synth.make_stereo_sequence(240, 320, FRAMES, index=2)
    for algo, algo_name in ((capi.STEREO_BM, "block_matching"), (capi.STEREO_SGM, "sgm")):
        ctx = hip.create(seq["K"], seq["b"], 240, 320, p, n_frames=3, n_pairs=1)
        sp = ctx.default_stereo_params(ndisp=64)
        sp.algorithm = algo
        ctx.close()
        for name, fill in SETTINGS:
            try:
                frames = run(hip, capi, seq, p, 1.0 / 16.0, fill, stereo=sp)
            except capi.BpvoError as e:      # (kept in the record: a run that ended is a row, too)
                rows_out.append(dict(kind="stereo", matcher=algo_name, rows=240, cols=320, setting=name, error=str(e)))
                print("stereo", algo_name, name, "error", e, flush=True)
                continue
            rows_out.append(dict(kind="stereo", matcher=algo_name, rows=240, cols=320, setting=name, frames=frames))
            print("stereo", algo_name, name, "terr_last %.5f" % frames[-1]["translation_error_m"], "rms", [fr["gated_rms_px"] for fr in frames],
                  "pts", [fr["points_finest"] for fr in frames], flush=True)
    with open(a.out, "w") as f:
        json.dump(dict(frames=FRAMES, settings=[s[0] for s in SETTINGS], rows=rows_out), f, indent=0)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
