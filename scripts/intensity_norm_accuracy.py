#!/usr/bin/env python3
"""What the normalised intensity is for (c_api.h bpvo_hip_set_intensity_normalization), on one GPU: the final translation and rotation error to the
truth of bpvo_hip_estimate_pose — Intensity, Huber, three levels, Identity start, synth.make_pair index 0 — when the CURRENT frame has another
exposure than the template, with plain Intensity and with radius 0 (whole image), 7 and 15 (local).  Written to
profiles/intensity_norm_accuracy.json and printed; a record, not a bar.

  scenes    plane and layered, at 240x320 and 640x480; and the plane at 120x160, the case of tests/test_gpu_intensity_norm.py
  exposure  unchanged; B // 2 + 10; rint(0.7 B + 30); a vignette 1 - 0.3 r^2 (r: distance from the image centre over the half diagonal); a gain
            ramp 0.6 -> 1.2 across the columns; the last two rounded to nearest and clipped to 0 .. 255
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

OUT = os.path.join(ROOT, "profiles", "intensity_norm_accuracy.json")
CASES = [("plane", 120, 160), ("plane", 240, 320), ("layered", 240, 320), ("plane", 480, 640), ("layered", 480, 640)]
MODES = (-1, 0, 7, 15)


def u8(x):
    return np.clip(np.rint(x), 0, 255).astype(np.uint8)


def exposures(B):
    rows, cols = B.shape
    y, x = np.mgrid[0:rows, 0:cols].astype(np.float64)
    r2 = ((x - (cols - 1) / 2.0) ** 2 + (y - (rows - 1) / 2.0) ** 2) / (((cols - 1) / 2.0) ** 2 + ((rows - 1) / 2.0) ** 2)
    f = B.astype(np.float64)
    return {"unchanged": B, "B//2+10": (B // 2 + 10).astype(np.uint8), "rint(0.7B+30)": u8(0.7 * f + 30.0), "vignette_1-0.3r2": u8(f * (1.0 - 0.3 * r2)),
            "ramp_0.6_to_1.2": u8(f * np.linspace(0.6, 1.2, cols)[None, :])}


def main():
    import torch
    if not torch.cuda.is_available():
        sys.exit("intensity_norm_accuracy: no GPU (a measurement does not fall back)")
    torch.cuda.init()
    import bpvo_amd
    from bpvo_amd import synth
    from util import make_params, pose_error
    hip = bpvo_amd.load()
    rows_out = []
    for scene, rows, cols in CASES:
        d = synth.make_pair(rows, cols, 0, scene=scene)
        for name, imgB in exposures(d["imgB"]).items():
            rec = dict(scene=scene, size=f"{cols}x{rows}", exposure=name)
            for mode in MODES:
                ctx = hip.create(d["K"], d["b"], rows, cols, make_params(hip, descriptor="intensity", loss="huber", levels=3), n_frames=2, n_pairs=1)
                ctx.set_intensity_normalization(mode)
                ctx.frame_set_data(0, d["imgA"], d["dispA"])
                ctx.frame_set_template(0)
                ctx.frame_set_data(1, imgB, d["dispB"])
                T, st = ctx.estimate_pose(0, 0, 1)
                ctx.close()
                er, et = pose_error(T, d["T_gt"])
                rec["plain" if mode < 0 else f"radius_{mode}"] = dict(translation_m=float(f"{et:.4g}"), rotation_rad=float(f"{er:.4g}"),
                                                                      iterations=[int(s["numIterations"]) for s in st])
            rows_out.append(rec)
            print(rec, flush=True)
    out = dict(what="normalised intensity, pose error to the truth: scripts/intensity_norm_accuracy.py", device=torch.cuda.get_device_name(0),
               settings="Intensity, Huber, numPyramidLevels 3, Identity start, synth.make_pair index 0; the current frame's exposure changed", results=rows_out)
    json.dump(out, open(OUT, "w"), indent=1)


if __name__ == "__main__":
    main()
