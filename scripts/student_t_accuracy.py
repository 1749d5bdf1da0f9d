#!/usr/bin/env python3
"""Final error to T_gt of the four losses (Huber, Tukey, L2, Student-t) on synthetic pairs: plane and layered scenes, with and without a pasted
occluder (the middle quarter of the current frame replaced by another scene's texture), intensity and bit-planes, 240x320 and 640x480, four
levels, from the Identity.  The table is reported as it comes out, the rows where the new loss loses included.

  python scripts/student_t_accuracy.py --out profiles/student_t_accuracy.json
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bpvo_amd  # noqa: E402
from bpvo_amd import capi, synth  # noqa: E402

LOSSES = {"huber": capi.LOSS_HUBER, "tukey": capi.LOSS_TUKEY, "l2": capi.LOSS_L2, "student_t": capi.LOSS_STUDENT_T}
DESCRIPTORS = {"intensity": capi.DESC_INTENSITY, "bitplanes": capi.DESC_BITPLANES}
SIZES = [(240, 320), (640 * 3 // 4, 640)]
INDEX, FOREIGN, LEVELS = 0, 11, 4


def errors(T, T_gt):
    T, T_gt = np.asarray(T, np.float64), np.asarray(T_gt, np.float64)
    E = T[:3, :3].T @ T_gt[:3, :3]
    w = 0.5 * np.array([E[2, 1] - E[1, 2], E[0, 2] - E[2, 0], E[1, 0] - E[0, 1]])
    return float(np.arcsin(min(1.0, np.linalg.norm(w)))), float(np.linalg.norm(T[:3, 3] - T_gt[:3, 3]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    hip = bpvo_amd.load()
    rows_out = []
    for rows, cols in SIZES:
        for scene in ("plane", "layered"):
            d = synth.make_pair(rows, cols, INDEX, scene=scene)
            foreign = synth.make_pair(rows, cols, FOREIGN)["imgB"]
            for occluder in (False, True):
                imgB = d["imgB"].copy()
                if occluder:
                    imgB[rows // 4: 3 * rows // 4, cols // 4: 3 * cols // 4] = foreign[rows // 4: 3 * rows // 4, cols // 4: 3 * cols // 4]
                for descriptor, dv in DESCRIPTORS.items():
                    row = dict(rows=rows, cols=cols, scene=scene, occluder=occluder, descriptor=descriptor)
                    for loss, lv in LOSSES.items():
                        p = hip.default_params()
                        p.verbosity, p.numPyramidLevels, p.descriptor, p.lossFunction = capi.VERB_SILENT, LEVELS, dv, lv
                        ctx = hip.create(d["K"], d["b"], rows, cols, p, n_frames=2, n_pairs=1)
                        ctx.frame_set_data(0, d["imgA"], d["dispA"])
                        ctx.frame_set_template(0)
                        ctx.frame_set_data(1, imgB, d["dispB"])
                        T, stats = ctx.estimate_pose(0, 0, 1)
                        rot, trans = errors(T, d["T_gt"])
                        row[loss] = dict(rot_rad=float("%.3g" % rot), trans_m=float("%.3g" % trans), iterations=[s["numIterations"] for s in stats],
                                         status=[s["status"] for s in stats])
                        ctx.close()
                    best = min(LOSSES, key=lambda l: row[l]["trans_m"])
                    row["best_translation"] = best
                    rows_out.append(row)
                    print(json.dumps(row), flush=True)
    res = dict(levels=LEVELS, index=INDEX, start="identity", rows=rows_out)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
