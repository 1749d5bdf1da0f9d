#!/usr/bin/env python3
"""Is the reported pose covariance (c_api.h bpvo_hip_pose_covariances) calibrated?  Monte-Carlo on the CPU oracle with the definition evaluated
in float64 (tests/pose_covariance_ref.py): the 96x128 plane pair, 2 pyramid levels, --draws (150) copies of frame B with N(0, 3) grey-level noise
(rounded, clipped to u8, np.random.default_rng(0)); per configuration the per-axis ratio of the empirical standard deviation of the estimated pose
to the mean reported one.  1 = calibrated, above 1 = the report is optimistic.  Needs no GPU.  Writes profiles/pose_covariance_calibration.json
and prints it.  A record: tests/test_pose_covariance_cpu.py asserts the intensity / Huber row, the bit-planes rows are the documented optimism
(INTEGRATION.md section 4).

  python scripts/pose_covariance_calibration.py      (the launcher; this file lives with the other tools that use the CPU checker)
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import __graft_entry__ as ge  # noqa: E402
import pose_covariance_ref as ref  # noqa: E402
from bpvo_amd import capi, synth  # noqa: E402

ROWS, COLS, LEVELS = 96, 128, 2
CONFIGS = (("intensity", "l2"), ("intensity", "huber"), ("intensity", "tukey"), ("bitplanes", "huber"), ("bitplanes", "tukey"))
DESC = {"intensity": capi.DESC_INTENSITY, "bitplanes": capi.DESC_BITPLANES}
LOSS = {"l2": capi.LOSS_L2, "huber": capi.LOSS_HUBER, "tukey": capi.LOSS_TUKEY}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--draws", type=int, default=150)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_covariance_calibration.json"))
    a = ap.parse_args()
    orc = capi.Binding(ge.build_oracle(), "bpvo_orc_")
    d = synth.make_pair(ROWS, COLS, 0)
    out = dict(rows=ROWS, cols=COLS, levels=LEVELS, draws=a.draws, noise_sigma_grey=3.0, seed=0, axes=["wx", "wy", "wz", "vx", "vy", "vz"],
               what="empirical / mean reported standard deviation of the estimated pose per twist axis (oracle + f64 evaluation of the definition)",
               configurations=[])
    for desc, loss in CONFIGS:
        p = orc.default_params()
        p.numPyramidLevels = LEVELS
        p.descriptor = DESC[desc]
        p.lossFunction = LOSS[loss]
        p.verbosity = capi.VERB_SILENT
        ctx = orc.create(d["K"], d["b"], ROWS, COLS, p, device=0, n_frames=2, n_pairs=1)
        ctx.frame_set_data(0, d["imgA"], d["dispA"])
        ctx.frame_set_template(0)

        def cov_of(c, T, loss=loss):
            e = ref.oracle_covariance(c, T, LOSS[loss])
            return e["covariance"], e["status"]
        ratio, bad = ref.calibration_ratio(ctx, d, cov_of, draws=a.draws)
        ctx.close()
        out["configurations"].append(dict(descriptor=desc, loss=loss, ratio=[round(float(v), 3) for v in ratio], min=round(float(ratio.min()), 3),
                                          max=round(float(ratio.max()), 3), draws_without_covariance=int(bad)))
        print(desc, loss, np.round(ratio, 3), "not OK:", bad, flush=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
