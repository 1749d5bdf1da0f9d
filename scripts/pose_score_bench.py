#!/usr/bin/env python3
"""What scoring P candidate poses costs (bpvo_hip_score_poses: one launch) against the only way to the same numbers without it: P calls of
bpvo_hip_linearize (five launches, an exact median and a host synchronisation each).  Wall time through the ctypes binding, host arrays.
  one pair     640x480, bit-planes and intensity, every pyramid level, P = 1, 16, 64, 256, 1024 poses around the identity
  pairs        bpvo_hip_score_poses_pairs of 64 pairs x 16 poses at the coarsest level, against 64 x 16 linearisations
A pass times 20 scoring calls back to back (reported per call) and then the P linearisations; a warm-up pass, then --repeats alternating passes;
medians, and the passes themselves so that their spread can be seen.  Writes profiles/pose_score_bench.json and prints it.  A record, not a bar: no ratio is fixed in advance.

  python scripts/pose_score_bench.py
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bpvo_amd  # noqa: E402
from bpvo_amd import capi, synth  # noqa: E402

TAU = {"bitplanes": 0.5, "intensity": 30.0}
POSE_COUNTS = (1, 16, 64, 256, 1024)


def params(b, descriptor):
    p = b.default_params()
    p.descriptor = capi.DESC_BITPLANES if descriptor == "bitplanes" else capi.DESC_INTENSITY
    p.verbosity = capi.VERB_SILENT
    return p


def poses_around_identity(n):
    tw = np.array([0.004, -0.003, 0.002, 0.02, -0.015, 0.03])
    return np.stack([synth.twist_to_matrix(tw * s).astype(np.float32) for s in np.linspace(-3.0, 3.0, n)])


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return 1e3 * (time.perf_counter() - t0)


SCORE_CALLS = 20      # a scoring call is tens of microseconds: a pass times this many back to back (each ends in its synchronisation) and reports one


def alternate(score, linearize, repeats):
    score(), linearize()
    a, b = [], []
    for _ in range(repeats):
        a.append(timed(lambda: [score() for _ in range(SCORE_CALLS)]) / SCORE_CALLS)
        b.append(timed(linearize))
    ms, ml = float(np.median(a)), float(np.median(b))
    return dict(score_ms=round(ms, 4), linearize_ms=round(ml, 4), linearize_over_score=round(ml / ms, 2), score_passes=[round(v, 4) for v in a],
                linearize_passes=[round(v, 4) for v in b])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_score_bench.json"))
    a = ap.parse_args()
    hip = bpvo_amd.load()
    rows, cols = 480, 640
    d = synth.make_pair(rows, cols, 1)
    out = dict(what="wall ms: one bpvo_hip_score_poses call for P poses against P bpvo_hip_linearize calls, medians of alternating passes",
               repeats=a.repeats, image="640x480", rows=[])
    for descriptor in ("bitplanes", "intensity"):
        ctx = hip.create(d["K"], d["b"], rows, cols, params(hip, descriptor), n_frames=2, n_pairs=1)
        ctx.frame_set_data(0, d["imgA"], d["dispA"])
        ctx.frame_set_template(0)
        ctx.frame_set_data(1, d["imgB"], d["dispB"])
        for level in range(ctx.L):
            for P in POSE_COUNTS:
                T = poses_around_identity(P)
                r = alternate(lambda: ctx.score_poses(0, 1, level, T, TAU[descriptor]),
                              lambda: [ctx.linearize(0, 0, 1, level, T[k], reset_scale=True) for k in range(P)], a.repeats)
                r = dict(dict(case="one pair", descriptor=descriptor, level=level, points=ctx.num_points(0, level), poses=P), **r)
                r["score_us_per_pose"] = round(1e3 * r["score_ms"] / P, 3)
                out["rows"].append(r)
                print(json.dumps(r), flush=True)
        ctx.close()
    n = a.pairs
    for descriptor in ("bitplanes", "intensity"):
        ctx = hip.create(d["K"], d["b"], rows, cols, params(hip, descriptor), n_frames=2 * n, n_pairs=n)
        ctx.frames_set_data(0, 1, np.stack([d["imgA"], d["imgB"]] * n), np.stack([d["dispA"], d["dispB"]] * n))
        ctx.frames_set_template(0, 2, n)
        refs, curs = [2 * i for i in range(n)], [2 * i + 1 for i in range(n)]
        level, P = ctx.L - 1, 16
        T = np.stack([poses_around_identity(P)] * n)
        r = alternate(lambda: ctx.score_poses_pairs(refs, curs, level, T, TAU[descriptor]),
                      lambda: [ctx.linearize(i, refs[i], curs[i], level, T[i, k], reset_scale=True) for i in range(n) for k in range(P)], a.repeats)
        r = dict(dict(case="%d pairs in one launch" % n, descriptor=descriptor, level=level, points=ctx.num_points(0, level), poses=P), **r)
        out["rows"].append(r)
        print(json.dumps(r), flush=True)
        ctx.close()
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(dict(written=a.out, rows=len(out["rows"]))))


if __name__ == "__main__":
    main()
