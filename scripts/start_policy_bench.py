#!/usr/bin/env python3
"""What the start policy (bpvo_hip_set_start_policy) costs and saves.  Bit-planes frames of 640x480 (make_sequence inputs), four pyramid levels,
default key-framing, with make_sequence's step_trans 0.03 (its default: the reference's start is good) and 0.3 (ten times the motion per frame).

Per step size and mode — 0 the reference's start, 1 constant velocity, 2 scored (Identity, the last motion, the last motion twice; tau 0.5 at the
coarsest level):
  * add_frame_ms          per bpvo_hip_add_frame call, host clock around the call: the latency path.  Mode 2 adds one scoring launch pair and one
                          host round trip in front of every estimate; `scored_minus_reference_ms` is that difference of the medians
  * add_frames_S{1,64}_ms per bpvo_hip_add_frames call (one frame of every sequence) for 1 and 64 sequences
  * iterations_per_frame  the Gauss-Newton iterations of a frame's Result, summed over its levels, averaged over the timed frames (and sequences)
  * translation_error_m   the median distance of Result.pose's translation from the truth over the timed frames (sequence 0)
The first two frames of every sequence (the first frame and the first estimate, which allocate) are fed untimed.  Every figure: the median of
--repeats (5) passes that ALTERNATE over the modes, with the passes' min and max.  Nothing here is a target: the numbers are what was measured.
Writes profiles/start_policy_bench.json and prints it as one JSON line.

  python scripts/start_policy_bench.py
  python scripts/start_policy_bench.py --sequences 1 --steps 0.03
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

ROWS, COLS, LEVELS, FRAMES, DISTINCT, WARM = 480, 640, 4, 12, 4, 2
MODES = [("0_keyframe_pose", dict(mode=capi.START_KEYFRAME_POSE, score_level=-1, tau=0.0)),
         ("1_constant_velocity", dict(mode=capi.START_CONSTANT_VELOCITY, score_level=-1, tau=0.0)),
         ("2_scored", dict(mode=capi.START_SCORED, score_level=-1, tau=0.5))]


def params(b):
    p = b.default_params()
    p.verbosity = capi.VERB_SILENT
    p.descriptor = capi.DESC_BITPLANES
    p.numPyramidLevels = LEVELS
    return p


def summary(runs):
    return dict(median=float(np.median(runs)), min=float(min(runs)), max=float(max(runs)), runs=[round(float(r), 4) for r in runs])


def truth(seq, k):
    return seq["poses"][k] @ np.linalg.inv(seq["poses"][k - 1])


def error(pose, T):
    return float(np.linalg.norm(np.asarray(pose, np.float64)[:3, 3] - T[:3, 3]))


def add_frame(hip, seq, p, repeats):
    """bpvo_hip_add_frame over the sequence under every mode, a fresh context per pass and mode (created outside the clock)"""
    runs = {name: [] for name, _ in MODES}
    info = {}
    for r in range(repeats + 1):                      # (pass 0: warm-up)
        for name, pol in MODES:
            ctx = hip.create(seq["K"], seq["b"], ROWS, COLS, p, n_frames=3, n_pairs=1)
            ctx.set_start_policy(pol)
            for k in range(WARM):
                ctx.add_frame(*seq["frames"][k])
            its, errs, chosen = 0, [], []
            t = time.perf_counter()
            res = [ctx.add_frame(*seq["frames"][k]) for k in range(WARM, FRAMES)]
            dt = time.perf_counter() - t
            for k, q in zip(range(WARM, FRAMES), res):
                its += sum(st["numIterations"] for st in q["stats"])
                errs.append(error(q["pose"], truth(seq, k)))
            if r:
                runs[name].append(1e3 * dt / (FRAMES - WARM))
            info[name] = dict(iterations_per_frame=its / (FRAMES - WARM), translation_error_m=float(np.median(errs)),
                              key_frames=sum(q["isKeyFrame"] for q in res))
            ctx.close()
    return {name: dict(info[name], add_frame_ms=summary(runs[name])) for name, _ in MODES}


def add_frames(hip, seqs, p, S, repeats):
    """bpvo_hip_add_frames, one frame of each of S sequences per call, every mode in every pass on one context"""
    ctx = hip.create(seqs[0]["K"], seqs[0]["b"], ROWS, COLS, p, n_frames=3 * S, n_pairs=S)
    imgs = [np.stack([seqs[s % DISTINCT]["frames"][k][0] for s in range(S)]) for k in range(FRAMES)]
    disps = [np.stack([seqs[s % DISTINCT]["frames"][k][1] for s in range(S)]) for k in range(FRAMES)]
    runs = {name: [] for name, _ in MODES}
    info = {}
    for r in range(repeats + 1):                      # (pass 0: warm-up)
        for name, pol in MODES:
            ctx.set_start_policy(pol)
            for s in range(S):
                ctx.seq_reset(s)
            for k in range(WARM):
                ctx.add_frames(imgs[k], disps[k])
            its, errs = 0, []
            t = time.perf_counter()
            res = [ctx.add_frames(imgs[k], disps[k]) for k in range(WARM, FRAMES)]
            dt = time.perf_counter() - t
            for k, call in zip(range(WARM, FRAMES), res):
                its += sum(st["numIterations"] for q in call for st in q["stats"])
                errs.append(error(call[0]["pose"], truth(seqs[0], k)))
            if r:
                runs[name].append(1e3 * dt / (FRAMES - WARM))
            info[name] = dict(iterations_per_frame=its / (S * (FRAMES - WARM)), translation_error_m=float(np.median(errs)))
    ctx.close()
    return {name: dict(info[name], add_frames_ms=summary(runs[name])) for name, _ in MODES}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", default="0.03,0.3", help="make_sequence's step_trans values")
    ap.add_argument("--sequences", default="1,64")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "start_policy_bench.json"))
    a = ap.parse_args()
    try:      # (torch's runtime first, where it is there: tests/conftest.py)
        import torch
        if torch.cuda.is_available():
            torch.cuda.init()
    except Exception:
        pass
    hip = bpvo_amd.load()
    p = params(hip)
    results = []
    for step in [float(x) for x in a.steps.split(",")]:
        seqs = [synth.make_sequence(ROWS, COLS, FRAMES, index=i, step_trans=step) for i in range(DISTINCT)]
        row = dict(step_trans=step, add_frame=add_frame(hip, seqs[0], p, a.repeats))
        med = {name: row["add_frame"][name]["add_frame_ms"]["median"] for name, _ in MODES}
        row["scored_minus_reference_ms"] = med["2_scored"] - med["0_keyframe_pose"]
        for S in [int(x) for x in a.sequences.split(",")]:
            row[f"add_frames_S{S}"] = add_frames(hip, seqs, p, S, a.repeats)
        results.append(row)
        print(json.dumps(row), file=sys.stderr)
    out = dict(bench="start_policy", rows=ROWS, cols=COLS, levels=LEVELS, frames=FRAMES, untimed_frames=WARM, repeats=a.repeats,
               modes={name: pol for name, pol in MODES}, results=results)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
