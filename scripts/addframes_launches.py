#!/usr/bin/env python3
"""The library's own per-kernel launch table (profiling level 2) for every call of three small runs, one per kind of batched addFrame call:
bpvo_hip_add_frames with S = 8 sequences, bpvo_hip_add_frames_rig with a rig of 4 cameras, bpvo_hip_add_frames_rigs with R = 4 rigs of 2 cameras
(120x160 intensity / Huber, 3 levels, 6 frames, a translation threshold that gives frames without a key frame and a key frame with
re-estimation).  Prints one line per call: kind, call, {kernel: launches}.  Run it on two builds (--lib) and diff the outputs: a change of the
host drivers that leaves the work alone leaves every line alone.

  python scripts/addframes_launches.py --lib bpvo_amd/csrc/libbpvo_hip.so
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

ROWS, COLS, FRAMES = 120, 160, 6


def params(b):
    p = b.default_params()
    p.numPyramidLevels = 3
    p.descriptor = capi.DESC_INTENSITY
    p.lossFunction = capi.LOSS_HUBER
    p.verbosity = capi.VERB_SILENT
    p.minTranslationMagToKeyFrame = 0.027
    p.minRotationMagToKeyFrame = 2.5
    p.maxFractionOfGoodPointsToKeyFrame = 0.0
    return p


def ring(n):
    return [synth.twist_to_matrix([0.0, 0.1 * (p - (n - 1) / 2.0), 0.0, 0.3 * np.cos(2.0 * np.pi * p / n), 0.05 * np.sin(2.0 * np.pi * p / n), 0.0]) for p in range(n)]


def report(kind, ctx, call):
    for k in range(FRAMES):
        ctx.profiling(2)
        res = call(k)
        flags = [(int(r["isKeyFrame"]), int(r["keyFramingReason"])) for r in res]
        print(kind, k, json.dumps(dict(key_frames=flags, launches={q["name"]: q["launches"] for q in ctx.kernel_stats() if q["launches"]}), sort_keys=True))
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default="", help="another build of libbpvo_hip.so")
    a = ap.parse_args()
    hip = capi.Binding(os.path.abspath(a.lib), "bpvo_hip_") if a.lib else bpvo_amd.load()
    seqs = [synth.make_sequence(ROWS, COLS, FRAMES, index=3 + (s % 2), step_trans=0.02 + 0.01 * (s % 3)) for s in range(8)]
    ctx = hip.create(seqs[0]["K"], seqs[0]["b"], ROWS, COLS, params(hip), n_frames=24, n_pairs=8)
    report("add_frames S=8", ctx, lambda k: ctx.add_frames(np.stack([s["frames"][k][0] for s in seqs]), np.stack([s["frames"][k][1] for s in seqs])))
    rig = synth.make_rig_sequence(ROWS, COLS, FRAMES, ring(4), index=3)
    ctx = hip.create_sequences([(rig["K"][p], rig["b"][p], ROWS, COLS) for p in range(4)], params(hip))
    ctx.rig_set(np.stack(rig["extrinsics"]))
    report("add_frames_rig of 4", ctx, lambda k: [ctx.add_frames_rig([f[0] for f in rig["frames"][k]], [f[1] for f in rig["frames"][k]])])
    two = synth.make_rig_sequence(ROWS, COLS, FRAMES, ring(2), index=3)
    ctx = hip.create_sequences([(two["K"][p], two["b"][p], ROWS, COLS) for p in range(2)] * 4, params(hip))
    ctx.rigs_set([np.stack(two["extrinsics"])] * 4)
    report("add_frames_rigs R=4", ctx, lambda k: ctx.add_frames_rigs([[f[0] for f in two["frames"][k]]] * 4, [[f[1] for f in two["frames"][k]]] * 4))


if __name__ == "__main__":
    main()
