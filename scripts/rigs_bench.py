#!/usr/bin/env python3
"""Several rigs in one call against one context per rig: ms per call of bpvo_hip_add_frames_rigs advancing R rigs of 4 cameras (640x480 bit-planes
frames, host buffers) in ONE context, and beside it the same R rigs in R contexts of their own (bpvo_hip_rig_set + bpvo_hip_add_frames_rig),
advanced one after the other in the same process — what a caller had to do before there were several rigs in a context.  Every rig sees the
same frames.  Both in one invocation, alternating pass by pass (fresh contexts per pass, created outside the timed region; the first frame of a
pass — templates only — is not timed), --repeats passes of each after a warm-up pass of each (scripts/rig_bench.py's protocol).  Writes
profiles/rigs_bench.json and prints it: per R the median ms per call of every pass, their min and max, and the ratio of the medians.  A record,
not a bar.

  python scripts/rigs_bench.py
  python scripts/rigs_bench.py --rigs 1,2 --repeats 3 --frames 8
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import bpvo_amd  # noqa: E402
from bpvo_amd import capi, synth  # noqa: E402
from rig_bench import COLS, ROWS, packed, params, rig_extrinsics  # noqa: E402

CAMERAS = 4


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def one_pass(hip, seq, inputs, R, together):
    cams = [(seq["K"][p], seq["b"][p], ROWS, COLS) for p in range(CAMERAS)]
    X = np.stack(seq["extrinsics"])
    if together:
        ctx = hip.create_sequences(cams * R, params(hip))
        ctx.rigs_set([X] * R)
        ctxs = [ctx]
    else:
        ctxs = []
        for _ in range(R):
            ctx = hip.create_sequences(cams, params(hip))
            ctx.rig_set(X)
            ctxs.append(ctx)
    res = (capi.Result * R)()
    times, key_frames = [], 0
    for k, (img, disp) in enumerate(inputs):
        t = time.perf_counter()
        if together:
            ctxs[0].call("add_frames_rigs", R, None, _p(img), _p(disp), 0, res)
        else:
            for r, ctx in enumerate(ctxs):
                ctx.call("add_frames_rig", _p(img), _p(disp), 0, ctypes.byref(res[r]))
        if k > 0:
            times.append(time.perf_counter() - t)
            key_frames += int(res[0].isKeyFrame)
    for ctx in ctxs:
        ctx.close()
    return 1e3 * float(np.median(times)), key_frames


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rigs", default="1,2,4,8,16")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--frames", type=int, default=12)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rigs_bench.json"))
    ap.add_argument("--lib", default="", help="another build of libbpvo_hip.so (A/B runs against an earlier commit's library)")
    a = ap.parse_args()
    hip = capi.Binding(os.path.abspath(a.lib), "bpvo_hip_") if a.lib else bpvo_amd.load()
    seq = synth.make_rig_sequence(ROWS, COLS, a.frames, rig_extrinsics(CAMERAS), index=0)
    calls = packed(seq)
    rows = []
    for R in [int(v) for v in a.rigs.split(",")]:
        # (every rig sees the same frames: the one call's input is the rig's frames R times over)
        inputs = {True: [(np.tile(img, R), np.tile(disp, R)) for img, disp in calls], False: calls}
        for together in (True, False):
            one_pass(hip, seq, inputs[together], R, together)      # warm-up: code objects, allocations
        ms = {True: [], False: []}
        kf = {True: 0, False: 0}
        for _ in range(max(1, a.repeats)):
            for together in (True, False):              # alternating: drift of the machine hits both alike
                m, k = one_pass(hip, seq, inputs[together], R, together)
                ms[together].append(m)
                kf[together] = k
        rows.append(dict(rigs=R, cameras_per_rig=CAMERAS, frames_timed=a.frames - 1,
                         one_call_ms=dict(median=float(np.median(ms[True])), min=min(ms[True]), max=max(ms[True]), passes=ms[True]),
                         contexts_in_sequence_ms=dict(median=float(np.median(ms[False])), min=min(ms[False]), max=max(ms[False]), passes=ms[False]),
                         one_call_over_contexts=float(np.median(ms[True]) / np.median(ms[False])),
                         key_frames_of_rig_0=dict(one_call=kf[True], contexts=kf[False])))
        print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
    out = dict(what="ms per call: bpvo_hip_add_frames_rigs over R rigs in one context against the same rigs in R contexts, bpvo_hip_add_frames_rig one after the other",
               image=[ROWS, COLS], descriptor="bitplanes", repeats=a.repeats, host_buffers=True, rows=rows)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
