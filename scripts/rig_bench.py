#!/usr/bin/env python3
"""Rig mode against independent sequences: ms per frame of bpvo_hip_add_frames_rig (ONE body pose from all cameras) for rigs of 2, 4 and 6 cameras
of 640x480 bit-planes frames, and beside each the same cameras' frames through bpvo_hip_add_frames as independent sequences.  Both in one
invocation, alternating pass by pass (a fresh context per pass, created outside the timed region; the first frame of a pass — templates only —
is not timed), --repeats passes of each after a warm-up pass of each; host buffers.  Writes profiles/rig_bench.json and prints it: per rig size
the median ms per frame of every pass, their min and max, and the ratio of the medians.  A record, not a bar.

  python scripts/rig_bench.py
  python scripts/rig_bench.py --sizes 2 --repeats 3 --frames 8
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

import bpvo_amd  # noqa: E402
from bpvo_amd import capi, synth  # noqa: E402

ROWS, COLS = 480, 640
KF_TRANSLATION = 0.065      # scripts/multi_sequence_bench.py's: about one key frame in four frames with make_sequence's default steps


def params(b):
    p = b.default_params()
    p.descriptor = capi.DESC_BITPLANES
    p.verbosity = capi.VERB_SILENT
    p.minTranslationMagToKeyFrame = KF_TRANSLATION
    return p


def rig_extrinsics(n):
    """n cameras on a ring of 0.3 m around the body's origin, each turned a little further outwards (camera_from_body)"""
    out = []
    for p in range(n):
        a = 2.0 * np.pi * p / n
        yaw = 0.1 * (p - (n - 1) / 2.0)
        out.append(synth.twist_to_matrix([0.0, yaw, 0.0, 0.3 * np.cos(a) if n > 1 else 0.0, 0.05 * np.sin(a), 0.0]))
    return out


def packed(seq):
    """[frames] of (u8 images, f32 disparities) of all cameras back to back, as both entry points take them"""
    return [(np.concatenate([f[0].reshape(-1) for f in frames]), np.concatenate([f[1].reshape(-1) for f in frames])) for frames in seq["frames"]]


def one_pass(hip, seq, calls, rig):
    n = len(seq["extrinsics"])
    cams = [(seq["K"][p], seq["b"][p], ROWS, COLS) for p in range(n)]
    ctx = hip.create_sequences(cams, params(hip))
    if rig:
        ctx.rig_set(np.stack(seq["extrinsics"]))
    res = (capi.Result * n)()
    times, key_frames = [], 0
    for k, (img, disp) in enumerate(calls):
        t = time.perf_counter()
        if rig:
            ctx.call("add_frames_rig", img.ctypes.data_as(ctypes.c_void_p), disp.ctypes.data_as(ctypes.c_void_p), 0, ctypes.byref(res[0]))
        else:
            ctx.call("add_frames", n, None, img.ctypes.data_as(ctypes.c_void_p), disp.ctypes.data_as(ctypes.c_void_p), 0, res)
        if k > 0:
            times.append(time.perf_counter() - t)
            key_frames += int(res[0].isKeyFrame)
    ctx.close()
    return 1e3 * float(np.median(times)), key_frames


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="2,4,6")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--frames", type=int, default=12)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rig_bench.json"))
    ap.add_argument("--lib", default="", help="another build of libbpvo_hip.so (A/B runs against an earlier commit's library)")
    a = ap.parse_args()
    hip = capi.Binding(os.path.abspath(a.lib), "bpvo_hip_") if a.lib else bpvo_amd.load()
    rows = []
    for n in [int(v) for v in a.sizes.split(",")]:
        seq = synth.make_rig_sequence(ROWS, COLS, a.frames, rig_extrinsics(n), index=0)
        calls = packed(seq)
        for rig in (True, False):
            one_pass(hip, seq, calls, rig)      # warm-up: code objects, allocations
        ms = {True: [], False: []}
        kf = {True: 0, False: 0}
        for _ in range(max(1, a.repeats)):
            for rig in (True, False):           # alternating: drift of the machine hits both alike
                m, k = one_pass(hip, seq, calls, rig)
                ms[rig].append(m)
                kf[rig] = k
        rows.append(dict(cameras=n, frames_timed=a.frames - 1,
                         rig_ms_per_frame=dict(median=float(np.median(ms[True])), min=min(ms[True]), max=max(ms[True]), passes=ms[True]),
                         independent_ms_per_call=dict(median=float(np.median(ms[False])), min=min(ms[False]), max=max(ms[False]), passes=ms[False]),
                         rig_over_independent=float(np.median(ms[True]) / np.median(ms[False])),
                         rig_key_frames=kf[True], independent_key_frames_of_camera_0=kf[False]))
    out = dict(what="ms per frame: bpvo_hip_add_frames_rig against the same cameras as independent bpvo_hip_add_frames sequences",
               image=[ROWS, COLS], descriptor="bitplanes", repeats=a.repeats, host_buffers=True, rows=rows)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
