#!/usr/bin/env python3
"""Many independent VisualOdometry sequences: bpvo_hip_add_frames against the same frames pushed through bpvo_hip_add_frame, one context per
sequence, round robin.  640x480, the default AlgorithmParameters (intensity descriptor) but for the key-framing translation threshold (one
frame in four to five key-frames), make_sequence inputs of 20 frames.  Prints one JSON line.

  python scripts/multi_sequence_bench.py                 # S = 1, 8, 32, 64: host buffers, device buffers, the add_frame baseline
  python scripts/multi_sequence_bench.py --only 8        # one size, add_frames from host buffers only (a run under rocprofv3 --kernel-trace)
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

ROWS, COLS, FRAMES = 480, 640, 20
KF_TRANSLATION = 0.065      # with make_sequence's default steps: about one key frame in four frames (the CPU oracle at 160x120: 0.06 -> 30 %, 0.08 -> 18 %)
DISTINCT = 16               # sequences s and s + 16 see the same frames (rendering is the slow part of the script; the device work is the same)


def params(b):
    p = b.default_params()
    p.verbosity = capi.VERB_SILENT
    p.minTranslationMagToKeyFrame = KF_TRANSLATION
    return p


def frames_for(S, cache):
    out = []
    for s in range(S):
        if s % DISTINCT not in cache:
            cache[s % DISTINCT] = synth.make_sequence(ROWS, COLS, FRAMES, index=s % DISTINCT)
        out.append(cache[s % DISTINCT])
    return out


def run_multi(hip, seqs, device, torch=None):
    S = len(seqs)
    K, base = seqs[0]["K"], seqs[0]["b"]
    ctx = hip.create(K, base, ROWS, COLS, params(hip), n_frames=3 * S, n_pairs=S)
    imgs = np.stack([np.stack([q["frames"][k][0] for q in seqs]) for k in range(FRAMES)])      # [FRAMES][S][R][W]
    disps = np.stack([np.stack([q["frames"][k][1] for q in seqs]) for k in range(FRAMES)])
    if device:
        d_imgs = torch.from_numpy(imgs).cuda()
        d_disps = torch.from_numpy(disps).cuda()
        torch.cuda.synchronize()

    def one_pass():
        times, kf = [], 0
        for k in range(FRAMES):
            t = time.perf_counter()
            if device:
                res = ctx.add_frames_device(S, d_imgs[k].data_ptr(), d_disps[k].data_ptr())
            else:
                res = ctx.add_frames(imgs[k], disps[k])
            times.append(time.perf_counter() - t)
            kf += sum(r["isKeyFrame"] for r in res[:] if k > 0)
        return times, kf

    one_pass()                               # warm-up (code objects, template storage)
    for s in range(S):
        ctx.seq_reset(s)
    times, kf = one_pass()
    ctx.close()
    total = sum(times)
    return dict(frames_per_s=S * FRAMES / total, ms_per_call=1e3 * total / FRAMES, kf_fraction=kf / (S * (FRAMES - 1)))


def run_baseline(hip, seqs):
    S = len(seqs)
    K, base = seqs[0]["K"], seqs[0]["b"]
    for timed in (False, True):              # a warm-up pass on contexts of their own, then the timed one on fresh contexts
        ctxs = [hip.create(K, base, ROWS, COLS, params(hip), n_frames=3, n_pairs=1) for _ in range(S)]
        t = time.perf_counter()
        for k in range(FRAMES):
            for s in range(S):
                ctxs[s].add_frame(*seqs[s]["frames"][k])
        total = time.perf_counter() - t
        for c in ctxs:
            c.close()
    return dict(frames_per_s=S * FRAMES / total, ms_per_frame=1e3 * total / (S * FRAMES))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1,8,32,64")
    ap.add_argument("--only", type=int, default=0, help="one size, add_frames from host buffers only")
    a = ap.parse_args()
    try:
        import torch
        if torch.cuda.is_available():
            torch.cuda.init()
    except Exception:
        torch = None
    hip = bpvo_amd.load()
    cache = {}
    if a.only:
        r = run_multi(hip, frames_for(a.only, cache), False)
        print(json.dumps(dict(bench="multi_sequence", S=a.only, rows=ROWS, cols=COLS, frames=FRAMES, host=r)))
        return
    out = []
    for S in [int(x) for x in a.sizes.split(",")]:
        seqs = frames_for(S, cache)
        row = dict(S=S, host=run_multi(hip, seqs, False))
        if torch is not None:
            row["device"] = run_multi(hip, seqs, True, torch)
        row["add_frame_round_robin"] = run_baseline(hip, seqs)
        row["speedup_host"] = row["host"]["frames_per_s"] / row["add_frame_round_robin"]["frames_per_s"]
        out.append(row)
        print(json.dumps(row), file=sys.stderr)
    print(json.dumps(dict(bench="multi_sequence", rows=ROWS, cols=COLS, frames=FRAMES, kf_translation=KF_TRANSLATION, results=out)))


if __name__ == "__main__":
    main()
