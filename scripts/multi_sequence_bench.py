#!/usr/bin/env python3
"""Many independent VisualOdometry sequences: bpvo_hip_add_frames against the same frames pushed through bpvo_hip_add_frame, one context per
sequence, round robin.  640x480, the default AlgorithmParameters (intensity descriptor) but for the key-framing translation threshold (one
frame in four to five key-frames), make_sequence inputs of 20 frames.  Prints one JSON line.

--cameras picks what the sequences look through:
  shared   one camera for all (bpvo_hip_create), the default
  calib    640x480, every sequence its own K and baseline (bpvo_hip_create_sequences; sixteen calibrations, one per distinct frame set)
  kitti    12 sequences, four of each KITTI odometry geometry: 1241x376 / fx 718.856, 1242x375 / 721.5377, 1226x370 / 707.0912 (--sizes ignored)

  python scripts/multi_sequence_bench.py                 # S = 1, 8, 32, 64: host buffers, device buffers, the add_frame baseline
  python scripts/multi_sequence_bench.py --only 8        # one size, add_frames from host buffers only (a run under rocprofv3 --kernel-trace)
  python scripts/multi_sequence_bench.py --cameras kitti --only 12
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

ROWS, COLS, FRAMES = 480, 640, 20
KF_TRANSLATION = 0.065      # with make_sequence's default steps: about one key frame in four frames (the CPU oracle at 160x120: 0.06 -> 30 %, 0.08 -> 18 %)
DISTINCT = 16               # sequences s and s + 16 see the same frames (rendering is the slow part of the script; the device work is the same)


def params(b):
    p = b.default_params()
    p.verbosity = capi.VERB_SILENT
    p.minTranslationMagToKeyFrame = KF_TRANSLATION
    return p


# (rows, cols, fx, cx, cy, baseline)
KITTI = [(376, 1241, 718.856, 607.1928, 185.2157, 0.5372), (375, 1242, 721.5377, 609.5593, 172.854, 0.5371),
         (370, 1226, 707.0912, 601.8873, 183.1104, 0.5372)]


def camera_for(cameras, s):
    """(K, baseline, rows, cols) of sequence s, or None: the shared camera of make_sequence"""
    if cameras == "calib":
        rng = np.random.default_rng(100 + s % DISTINCT)
        fx, fy = rng.uniform(560, 680, 2)
        K = np.array([[fx, 0, COLS / 2 + rng.uniform(-12, 12)], [0, fy, ROWS / 2 + rng.uniform(-12, 12)], [0, 0, 1]], np.float32)
        return K, float(np.float32(rng.uniform(0.08, 0.16))), ROWS, COLS
    if cameras == "kitti":
        r, c, fx, cx, cy, b = KITTI[s % 3]
        return np.array([[fx, 0, cx], [0, fx, cy], [0, 0, 1]], np.float32), b, r, c
    return None


def frames_for(S, cache, cameras="shared"):
    out = []
    for s in range(S):
        key = s if cameras == "kitti" else s % DISTINCT
        if key not in cache:
            cam = camera_for(cameras, s)
            if cam is None:
                cache[key] = synth.make_sequence(ROWS, COLS, FRAMES, index=key)
            else:
                cache[key] = synth.make_sequence(cam[2], cam[3], FRAMES, index=key, camera=cam[:2])
                cache[key]["camera"] = cam
        out.append(cache[key])
    return out


def run_multi(hip, seqs, device, torch=None):
    S = len(seqs)
    if "camera" in seqs[0]:
        ctx = hip.create_sequences([q["camera"] for q in seqs], params(hip))
    else:
        ctx = hip.create(seqs[0]["K"], seqs[0]["b"], ROWS, COLS, params(hip), n_frames=3 * S, n_pairs=S)
    # [FRAMES] packed calls: frame k of every sequence back to back (one size: [S][R][W])
    imgs = [np.concatenate([q["frames"][k][0].reshape(-1) for q in seqs]) for k in range(FRAMES)]
    disps = [np.concatenate([q["frames"][k][1].reshape(-1) for q in seqs]) for k in range(FRAMES)]
    shapes = [q["frames"][0][0].shape for q in seqs]
    mixed = len(set(shapes)) > 1
    if device:
        d_imgs = [torch.from_numpy(x).cuda() for x in imgs]
        d_disps = [torch.from_numpy(x).cuda() for x in disps]
        torch.cuda.synchronize()

    def one_pass():
        times, kf = [], 0
        for k in range(FRAMES):
            t = time.perf_counter()
            if device:
                res = ctx.add_frames_device(S, d_imgs[k].data_ptr(), d_disps[k].data_ptr())
            elif mixed:
                res = add_frames_packed(ctx, S, imgs[k], disps[k])
            else:
                res = ctx.add_frames(imgs[k].reshape(S, *shapes[0]), disps[k].reshape(S, *shapes[0]))
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


def add_frames_packed(ctx, n, img, disp):
    """Context.add_frames on frames already packed back to back (what it does with a list of differing shapes, without the packing copy)"""
    res = (capi.Result * n)()
    ctx.call("add_frames", n, None, img.ctypes.data_as(ctypes.c_void_p), disp.ctypes.data_as(ctypes.c_void_p), 0, res)
    return [ctx._result_dict(r) for r in res]


def run_baseline(hip, seqs):
    S = len(seqs)
    for timed in (False, True):              # a warm-up pass on contexts of their own, then the timed one on fresh contexts
        ctxs = [hip.create(q["K"], q["b"], *q["frames"][0][0].shape, params(hip), n_frames=3, n_pairs=1) for q in seqs]
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
    ap.add_argument("--cameras", choices=("shared", "calib", "kitti"), default="shared")
    a = ap.parse_args()
    if a.cameras == "kitti":
        a.sizes = "12"
    try:
        import torch
        if torch.cuda.is_available():
            torch.cuda.init()
    except Exception:
        torch = None
    hip = bpvo_amd.load()
    cache = {}
    if a.only:
        r = run_multi(hip, frames_for(a.only, cache, a.cameras), False)
        print(json.dumps(dict(bench="multi_sequence", cameras=a.cameras, S=a.only, rows=ROWS, cols=COLS, frames=FRAMES, host=r)))
        return
    out = []
    for S in [int(x) for x in a.sizes.split(",")]:
        seqs = frames_for(S, cache, a.cameras)
        row = dict(S=S, host=run_multi(hip, seqs, False))
        if torch is not None:
            row["device"] = run_multi(hip, seqs, True, torch)
        row["add_frame_round_robin"] = run_baseline(hip, seqs)
        row["speedup_host"] = row["host"]["frames_per_s"] / row["add_frame_round_robin"]["frames_per_s"]
        out.append(row)
        print(json.dumps(row), file=sys.stderr)
    print(json.dumps(dict(bench="multi_sequence", cameras=a.cameras, rows=ROWS, cols=COLS, frames=FRAMES, kf_translation=KF_TRANSLATION, results=out)))


if __name__ == "__main__":
    main()
