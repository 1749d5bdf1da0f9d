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
  python scripts/multi_sequence_bench.py --repeats 5 --sizes 8,64     # every timed pass five times: ms per call of each, their min and max

--sweep: a parameter sweep over one dataset.  S = 8 and 64 sequences of the SAME 640x480 bit-planes frames, each with its own parameter set
(bpvo_hip_seq_set_params: the eight sets of SWEEP — all three losses, maxIterations 3 / 50 / 200, both key-frame threshold sets, minSaliency
0.01 / 0.1 / 1, a disparity gate — cycled with the function tolerance varied, so that the S sets are distinct) in ONE context, against the
same S parameter sets as S contexts of their own fed the same frames one after the other (what a sweep cost before).  --repeats timed passes
of each after a warm-up pass; ms per add_frames call of every pass, their min and max, and the ratio of the medians.
--lib PATH: another build of libbpvo_hip.so (A/B runs of the uniform modes against an earlier commit's library).
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


def run_multi(hip, seqs, device, torch=None, repeats=1, seq_params=None, base=None):
    S = len(seqs)
    if seq_params is not None:
        ctx = hip.create(seqs[0]["K"], seqs[0]["b"], ROWS, COLS, base, n_frames=3 * S, n_pairs=S)
        for s, p in enumerate(seq_params):
            ctx.seq_set_params(s, p)
    elif "camera" in seqs[0]:
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
    runs = []
    for _ in range(max(1, repeats)):
        for s in range(S):
            ctx.seq_reset(s)
        times, kf = one_pass()
        runs.append(1e3 * sum(times) / FRAMES)
    ctx.close()
    total = 1e-3 * float(np.median(runs)) * FRAMES
    out = dict(frames_per_s=S * FRAMES / total, ms_per_call=1e3 * total / FRAMES, kf_fraction=kf / (S * (FRAMES - 1)))
    if repeats > 1:
        out.update(ms_per_call_runs=[round(r, 4) for r in runs], ms_per_call_min=min(runs), ms_per_call_max=max(runs))
    return out


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


# ---- --sweep ------------------------------------------------------------------------------------------------------------------------------
KF_A = dict(minTranslationMagToKeyFrame=0.1, minRotationMagToKeyFrame=2.5, maxFractionOfGoodPointsToKeyFrame=0.7, goodPointThreshold=0.8)
KF_B = dict(minTranslationMagToKeyFrame=0.25, minRotationMagToKeyFrame=2.5, maxFractionOfGoodPointsToKeyFrame=0.5, goodPointThreshold=0.6)
GATE = "gate"      # the median disparity of the first frame
SWEEP = [
    dict(lossFunction=capi.LOSS_TUKEY, maxIterations=50, minSaliency=0.1, **KF_A),
    dict(lossFunction=capi.LOSS_HUBER, maxIterations=200, minSaliency=0.01, parameterTolerance=1e-6, functionTolerance=1e-4, **KF_A),
    dict(lossFunction=capi.LOSS_L2, maxIterations=3, minSaliency=0.1, **KF_B),
    dict(lossFunction=capi.LOSS_TUKEY, maxIterations=3, minSaliency=1.0, functionTolerance=5e-4, **KF_A),
    dict(lossFunction=capi.LOSS_HUBER, maxIterations=50, minSaliency=0.1, maxValidDisparity=GATE, gradientTolerance=1e-6, **KF_A),
    dict(lossFunction=capi.LOSS_L2, maxIterations=200, minSaliency=0.01, parameterTolerance=1e-5, gradientTolerance=1e-4, **KF_B),
    dict(lossFunction=capi.LOSS_TUKEY, maxIterations=200, minSaliency=0.01, minValidDisparity=GATE, **KF_B),
    dict(lossFunction=capi.LOSS_HUBER, maxIterations=3, minSaliency=1.0, **KF_B),
]


def sweep_params(hip, S, first_disparity, one_loss=None):
    """the context's parameters and S distinct sets: SWEEP cycled, the function tolerance scaled by 1 + 0.05 (s // 8)"""
    base = hip.default_params()
    base.verbosity = capi.VERB_SILENT
    base.numPyramidLevels = 4
    base.descriptor = capi.DESC_BITPLANES
    for k, v in KF_A.items():
        setattr(base, k, v)
    gate = float(np.median(first_disparity[first_disparity > 0]))
    out = []
    for s in range(S):
        p = capi.Params.from_buffer_copy(base)
        for k, v in SWEEP[s % len(SWEEP)].items():
            setattr(p, k, gate if v == GATE else v)
        p.functionTolerance = p.functionTolerance * (1.0 + 0.05 * (s // len(SWEEP)))
        if one_loss is not None:
            p.lossFunction = one_loss
        out.append(p)
    return base, out


def run_sweep_contexts(hip, seq, plist, repeats):
    """the same parameter sets as contexts of their own, one after the other over the same frames; ms per frame INDEX over all S contexts (what one
    add_frames call of the sweep context replaces)"""
    runs = []
    for r in range(repeats + 1):             # (pass 0: warm-up)
        t = time.perf_counter()
        for p in plist:
            ctx = hip.create(seq["K"], seq["b"], ROWS, COLS, p, n_frames=3, n_pairs=1)
            for f in seq["frames"]:
                ctx.add_frame(*f)
            ctx.close()
        if r:
            runs.append(1e3 * (time.perf_counter() - t) / FRAMES)
    return dict(ms_per_call=float(np.median(runs)), ms_per_call_runs=[round(x, 4) for x in runs], ms_per_call_min=min(runs), ms_per_call_max=max(runs))


def run_sweep_contexts_kept(hip, seq, plist, repeats):
    """... and with the S contexts created once and advanced round robin (creation and destruction kept out of the timing)"""
    runs = []
    for r in range(repeats + 1):
        ctxs = [hip.create(seq["K"], seq["b"], ROWS, COLS, p, n_frames=3, n_pairs=1) for p in plist]
        t = time.perf_counter()
        for f in seq["frames"]:
            for ctx in ctxs:
                ctx.add_frame(*f)
        if r:
            runs.append(1e3 * (time.perf_counter() - t) / FRAMES)
        for ctx in ctxs:
            ctx.close()
    return dict(ms_per_call=float(np.median(runs)), ms_per_call_runs=[round(x, 4) for x in runs], ms_per_call_min=min(runs), ms_per_call_max=max(runs))


def main_sweep(hip, a):
    seq = synth.make_sequence(ROWS, COLS, FRAMES, index=5, step_rot=0.01, step_trans=0.06)
    out = []
    for S in [int(x) for x in a.sizes.split(",")]:
        base, plist = sweep_params(hip, S, seq["frames"][0][1])
        row = dict(S=S, one_context=run_multi(hip, [seq] * S, False, repeats=a.repeats, seq_params=plist, base=base))
        # the same sets with ONE loss: one estimate per call instead of one per loss (what the partition by loss costs)
        _, same = sweep_params(hip, S, seq["frames"][0][1], one_loss=capi.LOSS_TUKEY)
        row["one_context_one_loss"] = run_multi(hip, [seq] * S, False, repeats=a.repeats, seq_params=same, base=base)
        row["contexts_one_after_the_other"] = run_sweep_contexts(hip, seq, plist, a.repeats)
        row["contexts_round_robin"] = run_sweep_contexts_kept(hip, seq, plist, a.repeats)
        row["speedup_over_contexts_one_after_the_other"] = row["contexts_one_after_the_other"]["ms_per_call"] / row["one_context"]["ms_per_call"]
        row["speedup_over_contexts_round_robin"] = row["contexts_round_robin"]["ms_per_call"] / row["one_context"]["ms_per_call"]
        out.append(row)
        print(json.dumps(row), file=sys.stderr)
    print(json.dumps(dict(bench="multi_sequence_sweep", rows=ROWS, cols=COLS, frames=FRAMES, repeats=a.repeats, results=out)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1,8,32,64")
    ap.add_argument("--only", type=int, default=0, help="one size, add_frames from host buffers only")
    ap.add_argument("--cameras", choices=("shared", "calib", "kitti"), default="shared")
    ap.add_argument("--sweep", action="store_true", help="S parameter sets in one context against S contexts (sizes default to 8,64)")
    ap.add_argument("--repeats", type=int, default=1, help="timed passes per measurement (after the warm-up pass)")
    ap.add_argument("--lib", default="", help="another build of libbpvo_hip.so")
    ap.add_argument("--no-baseline", action="store_true", help="skip the add_frame round robin of the uniform modes")
    a = ap.parse_args()
    if a.sweep and a.sizes == "1,8,32,64":
        a.sizes = "8,64"
        a.repeats = max(a.repeats, 5)
    if a.cameras == "kitti":
        a.sizes = "12"
    try:
        import torch
        if torch.cuda.is_available():
            torch.cuda.init()
    except Exception:
        torch = None
    hip = capi.Binding(os.path.abspath(a.lib), "bpvo_hip_") if a.lib else bpvo_amd.load()
    if a.sweep:
        main_sweep(hip, a)
        return
    cache = {}
    if a.only:
        r = run_multi(hip, frames_for(a.only, cache, a.cameras), False)
        print(json.dumps(dict(bench="multi_sequence", cameras=a.cameras, S=a.only, rows=ROWS, cols=COLS, frames=FRAMES, host=r)))
        return
    out = []
    for S in [int(x) for x in a.sizes.split(",")]:
        seqs = frames_for(S, cache, a.cameras)
        row = dict(S=S, host=run_multi(hip, seqs, False, repeats=a.repeats))
        if torch is not None:
            row["device"] = run_multi(hip, seqs, True, torch, repeats=a.repeats)
        if not a.no_baseline:
            row["add_frame_round_robin"] = run_baseline(hip, seqs)
            row["speedup_host"] = row["host"]["frames_per_s"] / row["add_frame_round_robin"]["frames_per_s"]
        out.append(row)
        print(json.dumps(row), file=sys.stderr)
    print(json.dumps(dict(bench="multi_sequence", cameras=a.cameras, rows=ROWS, cols=COLS, frames=FRAMES, kf_translation=KF_TRANSLATION, results=out)))


if __name__ == "__main__":
    main()
