#!/usr/bin/env python3
"""What the pose covariance costs (option "pose_covariance", bpvo_hip_pose_covariances): wall time per call with the option on against off,
alternating pass by pass (a fresh context per pass, created outside the timed region; first frames — templates only — are not timed), medians
of --repeats passes after a warm-up pass of each; host buffers.
  add_frame    640x480 bit-planes, one sequence
  add_frames   the same frames as S = 8 and S = 64 sequences of one context
  batch        bpvo_hip_pose_covariances (the last estimates) behind a 128-pair 1241x376 bpvo_hip_batch_run, against the batch alone
The expectation was about one more finest-level linearisation per estimate.  Writes profiles/pose_covariance_bench.json and prints it.  A record,
not a bar.  (The pass's kernels have no event timers of their own: the reduction's time per launch is not in here.)

  python scripts/pose_covariance_bench.py
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

KF_TRANSLATION = 0.065      # scripts/multi_sequence_bench.py's: about one key frame in four frames with make_sequence's default steps


def params(b):
    p = b.default_params()
    p.descriptor = capi.DESC_BITPLANES
    p.verbosity = capi.VERB_SILENT
    p.minTranslationMagToKeyFrame = KF_TRANSLATION
    return p


def sequence_pass(hip, seq, S, on):
    """ms per call over the frames after the first; S = 0: bpvo_hip_add_frame"""
    rows, cols = seq["frames"][0][0].shape
    ctx = hip.create(seq["K"], seq["b"], rows, cols, params(hip), n_frames=3 * max(S, 1), n_pairs=max(S, 1))
    ctx.set_option("pose_covariance", on)
    times = []
    for k, (img, disp) in enumerate(seq["frames"]):
        if S:
            imgs, disps = np.stack([img] * S), np.stack([disp] * S)
        t0 = time.perf_counter()
        if S:
            ctx.add_frames(imgs, disps)
        else:
            ctx.add_frame(img, disp)
        if k:
            times.append(1e3 * (time.perf_counter() - t0))
    lin = ctx.total_linearizations()
    ctx.close()
    return float(np.median(times)), lin


def batch_pass(hip, batch, n, ask):
    rows, cols = batch["images"].shape[1:]
    ctx = hip.create(batch["K"], batch["b"], rows, cols, params(hip), n_frames=2 * n, n_pairs=n)
    t0 = time.perf_counter()
    ctx.batch_run(batch["images"], batch["disparities"])
    if ask:
        recs = ctx.pose_covariances(list(range(n)), [2 * i for i in range(n)], [2 * i + 1 for i in range(n)], 0)
        assert all(r["status"] == capi.COV_OK for r in recs)
    ms = 1e3 * (time.perf_counter() - t0)
    ctx.close()
    return ms, 0


def alternate(fn, repeats):
    """fn(on) -> (ms, extra): a warm-up pass of each, then `repeats` alternating passes; medians, spreads and the ratio"""
    fn(0), fn(1)
    off, on, extra = [], [], None
    for _ in range(repeats):
        a, ea = fn(0)
        b, eb = fn(1)
        off.append(a), on.append(b)
        extra = (ea, eb)
    mo, mn = float(np.median(off)), float(np.median(on))
    return dict(off_ms=round(mo, 3), on_ms=round(mn, 3), off_passes=[round(v, 3) for v in off], on_passes=[round(v, 3) for v in on],
                extra_ms=round(mn - mo, 3), ratio=round(mn / mo, 4), total_linearizations_off_on=extra)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--frames", type=int, default=9)
    ap.add_argument("--pairs", type=int, default=128)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_covariance_bench.json"))
    a = ap.parse_args()
    hip = bpvo_amd.load()
    seq = synth.make_sequence(480, 640, a.frames, index=1)
    out = dict(what="wall ms per call, option pose_covariance off / on, medians of alternating passes", repeats=a.repeats, frames=a.frames, rows=[])
    for S in (0, 8, 64):
        r = alternate(lambda on, S=S: sequence_pass(hip, seq, S, on), a.repeats)
        r["case"] = "add_frame 640x480 bit-planes" if S == 0 else "add_frames S = %d, 640x480 bit-planes" % S
        if S:
            r["extra_us_per_sequence"] = round(1e3 * r["extra_ms"] / S, 2)
        out["rows"].append(r)
        print(json.dumps(r), flush=True)
    few = synth.make_batch(376, 1241, 4)
    rep = a.pairs // 4
    batch = dict(K=few["K"], b=few["b"], images=np.concatenate([few["images"]] * rep), disparities=np.concatenate([few["disparities"]] * rep))
    r = alternate(lambda on: batch_pass(hip, batch, 4 * rep, on), a.repeats)
    r["case"] = "bpvo_hip_batch_run of %d pairs 1241x376 bit-planes, alone / followed by bpvo_hip_pose_covariances of all pairs" % (4 * rep)
    r["extra_us_per_pair"] = round(1e3 * r["extra_ms"] / (4 * rep), 2)
    out["rows"].append(r)
    print(json.dumps(r), flush=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
