#!/usr/bin/env python3
"""Timing of the stereo front-end for many cameras (bpvo_hip_stereo_frames, bpvo_hip_add_frames_stereo).  Prints one JSON line.

  front-end   ms per frame for 16 pairs resident in HBM at 1241x376 / 128 disparities, 640x480 / 64 and 320x240 / 64, block matching and SGM:
              bpvo_hip_stereo_frames where the library has it, bpvo_hip_stereo_bm otherwise (a build of the commit before it: --lib), SGM
              once per value of --per-launch (option "stereo_frames_per_launch"; 0 = the automatic rule) with the frames per launch it used
  whole call  16 sequences of the context's size (640x480, block matching / 64) advanced by bpvo_hip_stereo_bm device -> device +
              bpvo_hip_add_frames(on_device = 1), and by one bpvo_hip_add_frames_stereo call where the library has it
  mixed rig   the three KITTI geometries, 640x480 and 320x240 in one bpvo_hip_add_frames_stereo call, next to the sum of five contexts of
              their own driven by bpvo_hip_add_frame_stereo

Every figure: the median of --reps wall-clock repetitions after --warmup unmeasured ones, each ending in a device synchronisation (the
entry points synchronise themselves), with the spread (min, max) beside it.

  python scripts/stereo_sequences_bench.py [--lib path/to/libbpvo_hip.so] [--reps 20] [--per-launch 0,1,4,16]
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

KITTI = [(376, 1241, 718.856, 607.1928, 185.2157, 0.5372), (375, 1242, 721.5377, 609.5593, 172.854, 0.5371),
         (370, 1226, 707.0912, 601.8873, 183.1104, 0.5372)]
N = 16


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return dict(median_ms=float(np.median(ts)), min_ms=float(min(ts)), max_ms=float(max(ts)))


def params(b, levels=4):
    p = b.default_params()
    p.verbosity = capi.VERB_SILENT
    p.numPyramidLevels = levels
    return p


def stereo_params(ctx, algo, ndisp):
    sp = ctx.default_stereo_params(ndisp)
    if algo == "sgm":
        sp.algorithm = capi.STEREO_SGM
    return sp


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--per-launch", default="0,1,4,16")
    ap.add_argument("--skip-calls", action="store_true", help="front-end only")
    a = ap.parse_args()
    import torch
    torch.cuda.init()
    hip = capi.Binding(os.path.abspath(a.lib), "bpvo_hip_") if a.lib else bpvo_amd.load()
    new = hip.has("stereo_frames")
    out = dict(library=a.lib or "product", entry="bpvo_hip_stereo_frames" if new else "bpvo_hip_stereo_bm", reps=a.reps, front_end={})

    # ---- front-end only
    for rows, cols, ndisp in ((376, 1241, 128), (480, 640, 64), (240, 320, 64)):
        pairs = [synth.make_stereo_pair(rows, cols, i % 4) for i in range(4)]
        L = np.stack([pairs[i % 4]["left"] for i in range(N)])
        R = np.stack([pairs[i % 4]["right"] for i in range(N)])
        tl, tr = torch.from_numpy(L).cuda(), torch.from_numpy(R).cuda()
        td = torch.empty((N, rows, cols), dtype=torch.float32, device="cuda")
        K, b = synth.calibration(rows, cols)
        ctx = hip.create(K, b, rows, cols, params(hip, 2), n_frames=3, n_pairs=1)
        for algo in ("bm", "sgm"):
            sp = stereo_params(ctx, algo, ndisp)
            if new:
                cams = ctx._camera_array([(rows, cols)] * N)      # (built once: the call is what is timed)
                run = lambda: ctx.stereo_frames_device(cams, tl.data_ptr(), tr.data_ptr(), sp, td.data_ptr())
            else:
                run = lambda: ctx.stereo_bm_device(N, tl.data_ptr(), tr.data_ptr(), sp, td.data_ptr())
            settings = [int(v) for v in a.per_launch.split(",")] if (new and algo == "sgm") else [None]
            for per in settings:
                if per is not None:
                    ctx.set_option("stereo_frames_per_launch", per)
                t = timed(run, a.warmup, a.reps)
                rec = {k: v / N for k, v in t.items()}      # per frame
                name = f"{algo} {cols}x{rows} / {ndisp}" + (f" per_launch={per}" if per is not None else "")
                if per is not None:
                    rec["frames_per_launch_used"] = ctx.get_option("stereo_frames_per_launch_seen")
                    rec["free_mib_seen"] = ctx.get_option("stereo_free_mib_seen")
                out["front_end"][name] = rec
                print(name, json.dumps(rec), file=sys.stderr, flush=True)
            if new:
                ctx.set_option("stereo_frames_per_launch", 0)
        ctx.close()
        del tl, tr, td

    if not a.skip_calls:
        # ---- whole call: 16 sequences of the context's size
        rows, cols, ndisp, frames = 480, 640, 64, 6
        seqs = [synth.make_stereo_sequence(rows, cols, frames, index=40 + s % 4)["frames"] for s in range(4)]
        K, b = synth.calibration(rows, cols)
        stacks = [(torch.from_numpy(np.stack([seqs[s % 4][k][0] for s in range(N)])).cuda(), torch.from_numpy(np.stack([seqs[s % 4][k][1] for s in range(N)])).cuda())
                  for k in range(frames)]
        td = torch.empty((N, rows, cols), dtype=torch.float32, device="cuda")
        ctx = hip.create(K, b, rows, cols, params(hip), n_frames=3 * N, n_pairs=N)
        sp = stereo_params(ctx, "bm", ndisp)
        state = dict(k=0)

        def composed():
            tl, tr = stacks[state["k"] % frames]
            state["k"] += 1
            ctx.stereo_bm_device(N, tl.data_ptr(), tr.data_ptr(), sp, td.data_ptr())
            ctx.add_frames_device(N, tl.data_ptr(), td.data_ptr())

        def one_call():
            tl, tr = stacks[state["k"] % frames]
            state["k"] += 1
            ctx.add_frames_stereo_device(N, tl.data_ptr(), tr.data_ptr(), sp)

        out["whole_call_16x640x480_bm"] = dict(composed=timed(composed, a.warmup, a.reps))
        if new:
            for s in range(N):
                ctx.seq_reset(s)
            state["k"] = 0
            out["whole_call_16x640x480_bm"]["add_frames_stereo"] = timed(one_call, a.warmup, a.reps)
        ctx.close()

        # ---- mixed rig (information)
        cams = [(np.array([[fx, 0, cx], [0, fx, cy], [0, 0, 1]], np.float32), bb, r, c) for r, c, fx, cx, cy, bb in KITTI]
        for (r, c), bb in (((480, 640), 0.12), ((240, 320), 0.09)):
            cams.append((np.asarray(synth.calibration(r, c)[0], np.float32).reshape(3, 3), bb, r, c))
        rig = [synth.make_stereo_sequence(r, c, frames, index=50 + s, camera=(Kc, bb))["frames"] for s, (Kc, bb, r, c) in enumerate(cams)]
        own = [hip.create(Kc, bb, r, c, params(hip), n_frames=3, n_pairs=1) for Kc, bb, r, c in cams]
        spo = stereo_params(own[0], "bm", ndisp)
        state["k"] = 0

        def five_contexts():
            k = state["k"] % frames
            state["k"] += 1
            for s, cx in enumerate(own):
                cx.add_frame_stereo(rig[s][k][0], rig[s][k][1], spo)

        out["mixed_rig_bm"] = dict(five_own_contexts_add_frame_stereo=timed(five_contexts, a.warmup, a.reps))
        for cx in own:
            cx.close()
        if new:
            ctx = hip.create_sequences(cams, params(hip))
            state["k"] = 0

            def rig_call():
                k = state["k"] % frames
                state["k"] += 1
                ctx.add_frames_stereo([rig[s][k][0] for s in range(5)], [rig[s][k][1] for s in range(5)], spo)

            out["mixed_rig_bm"]["one_add_frames_stereo_call"] = timed(rig_call, a.warmup, a.reps)
            ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
