#!/usr/bin/env python3
"""The Student-t loss against Tukey in the same binary (Tukey's code is the parent's: the yardstick).  640x480, four levels, bit-planes and
intensity: bpvo_hip_add_frame over a sequence, bpvo_hip_add_frames with 64 sequences, bpvo_hip_batch_estimate of 64 and 256 pairs.  Per case
and loss: ms per call (median of 5 alternating passes), GN iterations per estimate, and for Student-t the passes of the scale fit per run of
the stage and the share of linearisations that ran with a frozen scale; then, from one more pass under bpvo_hip_profiling(2), the time of the
scale stage (the "median" row of bpvo_hip_get_kernel_stats: tscale_kernel stands in median_finish's launch) next to warp_residual's.

  python scripts/student_t_bench.py --out profiles/student_t_bench.json
  python scripts/student_t_bench.py --cache /tmp/student_t_inputs.npz      # keep the rendered inputs between runs (rendering is the slow part)
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

ROWS, COLS, LEVELS, FRAMES, DISTINCT, PASSES = 480, 640, 4, 10, 4, 5
LOSSES = {"tukey": capi.LOSS_TUKEY, "student_t": capi.LOSS_STUDENT_T}
DESCRIPTORS = {"bitplanes": capi.DESC_BITPLANES, "intensity": capi.DESC_INTENSITY}


def inputs(cache):
    if cache and os.path.exists(cache):
        z = np.load(cache)
        return {k: z[k] for k in z.files}
    seqs = [synth.make_sequence(ROWS, COLS, FRAMES, index=k) for k in range(DISTINCT)]
    batch = synth.make_batch(ROWS, COLS, 8, first_index=20, workers=8)
    out = dict(K=np.asarray(seqs[0]["K"], np.float32), b=np.float32(seqs[0]["b"]),
               seq_img=np.stack([[f[0] for f in q["frames"]] for q in seqs]), seq_disp=np.stack([[f[1] for f in q["frames"]] for q in seqs]),
               pair_img=batch["images"], pair_disp=batch["disparities"])
    if cache:
        np.savez(cache, **out)
    return out


def params(hip, descriptor, loss):
    p = hip.default_params()
    p.verbosity = capi.VERB_SILENT
    p.numPyramidLevels = LEVELS
    p.descriptor = DESCRIPTORS[descriptor]
    p.lossFunction = LOSSES[loss]
    p.minTranslationMagToKeyFrame = 0.065
    return p


def counters(ctx, calls_estimates):
    lin = ctx.total_linearizations()
    stages, passes = ctx.tscale_counts()
    out = dict(gn_iterations_per_estimate=round(lin / max(calls_estimates, 1), 2))
    if stages:
        out.update(tscale_passes_per_stage=round(passes / stages, 2), tscale_stages_per_linearisation=round(stages / max(lin, 1), 3),
                   share_of_linearisations_frozen=round(1.0 - stages / max(lin, 1), 3))
    return out


def stage_times(ctx):
    rows = {k["name"]: k for k in ctx.kernel_stats()}
    pick = lambda name: next((v for k, v in rows.items() if name in k), None)
    out = {}
    for label, name in (("scale_stage", "median"), ("warp_residual", "warp_residual"), ("irls_reduce", "irls_reduce")):
        k = pick(name)
        if k:
            out[label] = dict(launches=int(k["launches"]), total_ms=round(k["total_ms"], 3), us_per_launch=round(1e3 * k["total_ms"] / max(k["launches"], 1), 2))
    return out


class AddFrame:
    def __init__(self, hip, inp, descriptor, loss):
        self.ctx = hip.create(inp["K"], float(inp["b"]), ROWS, COLS, params(hip, descriptor, loss))
        self.img, self.disp = inp["seq_img"][0], inp["seq_disp"][0]
        self.estimates = FRAMES - 1
        self.ctx.add_frame(self.img[0], self.disp[0])      # the first frame; the passes then walk the sequence forth and back
        self.forward = True

    def one_pass(self):
        t = []
        for k in (range(1, FRAMES) if self.forward else range(FRAMES - 2, -1, -1)):
            t0 = time.perf_counter()
            self.ctx.add_frame(self.img[k], self.disp[k])
            t.append(time.perf_counter() - t0)
        self.forward = not self.forward
        return 1e3 * float(np.median(t))


class AddFrames:
    S = 64

    def __init__(self, hip, inp, descriptor, loss):
        S = self.S
        self.ctx = hip.create(inp["K"], float(inp["b"]), ROWS, COLS, params(hip, descriptor, loss), n_frames=3 * S, n_pairs=S)
        pick = np.arange(S) % DISTINCT
        self.imgs = [np.ascontiguousarray(inp["seq_img"][pick, k]) for k in range(FRAMES)]
        self.disps = [np.ascontiguousarray(inp["seq_disp"][pick, k]) for k in range(FRAMES)]
        self.estimates = S * (FRAMES - 1)

    def one_pass(self):
        t = []
        for s in range(self.S):
            self.ctx.seq_reset(s)
        for k in range(FRAMES):
            t0 = time.perf_counter()
            self.ctx.add_frames(self.imgs[k], self.disps[k])
            t.append(time.perf_counter() - t0)
        return 1e3 * float(np.median(t[1:]))


class Batch:
    def __init__(self, hip, inp, descriptor, loss, n):
        self.n = n
        self.ctx = hip.create(inp["K"], float(inp["b"]), ROWS, COLS, params(hip, descriptor, loss), n_frames=2 * n, n_pairs=n)
        pick = np.arange(n) % (len(inp["pair_img"]) // 2)
        idx = np.stack([2 * pick, 2 * pick + 1], axis=1).reshape(-1)
        self.ctx.frames_set_data(0, 1, np.ascontiguousarray(inp["pair_img"][idx]), np.ascontiguousarray(inp["pair_disp"][idx]))
        self.ctx.frames_set_template(0, 2, n)
        self.estimates = n

    def one_pass(self):
        t0 = time.perf_counter()
        self.ctx.batch_estimate(self.n)
        return 1e3 * (time.perf_counter() - t0)


def measure(make, profile=True):
    """5 alternating passes of the two losses after a warm-up pass each; then one pass each with every kernel timed"""
    runs = {loss: make(loss) for loss in LOSSES}
    for r in runs.values():
        r.one_pass()
    ms = {loss: [] for loss in LOSSES}
    for r in runs.values():
        r.ctx.profiling(0)      # (resets the counters)
    for _ in range(PASSES):
        for loss, r in runs.items():
            ms[loss].append(r.one_pass())
    out = {}
    for loss, r in runs.items():
        out[loss] = dict(ms_per_call=round(float(np.median(ms[loss])), 3), ms_min=round(min(ms[loss]), 3), ms_max=round(max(ms[loss]), 3),
                         **counters(r.ctx, PASSES * r.estimates))
        if profile:
            r.ctx.profiling(2)
            r.one_pass()
            out[loss]["kernels_all_timed"] = stage_times(r.ctx)
            r.ctx.profiling(0)
        r.ctx.close()
    out["student_t_over_tukey"] = round(out["student_t"]["ms_per_call"] / out["tukey"]["ms_per_call"], 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--cache", default=None)
    ap.add_argument("--render-only", action="store_true", help="fill --cache and stop (no GPU needed)")
    ap.add_argument("--skip", default="", help="comma-separated cases to leave out: add_frame, add_frames_64, batch_64, batch_256")
    a = ap.parse_args()
    inp = inputs(a.cache)
    if a.render_only:
        return
    hip = bpvo_amd.load()
    skip = set(a.skip.split(","))
    res = dict(rows=ROWS, cols=COLS, levels=LEVELS, passes=PASSES, cases={})
    for descriptor in DESCRIPTORS:
        cases = {"add_frame": lambda loss: AddFrame(hip, inp, descriptor, loss), "add_frames_64": lambda loss: AddFrames(hip, inp, descriptor, loss),
                 "batch_64": lambda loss: Batch(hip, inp, descriptor, loss, 64), "batch_256": lambda loss: Batch(hip, inp, descriptor, loss, 256)}
        for name, make in cases.items():
            if name in skip:
                continue
            res["cases"][f"{descriptor}/{name}"] = measure(make)
            print(f"{descriptor}/{name}", json.dumps(res["cases"][f"{descriptor}/{name}"]), flush=True)
    line = json.dumps(res, indent=1)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
