#!/usr/bin/env python3
"""What the point budget (bpvo_hip_set_point_budget) costs and saves.  Bit-planes frames of 640x480 and 1241x376 (make_sequence inputs), four
pyramid levels, the default selection (non-maximum suppression at the levels of at least 320x240 pixels) — and, with --dense, 640x480 without
non-maximum suppression (conf/tsukuba.cfg's dense templates).  Budgets: none, then 1/2, 1/4 and 1/8 of the unbudgeted point count of level 0,
a quarter of the level below at every level above it (multiples of 16, never below 256).

Per size and budget:
  * template_stage_ms     frame_set_template of one frame, host clock around the call (it synchronises); the unbudgeted row is the stage without
                          the budget's kernel, and `above_every_count` is a budget no level reaches: the kernel runs and leaves at once
  * point_budget_kernel_us  the budget's kernel alone, from HIP events (a profiling pass of its own)
  * add_frames_ms         per add_frames call (one frame of every sequence) for 1 and 64 sequences over a key-framing sequence
Every figure: the median of --repeats (5) passes that ALTERNATE over the budgets inside the same context, with the passes' min and max.
Writes profiles/point_budget_bench.json and prints it as one JSON line.

  python scripts/point_budget_bench.py
  python scripts/point_budget_bench.py --sizes 640x480 --sequences 1 --dense
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

LEVELS, FRAMES, DISTINCT = 4, 12, 4
FRACTIONS = [("none", 0), ("1/2", 2), ("1/4", 4), ("1/8", 8)]
KF_TRANSLATION = 0.065      # about one key frame in four frames of make_sequence's default steps (scripts/multi_sequence_bench.py)


def params(b, dense):
    p = b.default_params()
    p.verbosity = capi.VERB_SILENT
    p.descriptor = capi.DESC_BITPLANES
    p.numPyramidLevels = LEVELS
    p.minTranslationMagToKeyFrame = KF_TRANSLATION
    if dense:
        p.minNumPixelsForNonMaximaSuppression = 1 << 30
    return p


def quartered(finest):
    """the facade's setPointBudget(int): a quarter per level, multiples of 16, never below 256"""
    return [max(256, (finest >> (2 * l)) & ~15) for l in range(LEVELS)]


def summary(runs):
    return dict(median=float(np.median(runs)), min=float(min(runs)), max=float(max(runs)), runs=[round(float(r), 4) for r in runs])


def template_stage(hip, seq, rows, cols, p, repeats, calls=20):
    """frame_set_template of the first frame under every budget, alternating; then the budget's kernel alone from events"""
    ctx = hip.create(seq["K"], seq["b"], rows, cols, p, n_frames=2, n_pairs=1)
    ctx.frame_set_data(0, *seq["frames"][0])
    ctx.frame_set_template(0)
    counts = [ctx.selection_info(0, l)["n_candidates"] for l in range(LEVELS)]
    budgets = [(name, quartered(counts[0] // div) if div else []) for name, div in FRACTIONS] + [("above_every_count", [(c + 16) & ~15 for c in counts])]
    runs = {name: [] for name, _ in budgets}
    for r in range(repeats + 1):                      # (pass 0: warm-up)
        for name, b in budgets:
            ctx.set_point_budget(b)
            ctx.frame_set_template(0)
            t = time.perf_counter()
            for _ in range(calls):
                ctx.frame_set_template(0)
            if r:
                runs[name].append(1e3 * (time.perf_counter() - t) / calls)
    out = {}
    for name, b in budgets:
        ctx.set_point_budget(b)
        ctx.frame_set_template(0)
        ctx.profiling(1)
        for _ in range(calls):
            ctx.frame_set_template(0)
        ks = {k["name"]: k for k in ctx.kernel_stats()}
        ctx.profiling(0)
        pbk, sel = ks["point_budget"], ks["saliency_select"]
        out[name] = dict(budget=b, points=[ctx.num_points(0, l) for l in range(LEVELS)], template_stage_ms=summary(runs[name]),
                         point_budget_kernel_us=(1e3 * pbk["total_ms"] / max(1, calls)) if pbk["launches"] else 0.0,
                         point_budget_launches_per_stage=pbk["launches"] / calls,
                         saliency_select_us=1e3 * sel["total_ms"] / max(1, calls))
    ctx.close()
    return dict(candidates=counts, budgets=out)


def add_frames(hip, seqs, rows, cols, p, S, finest_count, repeats):
    """per add_frames call over FRAMES frames of S sequences, every budget in every pass"""
    ctx = hip.create(seqs[0]["K"], seqs[0]["b"], rows, cols, p, n_frames=3 * S, n_pairs=S)
    imgs = [np.stack([seqs[s % DISTINCT]["frames"][k][0] for s in range(S)]) for k in range(FRAMES)]
    disps = [np.stack([seqs[s % DISTINCT]["frames"][k][1] for s in range(S)]) for k in range(FRAMES)]
    budgets = [(name, quartered(finest_count // div) if div else []) for name, div in FRACTIONS]
    runs = {name: [] for name, _ in budgets}
    info = {}
    for r in range(repeats + 1):                      # (pass 0: warm-up)
        for name, b in budgets:
            ctx.set_point_budget(b)
            for s in range(S):
                ctx.seq_reset(s)
            kf, its = 0, 0
            t = time.perf_counter()
            for k in range(FRAMES):
                res = ctx.add_frames(imgs[k], disps[k])
                kf += sum(q["isKeyFrame"] for q in res) if k else 0
                its += sum(st["numIterations"] for q in res for st in q["stats"])
            if r:
                runs[name].append(1e3 * (time.perf_counter() - t) / FRAMES)
            info[name] = dict(budget=b, kf_fraction=kf / (S * (FRAMES - 1)), iterations_per_frame=its / (S * FRAMES),
                              points=[ctx.seq_num_points_at_level(0, l) for l in range(LEVELS)])
    ctx.close()
    return {name: dict(info[name], add_frames_ms=summary(runs[name])) for name, _ in budgets}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="640x480,1241x376")
    ap.add_argument("--sequences", default="1,64")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--dense", action="store_true", help="also 640x480 without non-maximum suppression (dense templates)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "point_budget_bench.json"))
    a = ap.parse_args()
    try:      # (torch's runtime first, where it is there: tests/conftest.py)
        import torch
        if torch.cuda.is_available():
            torch.cuda.init()
    except Exception:
        pass
    hip = bpvo_amd.load()
    cases = [(int(s.split("x")[1]), int(s.split("x")[0]), False) for s in a.sizes.split(",")]
    if a.dense:
        cases.append((480, 640, True))
    results = []
    for rows, cols, dense in cases:
        seqs = [synth.make_sequence(rows, cols, FRAMES, index=i) for i in range(DISTINCT)]
        p = params(hip, dense)
        row = dict(rows=rows, cols=cols, dense=dense, template=template_stage(hip, seqs[0], rows, cols, p, a.repeats))
        finest = row["template"]["candidates"][0]
        for S in [int(x) for x in a.sequences.split(",")]:
            row[f"add_frames_S{S}"] = add_frames(hip, seqs, rows, cols, p, S, finest, a.repeats)
        results.append(row)
        print(json.dumps(row), file=sys.stderr)
    out = dict(bench="point_budget", levels=LEVELS, frames=FRAMES, repeats=a.repeats, results=results)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
