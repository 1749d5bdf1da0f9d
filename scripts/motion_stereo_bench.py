#!/usr/bin/env python3
"""What motion stereo costs (c_api.h "motion stereo"), on one GPU.  Written to profiles/motion_stereo_bench.json and printed; a record, not a bar.

  kernel      the one launch of bpvo_hip_motion_stereo_frames for 1 / 16 / 64 pairs of views at 640x480 and 1241x376, radius 1 / 2 / 3 with steps
              2 / 4 / 8, device-resident inputs and outputs, HIP events around the launch (option "motion_stereo_last_kernel_ms" under
              bpvo_hip_profiling).  The pair is two frames of synth's plane a sideways step apart, the prior the frame's own disparity map with
              variance 0.25; the class counts and the tile paths of a launch are kept beside its time.  Terms: one squared difference of the
              window, (2 radius + 1)^2 (2 steps + 1) per pixel that reaches the sums (every class from "edge" on).  Algorithmic bytes: 18 per
              pixel — C and K once (2 B), the two prior maps (8 B), the two maps written (8 B) —, reported against the 8 TB/s peak.
  whole call  bpvo_hip_add_frames (640x480 bit-planes) for 1 and 64 sequences that fuse their disparities, with motion stereo off and on
              alternating in one run; with --parent-lib, the parent commit's library (fusion on) alternates with them, and its difference to
              "off" stands beside the passes' spread.
Every figure is the median of --passes alternating passes behind a warm-up pass; the passes themselves are kept so that their spread can be seen."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OUT = os.path.join(ROOT, "profiles", "motion_stereo_bench.json")
SIZES = ((480, 640), (376, 1241))
COUNTS = (1, 16, 64)
SETTINGS = ((1, 2), (2, 4), (3, 8))      # (radius, steps)
FUSION = dict(mode=1, measurement_sigma=0.5, process_sigma=0.1, gate=3.0, max_fill_sigma=2.0)
MOTION_STEREO = dict(mode=1, radius=2, steps=4, min_gain=0.25, noise_sigma=2.0, min_sigma=0.02, max_sigma=2.0, gate=3.0)
CLASSES = ("no_prior", "low_parallax", "border", "edge", "flat", "rejected", "fused")
VO_FRAMES = 6
PEAK_TB_S = 8.0
SIDEWAYS = 0.3      # metres between the two views: a gain of 3 pixels per disparity pixel at synth's baseline of 0.1 m (640x480)


def stats(passes, digits=3):
    return dict(median=round(float(np.median(passes)), digits), min=round(float(min(passes)), digits), max=round(float(max(passes)), digits),
                passes=[round(float(v), digits) for v in passes])


def kernel(hip, capi, synth, passes, calls):
    import torch
    out = []
    for rows, cols in SIZES:
        seq = synth.make_sequence_steps(rows, cols, [SIDEWAYS], (1.0, 0.0, 0.0), (0.0, 0.0, 0.0))
        (img0, _), (img1, d1) = seq["frames"]
        Q = np.linalg.inv(seq["poses"][1]).astype(np.float32)      # the frame is the first view, the frame before the second
        p = hip.default_params()
        p.numPyramidLevels = 1
        p.verbosity = capi.VERB_SILENT
        ctx = hip.create(seq["K"], seq["b"], rows, cols, p, n_frames=3, n_pairs=1)
        ctx.profiling(1)
        nmax = max(COUNTS)
        rep = lambda a: torch.from_numpy(np.ascontiguousarray(np.broadcast_to(a, (nmax, rows, cols)))).cuda()
        dC, dK, dPD = rep(img1), rep(img0), rep(np.asarray(d1, np.float32))
        dPV = rep(np.full((rows, cols), 0.25, np.float32))
        dD = torch.empty((nmax, rows, cols), dtype=torch.float32, device="cuda")
        dV = torch.empty((nmax, rows, cols), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        cases = [(n, r, j) for n in COUNTS for r, j in SETTINGS]
        samples = {c: [] for c in cases}
        tiles, classes = {}, {}
        for k in range(passes + 1):      # (pass 0 warms up)
            for case in cases:
                n, r, j = case
                ctx.set_motion_stereo(dict(MOTION_STEREO, radius=r, steps=j))
                cams = ctx._camera_array([(seq["K"], seq["b"], rows, cols)] * n)
                Qs = np.broadcast_to(Q, (n, 4, 4))
                ms = []
                c0 = ctx.motion_stereo_counts()
                for _ in range(calls):
                    ctx.motion_stereo_frames_device(cams, dC.data_ptr(), dK.data_ptr(), Qs, dPD.data_ptr(), dPV.data_ptr(), dD.data_ptr(), dV.data_ptr())
                    ms.append(ctx.get_option("motion_stereo_last_kernel_ms"))
                c1 = ctx.motion_stereo_counts()
                tiles[case] = [int(b - a) // calls for a, b in zip(c0[2], c1[2])]
                classes[case] = {name: int(c1[3][name] - c0[3][name]) // calls for name in CLASSES}
                if k:
                    samples[case].append(1e3 * float(np.median(ms)))
        ctx.close()
        for case in cases:
            n, r, j = case
            us = float(np.median(samples[case]))
            px = rows * cols * n
            searched = sum(classes[case][name] for name in ("edge", "flat", "rejected", "fused"))
            terms = (2 * r + 1) ** 2 * (2 * j + 1) * searched
            row = dict(rows=rows, cols=cols, pairs=n, radius=r, steps=j, kernel_us=stats(samples[case]), tiles_staged_direct_idle=tiles[case],
                       classes=classes[case], pixels_searched=searched, ns_per_pixel=round(1e3 * us / px, 4),
                       window_terms_per_ns=round(terms / (1e3 * us), 1), algorithmic_tb_per_s=round(18.0 * px / us * 1e-6, 4),
                       share_of_peak=round(18.0 * px / us * 1e-6 / PEAK_TB_S, 4))
            out.append(row)
            print(json.dumps(row), flush=True)
    return out


def whole_calls(hip, capi, synth, passes, parent_lib):
    rows, cols = 480, 640
    seq = synth.make_sequence(rows, cols, VO_FRAMES, index=0)
    libs = {"off": hip, "on": hip}
    if parent_lib:
        libs["parent"] = capi.Binding(parent_lib, "bpvo_hip_")
    out = {}
    for kind, n in (("add_frames_x1", 1), ("add_frames_x64", 64)):
        imgs = [np.ascontiguousarray(np.broadcast_to(f[0], (n, rows, cols))) for f in seq["frames"]]
        disps = [np.ascontiguousarray(np.broadcast_to(f[1], (n, rows, cols))) for f in seq["frames"]]
        samples = {name: [] for name in libs}
        for k in range(passes + 1):
            for name, lib in libs.items():
                p = lib.default_params()
                p.descriptor = capi.DESC_BITPLANES
                p.verbosity = capi.VERB_SILENT
                ctx = lib.create(seq["K"], seq["b"], rows, cols, p, n_frames=3 * n, n_pairs=n)
                ctx.set_disparity_fusion(FUSION)
                if name == "on":
                    ctx.set_motion_stereo(MOTION_STEREO)
                per_call = []
                for f in range(VO_FRAMES):
                    t0 = time.perf_counter()
                    ctx.add_frames(imgs[f], disps[f])
                    ctx.seq_disparity_fusion_info(0)      # (the last stage has finished: its counters are in)
                    per_call.append(1e3 * (time.perf_counter() - t0))
                ctx.close()
                if k:
                    samples[name].append(float(np.median(per_call[1:])))      # (the first frame estimates nothing)
        out[kind] = {name: stats(v) for name, v in samples.items()}
        out[kind]["feature_cost_ms"] = round(out[kind]["on"]["median"] - out[kind]["off"]["median"], 3)
        if parent_lib:
            out[kind]["off_minus_parent_ms"] = round(out[kind]["off"]["median"] - out[kind]["parent"]["median"], 3)
            out[kind]["spread_of_the_passes_ms"] = round(max(out[kind][name]["max"] - out[kind][name]["min"] for name in ("off", "parent")), 3)
        print(kind, json.dumps(out[kind]), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--parent-lib", default=None, help="libbpvo_hip.so built from the parent commit (motion stereo off against it)")
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    import torch
    torch.cuda.init()      # (torch's runtime first: tests/conftest.py says why)
    import bpvo_amd
    from bpvo_amd import capi, synth
    hip = bpvo_amd.load()
    res = dict(passes=a.passes, calls_per_pass=a.calls, fusion=FUSION, motion_stereo=MOTION_STEREO, sideways_m=SIDEWAYS, bytes_per_pixel=18,
               peak_tb_per_s=PEAK_TB_S, kernel=kernel(hip, capi, synth, a.passes, a.calls),
               whole_calls=whole_calls(hip, capi, synth, a.passes, a.parent_lib))
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
