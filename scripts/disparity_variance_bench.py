#!/usr/bin/env python3
"""What the measurement variance costs (c_api.h "measurement variance"), on one GPU.  Written to profiles/disparity_variance_bench.json and printed; a
record, not a bar.

  kernel      the one launch of bpvo_hip_disparity_variance_frames for 1 / 16 / 64 pairs at 640x480 and 1241x376, radii 1 / 3 / 7, device-resident
              inputs and output, HIP events around the launch (option "variance_last_kernel_ms" under bpvo_hip_profiling).  Two kinds of maps: a
              smooth one (every tile stages its right strip in LDS) and independent random disparities in [1, 280] per pixel (most tiles read the
              right image directly).  Algorithmic bytes: 10 per pixel — L and R once (2 B), M (4 B), the map written (4 B) —, reported against the
              8 TB/s peak; the tile counts of each path are kept beside it.
  whole call  bpvo_hip_add_frames_stereo (block matching, 64 disparities, 640x480 bit-planes) for 1 and 64 sequences that fuse their disparities,
              with the variance off and on alternating in one run; with --parent-lib, the parent commit's library (fusion on: its only form)
              alternates with them, and its difference to "variance off" stands beside the passes' spread.
Every figure is the median of --passes alternating passes behind a warm-up pass; the passes themselves are kept so that their spread can be seen."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OUT = os.path.join(ROOT, "profiles", "disparity_variance_bench.json")
SIZES = ((480, 640), (376, 1241))
COUNTS = (1, 16, 64)
RADII = (1, 3, 7)
FUSION = dict(mode=1, measurement_sigma=0.5, process_sigma=0.1, gate=3.0, max_fill_sigma=2.0)
VARIANCE = dict(mode=1, radius=2, noise_sigma=2.0, min_sigma=0.02, max_sigma=2.0)
VO_FRAMES = 6
PEAK_TB_S = 8.0


def stats(passes, digits=3):
    return dict(median=round(float(np.median(passes)), digits), min=round(float(min(passes)), digits), max=round(float(max(passes)), digits),
                passes=[round(float(v), digits) for v in passes])


def kernel(hip, capi, synth, passes, calls):
    import torch
    out = []
    for rows, cols in SIZES:
        pair = synth.make_stereo_pair(rows, cols, 0)
        maps = dict(smooth=np.asarray(pair["disp"], np.float32),
                    random=np.random.default_rng(3).integers(1, 281, (rows, cols)).astype(np.float32))
        p = hip.default_params()
        p.numPyramidLevels = 1
        p.verbosity = capi.VERB_SILENT
        ctx = hip.create(pair["K"], pair["b"], rows, cols, p, n_frames=3, n_pairs=1)
        ctx.profiling(1)
        nmax = max(COUNTS)
        dL = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(pair["left"], (nmax, rows, cols)))).cuda()
        dR = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(pair["right"], (nmax, rows, cols)))).cuda()
        dM = {k: torch.from_numpy(np.ascontiguousarray(np.broadcast_to(m, (nmax, rows, cols)))).cuda() for k, m in maps.items()}
        dO = torch.empty((nmax, rows, cols), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        cases = [(kind, n, r) for kind in maps for n in COUNTS for r in RADII]
        samples = {c: [] for c in cases}
        tiles = {}
        for k in range(passes + 1):      # (pass 0 warms up)
            for case in cases:
                kind, n, r = case
                cams = ctx._camera_array([(rows, cols)] * n)
                ms = []
                t0 = ctx.measurement_variance_counts()[2]
                for _ in range(calls):
                    ctx.disparity_variance_frames_device(cams, dL.data_ptr(), dR.data_ptr(), dM[kind].data_ptr(), p.minValidDisparity, p.maxValidDisparity,
                                                         dict(VARIANCE, radius=r), dO.data_ptr())
                    ms.append(ctx.get_option("variance_last_kernel_ms"))
                t1 = ctx.measurement_variance_counts()[2]
                tiles[case] = [int(b - a) // calls for a, b in zip(t0, t1)]
                if k:
                    samples[case].append(1e3 * float(np.median(ms)))
        ctx.close()
        for case in cases:
            kind, n, r = case
            us = float(np.median(samples[case]))
            px = rows * cols * n
            row = dict(rows=rows, cols=cols, pairs=n, radius=r, map=kind, kernel_us=stats(samples[case]), tiles_staged_direct_idle=tiles[case],
                       algorithmic_tb_per_s=round(10.0 * px / us * 1e-6, 4), share_of_peak=round(10.0 * px / us * 1e-6 / PEAK_TB_S, 4),
                       ns_per_pixel=round(1e3 * us / px, 4), window_terms_per_ns=round(3.0 * (2 * r + 1) ** 2 * px / (1e3 * us), 1))
            out.append(row)
            print(json.dumps(row), flush=True)
    return out


def whole_calls(hip, capi, synth, passes, parent_lib):
    rows, cols = 480, 640
    seq = synth.make_stereo_sequence(rows, cols, VO_FRAMES, index=0)
    libs = {"variance_off": hip, "variance_on": hip}
    if parent_lib:
        libs["parent"] = capi.Binding(parent_lib, "bpvo_hip_")
    out = {}
    for kind, n in (("add_frames_stereo_x1", 1), ("add_frames_stereo_x64", 64)):
        lefts = [np.ascontiguousarray(np.broadcast_to(f[0], (n, rows, cols))) for f in seq["frames"]]
        rights = [np.ascontiguousarray(np.broadcast_to(f[1], (n, rows, cols))) for f in seq["frames"]]
        samples = {name: [] for name in libs}
        for k in range(passes + 1):
            for name, lib in libs.items():
                p = lib.default_params()
                p.descriptor = capi.DESC_BITPLANES
                p.verbosity = capi.VERB_SILENT
                ctx = lib.create(seq["K"], seq["b"], rows, cols, p, n_frames=3 * n, n_pairs=n)
                ctx.set_disparity_fusion(FUSION)
                if name == "variance_on":
                    ctx.set_measurement_variance(VARIANCE)
                sp = ctx.default_stereo_params(ndisp=64)
                per_call = []
                for f in range(VO_FRAMES):
                    t0 = time.perf_counter()
                    ctx.add_frames_stereo(lefts[f], rights[f], sp)
                    ctx.seq_disparity_fusion_info(0)      # (the last stage has finished: its counters are in)
                    per_call.append(1e3 * (time.perf_counter() - t0))
                ctx.close()
                if k:
                    samples[name].append(float(np.median(per_call[1:])))      # (the first frame estimates nothing)
        out[kind] = {name: stats(v) for name, v in samples.items()}
        out[kind]["feature_cost_ms"] = round(out[kind]["variance_on"]["median"] - out[kind]["variance_off"]["median"], 3)
        if parent_lib:
            out[kind]["variance_off_minus_parent_ms"] = round(out[kind]["variance_off"]["median"] - out[kind]["parent"]["median"], 3)
            out[kind]["spread_of_the_passes_ms"] = round(max(out[kind][name]["max"] - out[kind][name]["min"] for name in ("variance_off", "parent")), 3)
        print(kind, json.dumps(out[kind]), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--parent-lib", default=None, help="libbpvo_hip.so built from the parent commit (variance off against it)")
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    import torch
    torch.cuda.init()      # (torch's runtime first: tests/conftest.py says why)
    import bpvo_amd
    from bpvo_amd import capi, synth
    hip = bpvo_amd.load()
    res = dict(passes=a.passes, calls_per_pass=a.calls, fusion=FUSION, variance=VARIANCE, bytes_per_pixel=10, peak_tb_per_s=PEAK_TB_S,
               kernel=kernel(hip, capi, synth, a.passes, a.calls),
               whole_calls=whole_calls(hip, capi, synth, a.passes, a.parent_lib))
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
