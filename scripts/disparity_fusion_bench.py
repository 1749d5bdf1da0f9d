#!/usr/bin/env python3
"""What disparity fusion costs (c_api.h "disparity fusion"), on one GPU.  Written to profiles/disparity_fusion_bench.json and printed; a record, not a bar.

  kernels     the two launches of a stage (splat, update) for 1 / 16 / 64 sequences at 640x480 and 1241x376 through bpvo_hip_fuse_disparities,
              the maps and motions of synth.make_sequence's plane (frames 1 and 2 alternating on carried maps of the other), HIP events around
              each launch (options "fusion_last_splat_ms" / "fusion_last_update_ms" under bpvo_hip_profiling).  Algorithmic bytes, as counted
              from the kernels: the splat reads Dc and Vc (8 B per pixel) and sends one 8-byte max atomic per surviving candidate; the update
              reads M and the z-buffer word (12 B), writes the slot, Dc and Vc (12 B) and a zero word where a candidate had arrived (8 B).  The
              candidates are counted by the numpy statement of the rule on the same inputs.  The splat's atomic rate = candidates x 8 B / its time.
  whole call  bpvo_hip_add_frame, and bpvo_hip_add_frames over 64 sequences, 640x480 bit-planes, with mode 0 and mode 1 alternating in one run;
              with --parent-lib, the parent commit's library in mode 0 alternates with them (the bar: within the passes' own spread).
  host        tests/cpp/disparity_fusion_harness.cc: the same rule as a single-thread C++ loop on this machine's host, for scale.
Every figure is the median of --passes alternating passes behind a warm-up pass; the passes themselves are kept so that their spread can be seen."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

OUT = os.path.join(ROOT, "profiles", "disparity_fusion_bench.json")
SIZES = ((480, 640), (376, 1241))
COUNTS = (1, 16, 64)
FUSION = dict(mode=1, measurement_sigma=0.5, process_sigma=0.1, gate=3.0, max_fill_sigma=2.0)
VO_FRAMES = 8


def stats(passes, digits=3):
    return dict(median=round(float(np.median(passes)), digits), min=round(float(min(passes)), digits), max=round(float(max(passes)), digits),
                passes=[round(float(v), digits) for v in passes])


def frames_and_motions(synth, rows, cols, n):
    seq = synth.make_sequence(rows, cols, n)
    rel = [np.eye(4, dtype=np.float32)] + [(seq["poses"][k] @ np.linalg.inv(seq["poses"][k - 1])).astype(np.float32) for k in range(1, n)]
    return seq, rel


def kernels(hip, capi, synth, ref, passes, calls):
    out = []
    for rows, cols in SIZES:
        seq, rel = frames_and_motions(synth, rows, cols, 3)
        p = hip.default_params()
        p.numPyramidLevels = 1
        p.verbosity = capi.VERB_SILENT
        K = np.asarray(seq["K"], np.float32)
        cam = ref.camera(rows, cols, fx=K[0, 0], fy=K[1, 1], cx=K[0, 2], cy=K[1, 2], b=seq["b"], lo=p.minValidDisparity, hi=p.maxValidDisparity)
        prm = ref.rule(FUSION["measurement_sigma"], FUSION["process_sigma"], FUSION["gate"], FUSION["max_fill_sigma"])
        # what a stage moves, from the numpy statement: frame 2 fused onto the carried maps of frames 0 -> 1
        D0, V0, _ = ref.step(cam, prm, seq["frames"][0][1])
        D1, V1, _ = ref.step(cam, prm, seq["frames"][1][1], D0, V0, rel[1])
        z = ref.splat(cam, prm, D1, V1, rel[2])
        carried = int((V1 >= 0).sum())
        survivors = int(ref.candidates(cam, prm, D1, V1, rel[2])[0].size)      # (one atomic each)
        row = dict(rows=rows, cols=cols, pixels=rows * cols, carried_pixels=carried, candidates=survivors, targets_hit=int(np.count_nonzero(z)), counts={})
        ctxs = {}
        for n in COUNTS:
            ctx = hip.create(seq["K"], seq["b"], rows, cols, p, n_frames=3 * n, n_pairs=n)
            ctx.set_disparity_fusion(FUSION)
            ctx.profiling(1)
            ctx.fuse_disparities([seq["frames"][0][1]] * n, [rel[0]] * n)
            ctx.fuse_disparities([seq["frames"][1][1]] * n, [rel[1]] * n)
            ctxs[n] = ctx
        samples = {n: dict(splat=[], update=[]) for n in COUNTS}
        for k in range(passes + 1):      # (pass 0 warms up)
            for n in COUNTS:
                ctx, sp, up = ctxs[n], [], []
                for c in range(calls):
                    f = 2 if c % 2 == 0 else 1      # (forth and back: the carried maps stay those of neighbouring frames)
                    P = rel[2] if f == 2 else np.linalg.inv(rel[2]).astype(np.float32)
                    ctx.fuse_disparities([seq["frames"][f][1]] * n, [P] * n)
                    sp.append(ctx.get_option("fusion_last_splat_ms"))
                    up.append(ctx.get_option("fusion_last_update_ms"))
                if k:
                    samples[n]["splat"].append(1e3 * float(np.median(sp)))
                    samples[n]["update"].append(1e3 * float(np.median(up)))
        for n in COUNTS:
            ctxs[n].close()
            s_us, u_us = float(np.median(samples[n]["splat"])), float(np.median(samples[n]["update"]))
            px = rows * cols * n
            splat_bytes = 8.0 * px + 8.0 * survivors * n
            update_bytes = 24.0 * px + 8.0 * row["targets_hit"] * n
            row["counts"][str(n)] = dict(
                splat_us=stats(samples[n]["splat"]), update_us=stats(samples[n]["update"]),
                splat_bytes_per_pixel=round(splat_bytes / px, 2), update_bytes_per_pixel=round(update_bytes / px, 2),
                splat_tb_per_s=round(splat_bytes / s_us * 1e-6, 3), update_tb_per_s=round(update_bytes / u_us * 1e-6, 3),
                splat_atomic_tb_per_s=round(8.0 * survivors * n / s_us * 1e-6, 3), splat_atomics_per_us=round(survivors * n / s_us, 1))
            print(rows, cols, n, json.dumps(row["counts"][str(n)]), flush=True)
        out.append(row)
    return out


def whole_calls(hip, capi, synth, passes, parent_lib):
    rows, cols = 480, 640
    seq, _ = frames_and_motions(synth, rows, cols, VO_FRAMES)
    libs = {"mode0": hip, "mode1": hip}
    if parent_lib:
        libs["parent_mode0"] = capi.Binding(parent_lib, "bpvo_hip_")
    out = {}
    for kind, n in (("add_frame", 1), ("add_frames_x64", 64)):
        imgs = np.stack([f[0] for f in seq["frames"]])
        disps = np.stack([f[1] for f in seq["frames"]])
        samples = {name: [] for name in libs}
        for k in range(passes + 1):
            for name, lib in libs.items():
                p = lib.default_params()
                p.descriptor = capi.DESC_BITPLANES
                p.verbosity = capi.VERB_SILENT
                ctx = lib.create(seq["K"], seq["b"], rows, cols, p, n_frames=3 * n, n_pairs=n)
                if name == "mode1":
                    ctx.set_disparity_fusion(FUSION)
                per_call = []
                for f in range(VO_FRAMES):
                    if kind == "add_frame":
                        t0 = time.perf_counter()
                        ctx.add_frame(imgs[f], disps[f])
                    else:
                        bi, bd = np.ascontiguousarray(np.broadcast_to(imgs[f], (n, rows, cols))), np.ascontiguousarray(np.broadcast_to(disps[f], (n, rows, cols)))
                        t0 = time.perf_counter()
                        ctx.add_frames(bi, bd)
                    if name == "mode1":
                        ctx.seq_disparity_fusion_info(0) if kind != "add_frame" else ctx.vo_disparity_fusion_info()      # (the stage has finished: its counters are in)
                    per_call.append(1e3 * (time.perf_counter() - t0))
                ctx.close()
                if k:
                    samples[name].append(float(np.median(per_call[1:])))      # (the first frame estimates nothing)
        out[kind] = {name: stats(v) for name, v in samples.items()}
        out[kind]["feature_cost_ms"] = round(out[kind]["mode1"]["median"] - out[kind]["mode0"]["median"], 3)
        print(kind, json.dumps(out[kind]), flush=True)
    return out


def host_loop(synth, ref, capi, passes):
    exe = os.path.join(tempfile.mkdtemp(), "df_harness")
    r = subprocess.run(["g++", "-std=c++11", "-O2", "-ffp-contract=off", "-I", os.path.join(ROOT, "bpvo_amd", "csrc"),
                        os.path.join(ROOT, "tests", "cpp", "disparity_fusion_harness.cc"), "-o", exe], capture_output=True, text=True)
    if r.returncode != 0:
        return dict(error=r.stderr[-400:])
    out = []
    for rows, cols in SIZES:
        seq, rel = frames_and_motions(synth, rows, cols, 3)
        K = np.asarray(seq["K"], np.float32)
        cam = ref.camera(rows, cols, fx=K[0, 0], fy=K[1, 1], cx=K[0, 2], cy=K[1, 2], b=seq["b"])
        prm = ref.rule(FUSION["measurement_sigma"], FUSION["process_sigma"], FUSION["gate"], FUSION["max_fill_sigma"])
        D0, V0, _ = ref.step(cam, prm, seq["frames"][0][1])
        tag = exe + "_%dx%d" % (cols, rows)
        np.concatenate([[rows, cols], [cam[k] for k in ("fx", "fy", "cx", "cy", "b", "lo", "hi")], [0.5, 0.1, 3.0, 2.0], [1.0], rel[1].reshape(-1)]).astype(np.float64).tofile(tag + ".p")
        seq["frames"][1][1].astype(np.float32).tofile(tag + ".m")
        D0.tofile(tag + ".dc")
        V0.tofile(tag + ".vc")
        r = subprocess.run([exe, "bench", tag + ".p", tag + ".m", tag + ".dc", tag + ".vc", str(passes)], capture_output=True, text=True)
        out.append(dict(rows=rows, cols=cols, ms_per_frame=stats([1e3 * float(v) for v in r.stdout.split()])))
        print("host", json.dumps(out[-1]), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--calls", type=int, default=6)
    ap.add_argument("--parent-lib", default=None, help="libbpvo_hip.so built from the parent commit (mode 0 against it)")
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    import bpvo_amd
    from bpvo_amd import capi, synth
    import disparity_fusion_ref as ref
    hip = bpvo_amd.load()
    res = dict(passes=a.passes, calls_per_pass=a.calls, fusion=FUSION,
               kernels=kernels(hip, capi, synth, ref, a.passes, a.calls),
               whole_calls=whole_calls(hip, capi, synth, a.passes, a.parent_lib),
               host_single_thread=host_loop(synth, ref, capi, a.passes))
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
