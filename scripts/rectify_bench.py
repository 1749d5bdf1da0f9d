#!/usr/bin/env python3
"""What rectification on the device costs (c_api.h "rectification on the device"), on one GPU.  Three measurements, written to
profiles/rectify_bench.json and printed; a record, not a bar.

  kernel      the rectify launch for 1 / 16 / 64 stereo pairs (2 n frames, each sequence's own two maps) at 640x480 and 1241x376, raw size =
              camera size, the hard lens of the tests scaled by 0.2, device input and output: HIP events around the launch (option
              "rectify_last_kernel_ms" under bpvo_hip_profiling) and the wall time of the whole bpvo_hip_rectify_frames call, which ends in its
              synchronisation.  One call of this script's kernel pass takes both sides as two calls of n frames (the entry point takes one side);
              the raw entry points launch once for both.  Algorithmic bytes per destination pixel: 8 (the map entry) + 1 (stored) + raw pixels /
              destination pixels (read once) = 10 here.
  whole call  bpvo_hip_add_frames_stereo_raw from host raw images against bpvo_hip_add_frames_stereo from host images rectified beforehand (that
              stage untimed), alternating in one run, block matching, the frames of a synthetic sequence given to every sequence of the call.
  host        tests/cpp/rectify_harness.cc: the plain C++ loop of the same rule, single thread, on this machine's host, for the same frame sizes.

Every figure is the median of --passes alternating passes behind a warm-up pass; the passes themselves are kept so that their spread can be seen.

  python scripts/rectify_bench.py                       # the three measurements
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/rectify_bench.py --trace-only     # a run of its own: launches only
  python scripts/rectify_bench.py --merge-trace DIR     # adds the trace's kernel durations to profiles/rectify_bench.json
"""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OUT = os.path.join(ROOT, "profiles", "rectify_bench.json")
SIZES = ((480, 640), (376, 1241))
PAIRS = (1, 16, 64)
S = max(PAIRS)
BYTES_PER_PIXEL = 10.0      # 8 + 1 + raw / destination pixels (raw size = camera size)
PEAK_TBS = 8.0
TRACE_WARM, TRACE_CALLS = 3, 10
DIST = np.array([-0.28, 0.09, 0.0012, -0.0008, -0.012, 0.01, 0.002, 0.0005]) * 0.2
ANGLES = np.array([0.05, -0.04, 0.03]) * 0.2


def rotation(rz, ry, rx):
    cz, sz, cy, sy, cx, sx = np.cos(rz), np.sin(rz), np.cos(ry), np.sin(ry), np.cos(rx), np.sin(rx)
    return (np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1.0]]) @ np.array([[cy, 0, sy], [0, 1.0, 0], [-sy, 0, cy]]) @
            np.array([[1.0, 0, 0], [0, cx, -sx], [0, sx, cx]]))


def lens_for(capi, K, rows, cols, s, side):
    """the mild lens of sequence s's side: every sequence and side its own map (the centre moves a little), raw size = camera size"""
    f = float(K[0, 0])
    return capi.lens((1.02 * f, 0.99 * f, cols / 2.0 - 0.7 + 0.05 * s + 0.4 * side, rows / 2.0 + 0.4 - 0.5 * side), DIST, rotation(*ANGLES), rows, cols)


def stats(passes, digits=4):
    return dict(median=round(float(np.median(passes)), digits), min=round(float(min(passes)), digits), max=round(float(max(passes)), digits),
                passes=[round(float(v), digits) for v in passes])


def make_context(hip, capi, synth, rows, cols):
    K, b = synth.calibration(rows, cols)
    K = np.asarray(K, np.float32).reshape(3, 3)
    p = hip.default_params()
    p.descriptor = capi.DESC_BITPLANES
    p.verbosity = capi.VERB_SILENT
    ctx = hip.create(K, b, rows, cols, p, n_frames=3 * S, n_pairs=S)
    for s in range(S):
        for side in (0, 1):
            ctx.set_rectification(side, lens_for(capi, K, rows, cols, s, side), seq=s)
    return ctx, K, b, p


def kernel_pass(ctx, torch, rows, cols, n, calls, t_raw, t_out):
    """`calls` times both sides of n pairs (two calls of n frames): (event ms per pair of calls, wall ms per pair of calls)"""
    ids = list(range(n))
    ev, t0 = 0.0, time.perf_counter()
    for _ in range(calls):
        for side in (0, 1):
            ctx.rectify_frames_ptr(n, side, t_raw[side].data_ptr(), True, t_out[side].data_ptr(), True, seq=ids)
            ev += ctx.get_option("rectify_last_kernel_ms")
    return ev / calls, 1e3 * (time.perf_counter() - t0) / calls


def measure_kernel(hip, capi, synth, torch, passes, trace_only=False):
    out = []
    for rows, cols in SIZES:
        ctx, _, _, _ = make_context(hip, capi, synth, rows, cols)
        ctx.profiling(1)
        g = torch.Generator(device="cpu").manual_seed(rows)
        t_raw = [torch.randint(0, 256, (S * rows * cols,), dtype=torch.uint8, generator=g).cuda() for _ in (0, 1)]
        t_out = [torch.zeros(S * rows * cols, dtype=torch.uint8, device="cuda") for _ in (0, 1)]
        if trace_only:
            for n in PAIRS:
                kernel_pass(ctx, torch, rows, cols, n, TRACE_WARM + TRACE_CALLS, t_raw, t_out)
            ctx.close()
            continue
        calls = {n: max(10, 200 // n) for n in PAIRS}
        for n in PAIRS:
            kernel_pass(ctx, torch, rows, cols, n, 5, t_raw, t_out)
        ev = {n: [] for n in PAIRS}
        wall = {n: [] for n in PAIRS}
        for _ in range(passes):
            for n in PAIRS:
                e, w = kernel_pass(ctx, torch, rows, cols, n, calls[n], t_raw, t_out)
                ev[n].append(e)
                wall[n].append(w)
        for n in PAIRS:
            gb = 2 * n * rows * cols * BYTES_PER_PIXEL / 1e9
            e = stats(ev[n])
            out.append(dict(size=f"{cols}x{rows}", pairs=n, frames=2 * n, algorithmic_mb=round(gb * 1e3, 3), event_ms_both_sides=e,
                            wall_ms_both_calls=stats(wall[n]), achieved_tb_per_s=round(gb / e["median"], 3) if e["median"] > 0 else None,
                            share_of_8_tb_per_s=round(gb / e["median"] / PEAK_TBS, 4) if e["median"] > 0 else None))
            print(out[-1], flush=True)
        ctx.close()
    return out


def measure_whole_call(hip, capi, synth, torch, passes, n_frames=6):
    out = []
    for rows, cols in SIZES:
        seq = synth.make_stereo_sequence(rows, cols, n_frames, index=3, step_rot=0.004, step_trans=0.03)
        ctx_raw, K, b, p = make_context(hip, capi, synth, rows, cols)
        ctx_rect = hip.create(K, b, rows, cols, p, n_frames=3 * S, n_pairs=S)
        sp = ctx_raw.default_stereo_params(64)
        for n in PAIRS:
            ids = list(range(n))
            raws = [[[seq["frames"][k][side]] * n for side in (0, 1)] for k in range(n_frames)]
            rect = [[ctx_raw.rectify_frames(raws[k][side], side, seq=ids) for side in (0, 1)] for k in range(n_frames)]      # (untimed)

            # the packed host buffers of every frame, made once: the timed loop is the C calls alone
            packed = {name: [[capi.pack_images(frames[k][side])[0] for side in (0, 1)] for k in range(n_frames)] for name, frames in (("raw", raws), ("rect", rect))}
            res = (capi.Result * n)()

            def run(ctx, entry, bufs):
                for s in ids:
                    ctx.seq_reset(s)
                t0 = time.perf_counter()
                for k in range(n_frames):
                    ctx.call(entry, n, None, bufs[k][0].ctypes.data_as(C.c_void_p), bufs[k][1].ctypes.data_as(C.c_void_p), 0, C.byref(sp), res)
                return 1e3 * (time.perf_counter() - t0) / n_frames
            run(ctx_raw, "add_frames_stereo_raw", packed["raw"]), run(ctx_rect, "add_frames_stereo", packed["rect"])
            a, r = [], []
            for _ in range(passes):
                a.append(run(ctx_raw, "add_frames_stereo_raw", packed["raw"]))
                r.append(run(ctx_rect, "add_frames_stereo", packed["rect"]))
            sa, sr = stats(a), stats(r)
            out.append(dict(size=f"{cols}x{rows}", sequences=n, frames_per_pass=n_frames, add_frames_stereo_raw_ms_per_call=sa,
                            add_frames_stereo_ms_per_call=sr, difference_ms_per_call=round(sa["median"] - sr["median"], 4),
                            difference_ms_per_sequence=round((sa["median"] - sr["median"]) / n, 4)))
            print(out[-1], flush=True)
        ctx_raw.close()
        ctx_rect.close()
    return out


def measure_host(capi, synth, passes):
    out = []
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "rectify_harness")
        r = subprocess.run(["g++", "-std=c++11", "-O2", "-ffp-contract=off", "-I", os.path.join(ROOT, "bpvo_amd", "csrc"),
                            os.path.join(ROOT, "tests", "cpp", "rectify_harness.cc"), "-o", exe], capture_output=True, text=True)
        if r.returncode != 0:
            return dict(error=r.stderr[-400:])
        for rows, cols in SIZES:
            K, _ = synth.calibration(rows, cols)
            K = np.asarray(K, np.float32).reshape(3, 3)
            q = lens_for(capi, K, rows, cols, 0, 0)
            p = np.concatenate([[rows, cols, rows, cols], np.float64([K[0, 0], K[1, 1], K[0, 2], K[1, 2]]), [q.fx, q.fy, q.cx, q.cy], list(q.dist), list(q.R)])
            path = os.path.join(tmp, f"params_{rows}.f64")
            p.astype(np.float64).tofile(path)
            res = subprocess.run([exe, "bench", path, "8", str(passes)], capture_output=True, text=True)
            if res.returncode != 0:
                out.append(dict(size=f"{cols}x{rows}", error=res.stderr[-200:]))
                continue
            per_frame = [1e3 * float(v) for v in res.stdout.split()]
            out.append(dict(size=f"{cols}x{rows}", what="plain C++ loop of rectify_math.h, g++ -O2, one thread, this machine's host; ms per frame (a pair is two)",
                            ms_per_frame=stats(per_frame), ms_per_stereo_pair=round(2 * float(np.median(per_frame)), 4)))
            print(out[-1], flush=True)
    return out


def merge_trace(trace_dir):
    rows = []
    for path in sorted(glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True)):
        with open(path, newline="") as f:
            rows += [r for r in csv.DictReader(f) if "rectify_frames_kernel" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    per = 2 * (TRACE_WARM + TRACE_CALLS)
    want = per * len(SIZES) * len(PAIRS)
    rec = json.load(open(OUT)) if os.path.exists(OUT) else {}
    if len(rows) != want:
        rec["kernel_trace"] = f"not measured: the trace holds {len(rows)} rectify launches, {want} expected"
    else:
        out, at = [], 0
        for rows_, cols in SIZES:
            for n in PAIRS:
                d = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows[at + 2 * TRACE_WARM:at + per]]      # us per launch (one side)
                at += per
                gb = n * rows_ * cols * BYTES_PER_PIXEL / 1e9
                med = float(np.median(d))
                out.append(dict(size=f"{cols}x{rows_}", pairs=n, frames_per_launch=n, launches=len(d), kernel_us_per_launch=stats(d, 2),
                                achieved_tb_per_s=round(gb / (med * 1e-6) / 1e3, 3), share_of_8_tb_per_s=round(gb / (med * 1e-6) / 1e3 / PEAK_TBS, 4)))
        rec["kernel_trace"] = out
    json.dump(rec, open(OUT, "w"), indent=1)
    print(json.dumps(rec.get("kernel_trace"), indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--trace-only", action="store_true")
    ap.add_argument("--merge-trace")
    a = ap.parse_args()
    if a.merge_trace:
        return merge_trace(a.merge_trace)
    import torch
    if not torch.cuda.is_available():
        sys.exit("rectify_bench: no GPU (a measurement does not fall back)")
    torch.cuda.init()
    import bpvo_amd
    from bpvo_amd import capi, synth
    hip = bpvo_amd.load()
    if a.trace_only:
        measure_kernel(hip, capi, synth, torch, a.passes, trace_only=True)
        return
    rec = dict(what="rectification on the device: scripts/rectify_bench.py", device=torch.cuda.get_device_name(0), passes=a.passes,
               bytes_per_destination_pixel=BYTES_PER_PIXEL, kernel_trace="not measured")
    rec["host"] = measure_host(capi, synth, a.passes)
    rec["kernel"] = measure_kernel(hip, capi, synth, torch, a.passes)
    rec["whole_call"] = measure_whole_call(hip, capi, synth, torch, a.passes)
    json.dump(rec, open(OUT, "w"), indent=1)
    print(json.dumps(rec, indent=1))


if __name__ == "__main__":
    main()
