#!/usr/bin/env python3
"""What the normalised intensity costs (c_api.h bpvo_hip_set_intensity_normalization), on one GPU.  Two measurements, written to
profiles/intensity_norm_bench.json and printed; a record, not a bar.

  data stage  bpvo_hip_frames_set_data over 1 / 16 / 64 device-resident frames of 640x480 and 1241x376, four levels, with the mode off, 0 (whole
              image), 7 and 15 (local): the HIP events the library puts around the descriptor launches of the stage under bpvo_hip_profiling
              (every level's: one launch of the local form or of intensity_kernel, two — histogram + table, apply — of the whole-image form;
              up to 8 frames the levels share a launch, above that each level has its own), and the wall time of the whole call, which ends in its
              synchronisation.  Algorithmic bytes: 5 per pixel of every level (1 read, 4 written), against the 8 TB/s HBM peak.
  whole call  bpvo_hip_add_frame, and bpvo_hip_add_frames over 64 sequences, host frames of a synthetic sequence, mode off against 7 and 0.

Every figure is the median of --passes passes behind a warm-up pass, the modes alternating inside a pass; the passes are kept so that their
spread can be seen."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OUT = os.path.join(ROOT, "profiles", "intensity_norm_bench.json")
SIZES = ((480, 640), (376, 1241))
FRAMES = (1, 16, 64)
S = max(FRAMES)
MODES = (-1, 0, 7, 15)
LEVELS = 4
BYTES_PER_PIXEL = 5.0
PEAK_TBS = 8.0


def stats(passes, digits=4):
    return dict(median=round(float(np.median(passes)), digits), min=round(float(min(passes)), digits), max=round(float(max(passes)), digits),
                passes=[round(float(v), digits) for v in passes])


def params(hip, capi):
    p = hip.default_params()
    p.descriptor = capi.DESC_INTENSITY
    p.lossFunction = capi.LOSS_HUBER
    p.numPyramidLevels = LEVELS
    p.verbosity = capi.VERB_SILENT
    return p


def data_stage_pass(ctx, n, calls, ti, td):
    """(descriptor-class event ms per call, timed sections per call — one: the events stand around all descriptor launches of a stage —, wall ms
    per call) of `calls` data stages over n frames"""
    ctx.profiling(1)
    t0 = time.perf_counter()
    for _ in range(calls):
        ctx.frames_set_data_device(0, 1, n, ti.data_ptr(), td.data_ptr())
    wall = 1e3 * (time.perf_counter() - t0) / calls
    d = [k for k in ctx.kernel_stats() if k["name"] == "descriptor"][0]
    return d["total_ms"] / calls, d["launches"] / calls, wall


def measure_data_stage(hip, capi, synth, torch, passes):
    out = []
    for rows, cols in SIZES:
        K, b = synth.calibration(rows, cols)
        ctxs = {}
        for mode in MODES:
            ctxs[mode] = hip.create(K, b, rows, cols, params(hip, capi), n_frames=S, n_pairs=1)
            ctxs[mode].set_intensity_normalization(mode)
        px = sum(ctxs[-1].level_size(l)[0] * ctxs[-1].level_size(l)[1] for l in range(LEVELS))
        g = torch.Generator(device="cpu").manual_seed(rows)
        ti = torch.randint(0, 256, (S * rows * cols,), dtype=torch.uint8, generator=g).cuda()
        td = torch.full((S * rows * cols,), 4.0, dtype=torch.float32, device="cuda")
        calls = {n: max(10, 200 // n) for n in FRAMES}
        for n in FRAMES:
            for mode in MODES:
                data_stage_pass(ctxs[mode], n, 3, ti, td)
        ev = {(n, m): [] for n in FRAMES for m in MODES}
        wall = {(n, m): [] for n in FRAMES for m in MODES}
        spans = {}
        for _ in range(passes):
            for n in FRAMES:
                for mode in MODES:
                    e, l, w = data_stage_pass(ctxs[mode], n, calls[n], ti, td)
                    ev[(n, mode)].append(e)
                    wall[(n, mode)].append(w)
                    spans[(n, mode)] = l
        for n in FRAMES:
            for mode in MODES:
                gb = n * px * BYTES_PER_PIXEL / 1e9
                e = stats([1e3 * v for v in ev[(n, mode)]], 2)      # us
                out.append(dict(size=f"{cols}x{rows}", frames=n, radius=mode, levels=LEVELS, launches_per_level=2 if mode == 0 else 1,
                                levels_share_a_launch=n <= 8, algorithmic_mb=round(gb * 1e3, 3), descriptor_us_per_stage=e,
                                wall_ms_per_data_stage=stats(wall[(n, mode)]),
                                achieved_tb_per_s=round(gb / (e["median"] * 1e-6) / 1e3, 3) if e["median"] > 0 else None,
                                share_of_8_tb_per_s=round(gb / (e["median"] * 1e-6) / 1e3 / PEAK_TBS, 4) if e["median"] > 0 else None))
                print(out[-1], flush=True)
        for c in ctxs.values():
            c.close()
    return out


def measure_whole_call(hip, capi, synth, passes, n_frames=6):
    out = []
    modes = (-1, 7, 0)
    for rows, cols in SIZES:
        seq = synth.make_sequence(rows, cols, n_frames, index=3, step_rot=0.004, step_trans=0.03)
        K, b = seq["K"], seq["b"]
        multis = {}
        for mode in modes:
            multis[mode] = hip.create(K, b, rows, cols, params(hip, capi), n_frames=3 * S, n_pairs=S)
            multis[mode].set_intensity_normalization(mode)
        imgs = [np.ascontiguousarray(np.stack([f[0]] * S)) for f in seq["frames"]]
        disps = [np.ascontiguousarray(np.stack([f[1]] * S)) for f in seq["frames"]]
        res = (capi.Result * S)()

        def run_single(mode):
            # a fresh context every pass (bpvo_hip_add_frame has no reset); its first frame — storage, the first key frame — is not timed
            ctx = hip.create(K, b, rows, cols, params(hip, capi), n_frames=3, n_pairs=1)
            ctx.set_intensity_normalization(mode)
            ctx.add_frame(*seq["frames"][0])
            t0 = time.perf_counter()
            for f in seq["frames"][1:]:
                ctx.add_frame(*f)
            ms = 1e3 * (time.perf_counter() - t0) / (n_frames - 1)
            ctx.close()
            return ms

        def run_multi(mode):
            ctx = multis[mode]
            for s in range(S):
                ctx.seq_reset(s)
            for k in range(n_frames):      # (the first frame of the sequences is not timed, as above)
                if k == 1:
                    t0 = time.perf_counter()
                ctx.call("add_frames", S, None, imgs[k].ctypes.data_as(C.c_void_p), disps[k].ctypes.data_as(C.c_void_p), 0, res)
            return 1e3 * (time.perf_counter() - t0) / (n_frames - 1)
        for name, run in (("add_frame", run_single), ("add_frames_x64", run_multi)):
            for mode in modes:
                run(mode)
            t = {m: [] for m in modes}
            for _ in range(passes):
                for mode in modes:
                    t[mode].append(run(mode))
            st = {m: stats(t[m]) for m in modes}
            out.append(dict(size=f"{cols}x{rows}", entry=name, timed_frames_per_pass=n_frames - 1, ms_per_call={f"radius_{m}": st[m] for m in modes},
                            difference_ms_per_call={f"radius_{m}": round(st[m]["median"] - st[-1]["median"], 4) for m in modes if m >= 0}))
            print(out[-1], flush=True)
        for c in multis.values():
            c.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=5)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("intensity_norm_bench: no GPU (a measurement does not fall back)")
    torch.cuda.init()
    import bpvo_amd
    from bpvo_amd import capi, synth
    hip = bpvo_amd.load()
    rec = dict(what="normalised intensity: scripts/intensity_norm_bench.py", device=torch.cuda.get_device_name(0), passes=a.passes,
               bytes_per_pixel=BYTES_PER_PIXEL, levels=LEVELS)
    rec["data_stage"] = measure_data_stage(hip, capi, synth, torch, a.passes)
    rec["whole_call"] = measure_whole_call(hip, capi, synth, a.passes)
    json.dump(rec, open(OUT, "w"), indent=1)
    print(json.dumps(rec, indent=1))


if __name__ == "__main__":
    main()
