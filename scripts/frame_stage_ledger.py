"""The ledger of the frame stage (bpvo_amd/csrc/frames.hip: setData and setTemplate for batches of frames): for every descriptor form, every
selection path (tiled, flag bytes, point budget), the levels in one launch and one by one, lazy and census-only template levels of pair batches,
every placement of the normalisation, staggered lanes and sequences with cameras of their own — what was launched (at profiling level 1 the
launches and units of the five frame classes and of the normalisation, read BEFORE any accessor: an accessor may form a lazy level's records or
saliency map on demand, which launches again) and what came out (frame state, point counts and selection records per level, and a digest of
every array the accessors hand out: image, descriptor channels, saliency, point indices, points, pixels, Jacobians, normalisation; poses for
batches and sequences).  Every number is exact: tests/test_gpu_frame_stage_ledger.py compares a run against tests/golden/frame_stage_ledger.json
key by key.  Through bpvo_amd.capi only (torch for the device-resident inputs), on 120x160 synthetic frames with 3 levels;
minNumPixelsForNonMaximaSuppression = 10000 puts non-maximum suppression on level 0 alone (1000: on every level).

What is kept (and compared) is the FOLDED ledger, so that the recorded file stays small: per case `launches` as [launches, units] in the order
of FRAME_CLASSES, the pose digests, and per slot [frame_state, num_points per level (null without a template), one digest of the slot's
selection records and of all its per-level array digests].  Every byte of every array still decides the outcome; which array of a slot
differs is found with `--full`, which prints the unfolded ledger (a digest per slot, level and array) to compare between two builds.

Three departures from the plainest reading of the cases:
  * where a stage may defer normalisation launches to the estimate that follows (batch_run on one lane, add_frame, add_frames), the number of
    normalisation launches the timers saw is not recorded (launches() below); their units are;
  * staggered lanes run 16 pairs, not 6: a context gives a batch one lane per 8 pairs, so 16 is the smallest batch that runs on two — with
    the team kernel off, which would otherwise take the 16 pairs on one lane.  The case checks that two data stages ran;
  * the slots of the 96x128 sequence record no image, descriptor or saliency digests: those accessors copy the context's (largest) level
    size, beyond what a smaller camera's stage writes.

    python scripts/frame_stage_ledger.py [--full] [out.json]
"""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from bpvo_amd import capi, synth  # noqa: E402

ROWS, COLS, LEVELS = 120, 160, 3
FRAME_CLASSES = ("pyramid", "descriptor", "saliency_select", "point_budget", "template_build", "normalization")
# every descriptor form of the data stage: (tag, descriptor, parameters)
FORMS = (
    ("bitplanes fused", capi.DESC_BITPLANES, {}),
    ("bitplanes smoothed census", capi.DESC_BITPLANES, dict(sigmaPriorToCensusTransform=0.75)),
    ("bitplanes unsmoothed", capi.DESC_BITPLANES, dict(sigmaBitPlanes=0.0)),
    ("intensity", capi.DESC_INTENSITY, {}),
    ("laplacian", capi.DESC_LAPLACIAN, {}),
    ("gradient", capi.DESC_GRADIENT, {}),
    ("fields 1st order", capi.DESC_FIELDS1, {}),
    ("fields 2nd order", capi.DESC_FIELDS2, {}),
    ("central difference r1", capi.DESC_CENTRAL_DIFFERENCE, dict(centralDifferenceRadius=1)),
    ("central difference r4", capi.DESC_CENTRAL_DIFFERENCE, dict(centralDifferenceRadius=4)),
    ("latch", capi.DESC_LATCH, {}),
)
KEYFRAMES = dict(minTranslationMagToKeyFrame=0.1, minRotationMagToKeyFrame=2.5, maxFractionOfGoodPointsToKeyFrame=0.0, goodPointThreshold=0.8)


def params(hip, descriptor=capi.DESC_BITPLANES, **kw):
    p = hip.default_params()
    p.numPyramidLevels = LEVELS
    p.descriptor = descriptor
    p.lossFunction = capi.LOSS_TUKEY
    p.verbosity = capi.VERB_SILENT
    p.minNumPixelsForNonMaximaSuppression = 10000
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]


def launches(ctx, may_defer=False):
    """{class: [launches, units]} of the frame classes: before any accessor.  may_defer: the stage may leave normalisation launches on the side
    streams for the estimate to join; such a launch is counted only if it has ended when the stage reads its timers, so the count depends on
    the moment and is left out (null) — its units are exact all the same."""
    st = {k["name"]: k for k in ctx.kernel_stats()}
    rec = {name: [int(st[name]["launches"]), float(st[name]["units"])] for name in FRAME_CLASSES}
    if may_defer:
        rec["normalization"][0] = None
    return rec


def results(ctx, slots, dense_slots=None, saliency_first=False):
    """state, counts and selection records of the slots first, then the digests of what their accessors return (dense_slots: the slots whose
    image, descriptor and saliency maps are read; None: all)"""
    rec = {}
    state = {s: ctx.frame_state(s) for s in slots}
    for s in slots:
        rec[f"slot {s} frame_state"] = [int(v) for v in state[s]]
        if state[s][1]:
            rec[f"slot {s} num_points"] = [ctx.num_points(s, l) for l in range(ctx.L)]
            info = [ctx.selection_info(s, l) for l in range(ctx.L)]
            rec[f"slot {s} selection_info"] = [[int(i["n_candidates"]), digest(np.float32(i["threshold"])), int(i["n_ties_kept"])] for i in info]
    for s in slots:
        dense = dense_slots is None or s in dense_slots
        for l in range(ctx.L):
            d = {}
            if dense and state[s][1] and saliency_first:
                d["saliency"] = digest(ctx.get_saliency(s, l))
            if dense and state[s][0]:
                d["image"] = digest(ctx.get_image(s, l))
                d["descriptor"] = [digest(ctx.get_descriptor_channel(s, l, ch)) for ch in range(ctx.Cn)]
            if state[s][1]:
                if dense and not saliency_first:
                    d["saliency"] = digest(ctx.get_saliency(s, l))
                d["point_indices"] = digest(ctx.get_point_indices(s, l))
                d["points"] = digest(ctx.get_points(s, l))
                d["pixels"] = digest(ctx.get_pixels(s, l))
                d["jacobians"] = digest(ctx.get_jacobians(s, l))
                d["normalization"] = digest(ctx.get_normalization(s, l)[0])
            if d:
                rec[f"slot {s} level {l}"] = d
    return rec


def make(hip, data, p, n_frames, n_pairs, options=None, budget=None, warp=None):
    ctx = hip.create(data["K"], data["b"], ROWS, COLS, p, device=0, n_frames=n_frames, n_pairs=n_pairs)
    for k, v in (options or {}).items():
        ctx.set_option(k, v)
    if warp is not None:
        ctx.set_warp_formulation(warp)
    if budget:
        ctx.set_point_budget(budget)
    ctx.profiling(1)
    return ctx


def one_frame(hip, pair, p, options=None, budget=None):
    """frame_set_data + frame_set_template on one frame"""
    ctx = make(hip, pair, p, 2, 1, options, budget)
    ctx.frame_set_data(0, pair["imgA"], pair["dispA"])
    ctx.frame_set_template(0)
    rec = dict(launches=launches(ctx), **results(ctx, [0]))
    ctx.close()
    return rec


def pair_batch(hip, b, p, options=None, budget=None, warp=None, device=False, saliency_first=False):
    """batch_run: the (A, B) frames of n pairs through both stages and the estimate"""
    n = b["images"].shape[0] // 2
    o = options or {}
    may_defer = o.get("normalization_side_stream", 1) != 0 and o.get("normalization_deferred", 1) != 0 and "lanes" not in o
    ctx = make(hip, b, p, 2 * n, n, options, budget, warp)
    if device:
        import torch
        di, dd = torch.from_numpy(b["images"]).cuda(), torch.from_numpy(b["disparities"]).cuda()
        poses, _ = ctx.batch_run_device(n, di.data_ptr(), dd.data_ptr())
    else:
        poses, _ = ctx.batch_run(b["images"], b["disparities"])
    rec = dict(launches=launches(ctx, may_defer), poses=[digest(T) for T in poses], **results(ctx, range(2 * n), saliency_first=saliency_first))
    ctx.close()
    return rec


def sequence(hip, p):
    """five add_frame calls: the skipped disparity upload, key frames with and without a second estimate"""
    seq = synth.make_sequence(ROWS, COLS, 5, index=5, step_rot=0.01, step_trans=0.06)
    ctx = make(hip, seq, p, 3, 1)
    out = [ctx.add_frame(img, disp) for img, disp in seq["frames"]]
    rec = dict(launches=launches(ctx, True), poses=[digest(r["pose"]) for r in out], key_frames=[int(r["isKeyFrame"]) for r in out], **results(ctx, range(3)))
    ctx.close()
    return rec


def sequences(hip, p, device):
    """three add_frames calls over three sequences, the last with a 96x128 camera: a stage per size (device inputs: the offsets' path)"""
    sizes = [(ROWS, COLS), (ROWS, COLS), (96, 128)]
    seqs = [synth.make_sequence(r, c, 3, index=7 + i, step_rot=0.01, step_trans=0.06) for i, (r, c) in enumerate(sizes)]
    ctx = hip.create_sequences([(s["K"], s["b"], r, c) for s, (r, c) in zip(seqs, sizes)], p)
    ctx.profiling(1)
    poses, key_frames = [], []
    for k in range(3):
        imgs, disps = [s["frames"][k][0] for s in seqs], [s["frames"][k][1] for s in seqs]
        if device:
            import torch
            img, disp, _ = capi.pack_frames(imgs, disps)
            ti, td = torch.from_numpy(img).cuda(), torch.from_numpy(disp).cuda()
            out = ctx.add_frames_device(3, ti.data_ptr(), td.data_ptr())
        else:
            out = ctx.add_frames(imgs, disps)
        poses.append([digest(r["pose"]) for r in out])
        key_frames.append([int(r["isKeyFrame"]) for r in out])
    # (sequence s owns slots 3 s .. 3 s + 2; the dense maps of those with the context's size only)
    dense_slots = [3 * s + k for s, size in enumerate(sizes) if size == (ctx.rows, ctx.cols) for k in range(3)]
    rec = dict(launches=launches(ctx, True), poses=poses, key_frames=key_frames, **results(ctx, range(ctx.n_frames), dense_slots))
    ctx.close()
    return rec


def fold(case):
    """a case's record with its per-slot, per-level, per-array digests folded into one digest per slot"""
    out = {k: v for k, v in case.items() if not k.startswith("slot ")}
    out["launches"] = [case["launches"][name] for name in FRAME_CLASSES]
    for s in sorted({int(k.split()[1]) for k in case if k.startswith("slot ")}):
        inner = {k: v for k, v in case.items() if k.startswith(f"slot {s} ") and k not in (f"slot {s} frame_state", f"slot {s} num_points")}
        out[f"slot {s}"] = [case[f"slot {s} frame_state"], case.get(f"slot {s} num_points"),
                            hashlib.sha256(json.dumps(inner, sort_keys=True).encode()).hexdigest()[:16]]
    return out


def ledger(hip, full=False):
    return full_ledger(hip) if full else {k: fold(v) for k, v in json.loads(json.dumps(full_ledger(hip))).items()}


def full_ledger(hip):
    pair = synth.make_pair(ROWS, COLS, 0)
    batches = {n: synth.make_batch(ROWS, COLS, n, first_index=11) for n in (2, 6, 16)}
    out = {}
    for merge in (8, 0):      # (levels_in_one_launch_max_frames: its default, and off)
        m = f"levels_in_one_launch_max_frames={merge}"
        opt = dict(levels_in_one_launch_max_frames=merge)
        for tag, desc, kw in FORMS:
            out[f"one frame, {tag}, {m}"] = one_frame(hip, pair, params(hip, desc, **kw), opt)
        for tag, desc in (("bitplanes fused", capi.DESC_BITPLANES), ("intensity", capi.DESC_INTENSITY)):
            for radius in (0, 2):      # (1: the forms above)
                out[f"one frame, {tag}, nonMaxSuppRadius={radius}, {m}"] = one_frame(hip, pair, params(hip, desc, nonMaxSuppRadius=radius), opt)
        out[f"one frame, bitplanes fused, nonMaxSuppRadius=2 on every level, {m}"] = \
            one_frame(hip, pair, params(hip, nonMaxSuppRadius=2, minNumPixelsForNonMaximaSuppression=1000), opt)
        for radius in (1, 2):
            out[f"one frame, point budget 200 / none / 48, nonMaxSuppRadius={radius}, {m}"] = \
                one_frame(hip, pair, params(hip, nonMaxSuppRadius=radius), opt, budget=[200, 0, 48])
    p = params(hip)
    for n in (2, 6):      # (4 frames: the levels in one launch; 12: level by level)
        for lazy_desc in (0, 1):
            for lazy_sal in (0, 1):
                out[f"{n} pairs, lazy_template_descriptor={lazy_desc}, lazy_template_saliency={lazy_sal}"] = \
                    pair_batch(hip, batches[n], p, dict(lazy_template_descriptor=lazy_desc, lazy_template_saliency=lazy_sal))
        out[f"{n} pairs, keep_current_disparity=1"] = pair_batch(hip, batches[n], p, dict(keep_current_disparity=1))
        out[f"{n} pairs, device inputs"] = pair_batch(hip, batches[n], p, device=True)
        out[f"{n} pairs, device inputs, keep_current_disparity=1"] = pair_batch(hip, batches[n], p, dict(keep_current_disparity=1), device=True)
        out[f"{n} pairs, point budget 200 on the census-only level"] = pair_batch(hip, batches[n], p, budget=[200])
        out[f"{n} pairs, saliency read before the descriptor"] = pair_batch(hip, batches[n], p, saliency_first=True)
    two = batches[2]
    for side in (0, 1):
        for defer in (0, 1):
            out[f"2 pairs, normalization_side_stream={side}, normalization_deferred={defer}"] = \
                pair_batch(hip, two, p, dict(normalization_side_stream=side, normalization_deferred=defer))
    out["2 pairs, dense templates (nonMaxSuppRadius=0, persist_max_points=10000)"] = \
        pair_batch(hip, two, params(hip, nonMaxSuppRadius=0), dict(persist_max_points=10000))
    out["2 pairs, withNormalization=0"] = pair_batch(hip, two, params(hip, withNormalization=0))
    out["2 pairs, disparity-space warp"] = pair_batch(hip, two, p, warp=2)
    staggered = pair_batch(hip, batches[16], p, dict(lanes=2, stagger=1, stagger_min_pairs=16, team=0))
    assert staggered["launches"]["descriptor"][0] == 2, "the 16-pair batch did not fan out over two lanes"
    out["16 pairs, staggered over 2 lanes"] = staggered
    out["add_frame, five frames"] = sequence(hip, params(hip, **KEYFRAMES))
    for device in (False, True):
        out["add_frames, three sequences, one 96x128 camera, " + ("device" if device else "host") + " inputs"] = \
            sequences(hip, params(hip, **KEYFRAMES), device)
    return out


def dumps(led):
    """one case per line"""
    return "{\n" + ",\n".join(" " + json.dumps(k) + ": " + json.dumps(led[k], sort_keys=True, separators=(",", ":")) for k in sorted(led)) + "\n}"


if __name__ == "__main__":
    try:      # (torch's own HIP runtime finds the GPU only when it comes up before the library's: tests/conftest.py)
        import torch
        if torch.cuda.is_available():
            torch.cuda.init()
    except Exception:
        pass
    import bpvo_amd
    args = [a for a in sys.argv[1:] if a != "--full"]
    text = dumps(ledger(bpvo_amd.load(), full="--full" in sys.argv))
    if args:
        with open(args[0], "w") as f:
            f.write(text + "\n")
    else:
        print(text)
