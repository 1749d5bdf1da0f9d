"""Helpers shared by the parity tests."""
import os

import numpy as np

from bpvo_amd import capi, synth

# pose tolerance of BASELINE.json's north_star: 1e-4 rad / 1e-3 m against the reference CPU path (= the oracle)
ROT_TOL = 1e-4
TRANS_TOL = 1e-3


def trans_tol(K):
    """1e-3 m, whatever the calibration.  (Rounds 1 and 2 scaled the bar with 615 / fx for the 160x120 test scenes, fx = 153.75 px;
    every parity test of the suite passes without that since round 3.  Only the randomised tool keeps a scaled bar for its random
    calibrations: tests/tools/fuzz_parity.py.)"""
    return TRANS_TOL


def make_params(b, descriptor="bitplanes", loss="tukey", levels=4, **kw):
    p = b.default_params()
    p.numPyramidLevels = levels
    p.descriptor = {"bitplanes": capi.DESC_BITPLANES, "intensity": capi.DESC_INTENSITY, "laplacian": capi.DESC_LAPLACIAN,
                    "gradient": capi.DESC_GRADIENT, "fields1": capi.DESC_FIELDS1, "fields2": capi.DESC_FIELDS2,
                    "centraldiff": capi.DESC_CENTRAL_DIFFERENCE, "latch": capi.DESC_LATCH}[descriptor]
    p.lossFunction = {"tukey": capi.LOSS_TUKEY, "huber": capi.LOSS_HUBER, "l2": capi.LOSS_L2}[loss]
    p.verbosity = capi.VERB_SILENT
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def setup_pair(b, rows, cols, index=0, n_frames=2, n_pairs=1, scene="plane", **pk):
    d = synth.make_pair(rows, cols, index, scene=scene)
    p = make_params(b, **pk)
    ctx = b.create(d["K"], d["b"], rows, cols, p, device=0, n_frames=n_frames, n_pairs=n_pairs)
    ctx.frame_set_data(0, d["imgA"], d["dispA"])
    ctx.frame_set_template(0)
    ctx.frame_set_data(1, d["imgB"], d["dispB"])
    return ctx, d, p


def rot_angle(Ra, Rb):
    """Angle of Ra^T Rb (radians), robust for tiny angles."""
    E = np.asarray(Ra, np.float64).T @ np.asarray(Rb, np.float64)
    w = np.array([E[2, 1] - E[1, 2], E[0, 2] - E[2, 0], E[1, 0] - E[0, 1]]) * 0.5
    return float(np.arcsin(min(1.0, np.linalg.norm(w))))


def pose_error(Ta, Tb):
    return rot_angle(Ta[:3, :3], Tb[:3, :3]), float(np.linalg.norm(np.asarray(Ta, np.float64)[:3, 3] - np.asarray(Tb, np.float64)[:3, 3]))


def bits_equal(a, b):
    a = np.ascontiguousarray(a)
    b = np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def options_string(**kw):
    """BPVO_HIP_OPTIONS: bpvo_hip_set_option(key, value) for every context created from here on, merged with what is already set."""
    cur = dict(kv.split("=", 1) for kv in os.environ.get("BPVO_HIP_OPTIONS", "").split(",") if kv)
    cur.update({k: str(v) for k, v in kw.items()})
    return ",".join(f"{k}={v}" for k, v in cur.items())


def set_options(monkeypatch, **kw):
    monkeypatch.setenv("BPVO_HIP_OPTIONS", options_string(**kw))


def both(hip, orc, rows, cols, levels, reference=False, **kw):
    """The same pair set up on the HIP path and the oracle (frame 0 = template of A, frame 1 = B); reference: the HIP context in
    validation mode reference_reduction."""
    ch, d, _ = setup_pair(hip, rows, cols, levels=levels, **kw)
    co, _, _ = setup_pair(orc, rows, cols, levels=levels, **kw)
    if reference:
        ch.set_option("reference_reduction", 1)
    return ch, co, d


def perturbed_pose(scale):
    tw = np.array([0.004, -0.003, 0.002, 0.02, -0.015, 0.03]) * scale
    return synth.twist_to_matrix(tw).astype(np.float32)


def normal_equations_f64(J, r, w, valid, C):
    """J^T W J, J^T W r, sqrt(sum w r^2) in float64 from the reference-layout arrays ([C*N][6], [C*N], [C*N], [N])."""
    J = np.asarray(J, np.float64).reshape(-1, 6)
    r = np.asarray(r, np.float64).reshape(-1)
    wv = np.asarray(w, np.float64).reshape(-1) * np.tile(np.asarray(valid, np.float64), C)
    H = (J * wv[:, None]).T @ J
    G = J.T @ (wv * r)
    return H, G, float(np.sqrt(np.sum(wv * r * r)))


def assert_same_run(Th, sh, rh, To, so, ro, what=""):
    """pose, per-level statistics and the per-linearisation trace (T, H, G, f_norm, sigma, valid count, dp, level) bit for bit"""
    assert len(rh) == len(ro), (what, "linearisations", len(rh), len(ro), [s["numIterations"] for s in sh], [s["numIterations"] for s in so])
    for i, (a, b) in enumerate(zip(rh, ro)):
        if not bits_equal(a, b):
            names = [("T", 0, 16), ("H", 16, 52), ("G", 52, 58), ("f_norm", 58, 59), ("sigma", 59, 60), ("num_valid", 60, 61), ("dp", 61, 67), ("level", 67, 68)]
            bad = [n for n, lo, hi in names if not bits_equal(a[lo:hi], b[lo:hi])]
            raise AssertionError(f"{what}: linearisation {i} (level {int(b[67])}) differs first in {bad}: hip {a[58:61]} oracle {b[58:61]}")
    for l, (a, b) in enumerate(zip(sh, so)):
        assert a["numIterations"] == b["numIterations"] and a["status"] == b["status"], (what, "level", l, a, b)
        assert np.float32(a["finalError"]).tobytes() == np.float32(b["finalError"]).tobytes(), (what, "finalError level", l, a, b)
        assert np.float32(a["firstOrderOptimality"]).tobytes() == np.float32(b["firstOrderOptimality"]).tobytes(), (what, "optimality level", l, a, b)
    assert bits_equal(Th, To), (what, "pose", Th, To)


def oracle_pairs(orc, batch, picks, p_kw, trace=False, chunks=1, f64=0):
    """The picked pairs of a make_batch `batch`, one at a time through the oracle.  chunks = 1: the serial sums of the reference's default
    build; chunks = n: the normal equations summed as n contiguous chunks, the decomposition of the reference's tbb::parallel_reduce
    (WITH_TBB, bpvo/linear_system_builder.cc:91-131,233-237); f64: the same terms accumulated in double (an instrument)."""
    out = []
    rows, cols = batch["images"].shape[1:]
    p = make_params(orc, **p_kw)
    ctx = orc.create(batch["K"], batch["b"], rows, cols, p, n_frames=2, n_pairs=1)
    ctx.call("set_num_threads", chunks)
    ctx.call("set_reduction", f64)
    for k in picks:
        ctx.frame_set_data(0, batch["images"][2 * k], batch["disparities"][2 * k])
        ctx.frame_set_template(0)
        ctx.frame_set_data(1, batch["images"][2 * k + 1], batch["disparities"][2 * k + 1])
        if trace:
            T, st, rec = ctx.estimate_pose_trace(0, 0, 1)
        else:
            (T, st), rec = ctx.estimate_pose(0, 0, 1), None
        out.append(dict(T=T, its=[s["numIterations"] for s in st], status=[s["status"] for s in st], trace=rec))
    ctx.close()
    return out


def assert_trace_reproduced(ch, trace, ws=0, ref=0, cur=1, h_tol=2e-4):
    """The per-iteration trace of an oracle run (estimate_pose_trace) reproduced by the HIP context `ch`, linearised at the poses the oracle
    visited.  The robust scale of a later linearisation of a level depends on the estimator's freeze history (Q6), which a pose alone does
    not reproduce — so the oracle's OWN sigma of that linearisation is handed to the HIP side (bpvo_hip_linearize_at_scale): valid count,
    H, G and f_norm are then compared at EVERY sampled pose; on the first linearisation of each level sigma itself is estimated on both
    sides and must be equal.  h_tol: H and G against the oracle's, relative to max |H| (the oracle's serial f32 sums set it)."""
    step = max(1, len(trace) // 24)
    first_of_level = {int(l): int(np.flatnonzero(trace[:, 67] == l)[0]) for l in np.unique(trace[:, 67])}
    picks = sorted(set(range(0, len(trace), step)) | set(first_of_level.values()))
    for i in picks:
        rec = trace[i]
        T = rec[:16].reshape(4, 4)
        level = int(rec[67])
        if i == first_of_level[level]:
            a = ch.linearize(ws, ref, cur, level, T, reset_scale=True)
            assert a["sigma"] == rec[59], (level, a["sigma"], rec[59])          # exact median, both sides from sigma = 1
        else:
            a = ch.linearize_at_scale(ws, ref, cur, level, T, float(rec[59]))
        assert a["num_valid"] == int(rec[60]), (level, i, a["num_valid"], rec[60])
        Ho, Go = rec[16:52].reshape(6, 6), rec[52:58]
        scale = np.abs(Ho).max()
        # the oracle sums serially in f32 (within 2e-4 of an f64 evaluation, test_linearize_parity); the GPU within 4e-6
        assert abs(a["f_norm"] - rec[58]) <= 1e-3 * max(rec[58], 1e-6), (level, i, a["f_norm"], rec[58])
        assert np.abs(a["H"] - Ho).max() <= h_tol * scale, (level, i, np.abs(a["H"] - Ho).max() / scale)
        assert np.abs(a["G"] - Go).max() <= h_tol * max(np.abs(Go).max(), 1e-3 * scale), (level, i)
