"""Rectification on the device (c_api.h "rectification on the device"): raw images through bpvo_hip_rectify_frames, and raw pairs through
bpvo_hip_add_frames_stereo_raw / bpvo_hip_add_frame_stereo_raw, against the numpy statement of the rule (tests/rectify_ref.py) — never against
the library itself.  Integer arithmetic on maps both sides build with the same f64 statements: no tolerance anywhere.  The lens cases are those of
tests/test_rectify_math_cpu.py (which holds them to the C++ header on the CPU); the composition runs at 120x160, the smallest size at which the
suite runs add_frames."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import rectify_ref as ref
from bpvo_amd import capi, synth
from test_gpu_multi_sequence import assert_same_result
from test_gpu_resources import DEVICE, EVENTS, PINNED, live
from util import bits_equal, make_params

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ERR_INVALID_ARG, ERR_UNSUPPORTED, ERR_NO_DATA = -1, -2, -3      # c_api.h BPVO_ERR_*


def lens_of(case):
    return capi.lens(case["K"], case["dist"], case["R"], case["raw_rows"], case["raw_cols"])


def raw_image(case, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(case["raw_rows"], case["raw_cols"]), dtype=np.uint8)


def own_context(hip, case):
    return hip.create(ref.camera_K(case), 0.1, case["rows"], case["cols"], make_params(hip, levels=2), n_frames=3, n_pairs=1)


def rc_and_error(ctx, name, *args):
    rc = ctx.b.fn(name)(ctx.h, *args)
    return rc, ctx.b.fn("last_error", C.c_char_p)(ctx.h).decode()


ALL_CASES = dict({k: v[0] for k, v in ref.hard_cases().items()}, identity=ref.identity_case())


# ---- 1. bpvo_hip_rectify_frames against numpy -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ALL_CASES))
def test_rectify_frames_equals_numpy_from_and_to_host_and_device(hip, name):
    import torch
    case = ALL_CASES[name]
    raws = [raw_image(case, 10 + k) for k in range(2)]
    want = [ref.rectify(case, r) for r in raws]
    ctx = own_context(hip, case)
    spare = np.zeros(case["rows"] * case["cols"], np.uint8)
    rc, err = rc_and_error(ctx, "rectify_frames", 1, None, 0, raws[0].ctypes.data_as(C.c_void_p), 0, spare.ctypes.data_as(C.c_void_p), 0)
    assert rc == ERR_NO_DATA and "left" in err
    ctx.set_rectification(0, lens_of(case))
    assert ctx.rectification_info(0) == (case["raw_rows"], case["raw_cols"], want[0][1])
    if name == "identity":
        assert want[0][1] == 0 and np.array_equal(want[0][0], raws[0])
    got = ctx.rectify_frames(raws, 0)      # host -> host, two frames of the context's own camera
    for k in range(2):
        assert np.array_equal(got[k], want[k][0]), (name, k, np.argwhere(got[k] != want[k][0])[:8])
    # device -> device, host -> device, device -> host; the outputs at an odd byte offset of their buffer (rows that begin off the dword grid)
    packed, _ = capi.pack_images(raws)
    n_out = 2 * case["rows"] * case["cols"]
    t_raw = torch.from_numpy(packed).cuda()
    for raw_dev, out_dev in ((True, True), (False, True), (True, False)):
        t_out = torch.full((n_out + 8,), 0xAB, dtype=torch.uint8, device="cuda")
        h_out = np.full(n_out + 8, 0xAB, np.uint8)
        at = 3
        ctx.rectify_frames_ptr(2, 0, t_raw.data_ptr() if raw_dev else packed.ctypes.data, raw_dev,
                               (t_out.data_ptr() if out_dev else h_out.ctypes.data) + at, out_dev)
        torch.cuda.synchronize()
        out = t_out.cpu().numpy() if out_dev else h_out
        assert np.all(out[:at] == 0xAB) and np.all(out[at + n_out:] == 0xAB), (name, raw_dev, out_dev, "wrote outside its output")
        both = out[at:at + n_out].reshape(2, case["rows"], case["cols"])
        for k in range(2):
            assert np.array_equal(both[k], want[k][0]), (name, raw_dev, out_dev, k)
    ctx.close()


def test_callers_maps_on_the_hostile_map(hip):
    case = ALL_CASES["hard_41x59"]
    rows, cols, raw_rows, raw_cols = case["rows"], case["cols"], case["raw_rows"], case["raw_cols"]
    raw = raw_image(case, 3)
    ctx = own_context(hip, case)
    for side, (mx, my) in enumerate((ref.hostile_maps(rows, cols, raw_rows, raw_cols), ref.last_pixel_maps(rows, cols, raw_rows, raw_cols))):
        xq, yq = ref.quantise(mx, my)
        ctx.set_rectification_maps(side, raw_rows, raw_cols, mx, my)
        assert ctx.rectification_info(side) == (raw_rows, raw_cols, int(ref.outside(raw_rows, raw_cols, xq, yq).sum()))
        got = ctx.rectify_frames([raw], side)[0]
        assert np.array_equal(got, ref.remap(raw, xq, yq)), (side, np.argwhere(got != ref.remap(raw, xq, yq))[:8])
    assert np.all(ctx.rectify_frames([raw], 1)[0] == raw[-1, -1])
    ctx.close()


# ---- 2. three cameras in one context, one launch per call --------------------------------------------------------------------------------------
def test_mixed_cameras_in_one_call_equal_contexts_of_their_own(hip):
    names = sorted(ref.hard_cases())
    left = [ref.hard_cases()[n][0] for n in names]
    # the right side of every camera: the same lens at half strength, its centre moved
    right = [ref.camera_case(ref.camera_K(c), c["rows"], c["cols"], c["raw_rows"] + 1, c["raw_cols"] + 3, strength=0.5, shift=(1.3, -0.6)) for c in left]
    for l, r in zip(left, right):
        assert np.array_equal(l["Kn"], r["Kn"])
    sides = (left, right)
    cams = [(ref.camera_K(c), 0.1, c["rows"], c["cols"]) for c in left]
    ctx = hip.create_sequences(cams, make_params(hip, levels=2))
    for side in (0, 1):
        for s, c in enumerate(sides[side]):
            ctx.set_rectification(side, lens_of(c), seq=s)
    raws = [[raw_image(c, 20 + 3 * side + s) for s, c in enumerate(sides[side])] for side in (0, 1)]
    alone = [[None] * 3, [None] * 3]
    for side in (0, 1):
        for s, c in enumerate(sides[side]):
            one = own_context(hip, c)
            one.set_rectification(side, lens_of(c))
            alone[side][s] = one.rectify_frames([raws[side][s]], side)[0]
            assert np.array_equal(alone[side][s], ref.rectify(c, raws[side][s])[0]), (side, s)
            assert one.rectification_info(side) == ctx.rectification_info(side, seq=s)
            one.close()
    pixels = [c["rows"] * c["cols"] for c in left]
    for side in (0, 1):
        for order in ([0, 1, 2], [2, 0, 1], [1]):
            before = ctx.rectify_counts()
            got = ctx.rectify_frames([raws[side][s] for s in order], side, seq=order)
            after = ctx.rectify_counts()
            assert after[0] == before[0] + 1, ("one launch per call", order, before, after)
            assert after[1] == before[1] + sum(pixels[s] for s in order)
            for k, s in enumerate(order):
                assert np.array_equal(got[k], alone[side][s]), (side, order, s)
    ctx.close()


# ---- 3. composition: raw pairs through the stereo front-end and the VO driver ----------------------------------------------------------------
ROWS, COLS, RAW_ROWS, RAW_COLS, NDISP, N_FRAMES = 120, 160, 132, 176, 32, 6
KF = dict(minTranslationMagToKeyFrame=0.05, minRotationMagToKeyFrame=2.5, maxFractionOfGoodPointsToKeyFrame=0.0, goodPointThreshold=0.8)


class Scene:
    """Two sequences at 120x160 of one camera: synth's rectified stereo frames, the raw frames numpy makes of them (stretched to 132x176), a mild
    lens per sequence and side (the hard lens x 0.2), and the numpy rectification of every raw frame — computed once for the module."""

    def __init__(self):
        K, _ = synth.calibration(ROWS, COLS)
        self.K, self.b = np.asarray(K, np.float32).reshape(3, 3), 0.8
        seqs = [synth.make_stereo_sequence(ROWS, COLS, N_FRAMES, index=30 + s, step_rot=0.006, step_trans=0.04, camera=(self.K, self.b)) for s in range(2)]
        self.cases = [[ref.camera_case(self.K, ROWS, COLS, RAW_ROWS, RAW_COLS, 0.2, shift=(0.9 * s + 0.4 * side, -0.5 * side)) for side in (0, 1)]
                      for s in range(2)]
        self.raw = [[[ref.raw_from_image(seqs[s]["frames"][k][side], RAW_ROWS, RAW_COLS) for side in (0, 1)] for s in range(2)] for k in range(N_FRAMES)]
        self.rect = [[[ref.rectify(self.cases[s][side], self.raw[k][s][side])[0] for side in (0, 1)] for s in range(2)] for k in range(N_FRAMES)]

    def context(self, hip, S=2, rectification=True, **kw):
        ctx = hip.create(self.K, self.b, ROWS, COLS, make_params(hip, levels=3, **KF), n_frames=3 * S, n_pairs=S)
        for s in range(min(S, 2) if rectification else 0):
            for side in (0, 1):
                ctx.set_rectification(side, lens_of(self.cases[s][side]), seq=s)
        return ctx


@pytest.fixture(scope="module")
def scene():
    return Scene()


def record(ctx, ids, res, out):
    for s, r in zip(ids, res):
        out[s].append(dict(res=r, cloud=ctx.seq_point_cloud(s) if r["hasPointCloud"] else None, npts=ctx.seq_num_points_at_level(s)))


def run_sequences(hip, scene, how):
    """both sequences, frame by frame, through one context; how: raw | raw_device | numpy | rectify_frames"""
    import torch
    ctx = scene.context(hip, rectification=how != "numpy")
    sp = ctx.default_stereo_params(NDISP)
    out = [[], []]
    for k in range(N_FRAMES):
        raws = [[scene.raw[k][s][side] for s in range(2)] for side in (0, 1)]
        if how == "raw":
            res = ctx.add_frames_stereo_raw(raws[0], raws[1], sp)
        elif how == "raw_device":
            t = [torch.from_numpy(capi.pack_images(raws[side])[0]).cuda() for side in (0, 1)]
            res = ctx.add_frames_stereo_raw_device(2, t[0].data_ptr(), t[1].data_ptr(), sp)
            torch.cuda.synchronize()
        elif how == "numpy":
            res = ctx.add_frames_stereo([scene.rect[k][s][0] for s in range(2)], [scene.rect[k][s][1] for s in range(2)], sp)
        else:
            t_out = [torch.zeros(2 * ROWS * COLS, dtype=torch.uint8, device="cuda") for _ in (0, 1)]
            for side in (0, 1):
                packed, _ = capi.pack_images(raws[side])
                ctx.rectify_frames_ptr(2, side, packed.ctypes.data, False, t_out[side].data_ptr(), True, seq=[0, 1])
            res = ctx.add_frames_stereo_device(2, t_out[0].data_ptr(), t_out[1].data_ptr(), sp)
            torch.cuda.synchronize()
        record(ctx, [0, 1], res, out)
    trajs = [ctx.seq_trajectory(s) for s in range(2)]
    ctx.close()
    return out, trajs


@pytest.fixture(scope="module")
def numpy_run(hip, scene):
    """bpvo_hip_add_frames_stereo fed the numpy-rectified images: what every raw path must reproduce"""
    out, trajs = run_sequences(hip, scene, "numpy")
    later = [o["res"] for s in range(2) for o in out[s][1:]]
    print("key-framing reasons:", [[o["res"]["keyFramingReason"] for o in out[s]] for s in range(2)])
    assert any(r["isKeyFrame"] for r in later), "the run should hold a key frame that is not a first frame"
    assert any(o["cloud"] is not None and len(o["cloud"][0]) > 0 for s in range(2) for o in out[s]), "the run should hold a point cloud"
    return out, trajs


@pytest.mark.parametrize("how", ["raw", "raw_device", "rectify_frames"])
def test_raw_pairs_equal_the_numpy_rectified_pairs(hip, scene, numpy_run, how):
    out, trajs = run_sequences(hip, scene, how)
    for s in range(2):
        assert len(out[s]) == N_FRAMES
        for k in range(N_FRAMES):
            assert_same_result(out[s][k], numpy_run[0][s][k], f"{how}: sequence {s} frame {k}")
        assert bits_equal(trajs[s], numpy_run[1][s]), (how, s, "trajectory")


def test_add_frame_stereo_raw_equals_add_frame_stereo(hip, scene):
    p = make_params(hip, levels=3, **KF)
    a = hip.create(scene.K, scene.b, ROWS, COLS, p, n_frames=3, n_pairs=1)
    b = hip.create(scene.K, scene.b, ROWS, COLS, p, n_frames=3, n_pairs=1)
    sp = a.default_stereo_params(NDISP)
    for side in (0, 1):
        a.set_rectification(side, lens_of(scene.cases[0][side]))
    keys = 0
    for k in range(N_FRAMES):
        ra = a.add_frame_stereo_raw(scene.raw[k][0][0], scene.raw[k][0][1], sp)
        rb = b.add_frame_stereo(scene.rect[k][0][0], scene.rect[k][0][1], sp)
        snap = [dict(res=r, cloud=c.get_point_cloud() if r["hasPointCloud"] else None, npts=c.vo_num_points_at_level()) for r, c in ((ra, a), (rb, b))]
        assert_same_result(snap[0], snap[1], f"frame {k}")
        keys += int(k > 0 and ra["isKeyFrame"])
    assert keys > 0 and bits_equal(a.trajectory(), b.trajectory())
    a.close()
    b.close()


def test_a_rig_of_two_cameras_through_the_composition(hip, scene):
    """bpvo_hip_rectify_frames with device output, bpvo_hip_stereo_frames with device output, bpvo_hip_add_frames_rig with device input — against
    the same rig fed the numpy-rectified images and the maps bpvo_hip_stereo_frames makes of them, through host memory."""
    import torch
    X = np.stack([np.eye(4), synth.twist_to_matrix((0, 0.14, 0.02, 0.3, 0.02, 0.1))]).astype(np.float32)
    got = []
    for composed in (True, False):
        ctx = scene.context(hip, rectification=composed)
        ctx.rig_set(X)
        sp = ctx.default_stereo_params(NDISP)
        sizes = [(ROWS, COLS)] * 2
        res = []
        for k in range(N_FRAMES):
            if composed:
                t_img = [torch.zeros(2 * ROWS * COLS, dtype=torch.uint8, device="cuda") for _ in (0, 1)]
                t_disp = torch.zeros(2 * ROWS * COLS, dtype=torch.float32, device="cuda")
                for side in (0, 1):
                    packed, _ = capi.pack_images([scene.raw[k][s][side] for s in range(2)])
                    ctx.rectify_frames_ptr(2, side, packed.ctypes.data, False, t_img[side].data_ptr(), True, seq=[0, 1])
                ctx.stereo_frames_device(sizes, t_img[0].data_ptr(), t_img[1].data_ptr(), sp, t_disp.data_ptr())
                res.append(ctx.add_frames_rig_device(t_img[0].data_ptr(), t_disp.data_ptr()))
                torch.cuda.synchronize()
            else:
                lefts, rights = [scene.rect[k][s][0] for s in range(2)], [scene.rect[k][s][1] for s in range(2)]
                res.append(ctx.add_frames_rig(lefts, ctx.stereo_frames(sizes, lefts, rights, sp)))
        got.append((res, ctx.rig_trajectory()))
        ctx.close()
    for k in range(N_FRAMES):
        a, b = got[0][0][k], got[1][0][k]
        assert bits_equal(a["pose"], b["pose"]) and a["isKeyFrame"] == b["isKeyFrame"] and a["keyFramingReason"] == b["keyFramingReason"], k
        assert [(s["numIterations"], s["status"]) for s in a["stats"]] == [(s["numIterations"], s["status"]) for s in b["stats"]], k
    assert bits_equal(got[0][1], got[1][1])


# ---- 4. errors ---------------------------------------------------------------------------------------------------------------------------------
def bad_lenses(case):
    """(what, expected status, lens) — the rows of the error table of c_api.h"""
    def changed(**kw):
        q = lens_of(case)
        for k, v in kw.items():
            if k in ("dist0", "R0"):
                getattr(q, k[:-1])[0] = v
            else:
                setattr(q, k, v)
        return q
    tilted = np.array(case["R"], np.float64)
    tilted[0, 1] += 1e-5
    q_tilted = lens_of(case)
    q_tilted.R[:] = [float(v) for v in tilted.reshape(9)]
    return [("fx not finite", ERR_INVALID_ARG, changed(fx=float("nan"))), ("a coefficient not finite", ERR_INVALID_ARG, changed(dist0=float("inf"))),
            ("R not finite", ERR_INVALID_ARG, changed(R0=float("nan"))), ("fx = 0", ERR_INVALID_ARG, changed(fx=0.0)), ("fy < 0", ERR_INVALID_ARG, changed(fy=-3.0)),
            ("R 1e-5 from orthonormal", ERR_INVALID_ARG, q_tilted), ("raw rows 1", ERR_INVALID_ARG, changed(raw_rows=1)),
            ("raw cols 0", ERR_INVALID_ARG, changed(raw_cols=0)), ("raw rows 32768", ERR_UNSUPPORTED, changed(raw_rows=32768)),
            ("raw cols 40000", ERR_UNSUPPORTED, changed(raw_cols=40000))]


def test_every_error_leaves_the_sequences_as_they_were(hip, scene, numpy_run):
    ctx = scene.context(hip, S=4)      # sequences 0, 1 as in the scene; 2 without a rectification; 3 gets a camera with skew
    sp = ctx.default_stereo_params(NDISP)
    skewed = scene.K.copy()
    skewed[0, 1] = 0.25
    ctx.seq_set_camera(3, (skewed, scene.b, ROWS, COLS))
    res = (capi.Result * 2)()
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    mapx = np.zeros((ROWS, COLS), np.float32)
    bad = bad_lenses(scene.cases[0][0])
    out = [[], []]
    for k in range(N_FRAMES):
        left, _ = capi.pack_images([scene.raw[k][s][0] for s in range(2)])
        right, _ = capi.pack_images([scene.raw[k][s][1] for s in range(2)])
        # a sequence without a rectification, one with the left side only; the sequence is named
        ids = np.int32([0, 2])
        rc, err = rc_and_error(ctx, "add_frames_stereo_raw", 2, ptr(ids), ptr(left), ptr(right), 0, C.byref(sp), res)
        assert rc == ERR_NO_DATA and "sequence 2" in err and ("left" if k == 0 else "right") in err, (rc, err)
        if k == 0:
            ctx.set_rectification(0, lens_of(scene.cases[0][0]), seq=2)
        rc, err = rc_and_error(ctx, "rectify_frames", 2, ptr(np.int32([1, 2])), 1, ptr(right), 0, ptr(np.zeros(2 * ROWS * COLS, np.uint8)), 0)
        assert rc == ERR_NO_DATA and "sequence 2" in err, (rc, err)
        # the lens table, against sequence 0's own left side (which must stay as it is), some rows per frame; the same through the maps call
        for what, status, q in bad[k::N_FRAMES] + bad[:2]:
            rc, err = rc_and_error(ctx, "seq_set_rectification", 0, 0, C.byref(q))
            assert rc == status and "sequence 0" in err, (what, rc, err)
        for raw_rows, status in ((1, ERR_INVALID_ARG), (32768, ERR_UNSUPPORTED)):
            rc, err = rc_and_error(ctx, "seq_set_rectification_maps", 1, 0, raw_rows, RAW_COLS, ptr(mapx), ptr(mapx))
            assert rc == status and "sequence 1" in err, (raw_rows, rc, err)
        rc, err = rc_and_error(ctx, "seq_set_rectification", 3, 0, C.byref(lens_of(scene.cases[0][0])))
        assert rc == ERR_UNSUPPORTED and "sequence 3" in err and "skew" in err, (rc, err)
        rc, err = rc_and_error(ctx, "seq_set_rectification_maps", 3, 1, RAW_ROWS, RAW_COLS, ptr(mapx), ptr(mapx))
        assert rc == ERR_UNSUPPORTED and "skew" in err, (rc, err)
        rc, _ = rc_and_error(ctx, "seq_set_rectification", 0, 2, C.byref(lens_of(scene.cases[0][0])))
        assert rc == ERR_INVALID_ARG
        rc, _ = rc_and_error(ctx, "seq_set_rectification", 9, 0, C.byref(lens_of(scene.cases[0][0])))
        assert rc == ERR_INVALID_ARG
        rc, _ = rc_and_error(ctx, "add_frames_stereo_raw", 2, None, None, ptr(right), 0, C.byref(sp), res)
        assert rc == ERR_INVALID_ARG
        # ... and the good call gives what a run without any of this gives
        record(ctx, [0, 1], ctx.add_frames_stereo_raw([scene.raw[k][s][0] for s in range(2)], [scene.raw[k][s][1] for s in range(2)], sp), out)
    assert len(bad) == 10 and {w for k in range(N_FRAMES) for w, _, _ in bad[k::N_FRAMES]} == {w for w, _, _ in bad}
    for s in range(2):
        for k in range(N_FRAMES):
            assert_same_result(out[s][k], numpy_run[0][s][k], f"sequence {s} frame {k}")
        assert bits_equal(ctx.seq_trajectory(s), numpy_run[1][s])
    # a camera change clears the sequence's rectification
    assert ctx.rectification_info(0, seq=2)[:2] == (RAW_ROWS, RAW_COLS)
    ctx.seq_set_camera(2, (scene.K, scene.b, ROWS - 8, COLS - 8))
    rc, err = rc_and_error(ctx, "seq_rectification_info", 2, 0, None, None, None)
    assert rc == ERR_NO_DATA and "sequence 2" in err
    ctx.close()


# ---- 5. resources ----------------------------------------------------------------------------------------------------------------------------------
def test_a_context_gives_back_what_rectification_took_and_takes_nothing_without_it(hip):
    case = ALL_CASES["hard_41x59"]
    raw = raw_image(case, 7)
    c0 = live(hip)
    plain = own_context(hip, case)
    held = live(hip) - c0      # what a context of this shape holds today
    plain.clear_rectification()
    rc, _ = rc_and_error(plain, "rectification_info", 0, None, None, None)
    assert rc == ERR_NO_DATA and (live(hip) - c0 == held).all()
    plain.close()
    assert (live(hip) == c0).all()
    ctx = own_context(hip, case)
    c1 = live(hip)
    assert (c1 - c0 == held).all()
    ctx.set_rectification(0, lens_of(case))
    ctx.set_rectification(1, lens_of(case))
    c2 = live(hip)
    assert c2[DEVICE] == c1[DEVICE] + 2 and (np.delete(c2, DEVICE) == np.delete(c1, DEVICE)).all()      # the two maps
    want = ref.rectify(case, raw)[0]
    assert np.array_equal(ctx.rectify_frames([raw], 0)[0], want)
    c3 = live(hip)
    # the raw staging, the output staging, the frame table (device and pinned) and its event
    assert c3[DEVICE] == c2[DEVICE] + 3 and c3[PINNED] == c2[PINNED] + 1 and c3[EVENTS] == c2[EVENTS] + 1
    ctx.set_rectification(0, lens_of(case))      # a table replaced: one goes, one comes
    assert np.array_equal(ctx.rectify_frames([raw], 0)[0], want)
    assert (live(hip) == c3).all()
    ctx.clear_rectification()
    c4 = live(hip)
    assert c4[DEVICE] == c3[DEVICE] - 2
    rc, _ = rc_and_error(ctx, "rectification_info", 1, None, None, None)
    assert rc == ERR_NO_DATA
    ctx.close()
    assert (live(hip) == c0).all()


# ---- 6. the C++ facade -------------------------------------------------------------------------------------------------------------------------------
def test_set_rectification_and_add_frames_raw_through_the_facade(hip, scene, tmp_path):
    exe = str(tmp_path / "rectify_facade")
    csrc = os.path.join(ROOT, "bpvo_amd", "csrc")
    r = subprocess.run(["g++", "-std=c++11", "-O2", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "rectify_facade.cc"),
                        "-o", exe, "-L", csrc, "-lbpvo_hip", f"-Wl,-rpath,{csrc}"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    n_frames = 3
    with open(tmp_path / "lens.bin", "wb") as f:
        for s in range(2):
            for side in (0, 1):
                f.write(bytes(lens_of(scene.cases[s][side])))
    for k in range(n_frames):
        for side, name in ((0, "left"), (1, "right")):
            capi.pack_images([scene.raw[k][s][side] for s in range(2)])[0].tofile(tmp_path / f"{name}_{k}.u8")
    K = scene.K
    r = subprocess.run([exe, str(tmp_path), str(ROWS), str(COLS), repr(float(K[0, 0])), repr(float(K[1, 1])), repr(float(K[0, 2])), repr(float(K[1, 2])),
                        repr(float(scene.b)), "2", str(n_frames), str(NDISP)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    poses = np.fromfile(tmp_path / "poses.bin", np.float32).reshape(n_frames, 2, 4, 4)
    single = np.fromfile(tmp_path / "poses_single.bin", np.float32).reshape(n_frames, 4, 4)
    flags = [line.split() for line in r.stdout.strip().splitlines()]
    # the same through the ctypes binding, with the facade's parameters (the defaults but three levels, bit-planes, Tukey)
    p = make_params(hip, levels=3)
    ctx = hip.create(K, scene.b, ROWS, COLS, p, n_frames=6, n_pairs=2)
    one = hip.create(K, scene.b, ROWS, COLS, p, n_frames=3, n_pairs=1)
    sp = ctx.default_stereo_params(NDISP)
    for side in (0, 1):
        one.set_rectification(side, lens_of(scene.cases[0][side]))
        for s in range(2):
            ctx.set_rectification(side, lens_of(scene.cases[s][side]), seq=s)
    for k in range(n_frames):
        res = ctx.add_frames_stereo_raw([scene.raw[k][s][0] for s in range(2)], [scene.raw[k][s][1] for s in range(2)], sp)
        for s in range(2):
            assert bits_equal(poses[k, s], res[s]["pose"]), (k, s)
            n_cloud = len(ctx.seq_point_cloud(s)[0]) if res[s]["hasPointCloud"] else 0
            assert flags[2 * k + s] == [str(int(res[s]["isKeyFrame"])), str(n_cloud)], (k, s, flags[2 * k + s])
        assert bits_equal(single[k], one.add_frame_stereo_raw(scene.raw[k][0][0], scene.raw[k][0][1], sp)["pose"]), k
    ctx.close()
    one.close()
