"""No-GPU checks of the motion-stereo rule (c_api.h "motion stereo"): bpvo_amd/csrc/motion_stereo_math.h, built into a stand-alone program around a
serial loop (tests/cpp/motion_stereo_harness.cc) — once plain, once under AddressSanitizer / UBSan, run as a child process —, against the numpy
statement of the same rule (tests/motion_stereo_ref.py): the disparity map, the variance map and the class map equal bit for bit, and the counts."""
import os
import re
import subprocess

import numpy as np
import pytest

import disparity_fusion_ref as fref
import motion_stereo_ref as ref
from bpvo_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bpvo_amd", "csrc")
F32 = np.float32


def _build(tmp, name, extra=()):
    exe = str(tmp / name)
    r = subprocess.run(["g++", "-std=c++11", "-O2", "-ffp-contract=off", "-Wall", "-Werror", *extra, "-I", CSRC,
                        os.path.join(ROOT, "tests", "cpp", "motion_stereo_harness.cc"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("motion_stereo")
    return dict(tmp=tmp, n=[0], plain=_build(tmp, "ms_harness"),
                san=_build(tmp, "ms_harness_san", ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")))


BUILDS = ("plain", "san")
SHAPES = [(1, 1), (5, 7), (24, 40), (37, 53)]
SETTINGS = ((1, 1), (3, 8), (2, 4), (1, 8), (3, 1))      # (radius, steps)


def _params(cam, prm, Q):
    return np.array([cam["rows"], cam["cols"], cam["lo"], cam["hi"], prm["radius"], prm["steps"], prm["min_gain"], prm["noise_sigma"], prm["min_sigma"],
                     prm["max_sigma"], prm["gate"], cam["fx"], cam["fy"], cam["cx"], cam["cy"], cam["b"]] + list(np.asarray(Q, F32).reshape(-1)[:12]), np.float64)


def _harness(work, build, cam, prm, C, K, Q, pd, pv):
    tmp = work["tmp"]
    work["n"][0] += 1
    tag = str(tmp / ("c%d_%s" % (work["n"][0], build)))
    rows, cols = cam["rows"], cam["cols"]
    _params(cam, prm, Q).tofile(tag + ".params")
    np.ascontiguousarray(C, np.uint8).tofile(tag + ".first")
    np.ascontiguousarray(K, np.uint8).tofile(tag + ".second")
    np.ascontiguousarray(pd, F32).tofile(tag + ".pd")
    np.ascontiguousarray(pv, F32).tofile(tag + ".pv")
    res = subprocess.run([work[build], tag + ".params", tag + ".first", tag + ".second", tag + ".pd", tag + ".pv", tag + ".out"], capture_output=True, text=True)
    assert res.returncode == 0, (res.stdout, res.stderr)
    return (np.fromfile(tag + ".out.d", F32).reshape(rows, cols), np.fromfile(tag + ".out.v", F32).reshape(rows, cols),
            np.fromfile(tag + ".out.c", np.uint8).reshape(rows, cols), dict(zip(ref.CLASSES, (int(v) for v in res.stdout.split()))))


def _both(work, build, cam, prm, C, K, Q, pd, pv):
    """The numpy statement's maps and counts, after the C++ loop has been found equal to them bit for bit."""
    D, V, cls, counts = ref.refine(cam, prm, C, K, Q, pd, pv)
    hD, hV, hcls, hcounts = _harness(work, build, cam, prm, C, K, Q, pd, pv)
    assert ref.same_bits(hD, D), np.argwhere(ref.bits(hD) != ref.bits(D))[:5]
    assert ref.same_bits(hV, V), np.argwhere(ref.bits(hV) != ref.bits(V))[:5]
    assert np.array_equal(hcls, cls), np.argwhere(hcls != cls)[:5]
    assert hcounts == counts and sum(counts.values()) == pd.size
    kept = cls != ref.FUSED      # every class but "fused" keeps the prior's own bits
    assert np.array_equal(ref.bits(D)[kept], ref.bits(pd)[kept]) and np.array_equal(ref.bits(V)[kept], ref.bits(pv)[kept])
    return D, V, cls, counts


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("name", ref.MOTIONS)
@pytest.mark.parametrize("shape", SHAPES)
def test_every_motion_under_hostile_priors_equals_numpy(work, build, name, shape):
    rows, cols = shape
    cam, C, K, Q, pd, pv = ref.rule_case(rows, cols, name)
    for radius, steps in SETTINGS:
        prm = ref.rule(radius, steps, 0.25, 2.0, 0.02, 2.0, 3.0)
        D, V, cls, counts = _both(work, build, cam, prm, C, K, Q, pd, pv)
        if min(rows, cols) < 8:      # 1 x 1 and 5 x 7: no window with its taps fits, whatever the radius
            assert counts["edge"] + counts["flat"] + counts["rejected"] + counts["fused"] == 0
            assert counts["border"] + counts["low_parallax"] + counts["no_prior"] == rows * cols
        if name == "rotation":       # no translation: every pixel with a prior is low_parallax
            assert counts["low_parallax"] + counts["no_prior"] == rows * cols and (counts["low_parallax"] > 0 or rows * cols == 1)
        fused = cls == ref.FUSED
        assert np.all(V[fused] <= pv[fused]) and np.all(D[fused] > 0) and np.all(fref.valid(D[fused], cam["lo"], cam["hi"]))


@pytest.mark.parametrize("build", BUILDS)
def test_small_images_are_all_border(work, build):
    """5 x 7 and 1 x 1 under a sideways motion and a clean prior: the gain is there, the windows are not."""
    for rows, cols in ((5, 7), (1, 1)):
        cam = fref.camera(rows, cols, lo=0.001, hi=64.0)
        Q = ref.case_motion("sideways")
        C, K, d = ref.textured_pair(cam, Q, seed=1)
        pd, pv = d.copy(), np.full(d.shape, 0.25, F32)
        for radius in (1, 3):
            _, _, _, counts = _both(work, build, cam, ref.rule(radius, 2, 0.25, 2.0, 0.02, 2.0, 3.0), C, K, Q, pd, pv)
            assert counts["border"] == rows * cols, counts


# exactly what tests/test_gpu_motion_stereo.py feeds the rule alone: three shapes under four motions at four settings, and the quarter turn
GPU_CASES = [(rows, cols, name, radius, steps) for rows, cols in ((9, 11), (24, 40), (37, 53)) for name in ("sideways", "forward", "rotation", "general")
             for radius, steps in ((1, 1), (3, 8), (1, 8), (3, 1))]
GPU_CASES += [(rows, cols, name, radius, steps) for rows, cols, name in ((72, 96, "roll"), (24, 40, "general")) for radius, steps in ((3, 8), (1, 8))]


def test_every_reachable_class_occurs_in_the_gpu_cases():
    """The condition on the inputs of tests/test_gpu_motion_stereo.py, on the numpy statement: every class has at least 8 pixels in at least one of
    the GPU cases — every class an input can reach.  "flat" is not one: j* is the FIRST minimum and, past the "edge" test, has a left neighbour,
    so S_{j*-1} > S_{j*} and S_{j*+1} >= S_{j*}, that is a2 >= 1.  The class is the rule's guard against a2 <= 0 (as the issue of this feature
    states it) and stays 0 in every case; this test asserts that, too, so a change of the rule that makes it reachable is noticed here."""
    best = {k: 0 for k in ref.CLASSES}
    for rows, cols, name, radius, steps in GPU_CASES:
        cam, C, K, Q, pd, pv = ref.rule_case(rows, cols, name)
        counts = ref.refine(cam, ref.rule(radius, steps, 0.25, 2.0, 0.02, 2.0, 3.0), C, K, Q, pd, pv)[3]
        for k in ref.CLASSES:
            best[k] = max(best[k], counts[k])
    print(best)
    assert all(best[k] >= 8 for k in ref.CLASSES if k != "flat"), best
    assert best["flat"] == 0, best


def test_constant_images_are_edge_not_flat():
    """All sums equal: the first minimum is j = -steps."""
    cam = fref.camera(24, 40, lo=0.001, hi=64.0)
    C = np.full((24, 40), 77, np.uint8)
    pd, pv = np.full((24, 40), 5.0, F32), np.full((24, 40), 0.25, F32)
    counts = ref.refine(cam, ref.rule(2, 2, 0.25, 2.0, 0.02, 2.0, 3.0), C, C, ref.case_motion("sideways"), pd, pv)[3]
    assert counts["edge"] > 0 and counts["edge"] + counts["border"] == 24 * 40


def helps_case(rows=48, cols=64, tx=0.2):
    """synth's plane pair under a sideways motion of tx metres (b = 0.1: a gain of tx / b = 2 pixels per disparity pixel): the current frame is
    the first image, the frame before the second, the prior the truth + 0.4 px with variance 0.25."""
    seq = synth.make_sequence_steps(rows, cols, [tx], (1.0, 0.0, 0.0), (0.0, 0.0, 0.0))
    Kc = np.asarray(seq["K"], F32)
    cam = fref.camera(rows, cols, fx=Kc[0, 0], fy=Kc[1, 1], cx=Kc[0, 2], cy=Kc[1, 2], b=seq["b"], lo=0.001, hi=512.0)
    (img0, _), (img1, d1) = seq["frames"]
    Q = np.linalg.inv(seq["poses"][1]).astype(F32)      # X_1 = T X_0, so X_K = T^-1 X_C
    pd = (d1 + F32(0.4)).astype(F32)
    return cam, img1, img0, Q, pd, np.full(d1.shape, 0.25, F32), d1


def helps_figures(radius=2, steps=2):
    """(fraction fused, RMS error of the prior over the fused pixels, RMS error of the result there).  steps = 2: the truth lies 0.8 steps below
    the prior and the scene's disparities are 0.55 .. 0.68 px, so pd - 2 delta is still positive for about half the pixels and is not for 3."""
    cam, C, K, Q, pd, pv, truth = helps_case()
    D, V, cls, counts = ref.refine(cam, ref.rule(radius, steps, 0.25, 2.0, 0.02, 2.0, 3.0), C, K, Q, pd, pv)
    fused = cls == ref.FUSED
    rms = lambda a: float(np.sqrt(np.mean((a[fused].astype(np.float64) - truth[fused]) ** 2)))
    return float(fused.mean()), rms(pd), rms(D), counts


def test_the_rule_helps_where_it_should():
    frac, before, after, counts = helps_figures()
    print(frac, before, after, counts)
    assert frac >= 0.25, counts
    assert after < before, (before, after)


@pytest.mark.parametrize("bad,field", [(dict(radius=0), "radius"), (dict(radius=4), "radius"), (dict(steps=0), "steps"), (dict(steps=9), "steps"),
                                       (dict(min_gain=0.0), "min_gain"), (dict(min_gain=np.nan), "min_gain"), (dict(noise_sigma=0.0), "noise_sigma"),
                                       (dict(noise_sigma=np.inf), "noise_sigma"), (dict(noise_sigma=1e-30), "noise_sigma"), (dict(min_sigma=0.0), "min_sigma"),
                                       (dict(min_sigma=1e-30), "min_sigma"), (dict(min_sigma=3.0), "max_sigma"), (dict(max_sigma=np.inf), "max_sigma"),
                                       (dict(max_sigma=1e30), "max_sigma"), (dict(gate=0.0), "gate"), (dict(gate=-1.0), "gate"), (dict(gate=np.nan), "gate")])
def test_the_harness_refuses_what_the_library_refuses_and_names_the_field(work, bad, field):
    s = dict(radius=2, steps=4, min_gain=0.25, noise_sigma=2.0, min_sigma=0.02, max_sigma=2.0, gate=3.0)
    s.update(bad)
    tag = str(work["tmp"] / "refusal")
    p = [1, 1, 0.0, 1.0, s["radius"], s["steps"]] + [F32(s[k]) for k in ("min_gain", "noise_sigma", "min_sigma", "max_sigma", "gate")] + [1, 1, 0, 0, 1] + [0] * 12
    np.array(p, np.float64).tofile(tag + ".params")
    for ext, dt in ((".first", np.uint8), (".second", np.uint8), (".pd", F32), (".pv", F32)):
        np.zeros(1, dt).tofile(tag + ext)
    res = subprocess.run([work["plain"], tag + ".params", tag + ".first", tag + ".second", tag + ".pd", tag + ".pv", tag + ".out"], capture_output=True, text=True)
    assert res.returncode == 2 and res.stderr.startswith("motion stereo: ") and field in res.stderr, res.stderr


def test_struct_and_entry_points_are_declared_as_the_binding_mirrors_them():
    import ctypes
    from bpvo_amd import capi
    src = open(os.path.join(ROOT, "include", "bpvo_hip", "c_api.h")).read()
    for struct, mirror in (("bpvo_hip_motion_stereo", capi.MotionStereo), ("bpvo_hip_motion_stereo_info", capi.MotionStereoInfo)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), src, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = [re.match(r"[A-Za-z_]\w*", n.strip()).group(0) for decl in re.findall(r"\b(?:float|int|uint32_t)\s+([^;]+);", body) for n in decl.split(",")]
        assert fields == [f[0] for f in mirror._fields_], (struct, fields)
    assert ctypes.sizeof(capi.MotionStereo) == 32 and ctypes.sizeof(capi.MotionStereoInfo) == 28 + 20 + 64
    assert tuple(f[0] for f in capi.MotionStereoInfo._fields_[:7]) == ref.CLASSES == capi.MOTION_STEREO_CLASSES
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ("set_motion_stereo", "get_motion_stereo", "seq_set_motion_stereo", "seq_get_motion_stereo", "vo_motion_stereo_info",
                 "seq_motion_stereo_info", "motion_stereo_counts", "motion_stereo_frames"):
        assert re.search(r"\bint bpvo_hip_%s\(" % name, code), name
    # the neighbouring settings keep their layout: the feature adds no mode and no field to them
    assert ctypes.sizeof(capi.DisparityFusion) == 20 and ctypes.sizeof(capi.MeasurementVariance) == 20


def test_the_built_library_exports_the_entry_points():
    import __graft_entry__ as ge
    assert os.path.exists(ge.HIP_LIB), "the library has not been built (__graft_entry__.build)"
    out = subprocess.run(["nm", "-D", "--defined-only", ge.HIP_LIB], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    names = set(line.split()[-1] for line in out.stdout.splitlines() if line.strip())
    for name in ("set_motion_stereo", "get_motion_stereo", "seq_set_motion_stereo", "seq_get_motion_stereo", "vo_motion_stereo_info",
                 "seq_motion_stereo_info", "motion_stereo_counts", "motion_stereo_frames"):
        assert "bpvo_hip_" + name in names, name


def test_the_header_includes_no_hip_header_and_the_fusion_rule_is_untouched():
    src = open(os.path.join(CSRC, "motion_stereo_math.h")).read()
    assert "#include <hip" not in src and re.findall(r'#include "([^"]+)"', src) == ["disparity_fusion_math.h", "rectify_math.h"]
    kernel = open(os.path.join(CSRC, "kernels_motion_stereo.hip")).read()
    for call in ("ms_locate(", "ms_hypothesis(", "ms_min_push(", "ms_finish("):      # the kernel computes the rule through the header
        assert call in kernel, call
    assert "atomicAdd(float" not in kernel and "hipStreamSynchronize" not in kernel and "hipDeviceSynchronize" not in kernel
    fusion = open(os.path.join(CSRC, "kernels_disparity_fusion.hip")).read()
    assert "motion_stereo" not in fusion and "motion_stereo" not in open(os.path.join(CSRC, "disparity_fusion_math.h")).read()


def test_the_facade_surface_compiles():
    src = os.path.join(ROOT, "tests", "cpp", "motion_stereo_facade.cc")
    out = subprocess.run(["g++", "-std=c++11", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"), src], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
