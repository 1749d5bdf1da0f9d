"""No-GPU checks of the measurement-variance rule (c_api.h "measurement variance"): bpvo_amd/csrc/disparity_variance_math.h, built into a stand-alone
program around a serial loop (tests/cpp/disparity_variance_harness.cc) — once plain, once under AddressSanitizer / UBSan, run as a child process —,
against the numpy statement of the same rule (tests/disparity_variance_ref.py): the variance map and the six class counts equal bit for bit."""
import os
import re
import subprocess

import numpy as np
import pytest

import disparity_fusion_ref as fref
import disparity_variance_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bpvo_amd", "csrc")
F32 = np.float32


def _build(tmp, name, extra=()):
    exe = str(tmp / name)
    r = subprocess.run(["g++", "-std=c++11", "-O2", "-ffp-contract=off", "-Wall", "-Werror", *extra, "-I", CSRC,
                        os.path.join(ROOT, "tests", "cpp", "disparity_variance_harness.cc"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("disparity_variance")
    return dict(tmp=tmp, n=[0], plain=_build(tmp, "dv_harness"),
                san=_build(tmp, "dv_harness_san", ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")))


BUILDS = ("plain", "san")
SHAPES = [(1, 1), (5, 7), (33, 65)]
RADII = (1, 3, 7)
# the template stage's default gate, and one that lets negatives and values beyond 2^30 through
GATES = ((0.001, 64.0), (-1.0e4, float(ref.F32_MAX)))


def _harness(work, build, prm, L, R, M, lo, hi):
    tmp = work["tmp"]
    work["n"][0] += 1
    tag = str(tmp / ("c%d_%s" % (work["n"][0], build)))
    rows, cols = M.shape
    np.array([rows, cols, F32(lo), F32(hi), prm["radius"], prm["noise_sigma"], prm["min_sigma"], prm["max_sigma"]], np.float64).tofile(tag + ".params")
    np.ascontiguousarray(L, np.uint8).tofile(tag + ".l")
    np.ascontiguousarray(R, np.uint8).tofile(tag + ".r")
    np.ascontiguousarray(M, F32).tofile(tag + ".m")
    res = subprocess.run([work[build], tag + ".params", tag + ".l", tag + ".r", tag + ".m", tag + ".out"], capture_output=True, text=True)
    assert res.returncode == 0, (res.stdout, res.stderr)
    return np.fromfile(tag + ".out", F32).reshape(rows, cols), dict(zip(ref.CLASSES, (int(v) for v in res.stdout.split())))


def _both(work, build, prm, L, R, M, lo, hi):
    """The numpy statement's map and counts, after the C++ loop has been found equal to them bit for bit."""
    R2, counts = ref.variance(prm, L, R, M, lo, hi)
    h2, hcounts = _harness(work, build, prm, L, R, M, lo, hi)
    assert ref.same_bits(h2, R2), np.argwhere(ref.bits(h2) != ref.bits(R2))[:5]
    assert hcounts == counts and sum(counts.values()) == M.size
    assert np.all(R2 > 0) and np.all(R2 <= ref.F32_MAX) and np.all(R2 >= prm["min2"]) and np.all(R2 <= prm["max2"])
    return R2, counts


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("shape", SHAPES)
def test_random_images_and_hostile_disparities_equal_numpy(work, build, radius, shape):
    rows, cols = shape
    prm = ref.rule(radius, 2.0, 0.02, 2.0)
    L, R = ref.random_pair(rows, cols, seed=cols + radius)
    seen = {k: 0 for k in ref.CLASSES}
    for lo, hi in GATES:
        M = ref.hostile_disparities(rows, cols, radius, seed=rows, hi=64.0)
        _, counts = _both(work, build, prm, L, R, M, lo, hi)
        for k in ref.CLASSES:
            seen[k] += counts[k]
    if shape == (33, 65) and radius < 7:      # (what the case is there for: invalid, border and the model's classes all occur)
        assert seen["invalid"] > 0 and seen["border"] > 0 and seen["model"] + seen["floor"] + seen["ceiling"] > 0, seen
    if 2 * radius + 1 > min(rows, cols):
        assert seen["model"] + seen["floor"] + seen["ceiling"] + seen["flat"] == 0      # no window fits


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("radius", RADII)
def test_smooth_disparities_on_a_shifted_texture_land_in_the_model(work, build, radius):
    rows, cols = 33, 65
    L, R = ref.random_pair(rows, cols, seed=7)      # (L is R moved by 3 px plus noise)
    M = np.full((rows, cols), 3.0, F32)
    prm = ref.rule(radius, 2.0, 0.02, 2.0)
    R2, counts = _both(work, build, prm, L, R, M, 0.001, 64.0)
    inner = (rows - 2 * radius) * (cols - 2 * radius - 1 - 3)      # full left windows whose right windows' span starts at column >= 0
    assert counts["border"] == rows * cols - inner and counts["invalid"] == 0
    assert counts["model"] + counts["floor"] == inner      # the true disparity of a random texture: a sharp minimum
    # the same map shifted by 3 px is a worse match almost everywhere: the variances rise
    R2b, _ = _both(work, build, prm, L, R, M + F32(3.0), 0.001, 64.0)
    both = (R2 < prm["max2"]) & (R2b <= prm["max2"])
    assert np.median(R2b[both]) > np.median(R2[both])


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("shape", SHAPES)
def test_checkerboard_against_its_inverse_and_a_constant_image(work, build, radius, shape):
    rows, cols = shape
    prm = ref.rule(radius, 2.0, 0.02, 2.0)
    L, R = ref.checkerboard_pair(rows, cols)
    M = np.full((rows, cols), 2.0, F32)      # an even shift: every difference of S_0 is 255, none of S_-1 and S_+1 is: a < 0
    M[::2, ::3] = 3.0                        # an odd one: S_0 = 0 and S_-1 = S_+1 = n 65025, the largest a
    R2, counts = _both(work, build, prm, L, R, M, 0.001, 64.0)
    assert counts["model"] + counts["ceiling"] == 0      # flat (a < 0) at the even shift, the floor at the odd one
    if shape == (33, 65):
        assert counts["flat"] > 0 and counts["floor"] > 0
    L, R = ref.constant_pair(rows, cols)
    R2, counts = _both(work, build, prm, L, R, M, 0.001, 64.0)
    assert counts["flat"] + counts["border"] == rows * cols and np.all(R2 == prm["max2"])      # every pixel with windows is flat


@pytest.mark.parametrize("build", BUILDS)
def test_ties_round_to_even_and_the_edges_of_the_image(work, build):
    """One row of full windows (3 x 16, radius 1) over a ramp-textured pair: 2.5 reads the windows of 2 and 3.5 those of 4; a right span that ends
    exactly on column 0 or on the last column is inside, one past either is border."""
    rows, cols, rho = 3, 16, 1
    prm = ref.rule(rho, 2.0, 0.02, 2.0)
    rng = np.random.default_rng(1)
    R = rng.integers(0, 256, (rows, cols), dtype=np.uint8)
    L = rng.integers(0, 256, (rows, cols), dtype=np.uint8)
    lo, hi = -100.0, 64.0
    M = np.full((rows, cols), np.nan, F32)
    M[1, 8], M[1, 9] = 2.5, 3.5
    a, _ = _both(work, build, prm, L, R, M, lo, hi)
    M2 = M.copy()
    M2[1, 8], M2[1, 9] = 2.0, 4.0
    b, _ = _both(work, build, prm, L, R, M2, lo, hi)
    assert ref.same_bits(a, b)
    for x in (rho, 6, cols - 1 - rho):
        for d, inside in ((x - rho - 1, True), (x - rho, False), (x + rho + 1 - (cols - 1), True), (x + rho + 1 - cols, False)):
            M = np.full((rows, cols), np.nan, F32)
            M[1, x] = d
            _, counts = _both(work, build, prm, L, R, M, lo, hi)
            assert counts["border"] == (0 if inside else 1) and counts["invalid"] == rows * cols - 1, (x, d, counts)


def test_the_numpy_step_with_a_variance_map_is_the_old_step_where_the_map_is_the_constant():
    cam, Ms, Ps = fref.chain_case(33, 65, seed=4)
    prm = fref.rule(0.5, 0.1, 3.0, 2.0)
    D0, V0, c0 = fref.step(cam, prm, Ms[0])
    assert all(ref.same_bits(a, b) for a, b in zip(ref.step_var(cam, prm, Ms[0], None)[:2], (D0, V0)))
    want = fref.step(cam, prm, Ms[1], D0, V0, Ps[1])
    for R2 in (None, np.full(Ms[1].shape, prm["r2"], F32), np.zeros(Ms[1].shape, F32), np.full(Ms[1].shape, np.nan, F32), np.full(Ms[1].shape, -1, F32),
               np.full(Ms[1].shape, np.inf, F32)):
        got = ref.step_var(cam, prm, Ms[1], R2, D0, V0, Ps[1])
        assert ref.same_bits(got[0], want[0]) and ref.same_bits(got[1], want[1]) and got[2] == want[2]
    # and a smaller variance pulls the fused value towards the measurement
    tight = ref.step_var(cam, prm, Ms[1], np.full(Ms[1].shape, 0.01, F32), D0, V0, Ps[1])
    fused = (tight[1] >= 0) & (want[1] >= 0) & (tight[0] != Ms[1]) & (want[0] != Ms[1])
    assert fused.any() and np.all(np.abs(tight[0][fused] - Ms[1][fused]) <= np.abs(want[0][fused] - Ms[1][fused]))


@pytest.mark.parametrize("bad", [dict(radius=0), dict(radius=8), dict(noise_sigma=0.0), dict(noise_sigma=np.nan), dict(min_sigma=0.0),
                                 dict(min_sigma=3.0), dict(max_sigma=np.inf), dict(min_sigma=1e-30), dict(max_sigma=1e30)])
def test_the_harness_refuses_what_the_library_refuses(work, bad):
    s = dict(radius=2, noise_sigma=2.0, min_sigma=0.02, max_sigma=2.0)
    s.update(bad)
    tmp = work["tmp"]
    tag = str(tmp / "refusal")
    np.array([1, 1, 0.0, 1.0, s["radius"], F32(s["noise_sigma"]), F32(s["min_sigma"]), F32(s["max_sigma"])], np.float64).tofile(tag + ".params")
    for ext, dt in ((".l", np.uint8), (".r", np.uint8), (".m", F32)):
        np.zeros(1, dt).tofile(tag + ext)
    res = subprocess.run([work["plain"], tag + ".params", tag + ".l", tag + ".r", tag + ".m", tag + ".out"], capture_output=True, text=True)
    assert res.returncode == 2 and "measurement variance" in res.stderr


def test_struct_and_entry_points_are_declared_as_the_binding_mirrors_them():
    import ctypes
    from bpvo_amd import capi
    src = open(os.path.join(ROOT, "include", "bpvo_hip", "c_api.h")).read()
    for struct, mirror in (("bpvo_hip_measurement_variance", capi.MeasurementVariance), ("bpvo_hip_measurement_variance_info", capi.MeasurementVarianceInfo)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct, struct), src, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = [n for decl in re.findall(r"\b(?:float|int|uint32_t)\s+([^;]+);", body) for n in re.findall(r"[A-Za-z_]\w*", decl)]
        assert fields == [f[0] for f in mirror._fields_], struct
    assert ctypes.sizeof(capi.MeasurementVariance) == 20 and ctypes.sizeof(capi.MeasurementVarianceInfo) == 24
    assert tuple(f[0] for f in capi.MeasurementVarianceInfo._fields_) == ref.CLASSES == capi.VARIANCE_CLASSES
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ("set_measurement_variance", "get_measurement_variance", "seq_set_measurement_variance", "seq_get_measurement_variance",
                 "vo_get_measurement_variance", "seq_get_measurement_variance_map", "vo_measurement_variance_info", "seq_measurement_variance_info",
                 "disparity_variance_frames", "fuse_disparities_var", "measurement_variance_counts"):
        assert re.search(r"\bint bpvo_hip_%s\(" % name, code), name
    # the fusion setting keeps its layout: the feature adds no mode and no field to it
    assert ctypes.sizeof(capi.DisparityFusion) == 20


def test_the_header_includes_no_hip_header_and_the_fusion_rule_is_untouched():
    src = open(os.path.join(CSRC, "disparity_variance_math.h")).read()
    assert "#include <hip" not in src and re.findall(r'#include "([^"]+)"', src) == ["disparity_fusion_math.h"]
    kernel = open(os.path.join(CSRC, "kernels_disparity_variance.hip")).read()
    assert "dv_locate(" in kernel and "dv_finish(" in kernel      # the kernel computes the rule through the header
    assert "atomicAdd(float" not in kernel and "hipStreamSynchronize" not in kernel and "hipDeviceSynchronize" not in kernel


def test_the_facade_surface_compiles():
    src = os.path.join(ROOT, "tests", "cpp", "disparity_variance_facade.cc")
    out = subprocess.run(["g++", "-std=c++11", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"), src], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
