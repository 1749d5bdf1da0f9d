"""Normalised intensity, without a GPU: the numpy statement of the rule (tests/intensity_norm_ref.py) on hand-worked cases; the library's own
statement (bpvo_amd/csrc/intensity_norm_math.h), built for the host by tests/cpp/intensity_norm_harness.cc, against it bit for bit; the invariance
the mode exists for, on the reference; the C ABI's, the binding's and the facade's surface; the frame plan's treatment of the new form."""
import os
import re
import subprocess

import numpy as np
import pytest

import bpvo_amd
import intensity_norm_ref as inr
from bpvo_amd import capi, synth
from util import bits_equal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_FUNCTIONS = ["bpvo_hip_set_intensity_normalization", "bpvo_hip_get_intensity_normalization"]
CXX = os.environ.get("CXX", "g++")


# ---- the reference against hand-worked cases

def test_constant_image():
    img = np.full((9, 11), 77, np.uint8)
    assert inr.median_mad(img) == (77, 0)                      # mad = 0 -> m = 1
    assert np.all(inr.whole_image(img) == 0) and inr.whole_image(img).dtype == np.float32
    for R in (1, 7, 15):
        X, V, n = inr.local_terms(img, R)
        assert np.all(X == 0) and np.all(V == 0) and np.all(inr.floor_binds(img, R))      # V = 0 < 4 n^2: the floor, D = 0
        assert np.all(inr.local(img, R) == 0)


def test_two_valued_image():
    # 6 pixels of 10 and 4 of 50: half = 5 -> med = 10; |I - 10| is 0 six times: mad = 0 -> m = 1, c = 32 / 1.4826
    img = np.array([[10] * 5, [10, 50, 50, 50, 50]], np.uint8)
    assert inr.median_mad(img) == (10, 0)
    c = 32.0 / 1.4826
    want = np.where(img == 10, np.float32(0), np.float32(40.0 * c))
    assert bits_equal(inr.whole_image(img), want.astype(np.float32))
    # 4 of 10 and 6 of 50: med = 50; |I - 50|: 0 six times -> mad 0
    assert inr.median_mad(255 - np.array([[205] * 5, [205, 245, 245, 245, 245]], np.uint8)) == (50, 0)
    # half 0, half 255: the lower median is 0, and half the pixels lie within 0 of it -> mad 0
    assert inr.median_mad(np.array([[0, 0, 255, 255]], np.uint8)) == (0, 0)
    # 3 x 3, R = 1, centre pixel: n = 9, S1 = 10 * 5 + 50 * 4 = 250, S2 = 500 + 10000 = 10500; X = 9 * 50 - 250 = 200,
    # V = 9 * 10500 - 62500 = 32000 > 4 * 81 -> D = 32 * 200 / sqrt(32000)
    img = np.array([[10, 50, 10], [50, 50, 10], [10, 50, 10]], np.uint8)
    n, S1, S2 = inr.window_sums(img, 1)
    assert (n[1, 1], S1[1, 1], S2[1, 1]) == (9, 250, 10500) and n[0, 0] == 4 and n[0, 1] == 6
    assert inr.local(img, 1)[1, 1] == np.float32(32.0 * 200.0 / np.sqrt(32000.0))
    # the corner: the window is cut to 2 x 2 = {10, 50, 50, 50}: X = 4 * 10 - 160 = -120, V = 4 * 7600 - 25600 = 4800
    assert inr.local(img, 1)[0, 0] == np.float32(32.0 * -120.0 / np.sqrt(4800.0))


def test_even_count_takes_the_lower_median():
    img = np.array([[1, 2, 3, 4]], np.uint8)                   # n_px = 4, half = 2: med = 2 (not 2.5, not 3)
    med, mad = inr.median_mad(img)
    assert med == 2 and mad == 1                               # |I - 2| = 1, 0, 1, 2: two within 0? no (one); three within 1
    img = np.array([[1, 2, 3, 4, 5]], np.uint8)                # n_px = 5, half = 3: med = 3; |I - 3| = 2, 1, 0, 1, 2 -> mad = 1
    assert inr.median_mad(img) == (3, 1)
    img = np.array([[0, 0, 0, 9, 200, 255]], np.uint8)         # half = 3: med = 0, and three pixels lie within 0
    assert inr.median_mad(img) == (0, 0)
    img = np.array([[0, 0, 9, 9, 200, 255]], np.uint8)         # med = 9; |I - 9| = 9, 9, 0, 0, 191, 246: two within 0, four within 9
    assert inr.median_mad(img) == (9, 9)
    assert bits_equal(inr.whole_image(img), ((img.astype(np.float64) - 9) * (32.0 / (1.4826 * 9.0))).astype(np.float32))


def test_window_sums_against_brute_force():
    rng = np.random.default_rng(11)
    img = rng.integers(0, 256, (13, 9), dtype=np.uint8)
    for R in (1, 3, 15):
        n, S1, S2 = inr.window_sums(img, R)
        for y in range(13):
            for x in range(9):
                w = img[max(y - R, 0):y + R + 1, max(x - R, 0):x + R + 1].astype(np.int64)
                assert (n[y, x], S1[y, x], S2[y, x]) == (w.size, w.sum(), (w * w).sum())


# ---- the header's rule, built for the host, against the reference

@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    d = tmp_path_factory.mktemp("intensity_norm")
    exe = str(d / "intensity_norm_harness")
    # -ffp-contract=off as the library is built: no fused multiply-add in the last step
    cmd = [CXX, "-O2", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-I", os.path.join(ROOT, "bpvo_amd", "csrc"), "-o", exe,
           os.path.join(ROOT, "tests", "cpp", "intensity_norm_harness.cc")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def run(img, R):
        src, dst = str(d / "image.u8"), str(d / "plane.f32")
        np.ascontiguousarray(img, np.uint8).tofile(src)
        out = subprocess.run([exe, str(img.shape[1]), str(img.shape[0]), str(R), src, dst], capture_output=True, text=True)
        assert out.returncode == 0, out.stderr
        return np.fromfile(dst, np.float32).reshape(img.shape)
    return run


@pytest.mark.parametrize("rows,cols", [(12, 17), (67, 45), (120, 160)])
def test_header_rule_equals_the_reference_bit_for_bit(harness, rows, cols):
    rng = np.random.default_rng(rows * 1000 + cols)
    images = [rng.integers(0, 256, (rows, cols), dtype=np.uint8),
              (rng.integers(0, 256, (rows, cols)) // 64 * 3 + 100).astype(np.uint8),      # four close values: the floor binds in many windows
              np.full((rows, cols), 200, np.uint8)]
    for img in images:
        for R in (0, 1, 7, 15):
            assert bits_equal(harness(img, R), inr.normalize(img, R)), (rows, cols, R)


# ---- the invariance the mode exists for, on the reference, bitwise

@pytest.mark.parametrize("scene", ["plane", "layered"])
def test_exact_affine_maps_leave_the_plane_unchanged(scene):
    imgB = synth.make_pair(120, 160, 0, scene=scene)["imgB"]
    I = (imgB >> 1).astype(np.uint8)
    J = (2 * I.astype(np.int32) + 10)
    assert J.max() <= 255
    J = J.astype(np.uint8)
    for R in (7, 15):
        assert not inr.floor_binds(I, R).any() and not inr.floor_binds(J, R).any(), (scene, R)
        a, b = inr.local(I, R), inr.local(J, R)
        assert bits_equal(a, b) and np.abs(a).max() > 1.0
    assert bits_equal(inr.whole_image(I), inr.whole_image(J)) and np.abs(inr.whole_image(I)).max() > 1.0
    assert not bits_equal(inr.normalize(I, -1), inr.normalize(J, -1))


# ---- the surface

def test_header_declares_and_library_exports_the_new_functions():
    doc = open(os.path.join(ROOT, "include", "bpvo_hip", "c_api.h")).read()
    src = re.sub(r"/\*.*?\*/", "", doc, flags=re.S)
    lib = bpvo_amd.load()
    for name in NEW_FUNCTIONS:
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), f"{name} is not declared in c_api.h"
        assert hasattr(lib.lib, name), f"{name} is not exported"
        assert re.search(name + r" \(an extension, no reference member", doc), name
    assert hasattr(capi.Context, "set_intensity_normalization") and hasattr(capi.Context, "get_intensity_normalization")


def test_no_field_was_added_to_the_parameters():
    assert not any("ormali" in name and name != "withNormalization" for name, _ in capi.Params._fields_)


def test_facade_compiles():
    src = os.path.join(ROOT, "tests", "cpp", "intensity_norm_compile.cc")
    out = subprocess.run([CXX, "-std=c++11", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"), src], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr


# ---- the frame plan: the new form where Intensity stands and the mode is on, merged into one launch where Intensity is

def test_frame_plan_gives_the_new_form_what_intensity_gets(tmp_path):
    exe = str(tmp_path / "intensity_norm_plan_harness")
    cmd = [CXX, "-O1", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "bpvo_amd", "csrc"), "-I", os.path.join(ROOT, "include"), "-o", exe,
           os.path.join(ROOT, "tests", "cpp", "intensity_norm_plan_harness.cc")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def plan(*q):
        out = subprocess.run([exe, *[str(v) for v in q]], capture_output=True, text=True)
        assert out.returncode == 0, out.stderr
        return [int(v) for v in out.stdout.split()]      # [new form with the radius, Intensity without, merged with, merged without]
    for radius in (0, 1, 7, 15):
        for count, max_frames, tested in [(1, 8, 3), (8, 8, 2), (9, 8, 3), (1, 0, 3), (1, 8, 1)]:
            few = int(count <= max_frames and tested > 1)
            assert plan(capi.DESC_INTENSITY, 1, radius, count, max_frames, tested) == [1, 1, few, few]
    assert plan(capi.DESC_INTENSITY, 1, -1, 1, 8, 3) == [0, 1, 1, 1]                 # off: plain Intensity
    # every other descriptor ignores the radius
    for desc, C in [(capi.DESC_LAPLACIAN, 1), (capi.DESC_BITPLANES, 8), (capi.DESC_GRADIENT, 3), (capi.DESC_FIELDS1, 5)]:
        got = plan(desc, C, 7, 1, 8, 3)
        assert got[0] == 0 and got[1] == 0 and got[2] == got[3]
