"""No-GPU checks of the rectification rule (c_api.h "rectification on the device"): bpvo_amd/csrc/rectify_math.h, built into a stand-alone program
by a plain C++ compiler (tests/cpp/rectify_harness.cc) — once plain, once under AddressSanitizer / UBSan —, against the numpy statement of the same
rule (tests/rectify_ref.py): every map entry, every output byte and the outside count equal."""
import os
import subprocess

import numpy as np
import pytest

import rectify_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bpvo_amd", "csrc")


def _build(tmp, name, extra=()):
    exe = str(tmp / name)
    r = subprocess.run(["g++", "-std=c++11", "-O2", "-ffp-contract=off", "-Wall", "-Werror", *extra, "-I", CSRC,
                        os.path.join(ROOT, "tests", "cpp", "rectify_harness.cc"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("rectify")
    return dict(tmp=tmp, plain=_build(tmp, "rectify_harness"),
                san=_build(tmp, "rectify_harness_san", ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all")))


BUILDS = ("plain", "san")


def _raw(rows, cols, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(rows, cols), dtype=np.uint8)


def _read(out, rows, cols):
    words = np.fromfile(out + ".map", np.int32).reshape(rows, cols, 2)
    return words[..., 0], words[..., 1], np.fromfile(out + ".img", np.uint8).reshape(rows, cols)


def _run_lens(work, build, case, raw, tag):
    tmp = work["tmp"]
    p, r, out = str(tmp / (tag + ".params")), str(tmp / (tag + ".raw")), str(tmp / (tag + "_" + build))
    ref.params_f64(case).tofile(p)
    raw.tofile(r)
    res = subprocess.run([work[build], "lens", p, r, out], capture_output=True, text=True)
    assert res.returncode == 0, (res.stdout, res.stderr)
    return (int(res.stdout.split()[0]),) + _read(out, case["rows"], case["cols"])


def _run_maps(work, build, rows, cols, raw, mx, my, tag):
    tmp = work["tmp"]
    names = [str(tmp / (tag + s)) for s in (".params", ".mapx", ".mapy", ".raw")]
    np.float64([rows, cols, raw.shape[0], raw.shape[1]]).tofile(names[0])
    mx.astype(np.float32).tofile(names[1])
    my.astype(np.float32).tofile(names[2])
    raw.tofile(names[3])
    out = str(tmp / (tag + "_" + build))
    res = subprocess.run([work[build], "maps", *names, out], capture_output=True, text=True)
    assert res.returncode == 0, (res.stdout, res.stderr)
    return (int(res.stdout.split()[0]),) + _read(out, rows, cols)


@pytest.mark.parametrize("build", BUILDS)
def test_identity_lens_returns_the_input(work, build):
    case = ref.identity_case()
    rows, cols = case["rows"], case["cols"]
    raw = _raw(rows, cols, 1)
    n_out, xq, yq, img = _run_lens(work, build, case, raw, "identity")
    v, u = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    assert np.array_equal(xq, 32 * u) and np.array_equal(yq, 32 * v)
    assert np.array_equal(img, raw)
    # the taps of the last row and column that lie outside carry weight 0: no pixel is outside
    assert n_out == 0
    rimg, rout, (rxq, ryq) = ref.rectify(case, raw)
    assert np.array_equal(rxq, xq) and np.array_equal(ryq, yq) and np.array_equal(rimg, raw) and rout == 0


@pytest.mark.parametrize("build", BUILDS)
@pytest.mark.parametrize("name", sorted(ref.hard_cases()))
def test_hard_lens_equals_numpy(work, build, name):
    case, share_seen = ref.hard_cases()[name]
    raw = _raw(case["raw_rows"], case["raw_cols"], 2)
    rimg, rout, (rxq, ryq) = ref.rectify(case, raw)
    # the precondition, on the numpy side only: the case reaches outside the raw image, on the low side too
    xs, ys = ref.lens_source(case)
    share = rout / float(case["rows"] * case["cols"])
    print(name, "outside", rout, "share %.4f" % share)
    assert 0.05 <= share <= 0.50 and (xs.min() < 0 or ys.min() < 0), (name, share, xs.min(), ys.min())
    assert abs(share - share_seen) < 0.0006, (name, share)
    n_out, xq, yq, img = _run_lens(work, build, case, raw, name)
    assert np.array_equal(xq, rxq) and np.array_equal(yq, ryq)
    assert np.array_equal(img, rimg)
    assert n_out == rout


def test_a_wider_rectified_camera_sees_less_outside():
    case = ref.lens_case(41, 59, 37, 53, 40.0, 0.7)
    _, rout, _ = ref.rectify(case, _raw(41, 59, 2))
    assert abs(rout / float(37 * 53) - 0.176) < 0.0006


@pytest.mark.parametrize("build", BUILDS)
def test_callers_maps_ties_negatives_and_sentinels(work, build):
    rows, cols, raw_rows, raw_cols = 37, 53, 41, 59
    raw = _raw(raw_rows, raw_cols, 3)
    mx, my = ref.hostile_maps(rows, cols, raw_rows, raw_cols)
    rxq, ryq = ref.quantise(mx, my)
    # what the case is there for, on the numpy side: ties to even on both sides of 0, sentinels, negative entries
    assert list(rxq[0, :8]) == [0, 2, 2, 0, -2, -2, 4, 4]
    assert np.all(rxq[2, :4] == ref.OUTSIDE) and np.all(ryq[2, :6] == ref.OUTSIDE) and np.all(rxq[2, 4:6] == ref.OUTSIDE)
    assert rxq[3, 0] != ref.OUTSIDE and rxq[3, 1] == ref.OUTSIDE and rxq[3, 2] == ref.OUTSIDE
    assert list(rxq[1, :6]) == [-32, -16, 0, 0, -24, -8]      # -31.968, -16, -0.32, the tie -0.5, -24, -8
    n_out, xq, yq, img = _run_maps(work, build, rows, cols, raw, mx, my, "hostile")
    assert np.array_equal(xq, rxq) and np.array_equal(yq, ryq)
    rimg = ref.remap(raw, rxq, ryq)
    assert np.array_equal(img, rimg)
    assert np.all(img[2, :6] == 0)
    assert n_out == int(ref.outside(raw_rows, raw_cols, rxq, ryq).sum())


@pytest.mark.parametrize("build", BUILDS)
def test_callers_maps_all_at_the_last_raw_pixel(work, build):
    rows, cols, raw_rows, raw_cols = 37, 53, 41, 59
    raw = _raw(raw_rows, raw_cols, 4)
    mx, my = ref.last_pixel_maps(rows, cols, raw_rows, raw_cols)
    n_out, xq, yq, img = _run_maps(work, build, rows, cols, raw, mx, my, "last")
    assert np.all(xq == 32 * (raw_cols - 1)) and np.all(yq == 32 * (raw_rows - 1))
    assert np.all(img == raw[-1, -1]) and n_out == 0
    assert np.array_equal(img, ref.remap(raw, *ref.quantise(mx, my)))


def test_lens_struct_and_entry_points_are_declared_as_the_binding_mirrors_them():
    import re
    from bpvo_amd import capi
    src = open(os.path.join(ROOT, "include", "bpvo_hip", "c_api.h")).read()
    body = re.search(r"typedef struct bpvo_hip_lens \{(.*?)\} bpvo_hip_lens;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [n for decl in re.findall(r"\b(?:double|int)\s+([^;]+);", body) for n in re.findall(r"[A-Za-z_]\w*", re.sub(r"\[\d+\]", "", decl))]
    assert fields == [f[0] for f in capi.Lens._fields_] and ctypes_size(capi.Lens) == 21 * 8 + 2 * 4
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ("seq_set_rectification", "seq_set_rectification_maps", "seq_clear_rectification", "seq_rectification_info", "set_rectification",
                 "set_rectification_maps", "clear_rectification", "rectification_info", "rectify_frames", "add_frames_stereo_raw",
                 "add_frame_stereo_raw", "rectify_counts"):
        assert re.search(r"\bint bpvo_hip_%s\(" % name, code), name
    assert "parity with cv::remap is unpinned" in src


def ctypes_size(t):
    import ctypes
    return ctypes.sizeof(t)


def test_header_and_numpy_state_one_outside_sentinel():
    src = open(os.path.join(CSRC, "rectify_math.h")).read()
    assert "kRectOutside = INT32_MIN" in src and int(ref.OUTSIDE) == -2 ** 31
