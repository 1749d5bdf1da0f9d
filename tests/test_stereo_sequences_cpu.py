"""No-GPU checks of the stereo front-end for many cameras (bpvo_hip_stereo_frames, bpvo_hip_add_frames_stereo): the header declares them as
the Python binding calls them, mixed-size left / right stacks pack like add_frames' frames, the C++ overload compiles, and
synth.make_stereo_sequence renders with a camera of its own while its default output stays what it was.  (test_cabi_cpu.py's export test
covers the two new C declarations.)"""
import inspect
import os
import re
import subprocess

import numpy as np

from bpvo_amd import capi, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "bpvo_hip", "c_api.h")


def _declaration(name):
    src = open(HEADER).read()
    m = re.search(r"\bint " + name + r"\((.*?)\);", src, re.S)
    assert m, name
    args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    return [" ".join(a.split()) for a in args.split(",")]


def test_header_declares_the_stereo_sequence_entry_points():
    assert _declaration("bpvo_hip_stereo_frames") == [
        "bpvo_hip_ctx* ctx", "int n", "const bpvo_hip_camera* cams", "const uint8_t* left", "const uint8_t* right", "int on_device",
        "const bpvo_hip_stereo_params* sp", "float* disparity", "int disparity_on_device"]
    assert _declaration("bpvo_hip_add_frames_stereo") == [
        "bpvo_hip_ctx* ctx", "int n", "const int* seq", "const uint8_t* left", "const uint8_t* right", "int on_device",
        "const bpvo_hip_stereo_params* sp", "bpvo_hip_result* results"]
    # the camera type is declared before the entry point that takes it, the stereo parameters likewise
    src = open(HEADER).read()
    assert src.index("} bpvo_hip_camera;") < src.index("int bpvo_hip_stereo_frames(")
    assert src.index("} bpvo_hip_stereo_params;") < src.index("int bpvo_hip_stereo_frames(")


def test_python_calls_pass_what_the_header_declares():
    """The binding passes positional ctypes arguments: their number and order per entry point against the declaration (the context first)."""
    for method, name in (("stereo_frames", "stereo_frames"), ("stereo_frames_device", "stereo_frames"), ("add_frames_stereo", "add_frames_stereo"),
                         ("add_frames_stereo_device", "add_frames_stereo")):
        fn = getattr(capi.Context, method, None)
        assert callable(fn), method
        src = inspect.getsource(fn)
        m = re.search(r'self\.call\("' + name + r'",(.*)\)\n', src)
        assert m, method
        depth, nargs = 0, 1
        for ch in m.group(1):
            depth += ch in "(["
            depth -= ch in ")]"
            nargs += ch == "," and depth == 0
        assert nargs == len(_declaration("bpvo_hip_" + name)) - 1, (method, nargs)


def test_pack_images_lays_mixed_sizes_back_to_back():
    rng = np.random.default_rng(5)
    shapes = [(376, 1241), (375, 1242), (370, 1226), (480, 640), (240, 320)]
    lefts = [rng.integers(0, 256, s, dtype=np.uint8) for s in shapes]
    rights = [rng.integers(0, 256, s, dtype=np.uint8) for s in shapes]
    left, got = capi.pack_images(lefts)
    right, got_r = capi.pack_images(rights)
    assert got == got_r == shapes
    assert left.dtype == right.dtype == np.uint8 and left.size == right.size == sum(r * c for r, c in shapes)
    at = 0
    for s, l, r in zip(shapes, lefts, rights):      # pair i begins at the sum of the pixels of the pairs before it, in both stacks
        assert np.array_equal(left[at:at + s[0] * s[1]], l.reshape(-1)) and np.array_equal(right[at:at + s[0] * s[1]], r.reshape(-1))
        at += s[0] * s[1]
    # the layout of add_frames' images (pack_frames), and of a plain stack where the sizes agree
    img, _, _ = capi.pack_frames(lefts, [np.zeros(s, np.float32) for s in shapes])
    assert np.array_equal(img, left)
    same = [rng.integers(0, 256, (8, 10), dtype=np.uint8) for _ in range(3)]
    assert np.array_equal(capi.pack_images(same)[0], np.stack(same).reshape(-1))


def test_camera_array_takes_cameras_tuples_and_sizes():
    K = np.array([[150.0, 0, 80.0], [0, 152.0, 60.0], [0, 0, 1]], np.float32)
    cams = capi.Context._camera_array([capi.camera(K, 0.1, 120, 160), (K, 0.2, 96, 128), (240, 320)])
    assert [(c.rows, c.cols) for c in cams] == [(120, 160), (96, 128), (240, 320)]
    assert cams[1].baseline == np.float32(0.2) and cams[0].K[0] == 150.0


def test_make_stereo_sequence_default_output_unchanged():
    """camera=None is what bench.py and the existing tests call: the same bytes as with synth.calibration(rows, cols) given, and the left
    images and true disparities are make_sequence's."""
    for rows, cols, n, kw in ((480, 640, 9, dict(index=23, step_rot=0.004, step_trans=0.03)), (240, 320, 4, dict(index=9))):
        plain = synth.make_stereo_sequence(rows, cols, n, **kw)
        given = synth.make_stereo_sequence(rows, cols, n, camera=synth.calibration(rows, cols), **kw)
        mono = synth.make_sequence(rows, cols, n, **kw)
        assert plain["b"] == given["b"] == mono["b"] and np.array_equal(plain["K"], given["K"]) and np.array_equal(plain["K"], mono["K"])
        assert len(plain["frames"]) == n
        for (la, ra), (lb, rb), da, db, (lm, dm) in zip(plain["frames"], given["frames"], plain["disps"], given["disps"], mono["frames"]):
            assert la.tobytes() == lb.tobytes() == lm.tobytes() and ra.tobytes() == rb.tobytes()
            assert da.tobytes() == db.tobytes() == dm.tobytes()


def test_make_stereo_sequence_renders_with_the_camera_given():
    rows, cols = 120, 160
    K = np.array([[150.0, 0, 80.0], [0, 152.0, 60.0], [0, 0, 1]], np.float32)
    for b in (0.1, 0.2):
        st = synth.make_stereo_sequence(rows, cols, 2, index=4, camera=(K, b))
        assert st["b"] == b and np.array_equal(st["K"], K)
        mono = synth.make_sequence(rows, cols, 2, index=4, camera=(K, b))
        for (left, right), disp, (lm, dm), T in zip(st["frames"], st["disps"], mono["frames"], st["poses"]):
            assert left.tobytes() == lm.tobytes() and disp.tobytes() == dm.tobytes()
            # the right image is what the left camera sees from the baseline along +x: the same scene rendered by make_sequence's renderer
            # from X_right = X_left - (b, 0, 0)
            shift = np.eye(4)
            shift[0, 3] = -b
            want, _ = synth._render(K, b, rows, cols, shift @ T, 1000 + 4, 10.0, (0.1, -0.15))
            assert right.tobytes() == want.tobytes()
    # on the first frame's plane the true disparity at the principal point is fx b / Z with Z = 10, and the right image is the left one moved
    # by that many pixels there: the row through the principal point matches best at that shift
    st = synth.make_stereo_sequence(rows, cols, 1, index=4, camera=(K, 0.2))
    (left, right), disp = st["frames"][0], st["disps"][0]
    d = float(disp[60, 80])
    assert abs(d - 150.0 * 0.2 / 10.0) <= 1e-5 * 30.0
    win = left[56:65, 60:100].astype(np.float64)
    errs = [np.abs(win - right[56:65, 60 - s:100 - s].astype(np.float64)).mean() for s in range(0, 8)]
    assert int(np.argmin(errs)) == int(round(d)), errs
    # twice the baseline: the same left image, twice the disparity
    a = synth.make_stereo_sequence(rows, cols, 1, index=4, camera=(K, 0.1))
    assert a["frames"][0][0].tobytes() == left.tobytes()
    np.testing.assert_allclose(disp, 2.0 * a["disps"][0], rtol=1e-6)


def test_visual_odometry_sequences_stereo_overload_compiles_as_cpp11():
    src = os.path.join(ROOT, "tests", "cpp", "stereo_sequences_compile.cc")
    out = subprocess.run(["g++", "-std=c++11", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"), src], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
