"""No-GPU checks of per-sequence cameras (bpvo_hip_create_sequences, bpvo_hip_seq_set_camera / get_camera): the header declares them with
the layout capi.Camera mirrors, the mixed-size packing of add_frames round-trips, the C++ surface compiles, and synth.make_sequence renders
with a camera of its own while its default output stays what it was."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import __graft_entry__ as ge
from bpvo_amd import capi, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "bpvo_hip", "c_api.h")


def test_header_declares_the_camera_entry_points():
    src = open(HEADER).read()
    for name in ("bpvo_hip_create_sequences", "bpvo_hip_seq_set_camera", "bpvo_hip_seq_get_camera"):
        assert name + "(" in src, name


def test_python_camera_matches_the_header_layout():
    src = open(HEADER).read()
    m = re.search(r"typedef struct bpvo_hip_camera \{(.*?)\} bpvo_hip_camera;", src, re.S)
    assert m, "bpvo_hip_camera"
    body = " ".join(m.group(1).split())
    assert body == "float K[9]; float baseline; int rows, cols;", body
    assert [f[0] for f in capi.Camera._fields_] == ["K", "baseline", "rows", "cols"]
    assert C.sizeof(capi.Camera) == 9 * 4 + 4 + 4 + 4
    assert capi.Camera.K.offset == 0 and capi.Camera.baseline.offset == 36 and capi.Camera.rows.offset == 40 and capi.Camera.cols.offset == 44
    cam = capi.camera(np.arange(9).reshape(3, 3), 0.25, 474, 632)
    assert list(cam.K) == [float(v) for v in range(9)] and cam.baseline == 0.25 and (cam.rows, cam.cols) == (474, 632)


def test_pack_frames_round_trips_mixed_sizes():
    rng = np.random.default_rng(3)
    shapes = [(376, 1241), (375, 1242), (370, 1226), (376, 1241), (12, 9)]
    imgs = [rng.integers(0, 256, s, dtype=np.uint8) for s in shapes]
    disps = [rng.standard_normal(s).astype(np.float32) for s in shapes]
    img, disp, got = capi.pack_frames(imgs, disps)
    assert got == shapes
    assert img.dtype == np.uint8 and disp.dtype == np.float32 and img.size == disp.size == sum(r * c for r, c in shapes)
    # frame i begins at the sum of the pixels of the frames before it (what bpvo_hip_add_frames reads)
    at = 0
    for s, im in zip(shapes, imgs):
        assert np.array_equal(img[at:at + s[0] * s[1]], im.reshape(-1))
        at += s[0] * s[1]
    ui, ud = capi.unpack_frames(img, disp, shapes)
    for a, b in zip(ui, imgs):
        assert np.array_equal(a, b)
    for a, b in zip(ud, disps):
        assert a.tobytes() == b.tobytes()
    # frames of one size: exactly the [n][rows * cols] layout
    same = [rng.integers(0, 256, (8, 10), dtype=np.uint8) for _ in range(3)]
    img, _, _ = capi.pack_frames(same, [np.zeros((8, 10), np.float32)] * 3)
    assert np.array_equal(img, np.stack(same).reshape(-1))


def test_make_sequence_renders_with_the_camera_given():
    rows, cols = 120, 160
    K = np.array([[150.0, 0, 80.0], [0, 152.0, 60.0], [0, 0, 1]], np.float32)
    for fx, b in ((150.0, 0.1), (171.0, 0.13)):
        Kc = K.copy()
        Kc[0, 0] = fx
        seq = synth.make_sequence(rows, cols, 2, index=4, camera=(Kc, b))
        assert seq["b"] == b and np.array_equal(seq["K"], Kc)
        img, disp = seq["frames"][0]
        assert img.shape == disp.shape == (rows, cols)
        # first frame (identity pose) of the plane Z = 10 + 0.1 X - 0.15 Y: the optical axis meets it at Z = 10, so disparity = fx b / 10 at (cx, cy)
        assert abs(float(disp[60, 80]) - fx * b / 10.0) <= 1e-5 * fx * b
    # the same camera with twice the baseline: twice the disparity everywhere, the same image
    a = synth.make_sequence(rows, cols, 1, index=4, camera=(K, 0.1))["frames"][0]
    d = synth.make_sequence(rows, cols, 1, index=4, camera=(K, 0.2))["frames"][0]
    assert np.array_equal(a[0], d[0])
    np.testing.assert_allclose(d[1], 2.0 * a[1], rtol=1e-6)


def test_make_sequence_default_output_unchanged():
    rows, cols = 96, 128
    for scene in ("plane", "layered"):
        plain = synth.make_sequence(rows, cols, 3, index=2, scene=scene)
        given = synth.make_sequence(rows, cols, 3, index=2, scene=scene, camera=synth.calibration(rows, cols))
        assert plain["b"] == given["b"] and np.array_equal(plain["K"], given["K"])
        for (ia, da), (ib, db) in zip(plain["frames"], given["frames"]):
            assert ia.tobytes() == ib.tobytes() and da.tobytes() == db.tobytes()


def test_binding_does_not_require_the_camera_symbols():
    """The oracle library shares Binding and has none of these entry points."""
    if not os.path.exists(ge.ORACLE_LIB):
        ge.build_oracle()
    orc = capi.Binding(ge.ORACLE_LIB, "bpvo_orc_")
    assert not orc.has("seq_set_camera") and not orc.has("create_sequences")
    assert isinstance(orc.default_params(), capi.Params)      # the binding works without them


def test_python_surface_has_the_camera_methods():
    for name in ("seq_set_camera", "seq_get_camera", "add_frames", "add_frames_device"):
        assert callable(getattr(capi.Context, name, None)), name
    assert callable(getattr(capi.Binding, "create_sequences", None))


def test_visual_odometry_sequences_with_cameras_compiles_as_cpp11():
    src = os.path.join(ROOT, "tests", "cpp", "seq_cameras_compile.cc")
    out = subprocess.run(["g++", "-std=c++11", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"), src], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
