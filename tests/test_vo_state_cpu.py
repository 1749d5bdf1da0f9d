"""The addFrame state machine of bpvo_hip_add_frame and bpvo_hip_add_frames (bpvo_amd/csrc/vo_state.h) without a GPU:
tests/cpp/vo_state_harness.cc includes only that header, is compiled by the host's C++ compiler — which proves the header free of HIP — and
drives it the way the drivers in vo.hip do.  Slot roles, flags and the copies of poses are checked against the values read off
bpvo/vo.cc:133-188 as oracle/src/pose_estimator.cc:331-402 restates them; the key-frame decision against a numpy float32 evaluation of
bpvo/vo.cc:199-224."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from bpvo_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = 3


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("vo_state") / "libvo_state.so")
    cmd = [os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared",
           "-I", os.path.join(ROOT, "bpvo_amd", "csrc"), "-o", out, os.path.join(ROOT, "tests", "cpp", "vo_state_harness.cc")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lib = C.CDLL(out)
    lib.vs_add_frame.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_float, C.c_size_t, C.c_void_p, C.c_void_p]
    lib.vs_keyframe_reason.argtypes = [C.c_void_p, C.c_void_p, C.c_uint, C.c_int, C.c_int]
    lib.vs_state.argtypes = [C.c_void_p] * 4
    lib.vs_init_result.argtypes = [C.c_int, C.c_void_p]
    return lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32).tolist()


def pose(angle=0.0, axis=(0.0, 0.0, 1.0), t=(0.0, 0.0, 0.0)):
    """A rigid pose as 16 row-major float32: Rodrigues' rotation by `angle` about `axis`, translation t."""
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    S = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(angle) * S + (1 - np.cos(angle)) * (S @ S)
    T[:3, 3] = t
    return np.ascontiguousarray(T.reshape(16), np.float32)


def key_frame_params():
    p = capi.Params()
    p.minTranslationMagToKeyFrame = 0.1
    p.minRotationMagToKeyFrame = 0.1
    p.maxFractionOfGoodPointsToKeyFrame = 0.6
    return p


class Machine:
    def __init__(self, lib):
        self.lib = lib
        self.p = key_frame_params()
        lib.vs_reset()

    def add(self, T_est, T_again=None, frac=0.9, cloud_points=123):
        ret = capi.Result()
        out = np.full(6, -7, np.int32)
        T_again = pose() if T_again is None else T_again
        self.lib.vs_add_frame(C.addressof(self.p), L, _p(T_est), _p(T_again), frac, cloud_points, C.addressof(ret), _p(out))
        return ret, out.tolist()

    def state(self):
        T_kf, cloud_pose, back = (np.full(16, np.nan, np.float32) for _ in range(3))
        n = C.c_size_t(0)
        size = self.lib.vs_state(_p(T_kf), _p(cloud_pose), _p(back), C.byref(n))
        return dict(T_kf=T_kf, cloud_pose=cloud_pose, back=back, size=size, cloud_n=n.value)


def flags(ret):
    return ret.isKeyFrame, ret.keyFramingReason, ret.hasPointCloud


IDENTITY = pose()
SMALL = pose(0.01, t=(0.01, 0.0, 0.02))            # no criterion of key_frame_params() met (with frac = 0.9)
SMALL2 = pose(-0.02, (1, 0, 0), t=(0.0, 0.03, 0.01))
LARGE = pose(0.02, t=(0.3, 0.0, 0.1))              # squared translation 0.1 against 0.01
AGAIN = pose(0.03, (0, 1, 0), t=(0.02, -0.01, 0.05))


def test_slot_roles_flags_and_pose_copies(harness):
    m = Machine(harness)
    # first frame (vo.cc:133-139): the frame read into cur = 1 becomes the key frame
    ret, out = m.add(SMALL)
    assert out == [1, 0, 2, 1, -1, 0] and flags(ret) == (1, capi.KF_FIRST_FRAME, 0)
    s = m.state()
    assert s["size"] == 1 and np.array_equal(s["back"], IDENTITY) and bits(ret.pose) == bits(IDENTITY) and s["cloud_n"] == 0
    # two frames that are no key frames (vo.cc:149-155): swap(prev, cur); T_kf is a copy of T_est
    ret, out = m.add(SMALL)
    assert out == [1, 2, 0, -1, -1, 0] and flags(ret) == (0, capi.KF_NO_KEYFRAMING, 0)
    assert bits(m.state()["T_kf"]) == bits(SMALL) and np.array_equal(np.asarray(ret.pose, np.float32), SMALL)      # (T_est * inverse(identity))
    ret, out = m.add(SMALL2)
    assert out == [1, 0, 2, -1, -1, 0] and flags(ret) == (0, capi.KF_NO_KEYFRAMING, 0)
    s = m.state()
    assert bits(s["T_kf"]) == bits(SMALL2) and s["size"] == 3 and s["cloud_n"] == 0 and bits(s["cloud_pose"]) == bits(IDENTITY)
    # key frame with a previous frame (vo.cc:174-188): swap(prev, ref), the old key frame (slot 1) is cleared, slot 2 gets the template,
    # the estimate is repeated from the identity and both T_kf and the pose are copies of it
    ret, out = m.add(LARGE, AGAIN, cloud_points=77)
    assert out == [2, 0, 1, 2, 1, 1] and flags(ret) == (1, capi.KF_LARGE_TRANSLATION, 1)
    s = m.state()
    assert bits(s["T_kf"]) == bits(AGAIN) and bits(ret.pose) == bits(AGAIN)
    assert s["cloud_n"] == 77 and s["size"] == 4 and bits(s["cloud_pose"]) == bits(s["back"])
    # a frame that is no key frame: the point cloud belonged to the Result before
    ret, out = m.add(SMALL)
    assert out == [2, 1, 0, -1, -1, 0] and flags(ret) == (0, capi.KF_NO_KEYFRAMING, 0)
    s = m.state()
    assert bits(s["T_kf"]) == bits(SMALL) and s["cloud_n"] == 0 and bits(s["cloud_pose"]) == bits(IDENTITY) and s["size"] == 5

    # after a reset: a first frame, then at once a key frame — no previous frame (vo.cc:161-173): swap(cur, ref), nothing cleared, no second
    # estimate, T_kf is the identity
    harness.vs_reset()
    s = m.state()
    assert s["size"] == 0 and bits(s["T_kf"]) == bits(IDENTITY)
    ret, out = m.add(SMALL)
    assert out == [1, 0, 2, 1, -1, 0] and flags(ret) == (1, capi.KF_FIRST_FRAME, 0)
    ret, out = m.add(SMALL, AGAIN, frac=0.3, cloud_points=5)
    assert out == [0, 1, 2, 0, -1, 0] and flags(ret) == (1, capi.KF_SMALL_FRAC_GOOD, 1)
    s = m.state()
    assert bits(s["T_kf"]) == bits(IDENTITY) and np.array_equal(np.asarray(ret.pose, np.float32), SMALL)
    assert s["cloud_n"] == 5 and s["size"] == 2 and bits(s["cloud_pose"]) == bits(s["back"])
    # ... and the frame after it has a previous frame to fall back on: the key frame with a second estimate again
    ret, out = m.add(SMALL2)
    assert out == [0, 2, 1, -1, -1, 0]
    ret, out = m.add(LARGE, AGAIN)
    assert out == [1, 2, 0, 1, 0, 1] and flags(ret) == (1, capi.KF_LARGE_TRANSLATION, 1)


def reason_f32(p, T, good, n, Cn):
    """bpvo/vo.cc:199-224 in numpy float32: the three comparisons in their order."""
    f = np.float32
    T = np.asarray(T, f)
    t_norm = f(f(T[3] * T[3] + T[7] * T[7]) + T[11] * T[11])
    if t_norm > f(p.minTranslationMagToKeyFrame) * f(p.minTranslationMagToKeyFrame):
        return capi.KF_LARGE_TRANSLATION
    eta = f(1.0 / np.float64(np.sqrt(f(T[0] * T[0] + T[4] * T[4]))))
    rz, ry, rx = np.arcsin(f(eta * T[4])), np.arcsin(f(-T[8])), np.arcsin(f(eta * T[9]))
    r_norm = f(f(rx * rx + ry * ry) + rz * rz)
    if r_norm > f(p.minRotationMagToKeyFrame) * f(p.minRotationMagToKeyFrame):
        return capi.KF_LARGE_ROTATION
    frac = f(f(good) / f(n * Cn))
    return capi.KF_SMALL_FRAC_GOOD if frac < f(p.maxFractionOfGoodPointsToKeyFrame) else capi.KF_NO_KEYFRAMING


def test_keyframe_reason(harness):
    """Squared norms a factor two or more from the thresholds (0.01 both) and fractions 0.05 or more from 0.6: no ulp of asinf decides."""
    p = key_frame_params()
    rng = np.random.default_rng(3)
    seen = set()
    n, Cn = 1000, 8
    for trial in range(400):
        t2 = [0.0, 0.001, 0.005, 0.02, 0.5][rng.integers(0, 5)]            # squared translation
        r2 = [0.0, 0.0005, 0.005, 0.02, 0.3][rng.integers(0, 5)]           # squared rotation angle
        frac = [0.0, 0.3, 0.55, 0.65, 0.9, 1.0][rng.integers(0, 6)]
        d = rng.standard_normal(3)
        axis = np.eye(3)[rng.integers(0, 3)]      # about one axis the three Euler angles are (angle, 0, 0) in some order: their squared norm is r2
        T = pose(np.sqrt(r2) * rng.choice([-1, 1]), axis, np.sqrt(t2) * d / np.linalg.norm(d))
        good = int(round(frac * n * Cn))
        got = harness.vs_keyframe_reason(C.addressof(p), _p(T), good, n, Cn)
        assert got == reason_f32(p, T, good, n, Cn), (trial, t2, r2, frac)
        want = capi.KF_LARGE_TRANSLATION if t2 > 0.01 else capi.KF_LARGE_ROTATION if r2 > 0.01 else \
            capi.KF_SMALL_FRAC_GOOD if frac < 0.6 else capi.KF_NO_KEYFRAMING
        assert got == want, (trial, t2, r2, frac)
        seen.add(got)
    assert seen == {capi.KF_LARGE_TRANSLATION, capi.KF_LARGE_ROTATION, capi.KF_SMALL_FRAC_GOOD, capi.KF_NO_KEYFRAMING}


def test_init_result_is_the_documented_default(harness):
    want = capi.Result()
    for i in range(4):
        want.pose[i * 5] = 1.0
    for i in range(6):
        want.covariance[i * 7] = 1.0
    for l in range(capi.MAX_LEVELS):
        want.optimizerStatistics[l] = capi.Stats(0, -1.0, -1.0, capi.STATUS_SOLVER_ERROR)
    want.numLevels = L
    want.isKeyFrame, want.keyFramingReason, want.hasPointCloud = 0, capi.KF_NO_KEYFRAMING, 0
    got = capi.Result()
    C.memset(C.addressof(got), 0xA5, C.sizeof(got))
    harness.vs_init_result(L, C.addressof(got))
    assert bytes(got) == bytes(want)
