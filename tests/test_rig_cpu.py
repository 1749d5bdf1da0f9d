"""Rig mode without a GPU: the maps of bpvo_amd/csrc/rig_math.h (Ad(X), A_p, A_p^-1, B_p = A_p^-1 Ad(X_p), the congruence B^T H B / B^T G, the
member pose X T X^-1) against numpy float64, the two identities the maps rest on — X exp(zeta) X^-1 = exp(Ad(X) zeta) and
N^-1 exp(xi) N = exp(A xi) — checked numerically with the project's own SE(3) exponential (independently of the code under test), and the rig
additions to bpvo_amd/csrc/vo_state.h (the transitions of a body, vo_rig_*): the pooled fraction of good points, one key-frame decision applied to
every member, cloud poses W_kf X_p^-1 — and, with null extrinsics, exactly the plain vo_* calls on one state, which is how the batched driver
advances a sequence.  tests/cpp/rig_harness.cc includes only the two headers and is compiled by the host's C++ compiler."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from bpvo_amd import capi, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = 3
EXTRINSIC_TWISTS = ((0, 0, 0, 0, 0, 0), (0, 0.14, 0.02, 0.3, 0.02, 0.1), (0.03, -0.2, 0, -0.4, 0, 0.05))
NORMALIZATIONS = ((1.0, 0.0, 0.0, 0.0), (0.37, 0.2, -0.1, 9.5), (12.5, -1.5, 0.75, 3.0))


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("rig") / "librig.so")
    cmd = [os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared",
           "-I", os.path.join(ROOT, "bpvo_amd", "csrc"), "-o", out, os.path.join(ROOT, "tests", "cpp", "rig_harness.cc")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lib = C.CDLL(out)
    lib.rg_fraction_good.restype = C.c_float
    lib.rg_fraction_good.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    lib.rg_fraction_good_one.restype = C.c_float
    lib.rg_fraction_good_one.argtypes = [C.c_uint, C.c_int, C.c_int]
    lib.rg_fraction_good_null.restype = C.c_float
    lib.rg_fraction_good_null.argtypes = [C.c_uint, C.c_int, C.c_int]
    lib.rg_plain_add_frame.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_uint, C.c_int, C.c_int, C.c_size_t, C.c_void_p, C.c_void_p]
    lib.rg_state_bytes.argtypes = [C.c_int, C.c_void_p, C.c_int]
    lib.rg_add_frame.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                 C.c_void_p, C.c_void_p]
    lib.rg_state.argtypes = [C.c_int] + [C.c_void_p] * 4
    return lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def f32(a):
    return np.ascontiguousarray(a, np.float32)


def extrinsics():
    return [f32(synth.twist_to_matrix(t)) for t in EXTRINSIC_TWISTS]


def skew(v):
    return np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]], np.float64)


def adjoint(X):
    X = np.asarray(X, np.float64)
    R, t = X[:3, :3], X[:3, 3]
    Ad = np.zeros((6, 6))
    Ad[:3, :3] = R
    Ad[3:, :3] = skew(t) @ R
    Ad[3:, 3:] = R
    return Ad


def norm_map(nrm):
    s, c = float(np.float32(nrm[0])), np.asarray(f32(nrm[1:]), np.float64)
    A = np.eye(6)
    A[3:, :3] = skew(c)
    A[3:, 3:] = np.eye(3) / s
    return A


def norm_matrix(nrm):
    s, c = float(np.float32(nrm[0])), np.asarray(f32(nrm[1:]), np.float64)      # (the f32 values norm_map reads)
    N = np.eye(4)
    N[:3, :3] *= s
    N[:3, 3] = -s * c
    return N


def test_maps_against_numpy_f64(harness):
    rng = np.random.default_rng(5)
    for X in extrinsics():
        Ad = np.empty((6, 6))
        harness.rg_adjoint(_p(X), _p(Ad))
        assert np.abs(Ad - adjoint(X)).max() <= 1e-15
        for nrm in NORMALIZATIONS:
            nf = f32(nrm)
            A, Ai, B = np.empty((6, 6)), np.empty((6, 6)), np.empty((6, 6))
            harness.rg_normalization_map(_p(nf), _p(A))
            harness.rg_normalization_map_inverse(_p(nf), _p(Ai))
            harness.rg_body_map(_p(X), _p(nf), _p(B))
            A_ref = norm_map(nrm)
            assert np.abs(A - A_ref).max() <= 1e-15 * max(1.0, np.abs(A_ref).max())
            assert np.abs(A @ Ai - np.eye(6)).max() <= 1e-13 * np.abs(Ai).max()
            B_ref = np.linalg.inv(A_ref) @ adjoint(X)
            assert np.abs(B - B_ref).max() <= 1e-13 * np.abs(B_ref).max()
            J = rng.standard_normal((40, 6))
            H, G = f32(J.T @ J), f32(J.T @ rng.standard_normal(40))
            Hb, Gb = np.empty((6, 6)), np.empty(6)
            harness.rg_congruence(_p(B), _p(H), _p(G), _p(Hb), _p(Gb))
            H_ref, G_ref = B.T @ H.astype(np.float64) @ B, B.T @ G.astype(np.float64)
            assert np.abs(Hb - H_ref).max() <= 1e-13 * np.abs(H_ref).max()
            assert np.abs(Gb - G_ref).max() <= 1e-13 * np.abs(G_ref).max()
    # the identity normalisation gives the identity map: without normalisation B = Ad(X)
    X = extrinsics()[1]
    B = np.empty((6, 6))
    harness.rg_body_map(_p(X), _p(f32(NORMALIZATIONS[0])), _p(B))
    assert np.array_equal(B, adjoint(X))


def test_member_pose_is_the_f64_conjugation_narrowed_once(harness):
    T = f32(synth.twist_to_matrix([0.004, -0.003, 0.002, 0.02, -0.015, 0.03]))
    for X in extrinsics():
        Tp = np.empty((4, 4), np.float32)
        harness.rg_member_pose(_p(X), _p(T), _p(Tp))
        Xd = X.astype(np.float64)
        ref = Xd @ T.astype(np.float64) @ np.linalg.inv(Xd)
        # one f32 rounding of an f64 value (6e-8 relative), X^-1 taken as the rigid inverse of a rotation that is orthonormal to f32
        assert np.abs(Tp - ref).max() <= 2e-7 * max(1.0, np.abs(ref[:3, 3]).max())
        assert np.array_equal(Tp[3], [0, 0, 0, 1])
    I = np.eye(4, dtype=np.float32)
    Tp = np.empty((4, 4), np.float32)
    harness.rg_member_pose(_p(I), _p(T), _p(Tp))
    assert np.array_equal(Tp, T)          # a member at the body's origin runs at the body pose, bit for bit


def test_the_documented_maps_are_the_conjugations_of_the_exponential():
    """Independently of the code: X exp(zeta) X^-1 = exp(Ad(X) zeta) and N^-1 exp(xi) N = exp(A xi) with twists ordered (omega, v) — so that the
    member update T_p N^-1 exp(-xi) N equals X (T exp(-zeta)) X^-1 exactly when A xi = Ad(X) zeta, i.e. xi = A^-1 Ad(X) zeta."""
    rng = np.random.default_rng(11)
    for tw in EXTRINSIC_TWISTS:
        X = synth.twist_to_matrix(tw)
        for scale in (1e-6, 1e-2, 0.3):
            zeta = rng.standard_normal(6) * scale
            lhs = X @ synth.twist_to_matrix(zeta) @ np.linalg.inv(X)
            assert np.abs(lhs - synth.twist_to_matrix(adjoint(X) @ zeta)).max() <= 1e-12
            for nrm in NORMALIZATIONS:
                N = norm_matrix(nrm)
                xi = rng.standard_normal(6) * scale
                lhs = np.linalg.inv(N) @ synth.twist_to_matrix(xi) @ N
                rhs = synth.twist_to_matrix(norm_map(nrm) @ xi)
                assert np.abs(lhs - rhs).max() <= 1e-12 * max(1.0, np.abs(rhs).max())
                # the member's step for a body step zeta
                B = np.linalg.inv(norm_map(nrm)) @ adjoint(X)
                member = np.linalg.inv(N) @ synth.twist_to_matrix(-(B @ zeta)) @ N
                body = X @ synth.twist_to_matrix(-zeta) @ np.linalg.inv(X)
                assert np.abs(member - body).max() <= 1e-11 * max(1.0, np.abs(body).max())


def test_extrinsic_check(harness):
    for X in extrinsics():
        assert harness.rg_extrinsic_ok(_p(X)) == 1
    X = extrinsics()[1]
    for bad in ("nan", "inf", "row", "w", "scale", "shear"):
        Y = X.copy()
        if bad == "nan":
            Y[0, 3] = np.nan
        elif bad == "inf":
            Y[1, 1] = np.inf
        elif bad == "row":
            Y[3, 0] = 1e-3
        elif bad == "w":
            Y[3, 3] = 2.0
        elif bad == "scale":
            Y[:3, :3] *= 1.001
        else:
            Y[0, 1] += 1e-3
        assert harness.rg_extrinsic_ok(_p(f32(Y))) == 0, bad
    Y = X.copy()
    Y[:3, :3] *= np.float32(1.00001)          # R^T R - I = 2e-5: inside the bound
    assert harness.rg_extrinsic_ok(_p(f32(Y))) == 1


def test_pooled_fraction_of_good_points(harness):
    good = np.array([1200, 10, 801], np.uint32)
    n_points = np.array([400, 160, 912], np.int32)
    for Cn in (1, 8):
        got = harness.rg_fraction_good(_p(good), _p(n_points), 3, Cn)
        assert got == np.float32(int(good.sum())) / np.float32(int(n_points.sum()) * Cn)
        # a rig of one: the single path's fraction, bit for bit
        assert harness.rg_fraction_good(_p(good), _p(n_points), 1, Cn) == harness.rg_fraction_good_one(1200, 400, Cn)


def pose(angle=0.0, axis=(0.0, 0.0, 1.0), t=(0.0, 0.0, 0.0)):
    a = np.asarray(axis, np.float64)
    a = a / np.linalg.norm(a)
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(angle) * skew(a) + (1 - np.cos(angle)) * (skew(a) @ skew(a))
    T[:3, 3] = t
    return f32(T)


class Rig:
    def __init__(self, lib, X):
        self.lib, self.X, self.n = lib, f32(np.stack(X)), len(X)
        self.p = capi.Params()
        self.p.minTranslationMagToKeyFrame = 0.1
        self.p.minRotationMagToKeyFrame = 0.1
        self.p.maxFractionOfGoodPointsToKeyFrame = 0.6
        lib.rg_reset(self.n)

    def add(self, T_est, T_again=None, good=None, n_points=None, Cn=8):
        ret = capi.Result()
        out = np.full((self.n, 6), -7, np.int32)
        n_points = np.full(self.n, 100, np.int32) if n_points is None else np.asarray(n_points, np.int32)
        good = (n_points * Cn * 9 // 10).astype(np.uint32) if good is None else np.asarray(good, np.uint32)
        cloud = np.asarray(n_points, np.uint64)
        T_again = pose() if T_again is None else T_again
        self.lib.rg_add_frame(C.byref(self.p), L, self.n, None if self.X is None else _p(self.X), _p(f32(T_est)), _p(f32(T_again)), _p(good), _p(n_points), Cn, _p(cloud),
                              C.byref(ret), _p(out))
        return ret, out

    def state(self, member):
        T_kf, cp, back = (np.zeros((4, 4), np.float32) for _ in range(3))
        n = C.c_size_t()
        length = self.lib.rg_state(member, _p(T_kf), _p(cp), _p(back), C.byref(n))
        return dict(T_kf=T_kf, cloud_pose=cp, back=back, cloud_n=n.value, length=length)


def test_one_decision_moves_every_member_alike_and_clouds_sit_at_W_kf_X_inverse(harness):
    X = extrinsics()
    rig = Rig(harness, X)
    ret, out = rig.add(pose())
    assert ret.isKeyFrame and ret.keyFramingReason == capi.KF_FIRST_FRAME
    assert out.tolist() == [[3 * p + 1, 3 * p, 3 * p + 2, 3 * p + 1, -1, 0] for p in range(3)]      # every member: the frame just read is its key frame
    assert rig.state(-1)["length"] == 1 and all(rig.state(p)["length"] == 1 for p in range(3))

    # a small motion, plenty of good points: no key frame; every member advances its slots, the body keeps T_kf
    T1 = pose(0.01, t=(0.01, 0.0, 0.02))
    ret, out = rig.add(T1)
    assert not ret.isKeyFrame and ret.keyFramingReason == capi.KF_NO_KEYFRAMING
    assert out.tolist() == [[3 * p + 1, 3 * p + 2, 3 * p, -1, -1, 0] for p in range(3)]
    assert np.array_equal(rig.state(-1)["T_kf"], T1.reshape(4, 4))
    for p in range(3):
        Tp = np.empty((4, 4), np.float32)
        harness.rg_member_pose(_p(X[p]), _p(T1), _p(Tp))
        assert np.array_equal(rig.state(p)["T_kf"], Tp)          # the member's own pose against its key frame: X_p T X_p^-1

    # ONE member short of good points does not decide: the pooled fraction does (0.9, 0.9, 0.1 of equal sizes -> 0.63 > 0.6)
    n_points = np.array([100, 100, 100], np.int32)
    ret, out = rig.add(T1, good=[720, 720, 80], n_points=n_points)
    assert not ret.isKeyFrame
    # ... and below the bound (0.9, 0.8, 0.05 -> 0.583) the rig key-frames: every member takes the same transition, with a previous frame
    T2 = pose(0.012, t=(0.012, 0.0, 0.025))
    T_again = pose(0.002, t=(0.002, 0.0, 0.005))
    ret, out = rig.add(T2, T_again=T_again, good=[720, 640, 40], n_points=n_points)
    assert ret.isKeyFrame and ret.keyFramingReason == capi.KF_SMALL_FRAC_GOOD and ret.hasPointCloud
    assert (out[:, 5] == 1).all() and (out[:, 3] == out[:, 0]).all() and (out[:, 4] == out[:, 2]).all()
    assert [o[0] - 3 * p for p, o in enumerate(out)] == [out[0][0]] * 3          # the same slot roles in every member
    body = rig.state(-1)
    assert np.array_equal(body["T_kf"], T_again.reshape(4, 4)) and np.array_equal(np.array(ret.pose, np.float32).reshape(4, 4), T_again.reshape(4, 4))
    assert body["length"] == 4 and np.array_equal(body["cloud_pose"], body["back"]) and body["cloud_n"] == 0
    for p in range(3):
        m = rig.state(p)
        assert m["cloud_n"] == 100 and m["length"] == 4
        want = body["cloud_pose"].astype(np.float64) @ np.linalg.inv(X[p].astype(np.float64))
        assert np.abs(m["cloud_pose"] - want).max() <= 2e-7 * max(1.0, np.abs(want).max())

    # a large translation of the BODY key-frames whatever the fractions; the key frame before cleared every member's previous frame, so this
    # frame itself becomes the key frame of every member (bpvo/vo.cc:161-173) and nothing is estimated again
    ret, out = rig.add(pose(0.0, t=(0.2, 0.0, 0.0)), T_again=pose(0.0, t=(0.05, 0, 0)))
    assert ret.isKeyFrame and ret.keyFramingReason == capi.KF_LARGE_TRANSLATION
    assert (out[:, 5] == 0).all() and (out[:, 4] == -1).all() and (out[:, 3] == out[:, 0]).all()
    assert np.array_equal(rig.state(-1)["T_kf"], np.eye(4, dtype=np.float32))


def test_a_rig_of_one_at_the_origin_is_the_single_state_machine(harness):
    rig = Rig(harness, [np.eye(4)])
    seq = [(pose(), None), (pose(0.01, t=(0.01, 0, 0.02)), None), (pose(0.0, t=(0.3, 0, 0)), pose(0.0, t=(0.1, 0, 0))), (pose(0.02), None)]
    for T, Ta in seq:
        rig.add(T, T_again=Ta)
        b, m = rig.state(-1), rig.state(0)
        for k in ("T_kf", "back", "length", "cloud_pose"):
            assert np.array_equal(b[k], m[k]), k


def test_null_extrinsics_are_the_plain_calls_on_one_state(harness):
    """What the batched driver does to a sequence — the transitions of a body with null extrinsics, the body its own member — against the plain
    vo_* calls in add_frame_impl's order, over every branch: first frame, no key frame, key frame with re-estimation (the previous slot holds
    data), key frame without (that key frame cleared it), and the decision left to the fraction of good points.  After every frame the whole
    SeqState (roles, T_kf, trajectory, cloud_n, cloud_pose) and the whole bpvo_hip_result are byte-identical."""
    rig = Rig(harness, [np.eye(4)])
    rig.X = None
    small, far = pose(0.01, t=(0.01, 0, 0.02)), pose(0.0, t=(0.3, 0, 0))
    Ta = pose(0.002, t=(0.002, 0.0, 0.005))
    # (T_est, T_again, good, n_points, C)
    series = [(pose(), Ta, 720, 100, 8), (small, Ta, 720, 100, 8), (far, Ta, 720, 100, 8), (far, Ta, 720, 100, 8), (small, Ta, 90, 100, 1),
              (pose(0.02), Ta, 400, 100, 8), (pose(0.3), Ta, 0, 7, 1)]
    branches = []
    for T, T2, good, n_points, Cn in series:
        ret, out = rig.add(T, T_again=T2, good=[good], n_points=[n_points], Cn=Cn)
        want, wout = capi.Result(), np.full(6, -7, np.int32)
        harness.rg_plain_add_frame(C.byref(rig.p), L, _p(f32(T)), _p(f32(T2)), good, n_points, Cn, n_points, C.byref(want), _p(wout))
        assert bytes(ret) == bytes(want), (len(branches), "result")
        assert out[0].tolist() == wout.tolist(), (len(branches), out, wout)
        a, b = np.zeros(4096, np.uint8), np.zeros(4096, np.uint8)
        na, nb = harness.rg_state_bytes(0, _p(a), a.size), harness.rg_state_bytes(1, _p(b), b.size)
        assert na == nb > 0 and a[:na].tobytes() == b[:nb].tobytes(), (len(branches), "SeqState")
        branches.append("first" if ret.keyFramingReason == capi.KF_FIRST_FRAME else "none" if not ret.isKeyFrame else "again" if out[0][5] else "swap")
        assert bool(ret.hasPointCloud) == (branches[-1] in ("again", "swap"))
    assert branches == ["first", "none", "again", "swap", "none", "again", "swap"], branches
    # the fraction of good points: the single form's float for every count an unsigned holds
    for good in (0, 1, 3, 2**24 - 1, 2**24 + 1, 2**31 - 1, 2**31, 2**31 + 129, 2**32 - 2, 2**32 - 1):
        for n_points, Cn in ((1, 1), (100, 8), (2**29, 8), (2**31 - 1, 1), (2**31 - 1, 8)):
            a = np.float32(harness.rg_fraction_good_null(good, n_points, Cn))
            b = np.float32(harness.rg_fraction_good_one(good, n_points, Cn))
            assert a.tobytes() == b.tobytes(), (good, n_points, Cn, a, b)


def test_rig_visual_odometry_compiles_as_cpp11():
    src = os.path.join(ROOT, "tests", "cpp", "rig_compile.cc")
    out = subprocess.run(["g++", "-std=c++11", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"), src], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr


def test_make_rig_sequence_renders_member_p_from_its_extrinsic_times_the_body_pose():
    X = extrinsics()
    seq = synth.make_rig_sequence(48, 64, 3, [x.astype(np.float64) for x in X], index=3)
    alone = synth.make_sequence(48, 64, 3, index=3)
    assert len(seq["frames"]) == 3 and all(len(f) == 3 for f in seq["frames"])
    for k in range(3):
        assert np.array_equal(seq["poses"][k], alone["poses"][k])                       # the body follows make_sequence's trajectory
        assert np.array_equal(seq["frames"][k][0][0], alone["frames"][k][0])            # the member at the body's origin sees make_sequence's frames
        assert np.array_equal(seq["frames"][k][0][1], alone["frames"][k][1])
        img, disp = synth._render(seq["K"][1], seq["b"][1], 48, 64, X[1].astype(np.float64) @ seq["poses"][k], 1003, 10.0, (0.1, -0.15))
        assert np.array_equal(seq["frames"][k][1][0], img) and np.array_equal(seq["frames"][k][1][1], disp)
