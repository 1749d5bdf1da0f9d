"""The pose covariance without a GPU: the f64 finish of bpvo_amd/csrc/pose_cov_math.h (LDL^T, the sandwich M^-1 Q M^-1, the maps to the body
twist, the pivot <= 0 rule, exact symmetry) compiled by the host's C++ compiler and compared with numpy (tests/cpp/pose_cov_harness.cc, which
also runs stand-alone under the address and undefined-behaviour sanitizers), the C++ facade's surface, the Python mirror of the ABI, and the
calibration of the definition itself on the CPU oracle: 150 noisy copies of a frame, the spread of the estimated pose against the covariance the
definition reports (tests/pose_covariance_ref.py)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import pose_covariance_ref as ref
from bpvo_amd import capi, synth
from util import make_params

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bpvo_amd", "csrc")
HARNESS = os.path.join(ROOT, "tests", "cpp", "pose_cov_harness.cc")
EXTRINSIC_TWISTS = ((0, 0, 0, 0, 0, 0), (0, 0.14, 0.02, 0.3, 0.02, 0.1), (0.03, -0.2, 0, -0.4, 0, 0.05))
NORMALIZATIONS = ((1.0, 0.0, 0.0, 0.0), (0.37, 0.2, -0.1, 9.5), (12.5, -1.5, 0.75, 3.0))


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("posecov") / "libposecov.so")
    cmd = [os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-I", CSRC, "-o", out, HARNESS]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return C.CDLL(out)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def f32(a):
    return np.ascontiguousarray(a, np.float32)


def spd_pair(rng, n=60):
    J = rng.standard_normal((n, 6)) * np.array([3.0, 2.0, 1.0, 0.5, 0.2, 0.1])      # a condition number in the thousands, like a camera's curvature
    g = J * rng.standard_normal((n, 1))
    return J.T @ J, g.T @ g


def norm_map(nrm):
    s, c = float(np.float32(nrm[0])), np.asarray(f32(nrm[1:]), np.float64)
    A = np.eye(6)
    A[3:, :3] = ref.skew(c)
    A[3:, 3:] = np.eye(3) / s
    return A


def test_ldlt_and_sandwich_against_numpy(harness):
    rng = np.random.default_rng(11)
    for _ in range(20):
        M, Q = spd_pair(rng)
        L, D, S = np.empty((6, 6)), np.empty(6), np.empty((6, 6))
        assert harness.pc_ldlt(_p(M), _p(L), _p(D)) == 1
        assert np.array_equal(np.triu(L, 1), np.zeros((6, 6))) and np.array_equal(np.diag(L), np.ones(6)) and np.all(D > 0)
        assert np.abs(L @ np.diag(D) @ L.T - M).max() <= 1e-13 * np.abs(M).max()
        b, x = rng.standard_normal(6), np.empty(6)
        harness.pc_ldlt_solve(_p(L), _p(D), _p(b), _p(x))
        x_ref = np.linalg.solve(M, b)
        assert np.abs(x - x_ref).max() <= 1e-10 * np.abs(x_ref).max()
        assert harness.pc_sandwich(_p(M), _p(Q), _p(S)) == ref.COV_OK
        S_ref = ref.sandwich(M, Q)
        assert np.abs(S - S_ref).max() <= 1e-10 * np.abs(S_ref).max()
        assert np.array_equal(S, S.T)                               # the upper triangle mirrored: exactly symmetric
        assert np.linalg.eigvalsh(S).min() > 0


def test_a_pivot_that_is_not_positive_is_indefinite(harness):
    rng = np.random.default_rng(12)
    M, Q = spd_pair(rng)
    S = np.full((6, 6), 7.0)
    for k in range(6):      # one negative direction, met at pivot k or later
        v = np.zeros(6)
        v[k] = 1.0
        Mi = M - 2.0 * M[k, k] * np.outer(v, v)
        assert np.linalg.eigvalsh(Mi).min() < 0
        assert harness.pc_sandwich(_p(Mi), _p(Q), _p(S)) == ref.COV_INDEFINITE
        assert np.all(S == 7.0)                                     # untouched
    Z = np.zeros((6, 6))
    assert harness.pc_sandwich(_p(Z), _p(Q), _p(S)) == ref.COV_INDEFINITE      # a pivot of exactly zero
    # positive semi-definite of rank 5: the last pivot is zero or rounding noise on either side of it — never OK with a finite result of any meaning;
    # a well-conditioned positive definite matrix next to it is OK
    assert harness.pc_sandwich(_p(M), _p(Q), _p(S)) == ref.COV_OK


def test_body_map_and_finish_against_numpy(harness):
    rng = np.random.default_rng(13)
    Xs = [f32(synth.twist_to_matrix(t)) for t in EXTRINSIC_TWISTS]
    for n in (1, 2, 3):
        Ms, Qs = zip(*(spd_pair(rng) for _ in range(n)))
        X = f32(np.stack(Xs[:n])).reshape(n, 16)
        nrm = f32(NORMALIZATIONS[:n])
        Mb, Qb, cov = np.empty((6, 6)), np.empty((6, 6)), np.empty((6, 6), np.float32)
        Mp, Qp = np.ascontiguousarray(np.stack(Ms)), np.ascontiguousarray(np.stack(Qs))
        st = harness.pc_body(n, _p(Mp), _p(Qp), _p(X), _p(nrm), 1, C.c_double(100.0), _p(Mb), _p(Qb), _p(cov))
        assert st == ref.COV_OK
        S_ref, Mb_ref, Qb_ref = ref.body_covariance([(Ms[p], Qs[p], norm_map(NORMALIZATIONS[p]), Xs[p].astype(np.float64)) for p in range(n)])
        assert np.abs(Mb - Mb_ref).max() <= 1e-12 * np.abs(Mb_ref).max() and np.abs(Qb - Qb_ref).max() <= 1e-12 * np.abs(Qb_ref).max()
        assert np.array_equal(Mb, Mb.T) and np.array_equal(Qb, Qb.T) and np.array_equal(cov, cov.T)
        sd = np.sqrt(np.diag(S_ref))
        assert np.abs(cov - S_ref).max() <= 1e-6 * np.outer(sd, sd).max() and np.all(np.abs(cov - S_ref) <= 1e-6 * np.outer(sd, sd))
    # one camera at the body's origin: Sigma = A Sigma_xi A^T
    M, Q = spd_pair(rng)
    nrm = f32(NORMALIZATIONS[1:2])
    I = f32(np.eye(4)).reshape(1, 16)
    Mb, Qb, cov = np.empty((6, 6)), np.empty((6, 6)), np.empty((6, 6), np.float32)
    assert harness.pc_body(1, _p(M), _p(Q), _p(I), _p(nrm), 1, C.c_double(6.0), _p(Mb), _p(Qb), _p(cov)) == ref.COV_OK
    A = norm_map(NORMALIZATIONS[1])
    S_ref = A @ ref.sandwich(M, Q) @ A.T
    sd = np.sqrt(np.diag(S_ref))
    assert np.all(np.abs(cov - S_ref) <= 1e-6 * np.outer(sd, sd))
    # the statuses that leave the Identity
    eye = np.eye(6, dtype=np.float32)
    for estimated, valid, Mx, want in ((1, 5.0, M, ref.COV_DEGENERATE), (0, 100.0, M, ref.COV_NONE), (1, 100.0, -M, ref.COV_INDEFINITE),
                                       (1, 100.0, M * np.nan, ref.COV_DEGENERATE), (1, 100.0, M * np.inf, ref.COV_DEGENERATE)):
        Mx = np.ascontiguousarray(Mx)
        assert harness.pc_body(1, _p(Mx), _p(Q), _p(I), _p(nrm), estimated, C.c_double(valid), _p(Mb), _p(Qb), _p(cov)) == want
        assert np.array_equal(cov, eye)


def test_harness_runs_clean_under_the_sanitizers(tmp_path):
    """The same harness as a stand-alone program with -fsanitize=address,undefined: every function of pose_cov_math.h once, no report."""
    exe = str(tmp_path / "pose_cov_harness")
    cmd = [os.environ.get("CXX", "g++"), "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-DPOSE_COV_HARNESS_MAIN", "-I", CSRC, "-o", exe, HARNESS]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "pose_cov_harness: ok" in out.stdout and not out.stderr, (out.stdout, out.stderr)


def test_facade_surface_compiles():
    src = os.path.join(ROOT, "tests", "cpp", "pose_cov_compile.cc")
    out = subprocess.run(["g++", "-std=c++11", "-fsyntax-only", "-Wall", "-I", os.path.join(ROOT, "include"), src], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr


def test_abi_mirror_and_exported_symbols(tmp_path):
    """capi.PoseCovariance against the header's struct as the C compiler lays it out; every entry point of the feature exported by the library."""
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include <bpvo_hip/c_api.h>\nint main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %d %d %d %d %d\\n", '
                   "sizeof(bpvo_hip_pose_covariance), offsetof(bpvo_hip_pose_covariance, T), offsetof(bpvo_hip_pose_covariance, covariance), "
                   "offsetof(bpvo_hip_pose_covariance, sigma), offsetof(bpvo_hip_pose_covariance, num_valid), offsetof(bpvo_hip_pose_covariance, level), "
                   "offsetof(bpvo_hip_pose_covariance, status), BPVO_COV_OK, BPVO_COV_INDEFINITE, BPVO_COV_DEGENERATE, BPVO_COV_NONE, BPVO_HIP_COV_GROUP); return 0; }\n")
    exe = str(tmp_path / "layout")
    r = subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), str(src), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = [int(v) for v in subprocess.run([exe], capture_output=True, text=True).stdout.split()]
    P = capi.PoseCovariance
    assert got == [C.sizeof(P), P.T.offset, P.covariance.offset, P.sigma.offset, P.num_valid.offset, P.level.offset, P.status.offset,
                   capi.COV_OK, capi.COV_INDEFINITE, capi.COV_DEGENERATE, capi.COV_NONE, capi.COV_GROUP]
    assert C.sizeof(P) == 224
    import bpvo_amd
    out = subprocess.run(["nm", "-D", "--defined-only", bpvo_amd.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (bpvo_hip_[a-z_]+)", out))
    for name in ("pose_covariances", "pose_covariance_rig", "vo_pose_covariance", "seq_pose_covariance", "rig_pose_covariance", "debug_pose_covariance_sums"):
        assert "bpvo_hip_" + name in exported, name


def test_reference_weights_are_the_oracles(orc):
    """The float32 weights of the numpy reference are MEstimator::ComputeWeights' (the oracle's restatement), bit for bit, and d is 1 exactly where
    Huber's weight is 1."""
    rng = np.random.default_rng(3)
    r = f32(np.concatenate([rng.normal(0, 4, 4000), [0.0, 1.345 * 1.7, -1.345 * 1.7, 4.685 * 1.7, 100.0, -100.0]]))
    valid = np.ones(r.size, np.uint16)
    for loss in (capi.LOSS_HUBER, capi.LOSS_TUKEY, capi.LOSS_L2):
        w, d = ref.weights_f32(r, 1.7, loss)
        w_orc = np.empty_like(r)
        orc.fn("compute_weights")(loss, _p(r), _p(valid), C.c_size_t(r.size), C.c_float(1.7), _p(w_orc))
        assert np.array_equal(w.view(np.uint32), w_orc.view(np.uint32)), loss
        if loss == capi.LOSS_HUBER:
            assert np.array_equal(d == 1.0, w == 1.0)
        if loss == capi.LOSS_TUKEY:
            assert np.all(d[np.abs(r) >= 4.685 * 1.7 * 1.0001] == 0) and d[r == 0][0] == 1.0 and d.min() < 0      # psi' is negative beyond 4.685 / sqrt(5)


def test_calibration_on_the_oracle(orc):
    """Monte-Carlo on the CPU oracle, intensity / Huber, 96x128, 2 levels: 150 draws of N(0, 3) grey-level noise on frame B (rounded, clipped to u8,
    np.random.default_rng(0)).  The per-axis ratio of the empirical standard deviation of the estimated pose to the mean reported one must lie in
    [0.85, 1.35]: 1.07 - 1.11 measured when the form was chosen, +- three sampling standard deviations of such a ratio from 150 draws
    (1 / sqrt(2 * 149) = 5.8 % each), rounded outwards."""
    rows, cols = 96, 128
    d = synth.make_pair(rows, cols, 0)
    p = make_params(orc, descriptor="intensity", loss="huber", levels=2)
    ctx = orc.create(d["K"], d["b"], rows, cols, p, device=0, n_frames=2, n_pairs=1)
    ctx.frame_set_data(0, d["imgA"], d["dispA"])
    ctx.frame_set_template(0)

    def cov_of(c, T):
        e = ref.oracle_covariance(c, T, capi.LOSS_HUBER)
        return e["covariance"], e["status"]
    ratio, bad = ref.calibration_ratio(ctx, d, cov_of, draws=150)
    ctx.close()
    print("empirical / reported standard deviation per axis:", np.round(ratio, 3), "draws without a covariance:", bad)
    assert bad == 0
    assert np.all(ratio >= 0.85) and np.all(ratio <= 1.35), ratio
