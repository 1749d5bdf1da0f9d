"""bpvo_amd/csrc/warp_rule.h without a GPU: the one statement of "where does a template point land and is it valid there" that every
Gauss-Newton kernel path calls, compiled by the host's C++ compiler (tests/cpp/warp_rule_harness.cc includes only that header) and held to
the numpy restatements of tests/hostile_poses.py at every hostile pose, on ALL points of a synthetic template, none excluded.

The f64 rule with the borders (0, 1) and (1, 3): the verdict on every point; xi, yi and the bit patterns of the fractions xf, yf on the valid
ones.  The f32 rule, plain and in disparity space: the verdict on every point; xi, yi and the bit patterns of the four coefficients on the
valid ones.  Every case must have its named property (check_property), so that no input set passes that never leaves the image."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import hostile_poses as hp
from util import setup_pair

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DESCRIPTORS = ["intensity", "bitplanes"]
_bundles = {}


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("warp_rule") / "libwarp_rule.so")
    cmd = [os.environ.get("CXX", "g++"), "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared",
           "-I", os.path.join(ROOT, "bpvo_amd", "csrc"), "-o", out, os.path.join(ROOT, "tests", "cpp", "warp_rule_harness.cc")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lib = C.CDLL(out)
    f64_args = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 5
    lib.wr_foot_0_1.argtypes = f64_args
    lib.wr_foot_1_3.argtypes = f64_args
    lib.wr_foot_f32.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float, C.c_int, C.c_int] + [C.c_void_p] * 4
    for f in (lib.wr_foot_0_1, lib.wr_foot_1_3, lib.wr_foot_f32):
        f.restype = None
    return lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def bundle(orc, size, descriptor):
    """A synthetic template's level-0 points as RigidBodyWarp keeps them and as DisparitySpaceWarp does, and the poses built from the former."""
    key = (size, descriptor)
    if key not in _bundles:
        rows, cols, levels = hp.SIZES[size]
        ctx, d, _ = setup_pair(orc, rows, cols, descriptor=descriptor, levels=levels)
        X = np.ascontiguousarray(ctx.get_points(0, 0), np.float32)
        ctx.set_warp_formulation(2)
        ctx.frame_set_template(0)
        Xd = np.ascontiguousarray(ctx.get_points(0, 0), np.float32)
        ctx.close()
        assert X.shape == Xd.shape and X.shape[1] == 4 and len(X) > 100
        _bundles[key] = dict(K=np.asarray(d["K"], np.float32), b=d["b"], X=X, Xd=Xd, rows=rows, cols=cols, poses=hp.poses(d["K"], X, rows, cols))
    return _bundles[key]


def same_bits(a, b):
    """Equal bit patterns, a NaN equal to a NaN."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape
    u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return bool(np.all((a.view(u) == b.view(u)) | (np.isnan(a) & np.isnan(b))))


@pytest.mark.parametrize("size", hp.SIZES)
@pytest.mark.parametrize("descriptor", DESCRIPTORS)
def test_f64_rule_against_numpy(orc, harness, descriptor, size):
    b = bundle(orc, size, descriptor)
    K, X, rows, cols = b["K"], b["X"], b["rows"], b["cols"]
    n = len(X)
    differ = 0
    for name, T in b["poses"].items():
        print(size, descriptor, hp.check_property(name, K, T, X, rows, cols))
        P = np.ascontiguousarray(hp.projection_matrix(K, T), np.float32)
        x, y = hp.np_project(K, T, X)
        xi_ref, yi_ref = hp.np_floor(x)[0], hp.np_floor(y)[0]
        with np.errstate(invalid="ignore"):
            xf_ref, yf_ref = x - xi_ref, y - yi_ref
        for (lo, hi), fn in (((0, 1), harness.wr_foot_0_1), ((1, 3), harness.wr_foot_1_3)):
            xi, yi, v = np.full(n, -7, np.int32), np.full(n, -7, np.int32), np.full(n, 7, np.uint8)
            xf, yf = np.full(n, -7.0), np.full(n, -7.0)
            fn(_p(P), _p(X), n, cols, rows, _p(xi), _p(yi), _p(v), _p(xf), _p(yf))
            ref = hp.np_valid(x, y, rows, cols, lo, hi)
            assert np.array_equal(v, ref.astype(np.uint8)), (name, lo, hi, int(v.sum()), int(ref.sum()), np.flatnonzero(v != ref)[:8])
            assert np.array_equal(xi[ref], xi_ref[ref]) and np.array_equal(yi[ref], yi_ref[ref]), (name, lo, hi)
            assert same_bits(xf[ref], xf_ref[ref]) and same_bits(yf[ref], yf_ref[ref]), (name, lo, hi)
            if (lo, hi) == (1, 3):
                differ += int(np.sum(ref != hp.np_valid(x, y, rows, cols)))
        if name in hp.NON_FINITE:
            assert not v.any()
    assert differ > 0      # the (1, 3) borders decide some points differently from (0, 1)


@pytest.mark.parametrize("size", hp.SIZES)
@pytest.mark.parametrize("descriptor", DESCRIPTORS)
@pytest.mark.parametrize("dspace", [False, True], ids=["plain", "dspace"])
def test_f32_rule_against_numpy(orc, harness, dspace, descriptor, size):
    b = bundle(orc, size, descriptor)
    K, rows, cols = b["K"], b["rows"], b["cols"]
    X = b["Xd"] if dspace else b["X"]
    n = len(X)
    k = hp.chosen_point(X)
    one = np.float32(1.0)
    for name, T in b["poses"].items():
        hp.check_property(name, K, T, b["X"], rows, cols)
        P = np.ascontiguousarray(hp.dspace_matrix(K, b["b"], T) if dspace else hp.projection_matrix(K, T), np.float32)
        x, y = hp.np_project_f32(K, T, X, b=b["b"] if dspace else None)
        ref = hp.np_valid_f32(x, y, rows, cols)
        xi_ref, yi_ref = hp.np_trunc_f32(x)[0], hp.np_trunc_f32(y)[0]
        with np.errstate(all="ignore"):
            fx, fy = x - xi_ref.astype(np.float32), y - yi_ref.astype(np.float32)
            xfyf = fx * fy
            cf_ref = np.stack([xfyf - fy - fx + one, fx - xfyf, fy - xfyf, xfyf], axis=1)
        assert cf_ref.dtype == np.float32
        xi, yi, v = np.full(n, -7, np.int32), np.full(n, -7, np.int32), np.full(n, 7, np.uint8)
        cf = np.full((n, 4), -7, np.float32)
        harness.wr_foot_f32(_p(P), _p(X), n, int(dspace), float(K[0, 2]), float(K[1, 2]), cols, rows, _p(xi), _p(yi), _p(v), _p(cf))
        assert np.array_equal(v, ref.astype(np.uint8)), (name, int(v.sum()), int(ref.sum()), np.flatnonzero(v != ref)[:8])
        assert np.array_equal(xi[ref], xi_ref[ref]) and np.array_equal(yi[ref], yi_ref[ref]), name
        assert same_bits(cf[ref], cf_ref[ref]), name
        # truncation: the chosen point of the two (-1, 0) cases is pixel 0 with a negative fraction, and valid
        if name == "x_in_minus_one_zero":
            assert -1 < x[k] < 0 and v[k] and xi[k] == 0
        if name == "y_in_minus_one_zero":
            assert -1 < y[k] < 0 and v[k] and yi[k] == 0
        if name in hp.NON_FINITE:
            assert not v.any()
