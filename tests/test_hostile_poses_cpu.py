"""The oracle's warp verdict against plain numpy at the hostile poses of tests/hostile_poses.py: points behind the camera, at zero depth,
on integer coordinates, in (-1, 0), on the image's last column, and NaN / Inf / beyond the int range.

Every comparison is on ALL points — none near an integer coordinate is left out: the numpy projection sums in the reference's order.  The
GPU side of the same cases is tests/test_gpu_hostile_poses.py."""
import numpy as np
import pytest

import hostile_poses as hp
from bpvo_amd import capi
from util import bits_equal, setup_pair

DESCRIPTORS = ["intensity", "bitplanes"]
INTERPS = {"cosine": capi.INTERP_COSINE, "cubic": capi.INTERP_CUBIC, "cubic_hermite": capi.INTERP_CUBIC_HERMITE}
_bundles = {}


def bundle(orc, size, descriptor, **kw):
    """One oracle context per (size, descriptor, parameters), its level-0 points and the poses built from them."""
    key = (size, descriptor, tuple(sorted(kw.items())))
    if key not in _bundles:
        rows, cols, levels = hp.SIZES[size]
        ctx, d, _ = setup_pair(orc, rows, cols, descriptor=descriptor, levels=levels, **kw)
        X = ctx.get_points(0, 0)
        _bundles[key] = dict(ctx=ctx, d=d, X=X, rows=rows, cols=cols, poses=hp.poses(d["K"], X, rows, cols))
    return _bundles[key]


@pytest.mark.parametrize("size", hp.SIZES)
@pytest.mark.parametrize("descriptor", DESCRIPTORS)
@pytest.mark.parametrize("name", hp.CASES)
def test_case_has_its_property(orc, name, descriptor, size):
    b = bundle(orc, size, descriptor)
    print(size, descriptor, hp.check_property(name, b["d"]["K"], b["poses"][name], b["X"], b["rows"], b["cols"]))


@pytest.mark.parametrize("size", hp.SIZES)
@pytest.mark.parametrize("descriptor", DESCRIPTORS)
@pytest.mark.parametrize("name", hp.CASES)
def test_mask_and_residuals_against_numpy(orc, name, descriptor, size):
    """Formulation 0, linear: get_valid is np_valid on every point; the residuals are the numpy bilinear evaluation (the form of
    test_linear_interpolation_against_numpy) bit for bit on the valid points and 0.0 elsewhere, every channel (C = 1 and C = 8).  Where no
    coordinate is inside the int range: sigma 1, f_norm 0, H finite (nothing valid, nothing summed)."""
    b = bundle(orc, size, descriptor)
    ctx, K, X, rows, cols = b["ctx"], b["d"]["K"], b["X"], b["rows"], b["cols"]
    T = b["poses"][name]
    a = ctx.linearize(0, 0, 1, 0, T, reset_scale=True)
    n, C = len(X), ctx.Cn
    v = ctx.get_valid(0).astype(bool)
    assert v.shape == (n,)
    x, y = hp.np_project(K, T, X)
    ref = hp.np_valid(x, y, rows, cols)
    assert np.array_equal(v, ref), (name, int(v.sum()), int(ref.sum()), np.flatnonzero(v != ref)[:8])
    assert a["num_valid"] == int(ref.sum())
    r = ctx.get_residuals(0).reshape(C, n)
    xi, yi = hp.np_floor(x)[0][ref], hp.np_floor(y)[0][ref]
    xf, yf = x[ref] - xi, y[ref] - yi
    wx = 1.0 - xf
    I0 = ctx.get_pixels(0, 0)
    for c in range(C):
        I1 = ctx.get_descriptor_channel(1, 0, c).astype(np.float64)
        Iw = (1.0 - yf) * (I1[yi, xi] * wx + I1[yi, xi + 1] * xf) + yf * (I1[yi + 1, xi] * wx + I1[yi + 1, xi + 1] * xf)
        assert bits_equal((Iw - I0[c][ref].astype(np.float64)).astype(np.float32), r[c][ref]), (name, c)
        assert np.all(r[c][~ref] == 0.0), (name, c)
    if name in hp.NON_FINITE:
        assert a["num_valid"] == 0 and a["sigma"] == 1.0 and a["f_norm"] == 0.0 and np.all(np.isfinite(a["H"])) and np.all(np.isfinite(a["G"]))


@pytest.mark.parametrize("size", hp.SIZES)
@pytest.mark.parametrize("descriptor", DESCRIPTORS)
@pytest.mark.parametrize("interp", INTERPS)
def test_interpolation_borders(orc, interp, descriptor, size):
    """Cosine keeps the (0, 1) borders, cubic and Hermite take (1, 3) (photo_error.cc:347-348): the mask is that rule at every case, and an
    invalid point's residual is 0."""
    b = bundle(orc, size, descriptor, interp=INTERPS[interp])
    ctx, K, X, rows, cols = b["ctx"], b["d"]["K"], b["X"], b["rows"], b["cols"]
    lo, hi = (0, 1) if interp == "cosine" else (1, 3)
    differ = 0
    for name, T in b["poses"].items():
        a = ctx.linearize(0, 0, 1, 0, T, reset_scale=True)
        v = ctx.get_valid(0).astype(bool)
        x, y = hp.np_project(K, T, X)
        ref = hp.np_valid(x, y, rows, cols, lo, hi)
        assert np.array_equal(v, ref), (name, int(v.sum()), int(ref.sum()), np.flatnonzero(v != ref)[:8])
        assert a["num_valid"] == int(ref.sum())
        assert np.all(ctx.get_residuals(0).reshape(ctx.Cn, -1)[:, ~ref] == 0.0), name
        differ += int(np.sum(ref != hp.np_valid(x, y, rows, cols)))
    assert (differ > 0) == (interp != "cosine")      # the (1, 3) borders decide some points differently from (0, 1)


@pytest.mark.parametrize("size", hp.SIZES)
@pytest.mark.parametrize("descriptor", DESCRIPTORS)
@pytest.mark.parametrize("formulation", [1, 2])
def test_f32_formulations_against_numpy(orc, formulation, descriptor, size):
    """projectPoints (formulation 1) and DisparitySpaceWarp (2) against the f32 restatement in numpy: sequential f32 sums, w = 1 / u_z,
    truncation, the int-range test, + (cx, cy) in disparity space — masks equal on every point of every case, and the chosen point of the
    two (-1, 0) cases is valid although the f64 rule rejects it.  An invalid point's residual is -I0 (operator() returns 0 there)."""
    b0 = bundle(orc, size, descriptor)
    rows, cols, levels = hp.SIZES[size]
    ctx, d, _ = setup_pair(orc, rows, cols, descriptor=descriptor, levels=levels)
    ctx.set_warp_formulation(formulation)
    ctx.frame_set_template(0)
    K, X = d["K"], ctx.get_points(0, 0)
    assert len(X) == len(b0["X"])
    k = hp.chosen_point(X)
    pix = ctx.get_pixels(0, 0)
    for name, T in b0["poses"].items():
        a = ctx.linearize(0, 0, 1, 0, T, reset_scale=True)
        v = ctx.get_valid(0).astype(bool)
        xf, yf = hp.np_project_f32(K, T, X, b=d["b"] if formulation == 2 else None)
        ref = hp.np_valid_f32(xf, yf, rows, cols)
        assert np.array_equal(v, ref), (name, int(v.sum()), int(ref.sum()), np.flatnonzero(v != ref)[:8], xf[v != ref][:8], yf[v != ref][:8])
        assert a["num_valid"] == int(ref.sum())
        r = ctx.get_residuals(0).reshape(ctx.Cn, -1)
        assert np.array_equal(r[:, ~ref], -pix[:, ~ref]), name
        if name == "x_in_minus_one_zero":
            assert -1 < xf[k] < 0 and v[k], (xf[k], yf[k])
        if name == "y_in_minus_one_zero":
            assert -1 < yf[k] < 0 and v[k], (xf[k], yf[k])
        if name in hp.NON_FINITE:
            assert not v.any()
    ctx.close()
