"""The motion-stereo rule (c_api.h "motion stereo") as numpy: the statement the C++ header bpvo_amd/csrc/motion_stereo_math.h and the kernel are
compared with, bit for bit.  It follows the header operation by operation: the epipolar curve and the hypotheses in f64 in the header's order, the
sums in int64 (exact), the measurement in f64 rounded once to f32 each, the update in f32 (numpy's f32 + - * / sqrt are single correctly rounded
operations and never contracted).  Also the inputs the CPU and the GPU tests share."""
import numpy as np

import disparity_fusion_ref as fref

F32, F64, U32, U64, I64 = np.float32, np.float64, np.uint32, np.uint64, np.int64
CLASSES = ("no_prior", "low_parallax", "border", "edge", "flat", "rejected", "fused")
NO_PRIOR, LOW_PARALLAX, BORDER, EDGE, FLAT, REJECTED, FUSED = range(7)
FIELDS = ("radius", "steps", "min_gain", "noise_sigma", "min_sigma", "max_sigma", "gate")


def rule(radius, steps, min_gain, noise_sigma, min_sigma, max_sigma, gate):
    ns, lo, hi = F32(noise_sigma), F32(min_sigma), F32(max_sigma)
    return dict(radius=int(radius), steps=int(steps), min_gain=F32(min_gain), noise2=F32(ns * ns), min2=F32(lo * lo), max2=F32(hi * hi), gate=F32(gate),
                noise_sigma=ns, min_sigma=lo, max_sigma=hi)


def setting(prm, mode=1):
    """The rule as the binding's setting dict."""
    return dict(mode=mode, radius=prm["radius"], steps=prm["steps"], min_gain=float(prm["min_gain"]), noise_sigma=float(prm["noise_sigma"]),
                min_sigma=float(prm["min_sigma"]), max_sigma=float(prm["max_sigma"]), gate=float(prm["gate"]))


def _centres(cam, Q, prm, pd, line, j):
    """Hypothesis j of every pixel: (ok, xq, yq) as ms_hypothesis has them (the test of the window in C is the caller's)."""
    fx, fy, cx, cy, e = line["fx"], line["fy"], line["cx"], line["cy"], line["e"]
    rows, cols, rho = cam["rows"], cam["cols"], prm["radius"]
    with np.errstate(all="ignore"):
        dj = pd.astype(F64) + F64(j) * line["delta"]
        ok = dj > 0
        N0 = line["h0"] + dj * e[0]
        N1 = line["h1"] + dj * e[1]
        D = line["h2"] + dj * e[2]
        ok &= D > 0
        u = (fx * N0) / D + cx
        v = (fy * N1) / D + cy
        ok &= (np.abs(u) < 2.0 ** 20) & (np.abs(v) < 2.0 ** 20)
        sx = u * 32.0
        sy = v * 32.0
        ok &= (np.abs(sx) < 2.0 ** 20) & (np.abs(sy) < 2.0 ** 20)
        xq = np.rint(np.where(ok, sx, 0.0)).astype(I64)      # ties to even
        yq = np.rint(np.where(ok, sy, 0.0)).astype(I64)
    ix, iy = xq >> 5, yq >> 5
    ok &= (ix - rho >= 0) & (ix + rho + 1 < cols) & (iy - rho >= 0) & (iy + rho + 1 < rows)
    return ok, xq, yq


def _search(cam, prm, Q, pd, pv, has):
    """Steps 1 - 3 for every pixel: (cls with -1 where the pixel goes on, ok_all, delta, {j: (xq, yq)})."""
    rows, cols = cam["rows"], cam["cols"]
    rho, J = prm["radius"], prm["steps"]
    lo, hi = cam["lo"], cam["hi"]
    Qd = np.asarray(Q, F32).reshape(-1)[:12].reshape(3, 4).astype(F64)
    fx, fy, cx, cy = F64(cam["fx"]), F64(cam["fy"]), F64(cam["cx"]), F64(cam["cy"])
    fb = fx * F64(cam["b"])
    with np.errstate(all="ignore"):
        e = [Qd[r, 3] / fb for r in range(3)]
        prior = (pv >= 0) & fref.valid(pd, lo, hi)
        if has is not None:
            prior &= has
        cls = np.full((rows, cols), -1, I64)
        cls[~prior] = NO_PRIOR
        y, x = np.mgrid[0:rows, 0:cols]
        xa = x.astype(F64) - cx
        a = xa / fx
        yb = y.astype(F64) - cy
        bq = yb / fy
        h0 = (Qd[0, 0] * a + Qd[0, 1] * bq) + Qd[0, 2]
        h1 = (Qd[1, 0] * a + Qd[1, 1] * bq) + Qd[1, 2]
        h2 = (Qd[2, 0] * a + Qd[2, 1] * bq) + Qd[2, 2]
        d = pd.astype(F64)
        N0 = h0 + d * e[0]
        N1 = h1 + d * e[1]
        D_ = h2 + d * e[2]
        DD = D_ * D_
        nu = e[0] * D_ - N0 * e[2]
        nv = e[1] * D_ - N1 * e[2]
        up = (fx * nu) / DD
        vp = (fy * nv) / DD
        gain = np.sqrt(up * up + vp * vp)
        low = ~(gain <= np.finfo(F64).max) | (gain < F64(prm["min_gain"]))
        cls[prior & low] = LOW_PARALLAX
        go = prior & ~low
        delta = 1.0 / gain
    line = dict(fx=fx, fy=fy, cx=cx, cy=cy, e=e, h0=h0, h1=h1, h2=h2, delta=delta)
    inside = (x - rho >= 0) & (x + rho < cols) & (y - rho >= 0) & (y + rho < rows)
    ok_all = go & inside
    cen = {}
    for j in range(-J, J + 1):
        ok, xq, yq = _centres(cam, Q, prm, pd, line, j)
        ok_all &= ok
        cen[j] = (xq, yq)
    cls[go & ~ok_all] = BORDER
    return cls, ok_all, delta, cen


def refine(cam, prm, C, K, Q, pd, pv, has=None):
    """(D f32, V f32, cls u8 [rows, cols], counts dict) of the first image C, the second image K (X_K = Q X_C) and the prior maps.  has: where a
    prior exists at all (None: where pv >= 0)."""
    C = np.ascontiguousarray(C, np.uint8)
    K = np.ascontiguousarray(K, np.uint8)
    pd = np.ascontiguousarray(pd, F32)
    pv = np.ascontiguousarray(pv, F32)
    rows, cols = cam["rows"], cam["cols"]
    assert C.shape == K.shape == pd.shape == pv.shape == (rows, cols)
    rho, J = prm["radius"], prm["steps"]
    n = (2 * rho + 1) ** 2
    lo, hi = cam["lo"], cam["hi"]
    cls, ok_all, delta, cen = _search(cam, prm, Q, pd, pv, has)
    y, x = np.mgrid[0:rows, 0:cols]
    ys, xs = y[ok_all], x[ok_all]
    Ci, Ki = C.astype(I64), K.astype(I64)
    S = np.zeros((2 * J + 1, ys.size), I64)
    for j in range(-J, J + 1):
        xq, yq = cen[j][0][ok_all], cen[j][1][ok_all]
        ix, iy, fxq, fyq = xq >> 5, yq >> 5, xq & 31, yq & 31
        acc = np.zeros(ys.size, I64)
        for jj in range(-rho, rho + 1):
            for ii in range(-rho, rho + 1):
                p00, p01 = Ki[iy + jj, ix + ii], Ki[iy + jj, ix + ii + 1]
                p10, p11 = Ki[iy + jj + 1, ix + ii], Ki[iy + jj + 1, ix + ii + 1]
                k = ((32 - fyq) * ((32 - fxq) * p00 + fxq * p01) + fyq * ((32 - fxq) * p10 + fxq * p11) + 512) >> 10
                diff = Ci[ys + jj, xs + ii] - k
                acc += diff * diff
        S[j + J] = acc
    js = np.argmin(S, axis=0) - J if ys.size else np.zeros(0, I64)      # the first minimum
    c = np.full(ys.size, -1, I64)
    edge = np.abs(js) == J
    c[edge] = EDGE
    at = np.where(edge, 0, js) + J
    col = np.arange(ys.size)
    s0 = S[at, col]
    sm = S[np.maximum(at - 1, 0), col]
    sp = S[np.minimum(at + 1, 2 * J), col]
    a2 = sm + sp - 2 * s0
    flat = ~edge & (a2 <= 0)
    c[flat] = FLAT
    live = ~edge & ~flat
    a2s = np.where(live, a2, 1)
    pd_, pv_ = pd[ok_all], pv[ok_all]
    dl = delta[ok_all]
    with np.errstate(all="ignore"):
        o = (sm - sp).astype(F64) / (2 * a2s).astype(F64)
        t = js.astype(F64) + o
        dt = (pd_.astype(F64) + t * dl).astype(F32)
        floor_ = F64(2 * n) * F64(prm["noise2"])
        num = F64(2.0) * np.maximum(floor_, s0.astype(F64))
        den = F64(n) * a2s.astype(F64)
        q = num / den
        d2 = dl * dl
        vt = (q * d2).astype(F32)
        vt = np.where(vt < prm["min2"], prm["min2"], vt)
        vt = np.where(vt > prm["max2"], prm["max2"], vt).astype(F32)
        s = pv_ + vt
        bound = prm["gate"] * np.sqrt(s)
        diff = dt - pd_
        cons = np.abs(diff) <= bound
        k = pv_ / s
        kd = k * diff
        f = pd_ + kd
        kv = k * pv_
        vf = pv_ - kv
        assert s.dtype == F32 and bound.dtype == F32 and f.dtype == F32 and vf.dtype == F32 and dt.dtype == F32
        good = cons & (f > 0) & fref.valid(f, lo, hi)
    c[live & ~good] = REJECTED
    c[live & good] = FUSED
    cls[ok_all] = c
    assert np.all(cls >= 0)
    D, V = pd.copy(), pv.copy()
    fused = np.zeros((rows, cols), bool)
    fused[ok_all] = c == FUSED
    Df, Vf = np.zeros((rows, cols), F32), np.zeros((rows, cols), F32)
    Df[ok_all], Vf[ok_all] = f, vf
    D[fused], V[fused] = Df[fused], Vf[fused]
    counts = {name: int((cls == k).sum()) for k, name in enumerate(CLASSES)}
    return D, V, cls.astype(np.uint8), counts


TILE_W, TILE_H, BOX_W, BOX_H = 32, 8, 96, 48      # the kernel's tile and the largest box of K it stages (kernels_motion_stereo.hip)


def tile_paths(cam, prm, Q, pd, pv, has=None):
    """(staged, direct, idle): the tiles of the kernel by the path they take — the bounding box of the K taps of a tile's pixels that go on to
    the sums fits the staged box, does not, or no pixel goes on."""
    pd = np.ascontiguousarray(pd, F32)
    pv = np.ascontiguousarray(pv, F32)
    rows, cols = cam["rows"], cam["cols"]
    rho, J = prm["radius"], prm["steps"]
    cls, ok_all, delta, cen = _search(cam, prm, Q, pd, pv, has)
    ix = np.stack([cen[j][0] >> 5 for j in range(-J, J + 1)])
    iy = np.stack([cen[j][1] >> 5 for j in range(-J, J + 1)])
    out = [0, 0, 0]
    for y0 in range(0, rows, TILE_H):
        for x0 in range(0, cols, TILE_W):
            go = ok_all[y0:y0 + TILE_H, x0:x0 + TILE_W]
            if not go.any():
                out[2] += 1
                continue
            tx, ty = ix[:, y0:y0 + TILE_H, x0:x0 + TILE_W][:, go], iy[:, y0:y0 + TILE_H, x0:x0 + TILE_W][:, go]
            bw = (tx.max() + rho + 1) - (tx.min() - rho) + 1
            bh = (ty.max() + rho + 1) - (ty.min() - rho) + 1
            out[0 if bw <= BOX_W and bh <= BOX_H else 1] += 1
    return tuple(out)


def refine_words(cam, prm, C, K, Q, z):
    """The stage on a z-buffer of keys (u64; 0: no candidate, and stays 0): (z', cls, counts)."""
    pd = (z >> U64(32)).astype(U32).view(F32)
    pv = (z & U64(0xFFFFFFFF)).astype(U32).view(F32)
    D, V, cls, counts = refine(cam, prm, C, K, Q, pd, pv, has=z != 0)
    out = (bits(D).astype(U64) << U64(32)) | bits(V).astype(U64)
    return np.where(z != 0, out, U64(0)), cls, counts


def bits(a):
    return np.ascontiguousarray(a, F32).view(U32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


# ---- the inputs the tests share ------------------------------------------------------------------------------------------------------------------
RULE = rule(2, 4, 0.25, 2.0, 0.02, 2.0, 3.0)
motion = fref.motion
MOTIONS = ("sideways", "forward", "rotation", "general", "roll")


def case_motion(name):
    """Q (f32 [4, 4], X_K = Q X_C) of the named motion for a camera with b = 0.1."""
    if name == "sideways":
        return motion(t=(0.25, 0.0, 0.0))
    if name == "forward":      # the epipole lies inside the image, off its centre
        return motion(t=(0.02, -0.01, 0.4))
    if name == "rotation":     # no translation at all: every pixel with a prior is low_parallax
        return motion(0.01, -0.02, 0.03)
    if name == "general":
        return motion(0.004, -0.006, 0.01, (0.15, -0.1, 0.05))
    if name == "roll":         # a quarter turn about the optical axis: a tile's row of 32 pixels is a column of K, taller than the staged box
        return motion(0.0, 0.0, 0.5 * np.pi, (0.0, 0.25, 0.0))
    raise KeyError(name)


def textured_pair(cam, Q, seed, d_lo=3.0, d_hi=9.0):
    """A pair with known disparities: K is smoothed noise, C is K looked up at every pixel's own image u(d), v(d) under Q (nearest pixel: the
    rule is what is compared, a match that is about right is enough to reach its later classes), and the true map d."""
    rows, cols = cam["rows"], cam["cols"]
    rng = np.random.default_rng(seed)
    big = rng.integers(0, 256, (rows + 2, cols + 2)).astype(F64)
    K = ((big[:-2, :-2] + big[:-2, 1:-1] + big[1:-1, :-2] + 2 * big[1:-1, 1:-1] + big[1:-1, 2:] + big[2:, 1:-1] + big[2:, 2:]) / 8.0)
    K = np.clip(np.rint(K), 0, 255).astype(np.uint8)
    y, x = np.mgrid[0:rows, 0:cols]
    d = (d_lo + (d_hi - d_lo) * x / max(cols - 1, 1) + 0.5 * y / max(rows - 1, 1)).astype(F32)
    Qd = np.asarray(Q, F64).reshape(4, 4)
    fx, fy, cx, cy = (F64(cam[k]) for k in ("fx", "fy", "cx", "cy"))
    Z = fx * F64(cam["b"]) / d.astype(F64)
    X = np.stack([(x - cx) / fx * Z, (y - cy) / fy * Z, Z, np.ones_like(Z)], -1) @ Qd.T
    with np.errstate(all="ignore"):
        u = np.rint(fx * X[..., 0] / X[..., 2] + cx)
        v = np.rint(fy * X[..., 1] / X[..., 2] + cy)
    ok = (X[..., 2] > 0) & (u >= 0) & (u < cols) & (v >= 0) & (v < rows)
    C = rng.integers(0, 256, (rows, cols)).astype(np.uint8)
    C[ok] = K[v[ok].astype(I64), u[ok].astype(I64)]
    return C, K, d


def hostile_prior(cam, d, seed):
    """Prior maps around the true map d: offsets of a fraction of a pixel and a few whole pixels, variances from 0 upwards, holes (pv < 0), NaN in
    either map, disparities outside the gate, zero and negative ones, and a band of a constant image value is the caller's to add."""
    rows, cols = cam["rows"], cam["cols"]
    rng = np.random.default_rng(seed)
    pd = (d + rng.normal(0.0, 0.3, d.shape)).astype(F32)
    pv = rng.choice(np.array([0.0, 0.01, 0.09, 0.25, 1.0], F32), d.shape).astype(F32)
    far = rng.random(d.shape) < 0.08
    pd[far] += F32(2.5)                                       # whole pixels off with a small variance: rejected or edge
    pv[far] = F32(0.0004)
    pv[rng.random(d.shape) < 0.1] = F32(-1.0)                 # holes
    special_d = np.array([np.nan, np.inf, -np.inf, -1.0, 0.0, -0.0, cam["lo"], cam["hi"], np.nextafter(cam["hi"], F32(np.inf)), 2.0 * cam["hi"], F32(1e-30)], F32)
    flat_d, flat_v = pd.reshape(-1), pv.reshape(-1)
    at = rng.permutation(flat_d.size)[:min(flat_d.size, 3 * special_d.size)]
    flat_d[at] = special_d[np.arange(at.size) % special_d.size]
    at = rng.permutation(flat_d.size)[:min(flat_d.size, 6)]
    flat_v[at] = np.array([np.nan, np.inf, 0.0, -0.0, 3.0e38, -np.inf], F32)[:at.size]
    return pd, pv


def rule_case(rows, cols, name, seed=0, hi=64.0):
    """(cam, C, K, Q, pd, pv) of the named motion at rows x cols: textured_pair under hostile_prior, with a constant patch in both images (flat)."""
    cam = fref.camera(rows, cols, lo=0.001, hi=hi)
    Q = case_motion(name)
    C, K, d = textured_pair(cam, Q, seed + rows)
    if rows >= 24:
        C[rows // 2 - 6:rows // 2 + 6, 4:cols // 3] = 90
        K[:, :] = np.where(np.abs(np.mgrid[0:rows, 0:cols][0] - rows // 2) < 9, np.where(np.mgrid[0:rows, 0:cols][1] < cols // 2, 90, K), K)
    pd, pv = hostile_prior(cam, d, seed + cols)
    return cam, C, K, Q, pd, pv
