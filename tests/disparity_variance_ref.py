"""The measurement-variance rule (c_api.h "measurement variance") as numpy: the statement the C++ header bpvo_amd/csrc/disparity_variance_math.h and
the kernel are compared with, bit for bit.  The sums are int64 (exact), the quotient one f64 division rounded to f32, as the header has it.  Also the
disparity-fusion step with a per-pixel measurement variance (disparity_fusion_ref's update with r2 a map), and the inputs the CPU and GPU tests share."""
import numpy as np

import disparity_fusion_ref as fref

F32, F64, U32, U64 = np.float32, np.float64, np.uint32, np.uint64
CLASSES = ("invalid", "border", "flat", "floor", "ceiling", "model")
F32_MAX = np.finfo(np.float32).max


def rule(radius, noise_sigma, min_sigma, max_sigma):
    ns, lo, hi = F32(noise_sigma), F32(min_sigma), F32(max_sigma)
    return dict(radius=int(radius), noise2=F32(ns * ns), min2=F32(lo * lo), max2=F32(hi * hi), noise_sigma=ns, min_sigma=lo, max_sigma=hi)


def setting(prm, mode=1):
    """The rule as the binding's setting dict."""
    return dict(mode=mode, radius=prm["radius"], noise_sigma=float(prm["noise_sigma"]), min_sigma=float(prm["min_sigma"]), max_sigma=float(prm["max_sigma"]))


def variance(prm, L, R, M, lo, hi):
    """(R2 f32 [rows, cols], counts dict) of the rectified u8 pair L, R and the measured map M under the gate lo .. hi."""
    L = np.ascontiguousarray(L, np.uint8)
    R = np.ascontiguousarray(R, np.uint8)
    M = np.ascontiguousarray(M, F32)
    rows, cols = M.shape
    rho = prm["radius"]
    n = (2 * rho + 1) ** 2
    cls = np.full((rows, cols), -1, np.int64)
    ok = fref.valid(M, F32(lo), F32(hi))
    cls[~ok] = 0
    with np.errstate(invalid="ignore"):
        small = ok & (np.abs(M) < F32(2.0 ** 30))
    d0 = np.zeros((rows, cols), np.int64)
    d0[small] = np.rint(M[small].astype(F64)).astype(np.int64)      # ties to even
    y, x = np.mgrid[0:rows, 0:cols]
    inside = small & (y - rho >= 0) & (y + rho < rows) & (x - rho >= 0) & (x + rho < cols) & (x - rho - d0 - 1 >= 0) & (x + rho - d0 + 1 < cols)
    cls[ok & ~inside] = 1
    S = np.zeros((3, rows, cols), np.int64)
    Li, Ri = L.astype(np.int64), R.astype(np.int64)
    ys, xs = y[inside], x[inside]
    ds = d0[inside]
    for k in (-1, 0, 1):
        acc = np.zeros(ys.shape, np.int64)
        for j in range(-rho, rho + 1):
            for i in range(-rho, rho + 1):
                diff = Li[ys + j, xs + i] - Ri[ys + j, xs + i - ds - k]
                acc += diff * diff
        S[k + 1][inside] = acc
    a = S[0] + S[2] - 2 * S[1]
    flat = inside & (a <= 0)
    cls[flat] = 2
    go = inside & ~flat
    num = F64(2.0) * np.maximum(F64(2 * n) * F64(prm["noise2"]), S[1].astype(F64))
    den = F64(n) * np.where(go, a, 1).astype(F64)
    with np.errstate(over="ignore"):
        v = (num / den).astype(F32)
    floor = go & (v < prm["min2"])
    ceil = go & (v > prm["max2"])
    cls[floor] = 3
    cls[ceil] = 4
    cls[go & ~floor & ~ceil] = 5
    R2 = np.full((rows, cols), prm["max2"], F32)
    R2[floor] = prm["min2"]
    model = cls == 5
    R2[model] = v[model]
    assert np.all(cls >= 0)
    counts = {name: int((cls == k).sum()) for k, name in enumerate(CLASSES)}
    return R2, counts


def bits(a):
    return np.ascontiguousarray(a, F32).view(U32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


# ---- the disparity-fusion step with a per-pixel measurement variance ---------------------------------------------------------------------------
def update_var(cam, prm, M, z, R2):
    """disparity_fusion_ref.update with r2 a map: an entry outside (0, FLT_MAX] takes the constant prm["r2"].  R2 None: the constant everywhere."""
    M = np.ascontiguousarray(M, F32)
    lo, hi, gate, fill2 = cam["lo"], cam["hi"], prm["gate"], prm["fill2"]
    r2 = np.full(M.shape, prm["r2"], F32)
    if R2 is not None:
        R2 = np.ascontiguousarray(R2, F32)
        with np.errstate(invalid="ignore"):
            use = (R2 > 0) & (R2 <= F32_MAX)
        r2[use] = R2[use]
    mv = fref.valid(M, lo, hi)
    has = z != 0
    pd = (z >> U64(32)).astype(U32).view(F32)
    pv = (z & U64(0xFFFFFFFF)).astype(U32).view(F32)
    with np.errstate(all="ignore"):
        s = pv + r2
        bound = gate * np.sqrt(s)
        diff = M - pd
        cons = np.abs(diff) <= bound
        k = pv / s
        f = pd + k * diff
        kv = k * pv
        vf = pv - kv
    assert s.dtype == F32 and bound.dtype == F32 and f.dtype == F32 and vf.dtype == F32
    fused = mv & has & cons
    replaced = mv & has & ~cons
    measured = mv & ~has
    filled = ~mv & has & (pv <= fill2)
    none = ~(fused | replaced | measured | filled)
    D = M.copy()
    V = np.full(M.shape, -1.0, F32)
    keep = fused & fref.valid(f, lo, hi)
    D[keep] = f[keep]
    V[fused] = vf[fused]
    V[replaced | measured] = r2[replaced | measured]
    D[filled] = pd[filled]
    V[filled] = pv[filled]
    counts = dict(zip(fref.CLASSES, (int(fused.sum()), int(replaced.sum()), int(measured.sum()), int(filled.sum()), int(none.sum()))))
    return D, V, counts


def step_var(cam, prm, M, R2, Dc=None, Vc=None, P=None):
    """disparity_fusion_ref.step with the measurement variance map R2 (None: the constant)."""
    if Dc is None or P is None:
        z = np.zeros((cam["rows"], cam["cols"]), U64)
    else:
        z = fref.splat(cam, prm, Dc, Vc, P)
    return update_var(cam, prm, M, z, R2)


# ---- the inputs the tests share ------------------------------------------------------------------------------------------------------------------
RULE = rule(2, 2.0, 0.02, 2.0)


def random_pair(rows, cols, seed):
    """A right image of smoothed noise and the left image that a disparity of about 3 plus texture noise makes of it."""
    rng = np.random.default_rng(seed)
    R = rng.integers(0, 256, (rows, cols), dtype=np.uint8)
    L = np.roll(R, 3, axis=1).astype(np.int64) + rng.integers(-6, 7, (rows, cols))
    return np.clip(L, 0, 255).astype(np.uint8), R


def checkerboard_pair(rows, cols):
    """An all-0 / all-255 checkerboard against its inverse: at an even disparity every difference is 255 (the largest sums)."""
    y, x = np.mgrid[0:rows, 0:cols]
    L = (((x + y) & 1) * 255).astype(np.uint8)
    return L, (255 - L).astype(np.uint8)


def constant_pair(rows, cols, value=77):
    return np.full((rows, cols), value, np.uint8), np.full((rows, cols), value, np.uint8)


def hostile_disparities(rows, cols, radius, seed, hi=64.0):
    """A measured map of ordinary values among x.5 ties, 0, negatives, NaN, +-Inf, values above the gate `hi`, values >= 2^30, and, in the rows that
    have a full left window, values that put the right windows exactly on and one past each image edge."""
    rng = np.random.default_rng(seed)
    M = rng.uniform(0.0, 8.0, (rows, cols)).astype(F32)
    special = np.array([2.5, 3.5, 0.5, 1.5, 0.0, -0.0, -1.0, -2.5, np.nan, np.inf, -np.inf, hi, np.nextafter(F32(hi), F32(np.inf)), 2.0 * hi,
                        2.0 ** 30, 2.0 ** 31, 3.0e38], F32)
    flat = M.reshape(-1)
    at = rng.permutation(flat.size)[:min(flat.size, 3 * special.size)]
    flat[at] = special[np.arange(at.size) % special.size]
    for y in range(radius, rows - radius):      # the right windows span x - radius - d - 1 .. x + radius - d + 1
        for x in range(radius, cols - radius):
            if (x + y) % 5:
                continue
            on_left, on_right = x - radius - 1, x + radius + 1 - (cols - 1)      # d that puts the span's ends on column 0 / on column cols - 1
            M[y, x] = (on_left, on_left + 1, on_right, on_right - 1)[((x + y) // 5) % 4]
    return M


def smooth_disparities(rows, cols, d_lo=3.0, d_hi=9.0):
    y, x = np.mgrid[0:rows, 0:cols]
    return (d_lo + (d_hi - d_lo) * x / max(cols - 1, 1) + 0.5 * y / max(rows - 1, 1)).astype(F32)
