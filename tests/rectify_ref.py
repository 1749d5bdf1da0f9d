"""The rule of the rectification on the device (include/bpvo_hip/c_api.h), a second time in numpy: the lens map statement by statement in f64,
the quantisation to 1/32 pixel, the integer remap, the outside mask — what tests/test_rectify_math_cpu.py holds bpvo_amd/csrc/rectify_math.h to and
tests/test_gpu_rectify.py the library; and the lens cases both use."""
import numpy as np

OUTSIDE = np.int32(-2 ** 31)      # both words of an entry without a source


def rot(rz, ry, rx):
    """Rz(rz) Ry(ry) Rx(rx), f64."""
    cz, sz, cy, sy, cx, sx = np.cos(rz), np.sin(rz), np.cos(ry), np.sin(ry), np.cos(rx), np.sin(rx)
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]], np.float64)
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]], np.float64)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]], np.float64)
    return Rz @ Ry @ Rx


HARD_DIST = np.array([-0.28, 0.09, 0.0012, -0.0008, -0.012, 0.01, 0.002, 0.0005], np.float64)
HARD_ANGLES = (0.05, -0.04, 0.03)


def lens_case(raw_rows, raw_cols, rows, cols, f, new_scale, strength=1.0):
    """The hard lens of the suite (strength 1) or a milder one: raw K = (1.02 f, 0.99 f, raw_cols / 2 - 0.7, raw_rows / 2 + 0.4), the distortion and
    the rotation angles scaled by `strength`, the rectified camera K' = (new_scale f, new_scale f, (cols - 1) / 2, (rows - 1) / 2) held in f32 as a
    camera of the library holds it."""
    Kn = np.float32([new_scale * f, new_scale * f, (cols - 1) / 2.0, (rows - 1) / 2.0])
    return dict(rows=rows, cols=cols, raw_rows=raw_rows, raw_cols=raw_cols, Kn=Kn,
                K=np.array([1.02 * f, 0.99 * f, raw_cols / 2.0 - 0.7, raw_rows / 2.0 + 0.4], np.float64),
                dist=HARD_DIST * strength, R=rot(*[a * strength for a in HARD_ANGLES]))


def camera_case(K, rows, cols, raw_rows, raw_cols, strength=0.2, shift=(0.0, 0.0)):
    """The hard lens scaled by `strength` in front of a GIVEN rectified camera (K 3x3, rows x cols): the raw camera has the rectified camera's
    focal length stretched to the raw size (x 1.02 and 0.99) and its centre near the raw image's; shift moves that centre (another side)."""
    K = np.asarray(K, np.float32).reshape(3, 3)
    Kn = np.float32([K[0, 0], K[1, 1], K[0, 2], K[1, 2]])
    f = float(K[0, 0]) * raw_cols / cols
    return dict(rows=rows, cols=cols, raw_rows=raw_rows, raw_cols=raw_cols, Kn=Kn,
                K=np.array([1.02 * f, 0.99 * f, raw_cols / 2.0 - 0.7 + shift[0], raw_rows / 2.0 + 0.4 + shift[1]], np.float64),
                dist=HARD_DIST * strength, R=rot(*[a * strength for a in HARD_ANGLES]))


def raw_from_image(img, raw_rows, raw_cols):
    """A raw image for the composition tests: the rectified image stretched to the raw size (nearest neighbour).  No camera would give it —
    physical consistency is not needed —, but what the mild lens makes of it resembles the image, so the matcher and the estimate have texture."""
    img = np.asarray(img, np.uint8)
    rows, cols = img.shape
    yy = np.minimum((np.arange(raw_rows) * rows) // raw_rows, rows - 1)
    xx = np.minimum((np.arange(raw_cols) * cols) // raw_cols, cols - 1)
    return np.ascontiguousarray(img[yy][:, xx])


def identity_case(rows=37, cols=53, f=40.0):
    Kn = np.float32([f, f, (cols - 1) / 2.0, (rows - 1) / 2.0])
    return dict(rows=rows, cols=cols, raw_rows=rows, raw_cols=cols, Kn=Kn, K=Kn.astype(np.float64), dist=np.zeros(8), R=np.eye(3))


def hard_cases():
    """name -> (case, the share of outside pixels found for it on the CPU when the suite was written)"""
    return {
        "hard_41x59": (lens_case(41, 59, 37, 53, 40.0, 0.62), 0.338),
        "hard_60x90": (lens_case(60, 90, 48, 64, 55.0, 0.5), 0.307),
        "hard_64x80": (lens_case(64, 80, 64, 80, 60.0, 0.75), 0.243),
    }


def camera_K(case):
    """the 3x3 f32 K of the case's rectified camera"""
    fx, fy, cx, cy = [float(v) for v in case["Kn"]]
    return np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], np.float32)


def params_f64(case):
    """the 29 doubles tests/cpp/rectify_harness.cc reads"""
    return np.concatenate([[case["rows"], case["cols"], case["raw_rows"], case["raw_cols"]], case["Kn"].astype(np.float64), case["K"], case["dist"],
                           np.asarray(case["R"], np.float64).reshape(9)]).astype(np.float64)


def lens_source(case):
    """(xs, ys): f64 [rows][cols], one operation per statement in the header's order"""
    fxn, fyn, cxn, cyn = [np.float64(v) for v in case["Kn"]]
    fx, fy, cx, cy = [np.float64(v) for v in case["K"]]
    k1, k2, p1, p2, k3, k4, k5, k6 = [np.float64(v) for v in case["dist"]]
    R = np.asarray(case["R"], np.float64)
    v, u = np.meshgrid(np.arange(case["rows"], dtype=np.float64), np.arange(case["cols"], dtype=np.float64), indexing="ij")
    a = (u - cxn) / fxn
    b = (v - cyn) / fyn
    t = R[0, 0] * a
    t2 = R[1, 0] * b
    X = (t + t2) + R[2, 0]
    t = R[0, 1] * a
    t2 = R[1, 1] * b
    Y = (t + t2) + R[2, 1]
    t = R[0, 2] * a
    t2 = R[1, 2] * b
    W = (t + t2) + R[2, 2]
    x = X / W
    y = Y / W
    x2 = x * x
    y2 = y * y
    r2 = x2 + y2
    xy = x * y
    num = k3 * r2
    num = num + k2
    num = num * r2
    num = num + k1
    num = num * r2
    num = 1.0 + num
    den = k6 * r2
    den = den + k5
    den = den * r2
    den = den + k4
    den = den * r2
    den = 1.0 + den
    rad = num / den
    tp1 = 2.0 * p1
    tp2 = 2.0 * p2
    t = x * rad
    t2 = tp1 * xy
    t = t + t2
    t2 = 2.0 * x2
    t2 = r2 + t2
    t2 = p2 * t2
    xd = t + t2
    t = y * rad
    t2 = 2.0 * y2
    t2 = r2 + t2
    t2 = p1 * t2
    t = t + t2
    t2 = tp2 * xy
    yd = t + t2
    xs = fx * xd
    xs = xs + cx
    ys = fy * yd
    ys = ys + cy
    return xs, ys


def quantise(x, y):
    """(xq, yq) int32 of f64 (or f32: widened) coordinates: nearbyint(x * 32), ties to even; not finite or |x * 32| >= 2^20 -> OUTSIDE in both"""
    x = np.asarray(x).astype(np.float64)
    y = np.asarray(y).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        sx, sy = x * 32.0, y * 32.0
        ok = (np.abs(sx) < 2.0 ** 20) & (np.abs(sy) < 2.0 ** 20)      # (NaN and Inf compare false)
    xq = np.where(ok, np.rint(np.where(ok, sx, 0.0)), float(OUTSIDE)).astype(np.int64).astype(np.int32)
    yq = np.where(ok, np.rint(np.where(ok, sy, 0.0)), float(OUTSIDE)).astype(np.int64).astype(np.int32)
    return xq, yq


def _taps(raw_rows, raw_cols, xq, yq):
    xq = xq.astype(np.int64)
    yq = yq.astype(np.int64)
    ix, fx = xq >> 5, xq & 31      # (numpy's >> on signed integers is arithmetic)
    iy, fy = yq >> 5, yq & 31
    x0 = (ix >= 0) & (ix < raw_cols)
    x1 = (ix + 1 >= 0) & (ix + 1 < raw_cols)
    y0 = (iy >= 0) & (iy < raw_rows)
    y1 = (iy + 1 >= 0) & (iy + 1 < raw_rows)
    return ix, fx, iy, fy, x0, x1, y0, y1


def outside(raw_rows, raw_cols, xq, yq):
    """the mask of destination pixels without a full source: the sentinel, or a tap with a non-zero weight outside the raw image"""
    ix, fx, iy, fy, x0, x1, y0, y1 = _taps(raw_rows, raw_cols, xq, yq)
    w = [((32 - fy) * (32 - fx), y0 & x0), ((32 - fy) * fx, y0 & x1), (fy * (32 - fx), y1 & x0), (fy * fx, y1 & x1)]
    miss = np.zeros(xq.shape, bool)
    for weight, inside in w:
        miss |= (weight != 0) & ~inside
    return miss | (xq == OUTSIDE)


def remap(raw, xq, yq):
    """the rectified u8 image of entries (xq, yq) from the raw u8 image"""
    raw = np.asarray(raw, np.uint8)
    raw_rows, raw_cols = raw.shape
    ix, fx, iy, fy, x0, x1, y0, y1 = _taps(raw_rows, raw_cols, xq, yq)
    big = np.zeros((raw_rows + 2, raw_cols + 2), np.int64)      # a border of zeros: the taps outside

    def tap(yy, xx, ok):
        return np.where(ok, big[np.clip(yy, -1, raw_rows) + 1, np.clip(xx, -1, raw_cols) + 1], 0)
    big[1:-1, 1:-1] = raw
    p00, p01 = tap(iy, ix, y0 & x0), tap(iy, ix + 1, y0 & x1)
    p10, p11 = tap(iy + 1, ix, y1 & x0), tap(iy + 1, ix + 1, y1 & x1)
    out = ((32 - fy) * ((32 - fx) * p00 + fx * p01) + fy * ((32 - fx) * p10 + fx * p11) + 512) >> 10
    out = np.where(xq == OUTSIDE, 0, out)
    assert out.min() >= 0 and out.max() <= 255
    return out.astype(np.uint8)


def rectify(case, raw):
    """(rectified image, outside count, (xq, yq)) of a lens case"""
    xq, yq = quantise(*lens_source(case))
    return remap(raw, xq, yq), int(outside(case["raw_rows"], case["raw_cols"], xq, yq).sum()), (xq, yq)


def hostile_maps(rows, cols, raw_rows, raw_cols, seed=5):
    """f32 maps with exact 1/64 offsets (ties with even and odd neighbours), negatives in (-1, 0), NaN, +-Inf, 1e9, values near the far edge"""
    rng = np.random.default_rng(seed)
    mx = (rng.integers(-64, 64 * (raw_cols + 1), size=(rows, cols)) / 64.0).astype(np.float32)      # multiples of 1/64: every odd one is a tie
    my = (rng.integers(-64, 64 * (raw_rows + 1), size=(rows, cols)) / 64.0).astype(np.float32)
    mx[0, :8] = [0.5 / 32, 1.5 / 32, 2.5 / 32, -0.5 / 32, -1.5 / 32, -2.5 / 32, 3.5 / 32, 4.5 / 32]      # ties: to 0, 2, 2, -0, -2, -2, 4, 4
    my[0, :8] = [1.5 / 32, 0.5 / 32, -0.5 / 32, 2.5 / 32, 1.0, -1.5 / 32, 2.0, -2.5 / 32]
    mx[1, :6] = [-0.999, -0.5, -0.01, -1.0 / 64, -0.75, -0.25]
    my[1, :6] = [3.0, -0.5, -0.01, 2.0, -0.99, 1.25]
    mx[2, :6] = [np.nan, np.inf, -np.inf, 1e9, 3.0, 3.0]
    my[2, :6] = [3.0, 3.0, 3.0, 3.0, np.nan, -1e9]
    mx[3, :4] = [32767.97, -32768.0, 32768.0, raw_cols - 1]      # the edge of the entry's range: |x * 32| < 2^20 holds for the first only
    my[3, :4] = [1.0, 1.0, 1.0, raw_rows - 1]
    return mx, my


def last_pixel_maps(rows, cols, raw_rows, raw_cols):
    """every destination pixel at the last raw pixel"""
    return np.full((rows, cols), raw_cols - 1, np.float32), np.full((rows, cols), raw_rows - 1, np.float32)
