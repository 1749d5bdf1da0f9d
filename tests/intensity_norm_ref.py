"""Normalised intensity (bpvo_hip_set_intensity_normalization): the rule of include/bpvo_hip/c_api.h in numpy.  Integer histograms, integer window
sums from an integral image, f64 for the last step, one rounding to f32.  Nothing else defines "expected" in the tests of the mode."""
import numpy as np

UNIT = 32.0
MAD_TO_SIGMA = 1.4826


def median_mad(img):
    """(med, mad) of a u8 image: the lower median from the 256-bin histogram, the MAD from the same histogram folded about it."""
    h = np.bincount(np.asarray(img, np.uint8).reshape(-1), minlength=256).astype(np.int64)
    half = (int(h.sum()) + 1) // 2
    med = int(np.searchsorted(np.cumsum(h), half))          # the smallest v with cum[v] >= half
    folded = np.zeros(256, np.int64)                        # folded[k] = #{|I - med| == k}
    for u in range(256):
        folded[abs(u - med)] += h[u]
    mad = int(np.searchsorted(np.cumsum(folded), half))
    return med, mad


def whole_image(img):
    img = np.asarray(img, np.uint8)
    med, mad = median_mad(img)
    c = np.float64(UNIT) / (np.float64(MAD_TO_SIGMA) * np.float64(max(mad, 1)))
    table = ((np.arange(256, dtype=np.int64) - med).astype(np.float64) * c).astype(np.float32)
    return table[img]


def window_sums(img, R):
    """(n, S1, S2) of every pixel's window [x - R, x + R] x [y - R, y + R] cut to the image, int64."""
    I = np.asarray(img, np.uint8).astype(np.int64)
    H, W = I.shape

    def box(a):
        ii = np.zeros((H + 1, W + 1), np.int64)
        ii[1:, 1:] = a.cumsum(0).cumsum(1)
        y0 = np.clip(np.arange(H) - R, 0, H)[:, None]
        y1 = np.clip(np.arange(H) + R + 1, 0, H)[:, None]
        x0 = np.clip(np.arange(W) - R, 0, W)[None, :]
        x1 = np.clip(np.arange(W) + R + 1, 0, W)[None, :]
        return ii[y1, x1] - ii[y0, x1] - ii[y1, x0] + ii[y0, x0]
    return box(np.ones_like(I)), box(I), box(I * I)


def local_terms(img, R):
    """(X, V, n) of the rule: X = n I - S1, V = n S2 - S1^2 (before the floor), int64."""
    I = np.asarray(img, np.uint8).astype(np.int64)
    n, S1, S2 = window_sums(img, R)
    return n * I - S1, n * S2 - S1 * S1, n


def floor_binds(img, R):
    """per pixel: the floor Vf = max(V, 4 n^2) changes V"""
    _, V, n = local_terms(img, R)
    return V < 4 * n * n


def local(img, R):
    X, V, n = local_terms(img, R)
    Vf = np.maximum(V, 4 * n * n)
    return (np.float64(UNIT) * X.astype(np.float64) / np.sqrt(Vf.astype(np.float64))).astype(np.float32)


def normalize(img, radius):
    """the descriptor plane of one level: radius -1 float(I), 0 whole image, 1 .. 15 local"""
    if radius < 0:
        return np.asarray(img, np.uint8).astype(np.float32)
    return whole_image(img) if radius == 0 else local(img, radius)
