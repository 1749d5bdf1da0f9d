"""The point budget's rule (include/bpvo_hip/c_api.h, bpvo_hip_set_point_budget), stated in numpy.

candidates(): the pixels the selection keeps today, in raster order — the rule tests/test_oracle_cpu.py::test_selection_rules documents: the
border max(nonMaxSuppRadius, 3) (rows and columns b .. size - b - 2), saliency >= minSaliency, where the level has non-maximum suppression
the strict maximum over rows -1 .. +1 and columns -1 .. +2 (radius 1; a larger radius r: over the other pixels of the (2r + 1)^2 window), and
the gate minValidDisparity <= d <= maxValidDisparity on the full-resolution disparity at (y << level, x << level).
select(): of those, at most K, the most salient first, ties at the threshold in raster order; then the cut to a multiple of 16.
"""
import numpy as np


def candidates(S, disp, level, nms_radius, min_saliency, min_disp, max_disp, nms_param_radius=None):
    """Raster-ordered linear indices (y * cols + x) of the candidates of a level.  nms_radius <= 0: the level has no non-maximum suppression;
    nms_param_radius: nonMaxSuppRadius of the parameters (it sets the border whether or not the level suppresses); default: nms_radius."""
    S = np.asarray(S, np.float32)
    R, W = S.shape
    b = max(nms_radius if nms_param_radius is None else nms_param_radius, 3)
    ok = np.zeros((R, W), bool)
    ok[b:R - b - 1, b:W - b - 1] = True
    ok &= S >= np.float32(min_saliency)
    if nms_radius > 0:
        offs = [(dy, dx) for dy in (-1, 0, 1) for dx in (-1, 0, 1, 2)] if nms_radius == 1 else \
               [(dy, dx) for dy in range(-nms_radius, nms_radius + 1) for dx in range(-nms_radius, nms_radius + 1)]
        ys, xs = np.nonzero(ok)
        keep = np.ones(len(ys), bool)
        for dy, dx in offs:
            if dy == 0 and dx == 0:
                continue
            keep &= S[ys, xs] > S[ys + dy, xs + dx]      # (the border keeps every neighbour inside the image)
        ok[:] = False
        ok[ys[keep], xs[keep]] = True
    ys, xs = np.nonzero(ok)      # (row-major order)
    d = np.asarray(disp, np.float32)[ys << level, xs << level]
    gate = (d >= np.float32(min_disp)) & (d <= np.float32(max_disp))
    return (ys[gate] * W + xs[gate]).astype(np.int64)


def select(sal_of_cand, K, cap=None):
    """The rule on the candidates' saliencies (raster order): (positions kept, before the cut to a multiple of 16; t; tie quota; bound).
    K = 0: no budget.  t is None and the quota 0 when the budget does not bind."""
    s = np.asarray(sal_of_cand, np.float32)
    n = len(s)
    if K <= 0 or n <= K:
        return np.arange(n), None, 0, False
    t = np.sort(s)[n - K]                      # the K-th largest
    above = np.flatnonzero(s > t)
    ties = np.flatnonzero(s == t)
    quota = K - len(above)
    assert 1 <= quota <= len(ties)
    return np.sort(np.concatenate([above, ties[:quota]])), np.float32(t), int(quota), True


def kept_indices(S, disp, level, nms_radius, min_saliency, min_disp, max_disp, K, cap=None, nms_param_radius=None):
    """dict(cand: the candidates' indices, t, quota, bound, kept: the raster-ordered indices of the template — after the budget, the capacity and
    the cut to a multiple of 16: N = min(|kept|, cap) & ~15)."""
    cand = candidates(S, disp, level, nms_radius, min_saliency, min_disp, max_disp, nms_param_radius)
    W = np.asarray(S).shape[1]
    pos, t, quota, bound = select(np.asarray(S, np.float32)[cand // W, cand % W], K)
    kept = cand[pos]
    n = len(kept) if cap is None else min(len(kept), int(cap))
    return dict(cand=cand, t=t, quota=quota, bound=bound, kept=kept[:n & ~15])


def brute_force(sal_of_cand, K):
    """select() by the definition, one candidate at a time: the K largest under the order (saliency descending, position ascending)."""
    s = [float(np.float32(v)) for v in sal_of_cand]
    if K <= 0 or len(s) <= K:
        return list(range(len(s)))
    order = sorted(range(len(s)), key=lambda i: (-s[i], i))
    return sorted(order[:K])
