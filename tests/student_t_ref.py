"""Numpy reference of the Student-t loss (include/bpvo_hip/c_api.h, BPVO_LOSS_STUDENT_T): the scale fit evaluated from the definition in f64, the
weight and the curvature in the f32 operations the header states, and the multisets the CPU tests run the serial harness on."""
import numpy as np

NU = 5.0
MAX_PASSES = 64
STOP_REL = 1e-4
FLOOR = 1e-6


def T(s, r):
    """T(s) = ((nu + 1) / n) sum r^2 s / (nu s + r^2), f64."""
    r2 = np.asarray(r, np.float64).reshape(-1) ** 2
    return (NU + 1.0) / r2.size * float(np.sum(r2 * s / (NU * s + r2)))


def exists(r):
    r = np.asarray(r).reshape(-1)
    return r.size > 0 and (NU + 1.0) * np.count_nonzero(r) > r.size


def fit(r, sigma_prev=None):
    """The scale of the multiset r (the residuals of the valid points).  sigma_prev: the scale the level holds (None: none yet — the first
    linearisation of a level, or after reset_scale; the state then reads 1).  Returns dict(sigma, exists, frozen, passes, delta): sigma as f32."""
    r = np.asarray(r, np.float64).reshape(-1)
    have_prev = sigma_prev is not None
    prev = np.float32(sigma_prev if have_prev else 1.0)

    def none():
        delta = abs(np.float32(1.0) - prev)
        return dict(sigma=np.float32(1.0), exists=False, frozen=not delta > np.float32(1e-6), passes=0, delta=float(delta))
    if not exists(r):
        return none()
    s = float(prev) ** 2 if have_prev else float(np.mean(r * r))
    if not s >= FLOOR * FLOOR:
        return none()
    sigma = np.sqrt(s)
    passes, stopped_first = 0, False
    while True:
        s1 = T(s, r)
        sigma1 = np.sqrt(s1)
        stop = abs(sigma1 - sigma) <= STOP_REL * sigma
        passes += 1
        if stop and passes == 1:
            stopped_first = True
        s, sigma = s1, sigma1
        if stop or passes >= MAX_PASSES or not s1 >= FLOOR * FLOOR:
            break
    out = np.float32(sigma)
    if not float(out) >= FLOOR:
        return dict(none(), exists=True, passes=passes)
    if have_prev and stopped_first:
        return dict(sigma=prev, exists=True, frozen=True, passes=passes, delta=0.0)
    return dict(sigma=out, exists=True, frozen=False, passes=passes, delta=max(float(abs(out - prev)), 2e-6))


def weights_f32(r, sigma):
    """x = r * sigma_inv; w = 6.0f / (5.0f + x * x): every operation an f32 one, in that order."""
    r = np.asarray(r, np.float32)
    sigma_inv = np.float32(1.0) / np.float32(sigma)
    x = r * sigma_inv
    return np.float32(6.0) / (np.float32(5.0) + x * x)


def curvature(u):
    """d(u) = psi'(u) = 6 (5 - u^2) / (5 + u^2)^2, f64."""
    u2 = np.asarray(u, np.float64) ** 2
    return 6.0 * (5.0 - u2) / (5.0 + u2) ** 2


def multisets():
    """name -> (f32 residuals, expectation): expectation "fit" (a positive fixed point, found in fewer than 64 passes) or "one" (sigma = 1)."""
    g = np.random.default_rng(20131)
    n = 6000

    def with_outliers(core, frac, lo, hi):
        r = core.copy()
        k = int(frac * r.size)
        r[g.choice(r.size, k, replace=False)] = g.uniform(lo, hi, k)
        return r

    def with_zeros(core, frac):
        r = core.copy()
        r[g.choice(r.size, int(round(frac * r.size)), replace=False)] = 0.0
        return r
    core = g.normal(0.0, 0.8, n)
    out = {
        "gaussian_core": (core, "fit"),
        "outliers_10": (with_outliers(core, 0.10, -20.0, 20.0), "fit"),
        "outliers_40": (with_outliers(core, 0.40, -20.0, 20.0), "fit"),
        "intensity_30": (with_outliers(g.normal(0.0, 6.0, n), 0.30, -255.0, 255.0), "fit"),
        "half_zeros": (with_zeros(core, 0.5), "fit"),
        "zeros_85": (with_zeros(core, 0.85), "one"),
        "zeros_90": (with_zeros(core, 0.90), "one"),
        "at_threshold": (np.concatenate([g.normal(0.0, 1.0, 1000), np.zeros(5000)]), "one"),      # (nu + 1) m == n
        "two_valued": (np.where(g.random(n) < 0.7, 0.25, -3.0), "fit"),
        "n8": (np.array([0.3, -0.2, 0.5, -0.7, 0.1, 0.9, -0.4, 0.6]), "fit"),
        "empty": (np.zeros(0), "one"),
    }
    return {k: (np.asarray(v, np.float32), e) for k, (v, e) in out.items()}
