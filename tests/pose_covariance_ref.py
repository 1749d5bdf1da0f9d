"""The pose covariance of include/bpvo_hip/c_api.h (bpvo_hip_pose_covariances) in numpy float64, from the reference-layout arrays the
accessors return: residuals r [C*N] channel-major, valid [N], Jacobians J [C, N, 6] in the level's Hartley-normalised twist, the robust scale
sigma.  Weights w(u) and the curvature weight d(u) = psi'(u) are taken per residual in the library's own float32 arithmetic (r * (1 / sigma), as
mest_weight does: their thresholds are discontinuities, and the definition says "the library's weight"); every sum and all linear algebra is float64."""
import numpy as np

LOSS_HUBER, LOSS_TUKEY, LOSS_L2 = 0x10, 0x11, 0x12
COV_OK, COV_INDEFINITE, COV_DEGENERATE, COV_NONE = 0, 1, 2, 3


def weights_f32(r, sigma, loss):
    """(w, d) per residual, float32: mest_weight and its curvature counterpart."""
    r = np.asarray(r, np.float32)
    one = np.float32(1.0)
    x = r * (one / np.float32(sigma))
    if loss == LOSS_HUBER:
        k = np.float32(1.345)
        ax = np.abs(x)
        return (k / np.maximum(ax, k)).astype(np.float32), (ax <= k).astype(np.float32)
    if loss == LOSS_TUKEY:
        t = np.float32(4.685)
        t_i = np.float32(1.0 / float(t))
        q = x * t_i
        inside = np.abs(x) < t
        w = one - q * q
        w = w * w
        q2 = q * q
        d = (one - q2) * (one - np.float32(5.0) * q2)
        return np.where(inside, w, np.float32(0)).astype(np.float32), np.where(inside, d, np.float32(0)).astype(np.float32)
    return np.ones_like(r), np.ones_like(r)


def in_front(X, T):
    """The definition's cheirality rule for RigidBodyWarp's points X [N, 4] at pose T: z > 0, float32 like the device ((T20 X + T21 Y) + T22 Z) + T23."""
    X, T = np.asarray(X, np.float32), np.asarray(T, np.float32)
    return (((T[2, 0] * X[:, 0] + T[2, 1] * X[:, 1]) + T[2, 2] * X[:, 2]) + T[2, 3]) > 0


def sums(r, valid, J, sigma, loss, front=None):
    """M = sum_p v_p sum_c d J^T J, Q = sum_p v_p g_p^T g_p, sum_p g_p, number of valid points — float64.  v_p: the valid flag, and (front, a mask
    from in_front; None: every point is) the point in front of the camera."""
    J = np.asarray(J, np.float64)
    C, N = J.shape[0], J.shape[1]
    r32 = np.asarray(r, np.float32).reshape(C, N)
    w, d = weights_f32(r32, sigma, loss)
    v = (np.asarray(valid).reshape(N) != 0).astype(np.float64)
    if front is not None:
        v = v * np.asarray(front, np.float64).reshape(N)
    r64 = r32.astype(np.float64)
    dv = d.astype(np.float64) * v[None, :]
    wv = w.astype(np.float64) * v[None, :]
    M = np.einsum("cn,cni,cnj->ij", dv, J, J)
    g = np.einsum("cn,cni->ni", wv * r64, J)      # [N, 6]: one cluster per point
    Q = g.T @ g
    return M, Q, g.sum(axis=0), int(v.sum())


def normalization_map(nrm_pair):
    """A = [[I, 0], [[c]x, I/s]] from the pair (N, N^-1) bpvo_hip_get_normalization returns, N = [sI, -s c; 0 1], N^-1 = [I/s, c; 0 1]: s and c as
    the library holds them (two identities: A = I)."""
    N, N_inv = (np.asarray(m, np.float32) for m in nrm_pair)
    s = float(N[0, 0])
    c = N_inv[:3, 3].astype(np.float64)
    A = np.eye(6)
    A[3:, :3] = skew(c)
    A[3:, 3:] = np.eye(3) / s
    return A


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


def sandwich(M, Q):
    Mi = np.linalg.inv(np.asarray(M, np.float64))
    S = Mi @ np.asarray(Q, np.float64) @ Mi
    return 0.5 * (S + S.T)


def status_of(M, Q, num_valid):
    if num_valid < 6 or not (np.all(np.isfinite(M)) and np.all(np.isfinite(Q))):
        return COV_DEGENERATE
    if np.linalg.eigvalsh(np.asarray(M, np.float64)).min() <= 0:
        return COV_INDEFINITE
    return COV_OK


def body_covariance(members):
    """members: (M_p, Q_p, A_p, X_p) per camera, sums in the member's normalised twist.  Sigma_b = M_b^-1 Q_b M_b^-1 with
    M_b = sum B^T M B, Q_b = sum B^T Q B, B = A^-1 Ad(X); one camera with X = I: A Sigma_xi A^T."""
    Mb, Qb = np.zeros((6, 6)), np.zeros((6, 6))
    for M, Q, A, X in members:
        B = np.linalg.inv(A) @ adjoint(X)
        Mb += B.T @ np.asarray(M, np.float64) @ B
        Qb += B.T @ np.asarray(Q, np.float64) @ B
    return sandwich(Mb, Qb), Mb, Qb


def covariance(r, valid, J, sigma, loss, nrm_pair, front=None):
    """The single camera's plain-twist covariance and its parts."""
    M, Q, g, nv = sums(r, valid, J, sigma, loss, front)
    A = normalization_map(nrm_pair)
    st = status_of(M, Q, nv)
    Sigma = A @ sandwich(M, Q) @ A.T if st == COV_OK else np.eye(6)
    return dict(M=M, Q=Q, g=g, num_valid=nv, status=st, covariance=Sigma, A=A)


# ---- calibration: does the reported covariance predict the spread of the estimate under image noise? ------------------------------------------
def se3_log(T):
    """The twist (omega, v) with twist_to_matrix(twist) = T, float64."""
    T = np.asarray(T, np.float64)
    R, t = T[:3, :3], T[:3, 3]
    w = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
    s = np.linalg.norm(w)
    theta = np.arctan2(s, 0.5 * (np.trace(R) - 1.0))
    omega = w * (theta / s) if s > 1e-12 else w
    W = skew(omega)
    k = 1.0 / 12.0 if theta < 1e-4 else (1.0 - theta * np.sin(theta) / (2.0 * (1.0 - np.cos(theta)))) / (theta * theta)
    V_inv = np.eye(3) - 0.5 * W + k * (W @ W)
    return np.concatenate([omega, V_inv @ t])


def noisy_frames(img, draws, sigma_grey=3.0, seed=0):
    """`draws` copies of a u8 image with N(0, sigma_grey) grey-level noise, rounded and clipped to u8 (np.random.default_rng(seed))."""
    rng = np.random.default_rng(seed)
    for _ in range(draws):
        yield np.clip(np.rint(img.astype(np.float64) + rng.normal(0.0, sigma_grey, img.shape)), 0, 255).astype(np.uint8)


def oracle_covariance(ctx, T, loss, level=0):
    """The definition evaluated in float64 on a context's own arrays (oracle or HIP library) at pose T: residuals, valid flags and the robust
    scale of a fresh linearisation there, the template's Jacobians and normalisation."""
    lin = ctx.linearize(0, 0, 1, level, T, reset_scale=True)
    return covariance(ctx.get_residuals(0), ctx.get_valid(0), ctx.get_jacobians(0, level), lin["sigma"], loss, ctx.get_normalization(0, level))


def calibration_ratio(ctx, d, cov_of, draws=150):
    """Per-axis ratio of the empirical standard deviation of the estimated pose over `draws` noisy copies of frame B to the mean reported one.
    ctx: a context with the template of frame A in slot 0; cov_of(ctx, T_est) -> (6x6 covariance, status) of the estimate just made on workspace 0.
    Returns (ratio [6], number of draws whose status was not OK)."""
    ctx.frame_set_data(1, d["imgB"], d["dispB"])
    T_ref, _ = ctx.estimate_pose(0, 0, 1)
    T_ref_inv = np.linalg.inv(np.asarray(T_ref, np.float64))
    eps, var, bad = [], [], 0
    for img in noisy_frames(d["imgB"], draws):
        ctx.frame_set_data(1, img, d["dispB"])
        T, _ = ctx.estimate_pose(0, 0, 1)
        S, st = cov_of(ctx, T)
        if st != COV_OK:
            bad += 1
            continue
        # T_true = T^ exp(eps): the spread of log(T^-1 T_ref) over the draws
        eps.append(se3_log(np.linalg.inv(np.asarray(T, np.float64)) @ np.linalg.inv(T_ref_inv)))
        var.append(np.diag(np.asarray(S, np.float64)))
    eps, var = np.array(eps), np.array(var)
    return eps.std(axis=0, ddof=1) / np.sqrt(var.mean(axis=0)), bad
