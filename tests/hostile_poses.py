"""Poses at which the warp's validity rule is decided by its edge cases, and the rule itself restated in numpy.

The rule is PhotoError::Impl::init (bpvo/photo_error.cc:344-363): x = normHomog(P.cast<double>() * X.cast<double>()) with the f32
P = K * T[0:3], Floor, valid = lo <= xi < W - hi && lo <= yi < R - 1.  There is no z > 0 test: a point behind the camera that projects into
the image is valid.  Floor is static_cast<int>, which on x86 (cvttsd2si) gives INT_MIN for NaN, infinities and everything beyond the int
range — never a valid pixel; the device code carries an explicit range test in its place (warp_rule.h, called from gn_warp.h,
gn_irls.h, kernels_gn_team.hip and kernels_gn.hip).  projectPoints (bpvo/project_points.cc:180-214), the all-f32 form that also serves
DisparitySpaceWarp, truncates instead of flooring, so x in (-1, 0) is a valid pixel 0 with a negative fraction.

poses(K, X, rows, cols) builds the named poses from a template's own points; PROPERTY names what each must exhibit there, and
check_property fails loudly when a case no longer has it (a change of the synthetic scenes, say).  Used by tests/test_hostile_poses_cpu.py
(the oracle against numpy), tests/test_warp_rule_cpu.py (warp_rule.h on the host against numpy) and tests/test_gpu_hostile_poses.py (every
device path against the oracle and numpy)."""
import numpy as np

# (rows, cols, pyramid levels): the size of the CPU re-derivations, and one at which xi and yi both pass 255 at level 0 (the tap-cache
# key packs yi << 16 | xi)
SIZES = {"96x128": (96, 128, 1), "264x328": (264, 328, 2)}

INT_RANGE = 2147483648.0

# what a case must exhibit (every name is a function of check_property's table)
PROPERTY = {
    "identity": ("all_valid", "some_on_integer_coordinates"),
    "half_turn_y": ("all_in_front", "partly_valid"),
    "all_behind": ("all_behind_and_valid",),
    "camera_in_plane": ("some_behind_some_in_front", "exactly_one_valid", "the_valid_are_behind"),
    "zero_depth": ("some_u_z_exactly_zero", "exactly_one_valid"),
    "tiny_depth": ("some_depths_below_1e-5", "no_u_z_exactly_zero", "exactly_one_valid"),
    "one_pixel_right": ("all_valid", "some_on_integer_coordinates"),
    "half_pixel_left": ("all_valid",),
    "nan": ("none_in_int_range",),
    "inf": ("none_in_int_range",),
    "overflow": ("none_in_int_range", "all_coordinates_finite_or_inf"),
    "x_in_minus_one_zero": ("chosen_x_in_minus_one_zero",),
    "y_in_minus_one_zero": ("chosen_y_in_minus_one_zero",),
    "right_edge": ("largest_valid_xi_is_W_minus_2", "some_floor_x_is_W_minus_1"),
}
# 264x328 keeps a quarter of the points (non-maximum suppression works there): the camera-in-the-plane cases leave 0 to 13 valid points
# rather than exactly one
PROPERTY_AT = {(264, 328): {
    "camera_in_plane": ("some_behind_some_in_front", "a_handful_valid_at_most"),
    "zero_depth": ("some_u_z_exactly_zero", "a_handful_valid_at_most"),
    "tiny_depth": ("some_depths_below_1e-5", "no_u_z_exactly_zero", "a_handful_valid_at_most"),
}}
CASES = list(PROPERTY)
NON_FINITE = ("nan", "inf", "overflow")
FINITE = [c for c in CASES if c not in NON_FINITE]
CHOSEN_AT = 0.4      # x_in_minus_one_zero / y_in_minus_one_zero: the chosen point lands at about -CHOSEN_AT


def chosen_point(X):
    """The index of the point the two (-1, 0) cases are built around."""
    return len(X) // 3


def projection_matrix(K, T):
    """RigidBodyWarp::setPose (bpvo/rigid_body_warp.h:111-114): P = K * T[0:3] in f32, index-order sums."""
    K = np.asarray(K, np.float32)
    T = np.asarray(T, np.float32)
    P = np.zeros((3, 4), np.float32)
    with np.errstate(all="ignore"):
        for r in range(3):
            for c in range(4):
                s = np.float32(K[r, 0] * T[0, c])
                s = np.float32(s + K[r, 1] * T[1, c])
                s = np.float32(s + K[r, 2] * T[2, c])
                P[r, c] = s
    return P


def np_homogeneous(K, T, X):
    """u = P.cast<double>() * X.cast<double>(), every row summed in index order as the fixed-size product does: [n, 3] f64."""
    P = projection_matrix(K, T).astype(np.float64)
    X = np.asarray(X, np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        u = P[:, 0][None, :] * X[:, 0:1]
        for k in (1, 2, 3):
            u = u + P[:, k][None, :] * X[:, k:k + 1]
    return u


def np_project(K, T, X):
    """The f64 projection of PhotoError::Impl::init with the f32 P = K * T[0:3]: (x, y) = normHomog(P X) = (u_x, u_y) * (1 / u_z)."""
    u = np_homogeneous(K, T, X)
    with np.errstate(all="ignore"):
        zi = 1.0 / u[:, 2]
        return zi * u[:, 0], zi * u[:, 1]


def np_floor(v):
    """Floor (bpvo/photo_error.cc:255-265) of the coordinates inside the int range, and which those are (NaN is not)."""
    v = np.asarray(v, np.float64)
    with np.errstate(invalid="ignore"):
        in_range = (v > -INT_RANGE) & (v < INT_RANGE)
    return np.floor(np.where(in_range, v, 0.0)).astype(np.int64), in_range


def np_valid(x, y, rows, cols, lo=0, hi=1):
    """The verdict: inside the int range, then lo <= xi < cols - hi && lo <= yi < rows - 1 on the floors ((0, 1): linear / cosine,
    (1, 3): cubic / Hermite; photo_error.cc:347-348)."""
    (xi, okx), (yi, oky) = np_floor(x), np_floor(y)
    return okx & oky & (xi >= lo) & (xi < cols - hi) & (yi >= lo) & (yi < rows - 1)


def _mul44(a, b):
    """Eigen's fixed 4x4 f32 product: every coefficient ((a0 b0 + a1 b1) + a2 b2) + a3 b3."""
    r = np.zeros((4, 4), np.float32)
    with np.errstate(all="ignore"):
        for i in range(4):
            for j in range(4):
                s = np.float32(a[i, 0] * b[0, j])
                for k in (1, 2, 3):
                    s = np.float32(s + a[i, k] * b[k, j])
                r[i, j] = s
    return r


def dspace_matrix(K, b, T):
    """DisparitySpaceWarp::setPose (bpvo/disparity_space_warp.h:36): H = G * T * G_inv in f32, left to right, G / G_inv as the constructor
    fills them (disparity_space_warp.cc:26-47); rows 0, 1, 3 of H."""
    K = np.asarray(K, np.float32)
    fx, fy, b = K[0, 0], K[1, 1], np.float32(b)
    G, Gi = np.zeros((4, 4), np.float32), np.zeros((4, 4), np.float32)
    G[0, 0], G[1, 1], G[2, 3], G[3, 2] = fx, fy, np.float32(fx * b), 1.0
    Gi[0, 0], Gi[1, 1], Gi[2, 3] = np.float32(1.0 / np.float64(fx)), np.float32(1.0 / np.float64(fy)), 1.0
    Gi[3, 2] = np.float32(1.0 / np.float64(np.float32(fx * b)))
    H = _mul44(_mul44(G, np.asarray(T, np.float32)), Gi)
    return H[[0, 1, 3]]


def np_project_f32(K, T, X, b=None):
    """projectPoints' scalar form (bpvo/project_points.cc:180-214) in f32: sequential sums, w = 1.0f / u_z, (x, y) = w * (u_x, u_y).
    b given: DisparitySpaceWarp::operator() (disparity_space_warp.h:66-71) on disparity-space points, + (cx, cy)."""
    K = np.asarray(K, np.float32)
    P = projection_matrix(K, T) if b is None else dspace_matrix(K, b, T)
    X = np.asarray(X, np.float32)
    with np.errstate(all="ignore"):
        u = []
        for r in range(3):
            s = P[r, 0] * X[:, 0]
            for k in (1, 2, 3):
                s = s + P[r, k] * X[:, k]
            assert s.dtype == np.float32
            u.append(s)
        w = np.float32(1.0) / u[2]
        x, y = w * u[0], w * u[1]
        if b is not None:
            x, y = x + K[0, 2], y + K[1, 2]
    assert x.dtype == np.float32 and y.dtype == np.float32
    return x, y


def np_trunc_f32(v):
    """(int) of an f32 coordinate inside the int range (cvttss2si: truncation), and which those are."""
    v = np.asarray(v, np.float32)
    with np.errstate(invalid="ignore"):
        in_range = (v > np.float32(-INT_RANGE)) & (v < np.float32(INT_RANGE))
    return np.trunc(np.where(in_range, v, np.float32(0))).astype(np.int64), in_range


def np_valid_f32(x, y, rows, cols):
    """projectPoints' verdict: 0 <= (int) x < cols - 1 && 0 <= (int) y < rows - 1 — x in (-1, 0) truncates to 0 and is valid."""
    (xi, okx), (yi, oky) = np_trunc_f32(x), np_trunc_f32(y)
    return okx & oky & (xi >= 0) & (xi < cols - 1) & (yi >= 0) & (yi < rows - 1)


def _translation(tx=0.0, ty=0.0, tz=0.0):
    T = np.eye(4, dtype=np.float32)
    T[:3, 3] = (tx, ty, tz)
    return T


def poses(K, X, rows, cols):
    """{name: 4x4 f32 pose} for a template's points X ([n, 4] f32, RigidBodyWarp's: get_points) and calibration K, in CASES' order."""
    K = np.asarray(K, np.float32)
    X = np.asarray(X, np.float32)
    fx, fy, cx, cy = (float(v) for v in (K[0, 0], K[1, 1], K[0, 2], K[1, 2]))
    Z = X[:, 2].astype(np.float64)
    n = len(X)
    out = {"identity": np.eye(4, dtype=np.float32)}
    T = np.diag([-1.0, 1.0, -1.0, 1.0]).astype(np.float32)      # half a turn about y, the plane kept in front
    T[2, 3] = 2.0 * Z.mean()
    out["half_turn_y"] = T
    out["all_behind"] = _translation(tz=-3.0 * Z.max())
    out["camera_in_plane"] = _translation(tz=-Z.mean())
    out["zero_depth"] = _translation(tz=-Z[n // 2])              # u_z = Z - Z[n/2]: exactly 0 wherever Z equals it (1/0, 0 * inf)
    out["tiny_depth"] = _translation(tz=-Z[n // 2] * (1.0 - 1e-7))
    out["one_pixel_right"] = _translation(tx=Z.mean() / fx)
    out["half_pixel_left"] = _translation(tx=-0.5 * Z.mean() / fx)
    T = np.eye(4, dtype=np.float32)
    T[0, 0] = np.nan
    out["nan"] = T
    T = np.eye(4, dtype=np.float32)
    T[0, 3] = np.inf
    out["inf"] = T
    T = np.eye(4, dtype=np.float32)
    T[:3, :3] *= np.float32(1e-30)
    T[0, 3] = 1e30
    out["overflow"] = T
    k = chosen_point(X)
    Xk, Yk, Zk = (float(v) for v in X[k, :3])
    out["x_in_minus_one_zero"] = _translation(tx=(-CHOSEN_AT - cx) * Zk / fx - Xk)
    out["y_in_minus_one_zero"] = _translation(ty=(-CHOSEN_AT - cy) * Zk / fy - Yk)
    # a whole-pixel shift (at the mean depth) to the right under which the image's last usable column W - 2 is reached by a valid point and
    # column W - 1 by an invalid one
    for px in range(1, 33):
        T = _translation(tx=px * Z.mean() / fx)
        x, y = np_project(K, T, X)
        xi = np_floor(x)[0]
        v = np_valid(x, y, rows, cols)
        if v.any() and xi[v].max() == cols - 2 and np.any(xi == cols - 1):
            out["right_edge"] = T
            break
    else:
        raise AssertionError("no whole-pixel shift up to 32 puts a valid point in column W - 2 and a point in column W - 1")
    assert list(out) == CASES
    return out


def properties_of(name, rows, cols):
    return PROPERTY_AT.get((rows, cols), {}).get(name, PROPERTY[name])


def check_property(name, K, T, X, rows, cols):
    """AssertionError unless the case `name` has every property PROPERTY names for it under pose T; returns a line for the log."""
    u = np_homogeneous(K, T, X)
    x, y = np_project(K, T, X)
    v = np_valid(x, y, rows, cols)
    (xi, okx), (yi, oky) = np_floor(x), np_floor(y)
    uz = u[:, 2]
    n = len(X)
    with np.errstate(invalid="ignore"):
        on_int = okx & oky & ((x == xi) | (y == yi))
        small = (np.abs(uz) > 0) & (np.abs(uz) < 1e-5)
    k = chosen_point(X)
    xf, yf = np_project_f32(K, T, X)
    table = {
        "all_valid": v.all(),
        "partly_valid": 0 < v.sum() < n,
        "all_in_front": np.all(uz > 0),
        "all_behind_and_valid": np.all(uz < 0) and v.all(),
        "some_behind_some_in_front": np.any(uz < 0) and np.any(uz > 0),
        "exactly_one_valid": v.sum() == 1,
        "a_handful_valid_at_most": v.sum() <= 16,
        "the_valid_are_behind": v.any() and np.all(uz[v] < 0),
        "some_u_z_exactly_zero": np.any(uz == 0.0),
        "no_u_z_exactly_zero": not np.any(uz == 0.0),
        "some_depths_below_1e-5": small.any(),
        "some_on_integer_coordinates": on_int.any(),
        "none_in_int_range": not np.any(okx & oky) and not v.any(),
        "all_coordinates_finite_or_inf": not np.any(np.isnan(x)),
        # the f64 rule rejects the chosen point (floor -1); the f32 form lands in (-1, 0) as well, truncates to 0 and accepts it
        "chosen_x_in_minus_one_zero": -1 < x[k] < 0 and -1 < xf[k] < 0 and not v[k] and np_valid_f32(xf, yf, rows, cols)[k],
        "chosen_y_in_minus_one_zero": -1 < y[k] < 0 and -1 < yf[k] < 0 and not v[k] and np_valid_f32(xf, yf, rows, cols)[k],
        "largest_valid_xi_is_W_minus_2": v.any() and xi[v].max() == cols - 2,
        "some_floor_x_is_W_minus_1": np.any(okx & (xi == cols - 1)),
    }
    for p in properties_of(name, rows, cols):
        assert table[p], (name, p, f"{rows}x{cols}", "valid", int(v.sum()), "of", n)
    return (f"{name}: {int(v.sum())} / {n} valid, {int(np.sum(uz < 0))} behind, {int(np.sum(uz == 0))} at u_z == 0, "
            f"{int(on_int.sum())} on an integer coordinate, {int(np.sum(~(okx & oky)))} outside the int range")


def interleaved(cases=CASES):
    """hostile, identity, hostile, ... and then the same list reversed: every case meets the tap cache the one before it left."""
    order = []
    for c in cases:
        if c != "identity":
            order += [c, "identity"]
    return order + order[::-1]
