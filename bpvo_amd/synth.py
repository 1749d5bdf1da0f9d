"""Deterministic synthetic stereo pairs for the dense-alignment hot path.

A textured plane is rendered analytically (ray/plane intersection, no resampling of a raster) from two camera
poses.  Frame A sits at the identity pose and also gets its disparity map ``b*fx/Z``; frame B is rendered from
``T_gt`` (X_B = T_gt * X_A), which is the pose ``estimatePose(A, B)`` has to recover
(reference convention: bpvo/rigid_body_warp.h:111-121, x_cur = K * T * X_ref).

Calibrations: 640x480 -> fx=fy=615, c=(320,240), b=0.1 (reference: apps/vo_example.cc:60-61);
1241x376 -> KITTI seq-00 style fx=fy=718.856, c=(607.1928,185.2157), b=0.5372.
Everything is seeded: seed = 1000 + pair index.

scene="layered" (every generator takes it; the default "plane" is the scene above, unchanged): a slanted background plane behind three
or four bounded planar patches at their own depths, ray-cast the same way (nearest hit inside a layer's bounds), each layer with its own
texture and brightness offset.  Its disparity maps carry holes (value-noise blobs and a band along every depth edge, filled with 0, -1
and 600), frame B carries sensor noise, and the pair also returns depthA, the layer label maps and the occlusion mask of A.
"""
from __future__ import annotations

import numpy as np

CALIB = {
    (480, 640): dict(fx=615.0, fy=615.0, cx=320.0, cy=240.0, b=0.1),
    (376, 1241): dict(fx=718.856, fy=718.856, cx=607.1928, cy=185.2157, b=0.5372),
}


def calibration(rows: int, cols: int):
    """(K 3x3 float32, baseline) for an image size; unknown sizes scale the 640x480 calibration."""
    if (rows, cols) in CALIB:
        c = CALIB[(rows, cols)]
    else:
        s = cols / 640.0
        c = dict(fx=615.0 * s, fy=615.0 * s, cx=cols / 2.0, cy=rows / 2.0, b=0.1)
    K = np.array([[c["fx"], 0, c["cx"]], [0, c["fy"], c["cy"]], [0, 0, 1]], dtype=np.float32)
    return K, float(c["b"])


def _hash01(ix, iy, salt):
    """Integer lattice -> [0,1) (splitmix64-style mixing, vectorised)."""
    x = (ix.astype(np.int64) * np.int64(0x1F123BB5) + iy.astype(np.int64) * np.int64(0x5F356495) + np.int64(salt)).astype(np.uint64)
    x ^= x >> np.uint64(30)
    x *= np.uint64(0xBF58476D1CE4E5B9)
    x ^= x >> np.uint64(27)
    x *= np.uint64(0x94D049BB133111EB)
    x ^= x >> np.uint64(31)
    return (x >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)


def _value_noise(u, v, cell, salt):
    """Bilinear value noise with lattice spacing `cell` (same units as u, v).

    The lattice hash is evaluated once on the bounding box of lattice nodes the image touches and gathered per pixel
    (identical values to hashing per pixel, ~4x faster for the 128-pair benchmark batches)."""
    fu, fv = u / cell, v / cell
    iu, iv = np.floor(fu), np.floor(fv)
    a, b = fu - iu, fv - iv
    iu, iv = iu.astype(np.int64), iv.astype(np.int64)
    u0, v0 = int(iu.min()), int(iv.min())
    gu, gv = np.meshgrid(np.arange(u0, int(iu.max()) + 2, dtype=np.int64), np.arange(v0, int(iv.max()) + 2, dtype=np.int64),
                         indexing="ij")
    table = _hash01(gu, gv, salt)
    ju, jv = iu - u0, iv - v0
    n00 = table[ju, jv]
    n10 = table[ju + 1, jv]
    n01 = table[ju, jv + 1]
    n11 = table[ju + 1, jv + 1]
    return (1 - b) * ((1 - a) * n00 + a * n10) + b * ((1 - a) * n01 + a * n11)


# lattice spacing in pixels at the plane's nominal depth, amplitude weight (sum 1)
OCTAVES = ((3.0, 0.30), (6.0, 0.25), (12.0, 0.20), (24.0, 0.15), (48.0, 0.10))


def _texture(u, v, seed, px_size):
    """Five octaves of value noise (lattice 3..48 px at the nominal depth), mapped to [16, 240].

    The fine octaves matter for the census-based descriptor: with only coarse (>= 8 px) bilinear cells the sign pattern of
    a 3x3 neighbourhood is constant inside a cell and the bit-planes carry almost no signal."""
    t = 0.0
    for k, (cell, wgt) in enumerate(OCTAVES):
        t = t + wgt * _value_noise(u, v, cell * px_size, seed * 7919 + 1 + k)
    return 16.0 + 224.0 * t


def twist_to_matrix(p):
    """SE(3) exponential, float64 (same formulas as bpvo/math_utils.h:140-168)."""
    p = np.asarray(p, dtype=np.float64)
    w, v = p[:3], p[3:]
    T = np.eye(4)
    th = np.linalg.norm(w)
    if th > 1e-8:
        a, b, ti = np.sin(th), 1 - np.cos(th), 1.0 / th
        S = ti * np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
        S2 = S @ S
        T[:3, :3] = np.eye(3) + a * S + b * S2
        T[:3, 3] = (np.eye(3) + b * ti * S + (th - a) * ti * S2) @ v
    else:
        T[:3, 3] = v
    return T


def _render(K, b, rows, cols, T_cam_from_A, seed, z0, plane):
    """Render the plane Z = z0 + a*X + b*Y (frame-A coordinates) seen from a camera with X_cam = T * X_A."""
    fx, fy, cx, cy = float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])
    pa, pb = plane
    n = np.array([-pa, -pb, 1.0])          # n . X_A = z0
    Tinv = np.linalg.inv(T_cam_from_A)
    R, t = Tinv[:3, :3], Tinv[:3, 3]       # X_A = R * X_cam + t
    xs, ys = np.meshgrid(np.arange(cols, dtype=np.float64), np.arange(rows, dtype=np.float64))
    d_cam = np.stack([(xs - cx) / fx, (ys - cy) / fy, np.ones_like(xs)], axis=-1)
    d_A = d_cam @ R.T
    denom = d_A @ n
    s = (z0 - float(n @ t)) / denom        # X_cam = s * d_cam, so depth in the camera frame = s
    X_A = s[..., None] * d_A + t
    px_size = z0 / fx                      # metres per pixel at the nominal depth
    img = _texture(X_A[..., 0], X_A[..., 1], seed, px_size)
    img = np.clip(np.rint(img), 0, 255).astype(np.uint8)
    disp = (b * fx / s).astype(np.float32)
    return img, disp


# ---- the layered scene ---------------------------------------------------------------------------------------------------------------
HOLE_VALUES = (0.0, -1.0, 600.0)          # what a hole of a layered disparity map holds (600 > maxValidDisparity = 512)
NOISE_SIGMA = 2.0                         # grey levels of sensor noise on frame B of a layered pair


def default_disp_range(rows: int, cols: int):
    """Front-surface disparities (px) of the layered scene: 15..96 at 1241x376 (below the stereo tests' 128), 3..30 at 640x480, in
    proportion to the width elsewhere."""
    if (rows, cols) == (376, 1241):
        return (15.0, 96.0)
    s = cols / 640.0
    return (3.0 * s, 30.0 * s)


def _layered_geometry(K, b, rows, cols, seed, disp_range):
    """The layers of one layered scene, drawn from a stream of their own (the pose stream stays make_pair's).  Layer 0 is the background
    plane Z = z + a X + b Y over the whole view; layers 1.. are patches Z = z + a (X - X0) + b (Y - Y0), bounded by a rectangle
    (|X - X0| <= hx, |Y - Y0| <= hy) or a disc ((X - X0)^2 + (Y - Y0)^2 <= r^2) in their own coordinates.  Patches 1 and 2 overlap in A."""
    rng = np.random.default_rng([seed, 0x1A7E])
    fx, fy, cx, cy = float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])
    bfx = b * fx
    lo, hi = disp_range
    layers = []
    # background: its farthest point over the view (A's corners) at disparity lo
    a, bb = rng.choice([-1.0, 1.0]) * rng.uniform(0.15, 0.3), rng.uniform(-0.1, 0.1)
    xs = np.array([-cx, cols - 1 - cx]) / fx
    ys = np.array([-cy, rows - 1 - cy]) / fy
    den_min = min(1.0 - a * x - bb * y for x in xs for y in ys)
    layers.append(dict(z=bfx / lo * den_min, a=a, b=bb, X0=0.0, Y0=0.0, shape="all"))
    n_patch = int(rng.integers(3, 5))
    # centre disparities: the nearest patch at ~0.88 hi, the others spread (log-uniformly) down to ~2.2 lo
    dl = np.exp(np.linspace(np.log(0.88 * hi), np.log(2.2 * lo), n_patch)) * rng.uniform(0.95, 1.05, n_patch)
    dl = dl[rng.permutation(n_patch)]
    area = rows * cols
    u1 = rng.uniform(0.3, 0.45) * cols
    for k in range(n_patch):
        frac = rng.uniform(0.08, 0.16)                     # share of frame A the patch's bounds would cover unoccluded
        if k == 0:
            uc, vc = u1, rng.uniform(0.4, 0.6) * rows
        elif k == 1:                                      # overlaps patch 1: centre shifted by about its half width
            uc, vc = layers[1]["uc"] + rng.choice([-1.0, 1.0]) * rng.uniform(0.12, 0.18) * cols, rng.uniform(0.3, 0.7) * rows
        else:
            uc, vc = rng.uniform(0.12, 0.88) * cols, rng.uniform(0.3, 0.7) * rows
        z = bfx / dl[k]
        X0, Y0 = (uc - cx) / fx * z, (vc - cy) / fy * z
        pa, pb = rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3)
        if rng.uniform() < 0.5:
            r_px = np.sqrt(frac * area / np.pi)
            geo = dict(shape="disc", r=r_px * z / fx)
        else:
            aspect = rng.uniform(0.6, 1.6)
            h_px = min(np.sqrt(frac * area / aspect), 0.8 * rows)
            w_px = frac * area / h_px
            geo = dict(shape="rect", hx=0.5 * w_px * z / fx, hy=0.5 * h_px * z / fy)
        layers.append(dict(z=z, a=pa, b=pb, X0=X0, Y0=Y0, uc=uc, **geo))
    offsets = rng.permutation(np.array([-40.0, -20.0, 0.0, 20.0, 40.0])[: n_patch + 1])
    for k, L in enumerate(layers):
        L["offset"] = float(offsets[k])
        L["tex_seed"] = 100000 + 16 * seed + k
    return layers


def _cast(K, layers, T_cam_from_A, xs, ys):
    """Cast the rays through pixels (xs, ys) of a camera with X_cam = T * X_A: depth of the nearest hit (inf where none), its layer label
    (-1 where none) and the hit in frame-A coordinates."""
    fx, fy, cx, cy = float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])
    Tinv = np.linalg.inv(T_cam_from_A)
    R, t = Tinv[:3, :3], Tinv[:3, 3]
    d_cam = np.stack([(xs - cx) / fx, (ys - cy) / fy, np.ones_like(xs)], axis=-1)
    d_A = d_cam @ R.T
    depth = np.full(xs.shape, np.inf)
    label = np.full(xs.shape, -1, np.int8)
    for k, L in enumerate(layers):
        n = np.array([-L["a"], -L["b"], 1.0])             # n . X_A = z - a X0 - b Y0
        c = L["z"] - L["a"] * L["X0"] - L["b"] * L["Y0"]
        with np.errstate(divide="ignore", invalid="ignore"):
            s = (c - float(n @ t)) / (d_A @ n)
        X = s[..., None] * d_A + t
        inside = s > 0
        if L["shape"] == "disc":
            inside &= (X[..., 0] - L["X0"]) ** 2 + (X[..., 1] - L["Y0"]) ** 2 <= L["r"] ** 2
        elif L["shape"] == "rect":
            inside &= (np.abs(X[..., 0] - L["X0"]) <= L["hx"]) & (np.abs(X[..., 1] - L["Y0"]) <= L["hy"])
        win = inside & (s < depth)
        depth = np.where(win, s, depth)
        label[win] = k
    X_A = depth[..., None] * d_A + t
    return depth, label, X_A


def _grid(rows, cols):
    return np.meshgrid(np.arange(cols, dtype=np.float64), np.arange(rows, dtype=np.float64))


def _shade(K, layers, depth, label, X_A):
    """Texture of every pixel from its own layer (texture coordinates = the hit's X, Y in frame A), plus the layer's brightness offset."""
    fx = float(K[0, 0])
    img = np.zeros(depth.shape)
    for k, L in enumerate(layers):
        m = label == k
        if m.any():
            img[m] = _texture(X_A[m, 0], X_A[m, 1], L["tex_seed"], L["z"] / fx) + L["offset"]
    return img


def _holes(disp, label, seed, salt):
    """Punch holes into a disparity map in place: value-noise blobs (6 % of the pixels) and a 2 px band along every label change (depth
    edge), filled with a per-pixel mix of HOLE_VALUES."""
    rows, cols = disp.shape
    xs, ys = _grid(rows, cols)
    blob = _value_noise(xs, ys, 0.05 * cols, seed * 7919 + salt) + 0.35 * _value_noise(xs, ys, 0.0125 * cols, seed * 7919 + salt + 1)
    hole = blob > np.quantile(blob, 0.94)
    dx = label[:, 1:] != label[:, :-1]
    dy = label[1:, :] != label[:-1, :]
    hole[:, 1:] |= dx
    hole[:, :-1] |= dx
    hole[1:, :] |= dy
    hole[:-1, :] |= dy
    pick = np.minimum((_hash01(xs, ys, seed * 7919 + salt + 2) * 3).astype(np.int64), 2)
    disp[hole] = np.asarray(HOLE_VALUES, np.float32)[pick[hole]]
    return disp


def _render_layered(K, b, rows, cols, T_cam_from_A, seed, layers, noise_stream=None, hole_salt=None):
    """One view of a layered scene: (u8 image, f32 disparity b*fx/depth, depth, labels, hits in frame A).  noise_stream: add Gaussian
    noise of NOISE_SIGMA grey levels from that RNG stream before rounding; hole_salt: punch holes into the disparity map."""
    xs, ys = _grid(rows, cols)
    depth, label, X_A = _cast(K, layers, T_cam_from_A, xs, ys)
    assert (label >= 0).all(), "the background plane covers every view"
    img = _shade(K, layers, depth, label, X_A)
    if noise_stream is not None:
        img = img + np.random.default_rng([seed, noise_stream]).normal(0.0, NOISE_SIGMA, img.shape)
    img = np.clip(np.rint(img), 0, 255).astype(np.uint8)
    disp = (b * float(K[0, 0]) / depth).astype(np.float32)
    if hole_salt is not None:
        _holes(disp, label, seed, hole_salt)
    return img, disp, depth, label, X_A


def _occluded(K, layers, T_gt, rows, cols, labelA, X_A):
    """A pixel of A is occluded when its 3-D point falls outside B or is hidden there: the ray of B through the point's exact (sub-pixel)
    projection first hits another layer."""
    fx, fy, cx, cy = float(K[0, 0]), float(K[1, 1]), float(K[0, 2]), float(K[1, 2])
    X_B = X_A @ T_gt[:3, :3].T + T_gt[:3, 3]
    with np.errstate(divide="ignore", invalid="ignore"):
        u = fx * X_B[..., 0] / X_B[..., 2] + cx
        v = fy * X_B[..., 1] / X_B[..., 2] + cy
    inside = (X_B[..., 2] > 0) & (u >= 0) & (u <= cols - 1) & (v >= 0) & (v <= rows - 1)
    _, lab_B, _ = _cast(K, layers, T_gt, np.where(inside, u, cx), np.where(inside, v, cy))
    return ~inside | (lab_B != labelA)


def _check_scene(scene):
    if scene not in ("plane", "layered"):
        raise ValueError(f"unknown scene {scene!r} (plane | layered)")


def make_pair(rows: int, cols: int, index: int = 0, max_rot: float = 0.01, max_trans: float = 0.05, scene: str = "plane", disp_range=None):
    """One synthetic pair. Returns dict(K, b, imgA, dispA, imgB, dispB, T_gt (float64 4x4), seed).  scene="layered": the layered scene
    (same T_gt for the same index), disparity front surfaces over disp_range (default_disp_range), with holes; the dict also holds depthA
    (float64), layerA, layerB (int8 labels, 0 = background) and occluded (bool, A's pixels whose point is hidden in B or falls outside it)."""
    seed = 1000 + int(index)
    rng = np.random.default_rng(seed)
    K, b = calibration(rows, cols)
    twist = np.concatenate([rng.uniform(-max_rot, max_rot, 3), rng.uniform(-max_trans, max_trans, 3)])
    T_gt = twist_to_matrix(twist)
    if scene == "layered":
        layers = _layered_geometry(K, b, rows, cols, seed, disp_range or default_disp_range(rows, cols))
        imgA, dispA, depthA, layerA, X_A = _render_layered(K, b, rows, cols, np.eye(4), seed, layers, hole_salt=11)
        imgB, dispB, _, layerB, _ = _render_layered(K, b, rows, cols, T_gt, seed, layers, noise_stream=1, hole_salt=23)
        occluded = _occluded(K, layers, T_gt, rows, cols, layerA, X_A)
        return dict(K=K, b=b, imgA=imgA, dispA=dispA, imgB=imgB, dispB=dispB, T_gt=T_gt, seed=seed, twist=twist, depthA=depthA,
                    layerA=layerA, layerB=layerB, occluded=occluded)
    _check_scene(scene)
    z0 = 10.0
    plane = (0.1, -0.15)
    imgA, dispA = _render(K, b, rows, cols, np.eye(4), seed, z0, plane)
    imgB, dispB = _render(K, b, rows, cols, T_gt, seed, z0, plane)
    return dict(K=K, b=b, imgA=imgA, dispA=dispA, imgB=imgB, dispB=dispB, T_gt=T_gt, seed=seed, twist=twist)


def make_stereo_pair(rows: int, cols: int, index: int = 0, z0: float = 10.0, scene: str = "plane", disp_range=None):
    """A rectified stereo pair of the plane scene: left image, right image (camera shifted by the baseline along +x), and the
    true disparity of the left image.  Returns dict(K, b, left, right, disp).  scene="layered": the layered scene of make_pair (z0 is
    not used; disp_range sets the depths), noise on the right image, disp without holes, plus layer (left labels) and occluded (left
    pixels hidden from the right camera or outside its view)."""
    seed = 1000 + int(index)
    K, b = calibration(rows, cols)
    if scene == "layered":
        layers = _layered_geometry(K, b, rows, cols, seed, disp_range or default_disp_range(rows, cols))
        T_right = np.eye(4)
        T_right[0, 3] = -b
        left, disp, _, layer, X_A = _render_layered(K, b, rows, cols, np.eye(4), seed, layers)
        right, _, _, _, _ = _render_layered(K, b, rows, cols, T_right, seed, layers, noise_stream=1)
        occluded = _occluded(K, layers, T_right, rows, cols, layer, X_A)
        return dict(K=K, b=b, left=left, right=right, disp=disp, seed=seed, layer=layer, occluded=occluded)
    _check_scene(scene)
    plane = (0.1, -0.15)
    left, disp = _render(K, b, rows, cols, np.eye(4), seed, z0, plane)
    T_right = np.eye(4)
    T_right[0, 3] = -b                     # X_right = X_left - (b, 0, 0)
    right, _ = _render(K, b, rows, cols, T_right, seed, z0, plane)
    return dict(K=K, b=b, left=left, right=right, disp=disp, seed=seed)


def make_sequence(rows: int, cols: int, n_frames: int, index: int = 0, step_rot: float = 0.004, step_trans: float = 0.03, scene: str = "plane",
                  disp_range=None, camera=None):
    """A short camera trajectory over the same plane for addFrame tests: list of (img, disp) and absolute poses.  scene="layered": over the
    layered scene of make_pair instead (the same trajectory), every disparity map with holes of its own, noise on every frame after the
    first.  camera=(K 3x3, baseline): render with that camera (disparity = fx * b / Z) instead of calibration(rows, cols)."""
    seed = 1000 + int(index)
    rng = np.random.default_rng(seed)
    if camera is None:
        K, b = calibration(rows, cols)
    else:
        K, b = np.asarray(camera[0], dtype=np.float32).reshape(3, 3), float(camera[1])
    if scene == "layered":
        layers = _layered_geometry(K, b, rows, cols, seed, disp_range or default_disp_range(rows, cols))
    else:
        _check_scene(scene)
    T = np.eye(4)
    frames, poses = [], []
    for f in range(n_frames):
        if scene == "layered":
            img, disp, _, _, _ = _render_layered(K, b, rows, cols, T, seed, layers, noise_stream=(f if f else None), hole_salt=11 + 12 * f)
        else:
            img, disp = _render(K, b, rows, cols, T, seed, 10.0, (0.1, -0.15))
        frames.append((img, disp))
        poses.append(T.copy())
        tw = np.concatenate([rng.uniform(-step_rot, step_rot, 3), rng.uniform(-step_trans, step_trans, 3)])
        T = twist_to_matrix(tw) @ T
    return dict(K=K, b=b, frames=frames, poses=poses)


def make_sequence_steps(rows: int, cols: int, steps, direction, rot, index: int = 0, extrinsics=None):
    """The plane scene along a trajectory of GIVEN steps (start-policy tests: an accelerating camera): len(steps) + 1 frames, frame k + 1 at
    twist_to_matrix((rot, steps[k] * direction)) @ T_k — a constant rotation step `rot` (3) and translation steps of steps[k] metres along
    `direction` (3, used as given).  Returns make_sequence's dict.  extrinsics: a list of 4x4 camera_from_body — the body follows that
    trajectory and the dict is make_rig_sequence's (frames [k][p], K and b per member, extrinsics)."""
    seed = 1000 + int(index)
    K, b = calibration(rows, cols)
    direction = np.asarray(direction, dtype=np.float64).reshape(3)
    rot = np.asarray(rot, dtype=np.float64).reshape(3)
    X = None if extrinsics is None else [np.asarray(x, dtype=np.float64).reshape(4, 4) for x in extrinsics]
    T = np.eye(4)
    frames, poses = [], []
    for f in range(len(steps) + 1):
        if X is None:
            frames.append(_render(K, b, rows, cols, T, seed, 10.0, (0.1, -0.15)))
        else:
            frames.append([_render(K, b, rows, cols, Xp @ T, seed, 10.0, (0.1, -0.15)) for Xp in X])
        poses.append(T.copy())
        if f < len(steps):
            T = twist_to_matrix(np.concatenate([rot, float(steps[f]) * direction])) @ T
    if X is None:
        return dict(K=K, b=b, frames=frames, poses=poses)
    return dict(K=[K] * len(X), b=[b] * len(X), frames=frames, poses=poses, extrinsics=X)


def make_rig_sequence(rows: int, cols: int, n_frames: int, extrinsics, index: int = 0, step_rot: float = 0.004, step_trans: float = 0.03, cameras=None):
    """make_sequence's plane seen by the cameras of a rigid rig: the body follows make_sequence's trajectory (poses[k] = T_k, body_k from
    body_0), member p with extrinsic extrinsics[p] (4x4 camera_from_body) is rendered from extrinsics[p] @ T_k.  cameras: None (every member
    calibration(rows, cols)) or per member (K 3x3, baseline, rows, cols).  Returns dict(K, b [per member], frames [k][p] = (img, disp),
    poses [k], extrinsics)."""
    seed = 1000 + int(index)
    rng = np.random.default_rng(seed)
    X = [np.asarray(x, dtype=np.float64).reshape(4, 4) for x in extrinsics]
    cams = []
    for p in range(len(X)):
        if cameras is None:
            K, b = calibration(rows, cols)
            cams.append((K, b, rows, cols))
        else:
            K, b, r, c = cameras[p]
            cams.append((np.asarray(K, dtype=np.float32).reshape(3, 3), float(b), int(r), int(c)))
    T = np.eye(4)
    frames, poses = [], []
    for f in range(n_frames):
        frames.append([_render(K, b, r, c, X[p] @ T, seed, 10.0, (0.1, -0.15)) for p, (K, b, r, c) in enumerate(cams)])
        poses.append(T.copy())
        tw = np.concatenate([rng.uniform(-step_rot, step_rot, 3), rng.uniform(-step_trans, step_trans, 3)])
        T = twist_to_matrix(tw) @ T
    return dict(K=[c[0] for c in cams], b=[c[1] for c in cams], frames=frames, poses=poses, extrinsics=X)


def make_stereo_sequence(rows: int, cols: int, n_frames: int, index: int = 0, step_rot: float = 0.004, step_trans: float = 0.03, camera=None):
    """make_sequence with the right image of every frame (the rig's right camera sits the baseline along +x of the left one):
    list of (left, right) and the true left disparities — input of the stereo front-end + addFrame.  camera=(K 3x3, baseline): as
    make_sequence's — both images rendered with that K, the right one that baseline away."""
    seq = make_sequence(rows, cols, n_frames, index, step_rot, step_trans, camera=camera)
    seed = 1000 + int(index)
    shift = np.eye(4)
    shift[0, 3] = -seq["b"]
    frames = []
    for (img, _disp), T in zip(seq["frames"], seq["poses"]):
        right, _ = _render(seq["K"], seq["b"], rows, cols, shift @ T, seed, 10.0, (0.1, -0.15))
        frames.append((img, right))
    return dict(K=seq["K"], b=seq["b"], frames=frames, disps=[f[1] for f in seq["frames"]], poses=seq["poses"])


def _pair_for_batch(args):
    rows, cols, idx, scene = args
    d = make_pair(rows, cols, idx, scene=scene)
    return d["imgA"], d["imgB"], d["dispA"], d["dispB"], d["T_gt"]


def make_batch(rows: int, cols: int, n_pairs: int, first_index: int = 0, workers: int = 1, scene: str = "plane"):
    """n_pairs pairs packed as the batch API wants them: images [2n, R, W] = A0,B0,A1,B1,..., disparities likewise.

    workers > 1 renders the pairs in a process pool (fork; call it before anything initialises the GPU).  scene: as make_pair's."""
    _check_scene(scene)
    imgs = np.empty((2 * n_pairs, rows, cols), dtype=np.uint8)
    disps = np.empty((2 * n_pairs, rows, cols), dtype=np.float32)
    T_gt = np.empty((n_pairs, 4, 4), dtype=np.float64)
    K, b = calibration(rows, cols)
    jobs = [(rows, cols, first_index + p, scene) for p in range(n_pairs)]
    if workers > 1 and n_pairs > 1:
        import multiprocessing as mp
        with mp.get_context("fork").Pool(min(workers, n_pairs)) as pool:
            results = pool.map(_pair_for_batch, jobs, chunksize=1)
    else:
        results = map(_pair_for_batch, jobs)
    for p, (ia, ib, da, db, tg) in enumerate(results):
        imgs[2 * p], imgs[2 * p + 1] = ia, ib
        disps[2 * p], disps[2 * p + 1] = da, db
        T_gt[p] = tg
    return dict(K=K, b=b, images=imgs, disparities=disps, T_gt=T_gt)
