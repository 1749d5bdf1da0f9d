"""ctypes view of the C ABI declared in include/bpvo_hip/c_api.h.

`Binding(lib_path, prefix)` is prefix-agnostic so that the tests can point the very same wrapper at a second library
with the same call shapes (the CPU checker used by tests/) and compare call by call; the product (`bpvo_amd.load()`)
only ever loads libbpvo_hip.so and raises if it is missing — there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

LOSS_HUBER, LOSS_TUKEY, LOSS_L2 = 0x10, 0x11, 0x12
LOSS_STUDENT_T = 0x13      # an extension (c_api.h): t-distribution weights, nu = 5, the scale fitted on the device; libbpvo_hip only
VERB_ITERATION, VERB_FINAL, VERB_SILENT, VERB_DEBUG = 0x20, 0x21, 0x22, 0x23
DESC_INTENSITY, DESC_GRADIENT, DESC_LAPLACIAN, DESC_BITPLANES = 0x30, 0x31, 0x36, 0x37
DESC_FIELDS1, DESC_FIELDS2, DESC_LATCH, DESC_CENTRAL_DIFFERENCE = 0x32, 0x33, 0x34, 0x35
GRAD_CD3, GRAD_CD5 = 0, 1
INTERP_LINEAR, INTERP_COSINE, INTERP_CUBIC, INTERP_CUBIC_HERMITE = 0, 1, 2, 3
STATUS_PARAMETER_TOL, STATUS_FUNCTION_TOL, STATUS_GRADIENT_TOL, STATUS_MAX_ITERATIONS, STATUS_SOLVER_ERROR = range(0x30, 0x35)
KF_LARGE_TRANSLATION, KF_LARGE_ROTATION, KF_SMALL_FRAC_GOOD, KF_NO_KEYFRAMING, KF_FIRST_FRAME = range(0x40, 0x45)
MAX_LEVELS = 8
TRACE_FLOATS = 68
STEREO_BM, STEREO_SGM, STEREO_SGBM = 0, 1, 2


class Params(C.Structure):
    """POD mirror of bpvo::AlgorithmParameters (reference: bpvo/types.h:171-413)."""
    _fields_ = [
        ("numPyramidLevels", C.c_int), ("minImageDimensionForPyramid", C.c_int),
        ("sigmaPriorToCensusTransform", C.c_float), ("sigmaBitPlanes", C.c_float),
        ("dfSigma1", C.c_float), ("dfSigma2", C.c_float),
        ("latchNumBytes", C.c_int), ("latchRotationInvariance", C.c_int), ("latchHalfSsdSize", C.c_int),
        ("centralDifferenceRadius", C.c_int),
        ("centralDifferenceSigmaBefore", C.c_float), ("centralDifferenceSigmaAfter", C.c_float),
        ("laplacianKernelSize", C.c_int), ("maxIterations", C.c_int),
        ("parameterTolerance", C.c_float), ("functionTolerance", C.c_float), ("gradientTolerance", C.c_float),
        ("relaxTolerancesForCoarseLevels", C.c_int), ("gradientEstimation", C.c_int), ("interp", C.c_int),
        ("lossFunction", C.c_int), ("descriptor", C.c_int), ("verbosity", C.c_int),
        ("minTranslationMagToKeyFrame", C.c_float), ("minRotationMagToKeyFrame", C.c_float),
        ("maxFractionOfGoodPointsToKeyFrame", C.c_float), ("goodPointThreshold", C.c_float),
        ("minNumPixelsForNonMaximaSuppression", C.c_int), ("nonMaxSuppRadius", C.c_int), ("minNumPixelsToWork", C.c_int),
        ("minSaliency", C.c_float), ("minValidDisparity", C.c_float), ("maxValidDisparity", C.c_float),
        ("maxTestLevel", C.c_int), ("withNormalization", C.c_int),
    ]


class Stats(C.Structure):
    _fields_ = [("numIterations", C.c_int), ("finalError", C.c_float), ("firstOrderOptimality", C.c_float), ("status", C.c_int)]


class Result(C.Structure):
    _fields_ = [("pose", C.c_float * 16), ("covariance", C.c_float * 36), ("optimizerStatistics", Stats * MAX_LEVELS),
                ("numLevels", C.c_int), ("isKeyFrame", C.c_int), ("keyFramingReason", C.c_int), ("hasPointCloud", C.c_int)]


COV_OK, COV_INDEFINITE, COV_DEGENERATE, COV_NONE = 0, 1, 2, 3
COV_GROUP = 64


class PoseCovariance(C.Structure):
    """bpvo_hip_pose_covariance (c_api.h): the robust sandwich covariance of an estimated pose."""
    _fields_ = [("T", C.c_float * 16), ("covariance", C.c_float * 36), ("sigma", C.c_float), ("num_valid", C.c_int), ("level", C.c_int),
                ("status", C.c_int)]


def _cov_dict(r: PoseCovariance):
    return dict(T=np.array(r.T, np.float32).reshape(4, 4), covariance=np.array(r.covariance, np.float32).reshape(6, 6), sigma=float(np.float32(r.sigma)),
                num_valid=int(r.num_valid), level=int(r.level), status=int(r.status))


class PoseScore(C.Structure):
    """bpvo_hip_pose_score (c_api.h): the truncated-L1 score of one candidate pose."""
    _fields_ = [("cost_sum", C.c_double), ("score", C.c_double), ("n_valid", C.c_int), ("n_below", C.c_int)]


# ... and the same 24 bytes as a numpy record, which is how Context.score_poses returns them
POSE_SCORE = np.dtype([("cost_sum", np.float64), ("score", np.float64), ("n_valid", np.int32), ("n_below", np.int32)])
assert POSE_SCORE.itemsize == C.sizeof(PoseScore) == 24

# the start policy (c_api.h: an extension, no reference member): where the addFrame drivers start Gauss-Newton
START_KEYFRAME_POSE, START_CONSTANT_VELOCITY, START_SCORED = 0, 1, 2
MAX_START_CANDIDATES, MAX_START_HINTS = 16, 13
START_KIND_IDENTITY, START_KIND_LAST_MOTION, START_KIND_LAST_MOTION_TWICE, START_KIND_HINT = 0, 1, 2, 3


class StartPolicy(C.Structure):
    """bpvo_hip_start_policy: mode (START_*), score_level (-1: the coarsest), tau (descriptor units; mode START_SCORED only)."""
    _fields_ = [("mode", C.c_int), ("score_level", C.c_int), ("tau", C.c_float)]


class StartInfo(C.Structure):
    """bpvo_hip_start_info: what an estimate of the last call started from."""
    _fields_ = [("n_candidates", C.c_int), ("chosen", C.c_int), ("kind", C.c_int * MAX_START_CANDIDATES), ("T_start", C.c_float * 16),
                ("scores", PoseScore * MAX_START_CANDIDATES)]


assert C.sizeof(StartPolicy) == 12 and C.sizeof(StartInfo) == 520


def start_policy(mode=START_KEYFRAME_POSE, score_level=-1, tau=0.0) -> StartPolicy:
    return StartPolicy(int(mode), int(score_level), float(tau))


def _start_info_dict(r: StartInfo):
    n = int(r.n_candidates)
    scores = np.frombuffer(bytes(r.scores), POSE_SCORE)[:n].copy()
    return dict(n_candidates=n, chosen=int(r.chosen), kind=[int(k) for k in r.kind[:n]], T_start=np.array(r.T_start, np.float32).reshape(4, 4),
                scores=scores)


class DisparityFusion(C.Structure):
    """bpvo_hip_disparity_fusion: mode (0 off, 1 on) and the filter's parameters, in disparity pixels (gate: standard deviations)."""
    _fields_ = [("mode", C.c_int), ("measurement_sigma", C.c_float), ("process_sigma", C.c_float), ("gate", C.c_float), ("max_fill_sigma", C.c_float)]


class DisparityFusionInfo(C.Structure):
    """bpvo_hip_disparity_fusion_info: the class counts of a sequence's last fusion, whether it predicted, the slot it wrote, the motion it used."""
    _fields_ = [("fused", C.c_uint32), ("replaced", C.c_uint32), ("measured", C.c_uint32), ("filled", C.c_uint32), ("none", C.c_uint32),
                ("predicted", C.c_int), ("slot", C.c_int), ("reserved_", C.c_int), ("motion", C.c_float * 16)]


def disparity_fusion(mode=1, measurement_sigma=0.0, process_sigma=0.0, gate=0.0, max_fill_sigma=0.0) -> DisparityFusion:
    return DisparityFusion(int(mode), float(measurement_sigma), float(process_sigma), float(gate), float(max_fill_sigma))


class MeasurementVariance(C.Structure):
    """bpvo_hip_measurement_variance: mode (0 off, 1 on), the window's radius, the pixel noise (grey levels) and the clamp (disparity pixels)."""
    _fields_ = [("mode", C.c_int), ("radius", C.c_int), ("noise_sigma", C.c_float), ("min_sigma", C.c_float), ("max_sigma", C.c_float)]


class MeasurementVarianceInfo(C.Structure):
    """bpvo_hip_measurement_variance_info: the class counts of a sequence's last measurement-variance map."""
    _fields_ = [("invalid", C.c_uint32), ("border", C.c_uint32), ("flat", C.c_uint32), ("floor", C.c_uint32), ("ceiling", C.c_uint32),
                ("model", C.c_uint32)]


VARIANCE_CLASSES = ("invalid", "border", "flat", "floor", "ceiling", "model")


def measurement_variance(mode=1, radius=0, noise_sigma=0.0, min_sigma=0.0, max_sigma=0.0) -> MeasurementVariance:
    return MeasurementVariance(int(mode), int(radius), float(noise_sigma), float(min_sigma), float(max_sigma))


class MotionStereo(C.Structure):
    """bpvo_hip_motion_stereo: mode (0 off, 1 on), the window's radius, the hypotheses on either side of the prior, the least gain (pixels per
    disparity pixel), the pixel noise (grey levels), the clamp (disparity pixels) and the gate (standard deviations)."""
    _fields_ = [("mode", C.c_int), ("radius", C.c_int), ("steps", C.c_int), ("min_gain", C.c_float), ("noise_sigma", C.c_float),
                ("min_sigma", C.c_float), ("max_sigma", C.c_float), ("gate", C.c_float)]


class MotionStereoInfo(C.Structure):
    """bpvo_hip_motion_stereo_info: the class counts of a sequence's last frame, whether a launch was made, the second view's slot, the motion Q."""
    _fields_ = [("no_prior", C.c_uint32), ("low_parallax", C.c_uint32), ("border", C.c_uint32), ("edge", C.c_uint32), ("flat", C.c_uint32),
                ("rejected", C.c_uint32), ("fused", C.c_uint32), ("launched", C.c_int), ("view_slot", C.c_int), ("reserved_", C.c_int * 3),
                ("motion", C.c_float * 16)]


MOTION_STEREO_CLASSES = ("no_prior", "low_parallax", "border", "edge", "flat", "rejected", "fused")


def motion_stereo(mode=1, radius=0, steps=0, min_gain=0.0, noise_sigma=0.0, min_sigma=0.0, max_sigma=0.0, gate=0.0) -> MotionStereo:
    return MotionStereo(int(mode), int(radius), int(steps), float(min_gain), float(noise_sigma), float(min_sigma), float(max_sigma), float(gate))


class Camera(C.Structure):
    """bpvo_hip_camera: one sequence's calibration and image size (bpvo_hip_create_sequences, bpvo_hip_seq_set_camera)."""
    _fields_ = [("K", C.c_float * 9), ("baseline", C.c_float), ("rows", C.c_int), ("cols", C.c_int)]


def camera(K, baseline, rows, cols) -> Camera:
    """A Camera from a 3x3 K (any float array), a baseline and an image size."""
    cam = Camera()
    cam.K[:] = [float(v) for v in np.asarray(K, dtype=np.float32).reshape(9)]
    cam.baseline, cam.rows, cam.cols = float(baseline), int(rows), int(cols)
    return cam


def _as_camera(c) -> Camera:
    return c if isinstance(c, Camera) else camera(*c)


class Lens(C.Structure):
    """bpvo_hip_lens: the raw camera of one side (intrinsics, Brown-Conrady k1 k2 p1 p2 k3 k4 k5 k6, the rotation raw -> rectified, the raw size)."""
    _fields_ = [("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double), ("dist", C.c_double * 8), ("R", C.c_double * 9),
                ("raw_rows", C.c_int), ("raw_cols", C.c_int)]


assert C.sizeof(Lens) == 21 * 8 + 2 * 4


def lens(K4, dist, R, raw_rows, raw_cols) -> Lens:
    """A Lens from (fx, fy, cx, cy), eight distortion coefficients, a 3x3 rotation and the raw image size."""
    q = Lens()
    q.fx, q.fy, q.cx, q.cy = [float(v) for v in K4]
    q.dist[:] = [float(v) for v in np.asarray(dist, dtype=np.float64).reshape(8)]
    q.R[:] = [float(v) for v in np.asarray(R, dtype=np.float64).reshape(9)]
    q.raw_rows, q.raw_cols = int(raw_rows), int(raw_cols)
    return q


def pack_frames(images, disps):
    """Frames of possibly different sizes back to back, as bpvo_hip_add_frames takes them: (u8 [sum of pixels], f32 [sum of pixels],
    [(rows, cols)] per frame)."""
    assert len(images) == len(disps), "one disparity per image"
    shapes = []
    for im, d in zip(images, disps):
        assert np.ndim(im) == 2 and np.shape(im) == np.shape(d), "frames are 2-D, image and disparity of one shape"
        shapes.append(tuple(int(v) for v in np.shape(im)))
    total = sum(r * w for r, w in shapes)
    img = np.empty(total, np.uint8)
    disp = np.empty(total, np.float32)
    at = 0
    for (r, w), im, d in zip(shapes, images, disps):
        img[at:at + r * w] = np.asarray(im, dtype=np.uint8).reshape(-1)
        disp[at:at + r * w] = np.asarray(d, dtype=np.float32).reshape(-1)
        at += r * w
    return img, disp, shapes


def pack_images(images):
    """u8 frames of possibly different sizes back to back (the left or the right images of a stereo call): (u8 [sum of pixels],
    [(rows, cols)] per frame) — pack_frames' layout without the disparities."""
    shapes = []
    for im in images:
        assert np.ndim(im) == 2, "frames are 2-D"
        shapes.append(tuple(int(v) for v in np.shape(im)))
    out = np.empty(sum(r * w for r, w in shapes), np.uint8)
    at = 0
    for (r, w), im in zip(shapes, images):
        out[at:at + r * w] = np.asarray(im, dtype=np.uint8).reshape(-1)
        at += r * w
    return out, shapes


def unpack_frames(img, disp, shapes):
    """pack_frames' inverse: lists of [rows, cols] arrays."""
    out_i, out_d, at = [], [], 0
    for r, w in shapes:
        out_i.append(np.asarray(img[at:at + r * w]).reshape(r, w))
        out_d.append(np.asarray(disp[at:at + r * w]).reshape(r, w))
        at += r * w
    return out_i, out_d


class StereoParams(C.Structure):
    """bpvo_hip_stereo_params: the CvStereoBMState fields the reference sets (utils/stereo_algorithm.cc:63-82)."""
    _fields_ = [("preFilterCap", C.c_int), ("SADWindowSize", C.c_int), ("minDisparity", C.c_int), ("numberOfDisparities", C.c_int),
                ("textureThreshold", C.c_int), ("uniquenessRatio", C.c_int),
                # StereoAlgorithm: 0 block matching, 1 SgmStereo (utils/sgm.h:33-46) with the fields below
                ("algorithm", C.c_int), ("sobelCapValue", C.c_int), ("censusRadius", C.c_int), ("windowRadius", C.c_int),
                ("smoothnessPenaltySmall", C.c_int), ("smoothnessPenaltyLarge", C.c_int), ("consistencyThreshold", C.c_int), ("reserved_", C.c_int),
                ("disparityFactor", C.c_double), ("censusWeightFactor", C.c_double),
                # StereoAlgorithm 2: cv::StereoSGBM (OpenCV 2.4) — its fields; it also reads minDisparity, numberOfDisparities, SADWindowSize,
                # preFilterCap, uniquenessRatio above
                ("P1", C.c_int), ("P2", C.c_int), ("disp12MaxDiff", C.c_int), ("speckleWindowSize", C.c_int), ("speckleRange", C.c_int), ("fullDP", C.c_int)]


class KernelStat(C.Structure):
    _fields_ = [("name", C.c_char * 48), ("launches", C.c_uint64), ("total_ms", C.c_double), ("units", C.c_double),
                ("bytes_per_unit", C.c_double)]


POINT_WITH_INFO = np.dtype([("xyzw", np.float32, 4), ("rgba", np.uint8, 4), ("weight", np.float32), ("pad", np.uint8, 8)])
assert POINT_WITH_INFO.itemsize == 32


class BpvoError(RuntimeError):
    """Non-zero status from the C ABI (the C++ facade maps the same statuses to bpvo::Error)."""


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


class Binding:
    def __init__(self, lib_path: str, prefix: str):
        if not os.path.exists(lib_path):
            raise FileNotFoundError(lib_path)
        self.lib = C.CDLL(lib_path)
        self.prefix = prefix
        self.path = lib_path

    def fn(self, name, restype=C.c_int):
        f = getattr(self.lib, self.prefix + name)
        f.restype = restype
        return f

    def has(self, name):
        return hasattr(self.lib, self.prefix + name)

    def debug_live_resources(self):
        """bpvo_hip_debug_live_resources: (device buffers, pinned buffers, streams, events) the library's contexts hold, process-wide."""
        counts = (C.c_int * 4)()
        rc = self.fn("debug_live_resources")(counts)
        if rc != 0:
            raise BpvoError(f"status {rc}")
        return tuple(counts)

    def default_params(self) -> Params:
        p = Params()
        self.fn("default_params", None)(C.byref(p))
        return p

    def create(self, K, baseline, rows, cols, params: Params, device=0, n_frames=3, n_pairs=1) -> "Context":
        return Context(self, K, baseline, rows, cols, params, device, n_frames, n_pairs)

    def create_sequences(self, cameras, params: Params, device=0) -> "Context":
        """bpvo_hip_create_sequences: a context for len(cameras) add_frames sequences, sequence s with cameras[s] (a Camera or
        (K, baseline, rows, cols))."""
        cams = (Camera * len(cameras))(*[_as_camera(c) for c in cameras])
        h = C.c_void_p()
        rc = self.fn("create_sequences")(C.byref(h), len(cameras), cams, C.byref(params), int(device))
        if rc != 0:
            msg = self.fn("last_error", C.c_char_p)(None)
            raise BpvoError(f"{self.prefix}create_sequences failed ({rc}): {msg.decode() if msg else ''}")
        S = len(cameras)
        return Context(self, None, None, max(c.rows for c in cams), max(c.cols for c in cams), params, device, 3 * S, S, handle=h)


class Context:
    """One bpvo_*_ctx. Methods mirror the C ABI one to one and return numpy arrays in the reference layouts."""

    def __init__(self, b: Binding, K, baseline, rows, cols, params, device, n_frames, n_pairs, handle=None):
        self.b = b
        self.h = C.c_void_p()
        self.rows, self.cols = int(rows), int(cols)
        if handle is not None:      # (Binding.create_sequences: the context exists already)
            self.h = handle
        else:
            Kf = _f32(K).reshape(9)
            rc = b.fn("create")(C.byref(self.h), Kf.ctypes.data_as(C.c_void_p), C.c_float(baseline), int(rows), int(cols),
                                C.byref(params), int(device), int(n_frames), int(n_pairs))
            if rc != 0:
                msg = b.fn("last_error", C.c_char_p)(None)
                raise BpvoError(f"{b.prefix}create failed ({rc}): {msg.decode() if msg else ''}")
        self.n_frames, self.n_pairs = n_frames, n_pairs
        self.L = b.fn("num_levels")(self.h)
        self.Cn = b.fn("num_channels")(self.h)

    def close(self):
        if self.h:
            self.b.fn("destroy", None)(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc):
        if rc != 0:
            msg = self.b.fn("last_error", C.c_char_p)(self.h)
            raise BpvoError(f"status {rc}: {msg.decode() if msg else ''}")

    def call(self, name, *args):
        self._ck(self.b.fn(name)(self.h, *args))

    def set_warp_formulation(self, mode):
        """0 = PhotoError f64 (active reference path, default), 1 = projectPoints / BilinearInterp all-f32 formulation,
        2 = DisparitySpaceWarp as the warp (+ the f32 interpolation); drops the templates when the warp changes."""
        self.call("set_warp_formulation", int(mode))

    # -- geometry
    def level_size(self, level):
        r, c = C.c_int(), C.c_int()
        self.call("level_size", int(level), C.byref(r), C.byref(c))
        return r.value, c.value

    # -- frames
    def frame_set_data(self, slot, img, disp):
        img = np.ascontiguousarray(img, dtype=np.uint8)
        disp = _f32(disp)
        assert img.shape == (self.rows, self.cols) and disp.shape == (self.rows, self.cols)
        self.call("frame_set_data", int(slot), img.ctypes.data_as(C.c_void_p), disp.ctypes.data_as(C.c_void_p))

    def frame_set_template(self, slot):
        self.call("frame_set_template", int(slot))

    def frame_clear(self, slot):
        self.call("frame_clear", int(slot))

    def frame_state(self, slot):
        a, b = C.c_int(), C.c_int()
        self.call("frame_state", int(slot), C.byref(a), C.byref(b))
        return bool(a.value), bool(b.value)

    def frames_set_data(self, first, stride, images, disps):
        images = np.ascontiguousarray(images, dtype=np.uint8)
        disps = _f32(disps)
        self.call("frames_set_data", int(first), int(stride), int(images.shape[0]), images.ctypes.data_as(C.c_void_p),
                  disps.ctypes.data_as(C.c_void_p), 0)

    def frames_set_data_device(self, first, stride, count, d_images_ptr, d_disps_ptr):
        self.call("frames_set_data", int(first), int(stride), int(count), C.c_void_p(d_images_ptr), C.c_void_p(d_disps_ptr), 1)

    def frames_set_template(self, first, stride, count):
        self.call("frames_set_template", int(first), int(stride), int(count))

    # -- accessors
    def get_image(self, slot, level):
        r, c = self.level_size(level)
        out = np.empty((r, c), np.uint8)
        self.call("get_image", int(slot), int(level), out.ctypes.data_as(C.c_void_p))
        return out

    def get_descriptor_channel(self, slot, level, ch):
        r, c = self.level_size(level)
        out = np.empty((r, c), np.float32)
        self.call("get_descriptor_channel", int(slot), int(level), int(ch), out.ctypes.data_as(C.c_void_p))
        return out

    def get_saliency(self, slot, level):
        r, c = self.level_size(level)
        out = np.empty((r, c), np.float32)
        self.call("get_saliency", int(slot), int(level), out.ctypes.data_as(C.c_void_p))
        return out

    def num_points(self, slot, level):
        n = C.c_int()
        self.call("num_points", int(slot), int(level), C.byref(n))
        return n.value

    def get_points(self, slot, level):
        out = np.empty((self.num_points(slot, level), 4), np.float32)
        self.call("get_points", int(slot), int(level), out.ctypes.data_as(C.c_void_p))
        return out

    def get_point_indices(self, slot, level):
        out = np.empty(self.num_points(slot, level), np.int32)
        self.call("get_point_indices", int(slot), int(level), out.ctypes.data_as(C.c_void_p))
        return out

    def get_pixels(self, slot, level):
        out = np.empty((self.Cn, self.num_points(slot, level)), np.float32)
        self.call("get_pixels", int(slot), int(level), out.ctypes.data_as(C.c_void_p))
        return out

    def get_jacobians(self, slot, level):
        out = np.empty((self.Cn, self.num_points(slot, level), 6), np.float32)
        self.call("get_jacobians", int(slot), int(level), out.ctypes.data_as(C.c_void_p))
        return out

    def get_normalization(self, slot, level):
        T, Ti = np.empty((4, 4), np.float32), np.empty((4, 4), np.float32)
        self.call("get_normalization", int(slot), int(level), T.ctypes.data_as(C.c_void_p), Ti.ctypes.data_as(C.c_void_p))
        return T, Ti

    # -- operator-level seam
    def linearize(self, ws, ref, cur, level, T, reset_scale=True):
        T = _f32(T).reshape(16)
        H, G = np.empty((6, 6), np.float32), np.empty(6, np.float32)
        f, s, nv = C.c_float(), C.c_float(), C.c_int()
        self.call("linearize", int(ws), int(ref), int(cur), int(level), T.ctypes.data_as(C.c_void_p), int(bool(reset_scale)),
                  H.ctypes.data_as(C.c_void_p), G.ctypes.data_as(C.c_void_p), C.byref(f), C.byref(s), C.byref(nv))
        return dict(H=H, G=G, f_norm=f.value, sigma=s.value, num_valid=nv.value)

    def linearize_at_scale(self, ws, ref, cur, level, T, sigma):
        """computeResiduals at T, then ComputeWeights / LinearSystemBuilder::Run with the GIVEN robust scale (HIP library only)."""
        T = _f32(T).reshape(16)
        H, G = np.empty((6, 6), np.float32), np.empty(6, np.float32)
        f, nv = C.c_float(), C.c_int()
        self.call("linearize_at_scale", int(ws), int(ref), int(cur), int(level), T.ctypes.data_as(C.c_void_p), C.c_float(sigma),
                  H.ctypes.data_as(C.c_void_p), G.ctypes.data_as(C.c_void_p), C.byref(f), C.byref(nv))
        return dict(H=H, G=G, f_norm=f.value, sigma=float(np.float32(sigma)), num_valid=nv.value)

    def _get_vec(self, name, ws, dtype):
        n = C.c_size_t()
        self.call(name, int(ws), None, C.byref(n))
        out = np.empty(n.value, dtype)
        self.call(name, int(ws), out.ctypes.data_as(C.c_void_p), C.byref(n))
        return out

    def get_residuals(self, ws=0):
        return self._get_vec("get_residuals", ws, np.float32)

    def get_valid(self, ws=0):
        return self._get_vec("get_valid", ws, np.uint16)

    def get_weights(self, ws=0):
        return self._get_vec("get_weights", ws, np.float32)

    def fraction_good(self, ws, thr):
        f = C.c_float()
        self.call("fraction_good", int(ws), C.c_float(thr), C.byref(f))
        return f.value

    # -- estimatePose
    def estimate_pose(self, ws, ref, cur, T_init=None):
        T0 = _f32(np.eye(4) if T_init is None else T_init).reshape(16)
        T = np.empty((4, 4), np.float32)
        st = (Stats * self.L)()
        self.call("estimate_pose", int(ws), int(ref), int(cur), T0.ctypes.data_as(C.c_void_p), T.ctypes.data_as(C.c_void_p), st)
        return T, [dict(numIterations=s.numIterations, finalError=s.finalError,
                        firstOrderOptimality=s.firstOrderOptimality, status=s.status) for s in st]

    def estimate_pose_trace(self, ws, ref, cur, T_init=None, max_records=4096):
        T0 = _f32(np.eye(4) if T_init is None else T_init).reshape(16)
        T = np.empty((4, 4), np.float32)
        st = (Stats * self.L)()
        rec = np.zeros((max_records, TRACE_FLOATS), np.float32)
        n = C.c_int()
        self.call("estimate_pose_trace", int(ws), int(ref), int(cur), T0.ctypes.data_as(C.c_void_p), T.ctypes.data_as(C.c_void_p),
                  st, rec.ctypes.data_as(C.c_void_p), int(max_records), C.byref(n))
        stats = [dict(numIterations=s.numIterations, finalError=s.finalError,
                      firstOrderOptimality=s.firstOrderOptimality, status=s.status) for s in st]
        return T, stats, rec[: min(n.value, max_records)]

    # -- VisualOdometry
    def add_frame(self, img, disp):
        img = np.ascontiguousarray(img, dtype=np.uint8)
        disp = _f32(disp)
        r = Result()
        self.call("add_frame", img.ctypes.data_as(C.c_void_p), disp.ctypes.data_as(C.c_void_p), C.byref(r))
        return dict(pose=np.array(r.pose, np.float32).reshape(4, 4), covariance=np.array(r.covariance, np.float32).reshape(6, 6),
                    stats=[dict(numIterations=s.numIterations, finalError=s.finalError,
                                firstOrderOptimality=s.firstOrderOptimality, status=s.status)
                           for s in r.optimizerStatistics[: r.numLevels]],
                    isKeyFrame=bool(r.isKeyFrame), keyFramingReason=r.keyFramingReason, hasPointCloud=bool(r.hasPointCloud))

    def default_stereo_params(self, ndisp=64):
        sp = StereoParams()
        self.b.fn("default_stereo_params", None)(C.byref(sp))
        sp.numberOfDisparities = int(ndisp)
        return sp

    def sgbm_params_from_config(self, minDisparity, numberOfDisparities, SADWindowSize=3, P1=0, P2=0, uniquenessRatio=0, speckleWindowSize=0,
                                speckleRange=0, fullDP=0):
        """bpvo_hip_stereo_params_sgbm_from_config: the struct the reference's StereoSGBM constructor call builds from the config KEYS."""
        sp = StereoParams()
        self.b.fn("stereo_params_sgbm_from_config", None)(C.byref(sp), int(minDisparity), int(numberOfDisparities), int(SADWindowSize), int(P1), int(P2),
                                                          int(uniquenessRatio), int(speckleWindowSize), int(speckleRange), int(fullDP))
        return sp

    def stereo_bm(self, left, right, sp):
        """StereoAlgorithm::run (block matching) on one pair or a stack [n, rows, cols]: f32 disparities, invalid = minDisparity - 1."""
        left = np.ascontiguousarray(left, dtype=np.uint8)
        right = np.ascontiguousarray(right, dtype=np.uint8)
        n = 1 if left.ndim == 2 else left.shape[0]
        out = np.empty(left.shape, np.float32)
        self.call("stereo_bm", n, left.ctypes.data_as(C.c_void_p), right.ctypes.data_as(C.c_void_p), 0, C.byref(sp), out.ctypes.data_as(C.c_void_p), 0)
        return out

    def stereo_bm_device(self, count, d_left_ptr, d_right_ptr, sp, d_disp_ptr):
        """StereoAlgorithm::run on `count` pairs already in device memory, f32 disparities written to device memory."""
        self.call("stereo_bm", int(count), C.c_void_p(d_left_ptr), C.c_void_p(d_right_ptr), 1, C.byref(sp), C.c_void_p(d_disp_ptr), 1)

    def add_frame_stereo(self, left, right, sp):
        left = np.ascontiguousarray(left, dtype=np.uint8)
        right = np.ascontiguousarray(right, dtype=np.uint8)
        r = Result()
        self.call("add_frame_stereo", left.ctypes.data_as(C.c_void_p), right.ctypes.data_as(C.c_void_p), C.byref(sp), C.byref(r))
        return self._result_dict(r)

    def add_frame_null(self):
        """addFrame(nullptr, nullptr) — must fail like THROW_ERROR_IF at bpvo/vo.cc:68-69."""
        r = Result()
        return self.b.fn("add_frame")(self.h, None, None, C.byref(r))

    def vo_num_points_at_level(self, level=-1):
        n = C.c_int()
        self.call("vo_num_points_at_level", int(level), C.byref(n))
        return n.value

    def vo_points_at_level(self, level=-1):
        out = np.empty((self.vo_num_points_at_level(level), 4), np.float32)
        self.call("vo_points_at_level", int(level), out.ctypes.data_as(C.c_void_p))
        return out

    def get_point_cloud(self):
        n = C.c_size_t()
        pose = np.empty((4, 4), np.float32)
        self.call("get_point_cloud", None, C.byref(n), pose.ctypes.data_as(C.c_void_p))
        pts = np.zeros(n.value, POINT_WITH_INFO)
        self.call("get_point_cloud", pts.ctypes.data_as(C.c_void_p), C.byref(n), pose.ctypes.data_as(C.c_void_p))
        return pts, pose

    def trajectory(self):
        n = C.c_int()
        self.call("trajectory_size", C.byref(n))
        out = np.empty((n.value, 4, 4), np.float32)
        if n.value:
            self.call("get_trajectory", out.ctypes.data_as(C.c_void_p))
        return out

    # -- many independent VisualOdometry sequences (bpvo_hip_add_frames)
    @staticmethod
    def _result_dict(r):
        return dict(pose=np.array(r.pose, np.float32).reshape(4, 4), covariance=np.array(r.covariance, np.float32).reshape(6, 6),
                    stats=[dict(numIterations=s.numIterations, finalError=s.finalError,
                                firstOrderOptimality=s.firstOrderOptimality, status=s.status)
                           for s in r.optimizerStatistics[: r.numLevels]],
                    isKeyFrame=bool(r.isKeyFrame), keyFramingReason=r.keyFramingReason, hasPointCloud=bool(r.hasPointCloud))

    @staticmethod
    def _seq_ids(n, seq):
        if seq is None:
            return None, None
        ids = np.ascontiguousarray(seq, dtype=np.int32).reshape(-1)
        assert ids.shape[0] == n, "one sequence id per frame"
        return ids, ids.ctypes.data_as(C.c_void_p)

    def add_frames(self, images, disps, seq=None):
        """Frame i of images [n, rows, cols] u8 / disps [n, rows, cols] f32 is the next frame of sequence seq[i] (None: 0 .. n-1);
        returns a list of n dicts in add_frame's format.  Sequences with cameras of their own (create_sequences, seq_set_camera): lists
        of 2-D arrays, frame i of its sequence's size, packed back to back (pack_frames)."""
        if isinstance(images, (list, tuple)):
            n = len(images)
            ids, p_ids = self._seq_ids(n, seq)
            for i in range(n):
                s = int(ids[i]) if ids is not None else i
                want = (self.rows, self.cols)
                if self.b.has("seq_get_camera") and 0 <= s < self.seq_capacity():
                    cam = self.seq_get_camera(s)
                    want = (cam.rows, cam.cols)
                assert np.shape(images[i]) == want, f"frame {i}: sequence {s} takes {want[0]}x{want[1]} frames"
            img, disp, _ = pack_frames(images, disps)
            res = (Result * n)()
            self.call("add_frames", n, p_ids, img.ctypes.data_as(C.c_void_p), disp.ctypes.data_as(C.c_void_p), 0, res)
            return [self._result_dict(r) for r in res]
        images = np.ascontiguousarray(images, dtype=np.uint8)
        disps = _f32(disps)
        n = images.shape[0]
        assert images.shape == (n, self.rows, self.cols) and disps.shape == images.shape
        ids, p_ids = self._seq_ids(n, seq)
        res = (Result * n)()
        self.call("add_frames", n, p_ids, images.ctypes.data_as(C.c_void_p), disps.ctypes.data_as(C.c_void_p), 0, res)
        return [self._result_dict(r) for r in res]

    def add_frames_device(self, n, d_images_ptr, d_disps_ptr, seq=None):
        """add_frames with the n images / disparities already in device memory (contiguous [n][rows*cols]; sequences with cameras of their
        own: frame i of its sequence's size, the frames back to back as pack_frames lays them out)."""
        ids, p_ids = self._seq_ids(n, seq)
        res = (Result * n)()
        self.call("add_frames", int(n), p_ids, C.c_void_p(d_images_ptr), C.c_void_p(d_disps_ptr), 1, res)
        return [self._result_dict(r) for r in res]

    # -- the stereo front-end for many cameras (bpvo_hip_stereo_frames, bpvo_hip_add_frames_stereo)
    @staticmethod
    def _camera_array(cams_or_sizes):
        """Cameras, (K, baseline, rows, cols) tuples or bare (rows, cols) sizes -> a ctypes array (the stereo front-end reads rows / cols only)."""
        if isinstance(cams_or_sizes, C.Array):      # (one made earlier: a caller that times the call builds it once)
            return cams_or_sizes
        out = (Camera * len(cams_or_sizes))()
        for i, c in enumerate(cams_or_sizes):
            if isinstance(c, Camera):
                out[i] = c
            elif len(c) == 2:
                out[i] = camera(np.eye(3), 1.0, c[0], c[1])
            else:
                out[i] = camera(*c)
        return out

    def stereo_frames(self, cams_or_sizes, lefts, rights, sp):
        """bpvo_hip_stereo_frames: pair i (2-D u8 arrays lefts[i], rights[i]) has the size of cams_or_sizes[i] (a Camera, a (K, baseline, rows,
        cols) tuple or a bare (rows, cols)); returns the list of f32 disparity maps, each of its pair's shape."""
        n = len(cams_or_sizes)
        assert len(lefts) == n and len(rights) == n, "one pair per camera"
        cams = self._camera_array(cams_or_sizes)
        for i in range(n):
            want = (cams[i].rows, cams[i].cols)
            assert np.shape(lefts[i]) == want and np.shape(rights[i]) == want, f"pair {i}: camera {i} takes {want[0]}x{want[1]} images"
        left, shapes = pack_images(lefts)
        right, _ = pack_images(rights)
        out = np.empty(left.size, np.float32)
        self.call("stereo_frames", n, cams, left.ctypes.data_as(C.c_void_p), right.ctypes.data_as(C.c_void_p), 0, C.byref(sp), out.ctypes.data_as(C.c_void_p), 0)
        maps, at = [], 0
        for r, w in shapes:
            maps.append(out[at:at + r * w].reshape(r, w))
            at += r * w
        return maps

    def stereo_frames_device(self, cams_or_sizes, d_left_ptr, d_right_ptr, sp, d_disp_ptr):
        """stereo_frames with the packed images already in device memory, the packed f32 maps written to device memory."""
        cams = self._camera_array(cams_or_sizes)
        self.call("stereo_frames", len(cams), cams, C.c_void_p(d_left_ptr), C.c_void_p(d_right_ptr), 1, C.byref(sp), C.c_void_p(d_disp_ptr), 1)

    def add_frames_stereo(self, lefts, rights, sp, seq=None):
        """bpvo_hip_add_frames_stereo: pair i (2-D u8 arrays, or stacks [n, rows, cols]) is the next frame of sequence seq[i] (None: 0 .. n-1),
        of that sequence's camera size; the disparities are computed on the device.  Returns n dicts in add_frame's format."""
        n = len(lefts)
        assert len(rights) == n, "one right image per left image"
        ids, p_ids = self._seq_ids(n, seq)
        for i in range(n):
            s = int(ids[i]) if ids is not None else i
            if 0 <= s < self.seq_capacity():
                cam = self.seq_get_camera(s)
                want = (cam.rows, cam.cols)
                assert np.shape(lefts[i]) == want and np.shape(rights[i]) == want, f"pair {i}: sequence {s} takes {want[0]}x{want[1]} images"
        left, _ = pack_images(lefts)
        right, _ = pack_images(rights)
        res = (Result * n)()
        self.call("add_frames_stereo", n, p_ids, left.ctypes.data_as(C.c_void_p), right.ctypes.data_as(C.c_void_p), 0, C.byref(sp), res)
        return [self._result_dict(r) for r in res]

    def add_frames_stereo_device(self, n, d_left_ptr, d_right_ptr, sp, seq=None):
        """add_frames_stereo with the n packed pairs already in device memory."""
        ids, p_ids = self._seq_ids(n, seq)
        res = (Result * n)()
        self.call("add_frames_stereo", int(n), p_ids, C.c_void_p(d_left_ptr), C.c_void_p(d_right_ptr), 1, C.byref(sp), res)
        return [self._result_dict(r) for r in res]

    # -- rectification on the device (c_api.h): seq None = the context's own camera
    def set_rectification(self, side, lens_, seq=None):
        """bpvo_hip_(seq_)set_rectification: the map of a side (0 left, 1 right) from a Lens."""
        if seq is None:
            self.call("set_rectification", int(side), C.byref(lens_))
        else:
            self.call("seq_set_rectification", int(seq), int(side), C.byref(lens_))

    def set_rectification_maps(self, side, raw_rows, raw_cols, mapx, mapy, seq=None):
        """bpvo_hip_(seq_)set_rectification_maps: the map of a side from the caller's f32 maps of the camera's size."""
        mapx, mapy = _f32(mapx), _f32(mapy)
        assert mapx.shape == mapy.shape
        args = (int(side), int(raw_rows), int(raw_cols), mapx.ctypes.data_as(C.c_void_p), mapy.ctypes.data_as(C.c_void_p))
        if seq is None:
            self.call("set_rectification_maps", *args)
        else:
            self.call("seq_set_rectification_maps", int(seq), *args)

    def clear_rectification(self, seq=None):
        if seq is None:
            self.call("clear_rectification")
        else:
            self.call("seq_clear_rectification", int(seq))

    def rectification_info(self, side, seq=None):
        """(raw_rows, raw_cols, outside_pixels) of a side's rectification."""
        r, w, o = C.c_int(), C.c_int(), C.c_uint64()
        if seq is None:
            self.call("rectification_info", int(side), C.byref(r), C.byref(w), C.byref(o))
        else:
            self.call("seq_rectification_info", int(seq), int(side), C.byref(r), C.byref(w), C.byref(o))
        return r.value, w.value, o.value

    def rectify_counts(self):
        """bpvo_hip_rectify_counts: (launches, destination pixels) so far."""
        a, b = C.c_uint64(), C.c_uint64()
        self.call("rectify_counts", C.byref(a), C.byref(b))
        return a.value, b.value

    def _rect_out_shapes(self, n, seq):
        if seq is None:
            return [(self.rows, self.cols)] * n
        return [(cam.rows, cam.cols) for cam in (self.seq_get_camera(int(s)) for s in seq)]

    def rectify_frames(self, raws, side, seq=None):
        """bpvo_hip_rectify_frames, host to host: raws[i] (2-D u8, the raw size of seq[i]'s side; seq None: the context's own camera) -> the list of
        rectified images, each of its camera's size."""
        n = len(raws)
        ids, p_ids = self._seq_ids(n, seq)
        raw, _ = pack_images(raws)
        shapes = self._rect_out_shapes(n, ids)
        out = np.empty(sum(r * w for r, w in shapes), np.uint8)
        self.call("rectify_frames", n, p_ids, int(side), raw.ctypes.data_as(C.c_void_p), 0, out.ctypes.data_as(C.c_void_p), 0)
        imgs, at = [], 0
        for r, w in shapes:
            imgs.append(out[at:at + r * w].reshape(r, w))
            at += r * w
        return imgs

    def rectify_frames_ptr(self, n, side, raw_ptr, raw_on_device, out_ptr, out_on_device, seq=None):
        """bpvo_hip_rectify_frames on packed buffers given by address, each in host or device memory."""
        ids, p_ids = self._seq_ids(n, seq)
        self.call("rectify_frames", int(n), p_ids, int(side), C.c_void_p(raw_ptr), int(bool(raw_on_device)), C.c_void_p(out_ptr), int(bool(out_on_device)))

    def add_frames_stereo_raw(self, lefts, rights, sp, seq=None):
        """bpvo_hip_add_frames_stereo_raw: raw pair i (2-D u8 arrays of the raw sizes of sequence seq[i]'s sides; None: 0 .. n-1) is rectified on the
        device and becomes the next frame of its sequence.  Returns n dicts in add_frame's format."""
        n = len(lefts)
        assert len(rights) == n, "one right image per left image"
        ids, p_ids = self._seq_ids(n, seq)
        left, _ = pack_images(lefts)
        right, _ = pack_images(rights)
        res = (Result * n)()
        self.call("add_frames_stereo_raw", n, p_ids, left.ctypes.data_as(C.c_void_p), right.ctypes.data_as(C.c_void_p), 0, C.byref(sp), res)
        return [self._result_dict(r) for r in res]

    def add_frames_stereo_raw_device(self, n, d_left_ptr, d_right_ptr, sp, seq=None):
        """add_frames_stereo_raw with the n packed raw pairs already in device memory."""
        ids, p_ids = self._seq_ids(n, seq)
        res = (Result * n)()
        self.call("add_frames_stereo_raw", int(n), p_ids, C.c_void_p(d_left_ptr), C.c_void_p(d_right_ptr), 1, C.byref(sp), res)
        return [self._result_dict(r) for r in res]

    def add_frame_stereo_raw(self, left, right, sp):
        """bpvo_hip_add_frame_stereo_raw: the context's own camera, a raw pair from host memory."""
        left = np.ascontiguousarray(left, dtype=np.uint8)
        right = np.ascontiguousarray(right, dtype=np.uint8)
        r = Result()
        self.call("add_frame_stereo_raw", left.ctypes.data_as(C.c_void_p), right.ctypes.data_as(C.c_void_p), C.byref(sp), C.byref(r))
        return self._result_dict(r)

    def seq_capacity(self):
        n = C.c_int()
        self.call("seq_capacity", C.byref(n))
        return n.value

    def seq_reset(self, s):
        self.call("seq_reset", int(s))

    def seq_set_camera(self, s, cam):
        """bpvo_hip_seq_set_camera: cam is a Camera or (K, baseline, rows, cols); only while sequence s holds no frame."""
        cam = _as_camera(cam)
        self.call("seq_set_camera", int(s), C.byref(cam))

    def seq_set_params(self, s, params: Params):
        """bpvo_hip_seq_set_params: sequence s runs with its own Params (loss, iteration limit, tolerances, key-frame thresholds, minSaliency,
        disparity gate); only while it holds no frame."""
        self.call("seq_set_params", int(s), C.byref(params))

    def seq_get_params(self, s) -> Params:
        p = Params()
        self._ck(self.b.fn("seq_get_params")(self.h, int(s), C.byref(p)))
        return p

    # -- normalised intensity (an extension: no reference member)
    def set_intensity_normalization(self, radius):
        """bpvo_hip_set_intensity_normalization: -1 off (the default), 0 whole image (median / MAD), 1 .. 15 local ((2 R + 1)^2 window); only
        on an Intensity context and while no frame slot holds data."""
        self.call("set_intensity_normalization", int(radius))

    def get_intensity_normalization(self):
        r = C.c_int()
        self._ck(self.b.fn("get_intensity_normalization")(self.h, C.byref(r)))
        return int(r.value)

    # -- point budget (an extension: no reference member)
    @staticmethod
    def _budget_arg(max_points):
        mp = [int(k) for k in (max_points if max_points is not None else [])]
        return ((C.c_int * len(mp))(*mp) if mp else None), len(mp)

    def set_point_budget(self, max_points):
        """bpvo_hip_set_point_budget: at most max_points[l] template points at level l, the most salient first (0 / levels beyond the list: no
        budget); from the next set_template on."""
        arr, n = self._budget_arg(max_points)
        self.call("set_point_budget", arr, n)

    def get_point_budget(self):
        out = (C.c_int * MAX_LEVELS)()
        self._ck(self.b.fn("get_point_budget")(self.h, out))
        return [int(v) for v in out][:self.L]

    def seq_set_point_budget(self, s, max_points):
        """bpvo_hip_seq_set_point_budget: sequence s's own budget in the place of the context's; an empty list returns it to the context's."""
        arr, n = self._budget_arg(max_points)
        self.call("seq_set_point_budget", int(s), arr, n)

    def seq_get_point_budget(self, s):
        """(budget per level, True if it is the sequence's own)"""
        out, own = (C.c_int * MAX_LEVELS)(), C.c_int()
        self._ck(self.b.fn("seq_get_point_budget")(self.h, int(s), out, C.byref(own)))
        return [int(v) for v in out][:self.L], bool(own.value)

    def selection_info(self, slot, level):
        """bpvo_hip_get_selection_info: dict(n_candidates, threshold, n_ties_kept) of the slot's template at `level`."""
        n, t, k = C.c_int(), C.c_float(), C.c_int()
        self.call("get_selection_info", int(slot), int(level), C.byref(n), C.byref(t), C.byref(k))
        return dict(n_candidates=n.value, threshold=np.float32(t.value), n_ties_kept=k.value)

    def seq_get_camera(self, s) -> Camera:
        cam = Camera()
        self._ck(self.b.fn("seq_get_camera")(self.h, int(s), C.byref(cam)))
        return cam

    def seq_num_points_at_level(self, s, level=-1):
        n = C.c_int()
        self.call("seq_num_points_at_level", int(s), int(level), C.byref(n))
        return n.value

    def seq_point_cloud(self, s):
        n = C.c_size_t()
        pose = np.empty((4, 4), np.float32)
        self.call("seq_get_point_cloud", int(s), None, C.byref(n), pose.ctypes.data_as(C.c_void_p))
        pts = np.zeros(n.value, POINT_WITH_INFO)
        self.call("seq_get_point_cloud", int(s), pts.ctypes.data_as(C.c_void_p), C.byref(n), pose.ctypes.data_as(C.c_void_p))
        return pts, pose

    def seq_trajectory(self, s):
        n = C.c_int()
        self.call("seq_trajectory_size", int(s), C.byref(n))
        out = np.empty((n.value, 4, 4), np.float32)
        if n.value:
            self.call("seq_get_trajectory", int(s), out.ctypes.data_as(C.c_void_p))
        return out

    # -- rig mode: the cameras of a rigid rig estimated as one body pose (bpvo_hip_*_rig)
    @staticmethod
    def _rig_members(wss, refs, curs, X):
        w = np.ascontiguousarray(wss, dtype=np.int32).reshape(-1)
        r = np.ascontiguousarray(refs, dtype=np.int32).reshape(-1)
        c = np.ascontiguousarray(curs, dtype=np.int32).reshape(-1)
        Xf = _f32(X).reshape(-1, 16)
        assert r.shape == w.shape and c.shape == w.shape and Xf.shape[0] == w.shape[0], "one template, current frame and extrinsic per member"
        return w, r, c, Xf

    def linearize_rig(self, wss, refs, curs, X, level, T_body, reset_scale=True):
        """bpvo_hip_linearize_rig: the joint normal equations of the members (workspace wss[i], template refs[i], current curs[i], extrinsic
        X[i] camera_from_body) at the body pose T_body; T_members: the member poses the kernels were run at."""
        w, r, c, Xf = self._rig_members(wss, refs, curs, X)
        n = w.shape[0]
        T = _f32(T_body).reshape(16)
        H, G, Tm = np.empty((6, 6), np.float32), np.empty(6, np.float32), np.empty((n, 4, 4), np.float32)
        f, nv = C.c_float(), C.c_int()
        self.call("linearize_rig", n, w.ctypes.data_as(C.c_void_p), r.ctypes.data_as(C.c_void_p), c.ctypes.data_as(C.c_void_p),
                  Xf.ctypes.data_as(C.c_void_p), int(level), T.ctypes.data_as(C.c_void_p), int(bool(reset_scale)), H.ctypes.data_as(C.c_void_p),
                  G.ctypes.data_as(C.c_void_p), C.byref(f), C.byref(nv), Tm.ctypes.data_as(C.c_void_p))
        return dict(H=H, G=G, f_norm=f.value, num_valid=nv.value, T_members=Tm)

    def estimate_pose_rig(self, wss, refs, curs, X, T_init=None):
        """bpvo_hip_estimate_pose_rig: (body pose, per-level statistics of the joint system)."""
        w, r, c, Xf = self._rig_members(wss, refs, curs, X)
        T0 = _f32(np.eye(4) if T_init is None else T_init).reshape(16)
        T = np.empty((4, 4), np.float32)
        st = (Stats * self.L)()
        self.call("estimate_pose_rig", w.shape[0], w.ctypes.data_as(C.c_void_p), r.ctypes.data_as(C.c_void_p), c.ctypes.data_as(C.c_void_p),
                  Xf.ctypes.data_as(C.c_void_p), T0.ctypes.data_as(C.c_void_p), T.ctypes.data_as(C.c_void_p), st)
        return T, [dict(numIterations=s.numIterations, finalError=s.finalError,
                        firstOrderOptimality=s.firstOrderOptimality, status=s.status) for s in st]

    def rig_set(self, X, seq=None):
        """bpvo_hip_rig_set: the rig's members are sequences seq (None: 0 .. n-1) with extrinsics X [n, 4, 4] (camera_from_body)."""
        Xf = _f32(X).reshape(-1, 16)
        ids, p_ids = self._seq_ids(Xf.shape[0], seq)
        self.call("rig_set", Xf.shape[0], p_ids, Xf.ctypes.data_as(C.c_void_p))

    def rig_get(self):
        """(sequence ids [n], extrinsics [n, 4, 4]) of the declared rig; n = 0: none."""
        n = C.c_int()
        self._ck(self.b.fn("rig_get")(self.h, C.byref(n), None, None))
        ids, X = np.empty(n.value, np.int32), np.empty((n.value, 4, 4), np.float32)
        if n.value:
            self._ck(self.b.fn("rig_get")(self.h, C.byref(n), ids.ctypes.data_as(C.c_void_p), X.ctypes.data_as(C.c_void_p)))
        return ids, X

    def add_frames_rig(self, images, disps):
        """bpvo_hip_add_frames_rig: the next frame of every member (lists of 2-D arrays in member order, each of its camera's size, or stacks
        [n, rows, cols]); returns the body's result in add_frame's format."""
        ids, _ = self.rig_get()
        assert len(images) == len(ids), f"the rig has {len(ids)} members"
        for i, s in enumerate(ids):
            cam = self.seq_get_camera(int(s))
            assert np.shape(images[i]) == (cam.rows, cam.cols), f"frame {i}: member {i} (sequence {s}) takes {cam.rows}x{cam.cols} frames"
        img, disp, _ = pack_frames(list(images), list(disps))
        r = Result()
        self.call("add_frames_rig", img.ctypes.data_as(C.c_void_p), disp.ctypes.data_as(C.c_void_p), 0, C.byref(r))
        return self._result_dict(r)

    def add_frames_rig_device(self, d_images_ptr, d_disps_ptr):
        """add_frames_rig with the packed frames already in device memory."""
        r = Result()
        self.call("add_frames_rig", C.c_void_p(d_images_ptr), C.c_void_p(d_disps_ptr), 1, C.byref(r))
        return self._result_dict(r)

    def rig_trajectory(self):
        n = C.c_int()
        self.call("rig_trajectory_size", C.byref(n))
        out = np.empty((n.value, 4, 4), np.float32)
        if n.value:
            self.call("rig_get_trajectory", out.ctypes.data_as(C.c_void_p))
        return out

    # -- several rigs in one context (bpvo_hip_rigs_*; HIP library only)
    def rigs_set(self, Xs, seqs=None):
        """bpvo_hip_rigs_set: rig r has the extrinsics Xs[r] [n_r, 4, 4] and the member sequences seqs[r] (seqs None: 0, 1, 2, ... rig after rig)."""
        counts = np.ascontiguousarray([len(X) for X in Xs], dtype=np.int32)
        Xf = _f32(np.concatenate([_f32(X).reshape(-1, 16) for X in Xs], axis=0)) if len(Xs) else np.zeros((0, 16), np.float32)
        ids, p_ids = (None, None) if seqs is None else self._seq_ids(int(counts.sum()), np.concatenate([np.asarray(q, np.int32).reshape(-1) for q in seqs]))
        self.call("rigs_set", len(Xs), counts.ctypes.data_as(C.c_void_p), p_ids, Xf.ctypes.data_as(C.c_void_p))

    def rigs_get(self):
        """[(sequence ids [n_r], extrinsics [n_r, 4, 4])] of the declared rigs."""
        R = C.c_int()
        self._ck(self.b.fn("rigs_get")(self.h, C.byref(R), None, None, None))
        if not R.value:
            return []
        counts = np.empty(R.value, np.int32)
        self._ck(self.b.fn("rigs_get")(self.h, C.byref(R), counts.ctypes.data_as(C.c_void_p), None, None))
        total = int(counts.sum())
        ids, X = np.empty(total, np.int32), np.empty((total, 4, 4), np.float32)
        self._ck(self.b.fn("rigs_get")(self.h, C.byref(R), counts.ctypes.data_as(C.c_void_p), ids.ctypes.data_as(C.c_void_p), X.ctypes.data_as(C.c_void_p)))
        at = np.concatenate([[0], np.cumsum(counts)])
        return [(ids[at[r]:at[r + 1]].copy(), X[at[r]:at[r + 1]].copy()) for r in range(R.value)]

    def rigs_set_params(self, rig, params: Params):
        """bpvo_hip_rigs_set_params: rig `rig` runs with its own Params (the fields seq_set_params accepts); only while its members hold no frame."""
        self.call("rigs_set_params", int(rig), C.byref(params))

    def rigs_get_params(self, rig) -> Params:
        p = Params()
        self._ck(self.b.fn("rigs_get_params")(self.h, int(rig), C.byref(p)))
        return p

    def add_frames_rigs(self, images, disps, rigs=None):
        """bpvo_hip_add_frames_rigs: images[i] / disps[i] are the next frames of the members of rig rigs[i] (None: 0 .. n-1), lists of 2-D arrays in
        member order, each of its camera's size; returns the bodies' results, one dict per named rig."""
        n = len(images)
        ids, p_ids = self._seq_ids(n, rigs)
        declared = self.rigs_get()
        flat_i, flat_d = [], []
        for i in range(n):
            r = int(ids[i]) if ids is not None else i
            if 0 <= r < len(declared):
                assert len(images[i]) == len(declared[r][0]), f"rig {r} has {len(declared[r][0])} members"
                for k, s in enumerate(declared[r][0]):
                    cam = self.seq_get_camera(int(s))
                    assert np.shape(images[i][k]) == (cam.rows, cam.cols), f"rig {r}: member {k} (sequence {s}) takes {cam.rows}x{cam.cols} frames"
            flat_i += list(images[i])
            flat_d += list(disps[i])
        img, disp, _ = pack_frames(flat_i, flat_d)
        res = (Result * n)()
        self.call("add_frames_rigs", n, p_ids, img.ctypes.data_as(C.c_void_p), disp.ctypes.data_as(C.c_void_p), 0, res)
        return [self._result_dict(r) for r in res]

    def add_frames_rigs_device(self, n, d_images_ptr, d_disps_ptr, rigs=None):
        """add_frames_rigs with the packed frames already in device memory."""
        ids, p_ids = self._seq_ids(n, rigs)
        res = (Result * n)()
        self.call("add_frames_rigs", int(n), p_ids, C.c_void_p(d_images_ptr), C.c_void_p(d_disps_ptr), 1, res)
        return [self._result_dict(r) for r in res]

    def rigs_trajectory(self, rig):
        n = C.c_int()
        self.call("rigs_trajectory_size", int(rig), C.byref(n))
        out = np.empty((n.value, 4, 4), np.float32)
        if n.value:
            self.call("rigs_get_trajectory", int(rig), out.ctypes.data_as(C.c_void_p))
        return out

    def rigs_pose_covariance(self, rig):
        out = PoseCovariance()
        self.call("rigs_pose_covariance", int(rig), C.byref(out))
        return _cov_dict(out)

    def estimate_pose_rigs(self, wss, refs, curs, X, T_init=None):
        """bpvo_hip_estimate_pose_rigs: wss / refs / curs / X are lists with one entry per rig (as estimate_pose_rig takes them), T_init [n_rigs, 4, 4]
        (None: identities); returns (body poses [n_rigs, 4, 4], [per-level statistics] per rig)."""
        R = len(wss)
        parts = [self._rig_members(wss[r], refs[r], curs[r], X[r]) for r in range(R)]
        counts = np.ascontiguousarray([q[0].shape[0] for q in parts], dtype=np.int32)
        w, r_, c_, Xf = (np.ascontiguousarray(np.concatenate([q[k] for q in parts], axis=0)) for k in range(4))
        T0 = _f32(np.tile(np.eye(4), (R, 1, 1)) if T_init is None else T_init).reshape(R, 16)
        T = np.empty((R, 4, 4), np.float32)
        st = (Stats * (self.L * R))()
        self.call("estimate_pose_rigs", R, counts.ctypes.data_as(C.c_void_p), w.ctypes.data_as(C.c_void_p), r_.ctypes.data_as(C.c_void_p),
                  c_.ctypes.data_as(C.c_void_p), Xf.ctypes.data_as(C.c_void_p), T0.ctypes.data_as(C.c_void_p), T.ctypes.data_as(C.c_void_p), st)
        stats = [[dict(numIterations=s.numIterations, finalError=s.finalError, firstOrderOptimality=s.firstOrderOptimality, status=s.status)
                  for s in st[k * self.L:(k + 1) * self.L]] for k in range(R)]
        return T, stats

    # -- pose covariance (bpvo_hip_pose_covariances ...; HIP library only)
    def pose_covariances(self, wss, refs, curs, level, T=None, sigma=None):
        """One record (dict) per workspace: at the poses T [n, 4, 4] and scales sigma [n], or (both None) of each workspace's last estimate."""
        w, r, c, _ = self._rig_members(wss, refs, curs, np.zeros((len(np.atleast_1d(wss)), 16)))
        n = w.shape[0]
        out = (PoseCovariance * n)()
        Tf = None if T is None else _f32(T).reshape(n, 16)
        sf = None if sigma is None else _f32(sigma).reshape(n)
        self.call("pose_covariances", n, w.ctypes.data_as(C.c_void_p), r.ctypes.data_as(C.c_void_p), c.ctypes.data_as(C.c_void_p), int(level),
                  None if Tf is None else Tf.ctypes.data_as(C.c_void_p), None if sf is None else sf.ctypes.data_as(C.c_void_p), out)
        return [_cov_dict(o) for o in out]

    def pose_covariance_rig(self, wss, refs, curs, X, level, T_body=None, sigma=None):
        """The body pose's record from the members (as linearize_rig takes them); sigma: every member's own scale."""
        w, r, c, Xf = self._rig_members(wss, refs, curs, X)
        n = w.shape[0]
        out = PoseCovariance()
        Tf = None if T_body is None else _f32(T_body).reshape(16)
        sf = None if sigma is None else _f32(sigma).reshape(n)
        self.call("pose_covariance_rig", n, w.ctypes.data_as(C.c_void_p), r.ctypes.data_as(C.c_void_p), c.ctypes.data_as(C.c_void_p),
                  Xf.ctypes.data_as(C.c_void_p), int(level), None if Tf is None else Tf.ctypes.data_as(C.c_void_p),
                  None if sf is None else sf.ctypes.data_as(C.c_void_p), C.byref(out))
        return _cov_dict(out)

    def vo_pose_covariance(self):
        out = PoseCovariance()
        self.call("vo_pose_covariance", C.byref(out))
        return _cov_dict(out)

    def seq_pose_covariance(self, s):
        out = PoseCovariance()
        self.call("seq_pose_covariance", int(s), C.byref(out))
        return _cov_dict(out)

    def rig_pose_covariance(self):
        out = PoseCovariance()
        self.call("rig_pose_covariance", C.byref(out))
        return _cov_dict(out)

    def debug_pose_covariance_sums(self, ws):
        """(M, Q) of the last pose-covariance pass on workspace ws, in its normalised twist."""
        M, Q = np.empty((6, 6), np.float32), np.empty((6, 6), np.float32)
        self.call("debug_pose_covariance_sums", int(ws), M.ctypes.data_as(C.c_void_p), Q.ctypes.data_as(C.c_void_p))
        return M, Q

    # -- pose scoring (bpvo_hip_score_poses ...; HIP library only)
    def score_poses(self, ref, cur, level, poses, tau):
        """The truncated-L1 score of every pose [P, 4, 4] of the pair (ref, cur) at `level` in one launch: a POSE_SCORE record array [P]."""
        Tf = _f32(poses).reshape(-1, 16)
        out = np.zeros(Tf.shape[0], POSE_SCORE)
        self.call("score_poses", int(ref), int(cur), int(level), int(Tf.shape[0]), Tf.ctypes.data_as(C.c_void_p), C.c_float(tau),
                  out.ctypes.data_as(C.c_void_p))
        return out

    def score_poses_pairs(self, refs, curs, level, poses, tau):
        """... of n pairs in one launch, poses [n, P, 4, 4]: a POSE_SCORE record array [n, P]."""
        r = np.ascontiguousarray(refs, dtype=np.int32).reshape(-1)
        c = np.ascontiguousarray(curs, dtype=np.int32).reshape(-1)
        n = r.shape[0]
        assert c.shape[0] == n, "one current frame per template"
        Tf = _f32(poses).reshape(n, -1, 16)
        out = np.zeros((n, Tf.shape[1]), POSE_SCORE)
        self.call("score_poses_pairs", n, r.ctypes.data_as(C.c_void_p), c.ctypes.data_as(C.c_void_p), int(level), int(Tf.shape[1]),
                  Tf.ctypes.data_as(C.c_void_p), C.c_float(tau), out.ctypes.data_as(C.c_void_p))
        return out

    def estimate_pose_best_start(self, ws, ref, cur, candidates, tau, score_level=-1):
        """estimate_pose from the best-scoring of the candidate starts [n, 4, 4] (score_level < 0: the coarsest level):
        (T, stats, chosen index, POSE_SCORE records [n])."""
        Tf = _f32(candidates).reshape(-1, 16)
        n = Tf.shape[0]
        T = np.empty((4, 4), np.float32)
        st = (Stats * self.L)()
        chosen = C.c_int(-1)
        scores = np.zeros(n, POSE_SCORE)
        self.call("estimate_pose_best_start", int(ws), int(ref), int(cur), n, Tf.ctypes.data_as(C.c_void_p), int(score_level), C.c_float(tau),
                  T.ctypes.data_as(C.c_void_p), st, C.byref(chosen), scores.ctypes.data_as(C.c_void_p))
        stats = [dict(numIterations=s.numIterations, finalError=s.finalError, firstOrderOptimality=s.firstOrderOptimality, status=s.status) for s in st]
        return T, stats, chosen.value, scores

    # -- start policy (bpvo_hip_set_start_policy ...; an extension: no reference member; HIP library only)
    @staticmethod
    def _policy_arg(policy):
        if policy is None or isinstance(policy, StartPolicy):
            return policy
        if isinstance(policy, dict):
            return start_policy(**policy)
        return start_policy(*policy)

    @staticmethod
    def _policy_dict(p: StartPolicy):
        return dict(mode=int(p.mode), score_level=int(p.score_level), tau=float(np.float32(p.tau)))

    @staticmethod
    def _hints_arg(hints):
        M = _f32(hints if hints is not None and len(hints) else np.zeros((0, 4, 4))).reshape(-1, 16)
        return M.shape[0], (M.ctypes.data_as(C.c_void_p) if M.shape[0] else None), M

    def set_start_policy(self, policy):
        """bpvo_hip_set_start_policy: the context's policy — a StartPolicy, a dict(mode, score_level, tau) or a (mode, score_level, tau) tuple."""
        p = self._policy_arg(policy)
        self.call("set_start_policy", C.byref(p))

    def get_start_policy(self):
        p = StartPolicy()
        self._ck(self.b.fn("get_start_policy")(self.h, C.byref(p)))
        return self._policy_dict(p)

    def seq_set_start_policy(self, s, policy):
        """bpvo_hip_seq_set_start_policy: sequence s's own policy; None returns it to the context's."""
        p = self._policy_arg(policy)
        self.call("seq_set_start_policy", int(s), None if p is None else C.byref(p))

    def seq_get_start_policy(self, s):
        """(policy dict, True if it is the sequence's own)"""
        p, own = StartPolicy(), C.c_int()
        self._ck(self.b.fn("seq_get_start_policy")(self.h, int(s), C.byref(p), C.byref(own)))
        return self._policy_dict(p), bool(own.value)

    def rigs_set_start_policy(self, rig, policy):
        p = self._policy_arg(policy)
        self.call("rigs_set_start_policy", int(rig), None if p is None else C.byref(p))

    def rigs_get_start_policy(self, rig):
        p, own = StartPolicy(), C.c_int()
        self._ck(self.b.fn("rigs_get_start_policy")(self.h, int(rig), C.byref(p), C.byref(own)))
        return self._policy_dict(p), bool(own.value)

    def vo_set_start_hints(self, hints):
        """bpvo_hip_vo_set_start_hints: the pending hints [n, 4, 4] (frame-to-frame guesses in Result.pose's convention) of add_frame's next estimate."""
        n, ptr, _keep = self._hints_arg(hints)
        self.call("vo_set_start_hints", n, ptr)

    def seq_set_start_hints(self, s, hints):
        n, ptr, _keep = self._hints_arg(hints)
        self.call("seq_set_start_hints", int(s), n, ptr)

    def rigs_set_start_hints(self, rig, hints):
        n, ptr, _keep = self._hints_arg(hints)
        self.call("rigs_set_start_hints", int(rig), n, ptr)

    def vo_start_info(self, which=0):
        """bpvo_hip_vo_start_info: dict(n_candidates, chosen, kind [n], T_start [4, 4], scores POSE_SCORE [n]) of estimate `which` of the last add_frame."""
        out = StartInfo()
        self.call("vo_start_info", int(which), C.byref(out))
        return _start_info_dict(out)

    def seq_start_info(self, s, which=0):
        out = StartInfo()
        self.call("seq_start_info", int(s), int(which), C.byref(out))
        return _start_info_dict(out)

    def rigs_start_info(self, rig, which=0):
        out = StartInfo()
        self.call("rigs_start_info", int(rig), int(which), C.byref(out))
        return _start_info_dict(out)

    # -- disparity fusion (bpvo_hip_set_disparity_fusion ...; an extension: no reference member; HIP library only)
    @staticmethod
    def _fusion_arg(f):
        if f is None or isinstance(f, DisparityFusion):
            return f
        if isinstance(f, dict):
            return disparity_fusion(**f)
        return disparity_fusion(*f)

    @staticmethod
    def _fusion_dict(f: DisparityFusion):
        return dict(mode=int(f.mode), measurement_sigma=float(f.measurement_sigma), process_sigma=float(f.process_sigma), gate=float(f.gate),
                    max_fill_sigma=float(f.max_fill_sigma))

    @staticmethod
    def _fusion_info_dict(r: DisparityFusionInfo):
        return dict(fused=int(r.fused), replaced=int(r.replaced), measured=int(r.measured), filled=int(r.filled), none=int(r.none),
                    predicted=bool(r.predicted), slot=int(r.slot), motion=np.array(r.motion, np.float32).reshape(4, 4))

    def set_disparity_fusion(self, fusion):
        """bpvo_hip_set_disparity_fusion: the context's setting — a DisparityFusion, a dict of its fields or a tuple in their order."""
        f = self._fusion_arg(fusion)
        self.call("set_disparity_fusion", C.byref(f))

    def get_disparity_fusion(self):
        f = DisparityFusion()
        self._ck(self.b.fn("get_disparity_fusion")(self.h, C.byref(f)))
        return self._fusion_dict(f)

    def seq_set_disparity_fusion(self, s, fusion):
        """bpvo_hip_seq_set_disparity_fusion: sequence s's own setting; None returns it to the context's."""
        f = self._fusion_arg(fusion)
        self.call("seq_set_disparity_fusion", int(s), None if f is None else C.byref(f))

    def seq_get_disparity_fusion(self, s):
        """(setting dict, True if it is the sequence's own)"""
        f, own = DisparityFusion(), C.c_int()
        self._ck(self.b.fn("seq_get_disparity_fusion")(self.h, int(s), C.byref(f), C.byref(own)))
        return self._fusion_dict(f), bool(own.value)

    def _fused_maps(self, name, args, shape):
        D, V = np.empty(shape, np.float32), np.empty(shape, np.float32)
        self.call(name, *args, D.ctypes.data_as(C.c_void_p), V.ctypes.data_as(C.c_void_p))
        return D, V

    def vo_get_fused_disparity(self):
        """bpvo_hip_vo_get_fused_disparity: (disparity, variance) [rows, cols] f32 that add_frame's sequence carries."""
        return self._fused_maps("vo_get_fused_disparity", (), (self.rows, self.cols))

    def seq_get_fused_disparity(self, s):
        cam = self.seq_get_camera(int(s))
        return self._fused_maps("seq_get_fused_disparity", (int(s),), (cam.rows, cam.cols))

    def vo_disparity_fusion_info(self):
        out = DisparityFusionInfo()
        self.call("vo_disparity_fusion_info", C.byref(out))
        return self._fusion_info_dict(out)

    def seq_disparity_fusion_info(self, s):
        out = DisparityFusionInfo()
        self.call("seq_disparity_fusion_info", int(s), C.byref(out))
        return self._fusion_info_dict(out)

    def fuse_disparities(self, disps, poses, seq=None):
        """bpvo_hip_fuse_disparities: the carried maps of sequence seq[i] (None: 0 .. n-1) advance by poses[i] [4, 4] with the measured map disps[i]
        (2-D f32 of the sequence's camera size)."""
        n = len(disps)
        ids, p_ids = self._seq_ids(n, seq)
        packed = np.concatenate([_f32(d).reshape(-1) for d in disps])
        Tf = _f32(poses).reshape(n, 16)
        self.call("fuse_disparities", n, p_ids, packed.ctypes.data_as(C.c_void_p), 0, Tf.ctypes.data_as(C.c_void_p))

    def fuse_disparities_device(self, n, d_disps_ptr, poses, seq=None):
        """fuse_disparities with the packed maps already in device memory."""
        ids, p_ids = self._seq_ids(n, seq)
        Tf = _f32(poses).reshape(n, 16)
        self.call("fuse_disparities", int(n), p_ids, C.c_void_p(d_disps_ptr), 1, Tf.ctypes.data_as(C.c_void_p))

    def get_disparity(self, slot, shape=None):
        """bpvo_hip_get_disparity: frame slot `slot`'s disparity map (shape: the slot's camera size; None: the context's)."""
        out = np.empty((self.rows, self.cols) if shape is None else tuple(shape), np.float32)
        self.call("get_disparity", int(slot), out.ctypes.data_as(C.c_void_p))
        return out

    def disparity_fusion_counts(self):
        """bpvo_hip_disparity_fusion_counts: (kernel launches, pixels updated) so far."""
        a, b = C.c_uint64(), C.c_uint64()
        self.call("disparity_fusion_counts", C.byref(a), C.byref(b))
        return a.value, b.value

    # -- measurement variance (bpvo_hip_set_measurement_variance ...; an extension: no reference member; HIP library only)
    @staticmethod
    def _variance_arg(v):
        if v is None or isinstance(v, MeasurementVariance):
            return v
        if isinstance(v, dict):
            return measurement_variance(**v)
        return measurement_variance(*v)

    @staticmethod
    def _variance_dict(v: MeasurementVariance):
        return dict(mode=int(v.mode), radius=int(v.radius), noise_sigma=float(v.noise_sigma), min_sigma=float(v.min_sigma), max_sigma=float(v.max_sigma))

    @staticmethod
    def _variance_info_dict(r: MeasurementVarianceInfo):
        return {k: int(getattr(r, k)) for k in VARIANCE_CLASSES}

    def set_measurement_variance(self, setting):
        """bpvo_hip_set_measurement_variance: the context's setting — a MeasurementVariance, a dict of its fields or a tuple in their order."""
        v = self._variance_arg(setting)
        self.call("set_measurement_variance", C.byref(v))

    def get_measurement_variance(self):
        v = MeasurementVariance()
        self._ck(self.b.fn("get_measurement_variance")(self.h, C.byref(v)))
        return self._variance_dict(v)

    def seq_set_measurement_variance(self, s, setting):
        """bpvo_hip_seq_set_measurement_variance: sequence s's own setting; None returns it to the context's."""
        v = self._variance_arg(setting)
        self.call("seq_set_measurement_variance", int(s), None if v is None else C.byref(v))

    def seq_get_measurement_variance(self, s):
        """(setting dict, True if it is the sequence's own)"""
        v, own = MeasurementVariance(), C.c_int()
        self._ck(self.b.fn("seq_get_measurement_variance")(self.h, int(s), C.byref(v), C.byref(own)))
        return self._variance_dict(v), bool(own.value)

    def vo_get_measurement_variance(self):
        """bpvo_hip_vo_get_measurement_variance: the map [rows, cols] f32 of add_frame_stereo's last frame."""
        out = np.empty((self.rows, self.cols), np.float32)
        self.call("vo_get_measurement_variance", out.ctypes.data_as(C.c_void_p))
        return out

    def seq_get_measurement_variance_map(self, s):
        cam = self.seq_get_camera(int(s))
        out = np.empty((cam.rows, cam.cols), np.float32)
        self.call("seq_get_measurement_variance_map", int(s), out.ctypes.data_as(C.c_void_p))
        return out

    def vo_measurement_variance_info(self):
        out = MeasurementVarianceInfo()
        self.call("vo_measurement_variance_info", C.byref(out))
        return self._variance_info_dict(out)

    def seq_measurement_variance_info(self, s):
        out = MeasurementVarianceInfo()
        self.call("seq_measurement_variance_info", int(s), C.byref(out))
        return self._variance_info_dict(out)

    def disparity_variance_frames(self, lefts, rights, disps, lo, hi, setting):
        """bpvo_hip_disparity_variance_frames: the rule for the pairs (2-D u8 arrays) with the measured maps disps (2-D f32, each of its pair's
        shape) under the gate lo .. hi: (list of f32 variance maps, list of class-count dicts)."""
        n = len(lefts)
        assert len(rights) == n and len(disps) == n, "one right image and one map per left image"
        cams = self._camera_array([np.shape(l) for l in lefts])
        left, shapes = pack_images(lefts)
        right, _ = pack_images(rights)
        disp = np.concatenate([_f32(d).reshape(-1) for d in disps])
        assert right.size == left.size and disp.size == left.size, "a pair's images and its map have one shape"
        v = self._variance_arg(setting)
        out = np.empty(left.size, np.float32)
        counts = np.zeros((n, 6), np.uint32)
        self.call("disparity_variance_frames", n, cams, left.ctypes.data_as(C.c_void_p), right.ctypes.data_as(C.c_void_p), disp.ctypes.data_as(C.c_void_p), 0,
                  C.c_float(lo), C.c_float(hi), C.byref(v), out.ctypes.data_as(C.c_void_p), 0, counts.ctypes.data_as(C.c_void_p))
        maps, at = [], 0
        for r, w in shapes:
            maps.append(out[at:at + r * w].reshape(r, w))
            at += r * w
        return maps, [dict(zip(VARIANCE_CLASSES, (int(x) for x in row))) for row in counts]

    def disparity_variance_frames_device(self, cams_or_sizes, d_left_ptr, d_right_ptr, d_disp_ptr, lo, hi, setting, d_out_ptr):
        """disparity_variance_frames with the packed inputs in device memory, the packed maps written to device memory; no counts."""
        cams = self._camera_array(cams_or_sizes)
        v = self._variance_arg(setting)
        self.call("disparity_variance_frames", len(cams), cams, C.c_void_p(d_left_ptr), C.c_void_p(d_right_ptr), C.c_void_p(d_disp_ptr), 1,
                  C.c_float(lo), C.c_float(hi), C.byref(v), C.c_void_p(d_out_ptr), 1, None)

    def fuse_disparities_var(self, disps, variances, poses, seq=None):
        """bpvo_hip_fuse_disparities_var: fuse_disparities with the measurements' variance maps (2-D f32, each of its map's shape)."""
        n = len(disps)
        assert len(variances) == n
        ids, p_ids = self._seq_ids(n, seq)
        packed = np.concatenate([_f32(d).reshape(-1) for d in disps])
        var = np.concatenate([_f32(v).reshape(-1) for v in variances])
        assert var.size == packed.size
        Tf = _f32(poses).reshape(n, 16)
        self.call("fuse_disparities_var", n, p_ids, packed.ctypes.data_as(C.c_void_p), var.ctypes.data_as(C.c_void_p), 0, Tf.ctypes.data_as(C.c_void_p))

    def measurement_variance_counts(self):
        """bpvo_hip_measurement_variance_counts: (launches, pixels, (tiles staged, tiles direct, tiles idle)) so far."""
        a, b, t = C.c_uint64(), C.c_uint64(), (C.c_uint64 * 3)()
        self.call("measurement_variance_counts", C.byref(a), C.byref(b), t)
        return a.value, b.value, tuple(int(x) for x in t)

    # -- motion stereo (bpvo_hip_set_motion_stereo ...; an extension: no reference member; HIP library only)
    @staticmethod
    def _motion_stereo_arg(v):
        if v is None or isinstance(v, MotionStereo):
            return v
        if isinstance(v, dict):
            return motion_stereo(**v)
        return motion_stereo(*v)

    @staticmethod
    def _motion_stereo_dict(v: MotionStereo):
        return dict(mode=int(v.mode), radius=int(v.radius), steps=int(v.steps), min_gain=float(v.min_gain), noise_sigma=float(v.noise_sigma),
                    min_sigma=float(v.min_sigma), max_sigma=float(v.max_sigma), gate=float(v.gate))

    @staticmethod
    def _motion_stereo_info_dict(r: MotionStereoInfo):
        out = {k: int(getattr(r, k)) for k in MOTION_STEREO_CLASSES}
        out.update(launched=int(r.launched), view_slot=int(r.view_slot), motion=np.array(r.motion, np.float32).reshape(4, 4))
        return out

    def set_motion_stereo(self, setting):
        """bpvo_hip_set_motion_stereo: the context's setting — a MotionStereo, a dict of its fields or a tuple in their order."""
        v = self._motion_stereo_arg(setting)
        self.call("set_motion_stereo", C.byref(v))

    def get_motion_stereo(self):
        v = MotionStereo()
        self._ck(self.b.fn("get_motion_stereo")(self.h, C.byref(v)))
        return self._motion_stereo_dict(v)

    def seq_set_motion_stereo(self, s, setting):
        """bpvo_hip_seq_set_motion_stereo: sequence s's own setting; None returns it to the context's."""
        v = self._motion_stereo_arg(setting)
        self.call("seq_set_motion_stereo", int(s), None if v is None else C.byref(v))

    def seq_get_motion_stereo(self, s):
        """(setting dict, True if it is the sequence's own)"""
        v, own = MotionStereo(), C.c_int()
        self._ck(self.b.fn("seq_get_motion_stereo")(self.h, int(s), C.byref(v), C.byref(own)))
        return self._motion_stereo_dict(v), bool(own.value)

    def vo_motion_stereo_info(self):
        out = MotionStereoInfo()
        self.call("vo_motion_stereo_info", C.byref(out))
        return self._motion_stereo_info_dict(out)

    def seq_motion_stereo_info(self, s):
        out = MotionStereoInfo()
        self.call("seq_motion_stereo_info", int(s), C.byref(out))
        return self._motion_stereo_info_dict(out)

    def motion_stereo_frames(self, cams, firsts, seconds, motions, prior_disparities, prior_variances):
        """bpvo_hip_motion_stereo_frames: the rule under the context's setting for the image pairs (2-D u8 arrays) of the cameras (Camera, or
        (K, baseline, rows, cols)), the motions [n, 4, 4] (X_second = Q X_first) and the prior maps (2-D f32; no prior where the variance < 0):
        (list of f32 disparity maps, list of f32 variance maps, list of u8 class maps)."""
        n = len(firsts)
        assert len(seconds) == n and len(prior_disparities) == n and len(prior_variances) == n and len(cams) == n
        cams = self._camera_array(cams)
        first, shapes = pack_images(firsts)
        second, _ = pack_images(seconds)
        pd = np.concatenate([_f32(d).reshape(-1) for d in prior_disparities])
        pv = np.concatenate([_f32(d).reshape(-1) for d in prior_variances])
        assert second.size == first.size and pd.size == first.size and pv.size == first.size, "a pair's images and its priors have one shape"
        Q = np.ascontiguousarray(_f32(motions).reshape(n, 16))
        D, V, cls = np.empty(first.size, np.float32), np.empty(first.size, np.float32), np.empty(first.size, np.uint8)
        self.call("motion_stereo_frames", n, cams, first.ctypes.data_as(C.c_void_p), second.ctypes.data_as(C.c_void_p), Q.ctypes.data_as(C.c_void_p),
                  pd.ctypes.data_as(C.c_void_p), pv.ctypes.data_as(C.c_void_p), 0, D.ctypes.data_as(C.c_void_p), V.ctypes.data_as(C.c_void_p),
                  cls.ctypes.data_as(C.c_void_p))
        Ds, Vs, Cs, at = [], [], [], 0
        for r, w in shapes:
            Ds.append(D[at:at + r * w].reshape(r, w))
            Vs.append(V[at:at + r * w].reshape(r, w))
            Cs.append(cls[at:at + r * w].reshape(r, w))
            at += r * w
        return Ds, Vs, Cs

    def motion_stereo_frames_device(self, cams, d_first_ptr, d_second_ptr, motions, d_pd_ptr, d_pv_ptr, d_out_d_ptr, d_out_v_ptr, d_out_c_ptr=None):
        """motion_stereo_frames with the packed inputs in device memory, the packed outputs written to device memory."""
        cams = self._camera_array(cams)
        Q = np.ascontiguousarray(_f32(motions).reshape(len(cams), 16))
        self.call("motion_stereo_frames", len(cams), cams, C.c_void_p(d_first_ptr), C.c_void_p(d_second_ptr), Q.ctypes.data_as(C.c_void_p),
                  C.c_void_p(d_pd_ptr), C.c_void_p(d_pv_ptr), 1, C.c_void_p(d_out_d_ptr), C.c_void_p(d_out_v_ptr),
                  None if d_out_c_ptr is None else C.c_void_p(d_out_c_ptr))

    def motion_stereo_counts(self):
        """bpvo_hip_motion_stereo_counts: (launches, pixels, (tiles staged, tiles direct, tiles idle), class-count dict over all launches) so far."""
        a, b, t, k = C.c_uint64(), C.c_uint64(), (C.c_uint64 * 3)(), (C.c_uint64 * 7)()
        self.call("motion_stereo_counts", C.byref(a), C.byref(b), t, k)
        return a.value, b.value, tuple(int(x) for x in t), dict(zip(MOTION_STEREO_CLASSES, (int(x) for x in k)))

    # -- batches
    def _stats_array(self, st, n_pairs):
        a = np.ctypeslib.as_array(C.cast(st, C.POINTER(C.c_int32)), shape=(n_pairs, self.L, 4)).copy()
        out = np.empty((n_pairs, self.L), dtype=[("numIterations", np.int32), ("finalError", np.float32),
                                                  ("firstOrderOptimality", np.float32), ("status", np.int32)])
        out["numIterations"] = a[..., 0]
        out["finalError"] = a[..., 1].view(np.float32)
        out["firstOrderOptimality"] = a[..., 2].view(np.float32)
        out["status"] = a[..., 3]
        return out

    def batch_run(self, images, disps):
        images = np.ascontiguousarray(images, dtype=np.uint8)
        disps = _f32(disps)
        n_pairs = images.shape[0] // 2
        poses = np.empty((n_pairs, 4, 4), np.float32)
        st = (Stats * (n_pairs * self.L))()
        self.call("batch_run", n_pairs, images.ctypes.data_as(C.c_void_p), disps.ctypes.data_as(C.c_void_p), 0,
                  poses.ctypes.data_as(C.c_void_p), st)
        return poses, self._stats_array(st, n_pairs)

    def batch_run_device(self, n_pairs, d_images_ptr, d_disps_ptr):
        poses = np.empty((n_pairs, 4, 4), np.float32)
        st = (Stats * (n_pairs * self.L))()
        self.call("batch_run", int(n_pairs), C.c_void_p(d_images_ptr), C.c_void_p(d_disps_ptr), 1,
                  poses.ctypes.data_as(C.c_void_p), st)
        return poses, self._stats_array(st, n_pairs)

    def batch_estimate(self, n_pairs, T_init=None):
        poses = np.empty((n_pairs, 4, 4), np.float32)
        st = (Stats * (n_pairs * self.L))()
        T0 = None if T_init is None else _f32(T_init).reshape(-1)
        self.call("batch_estimate", int(n_pairs), None if T0 is None else T0.ctypes.data_as(C.c_void_p),
                  poses.ctypes.data_as(C.c_void_p), st)
        return poses, self._stats_array(st, n_pairs)

    def batch_result_records_device(self):
        p, n = C.c_void_p(), C.c_int()
        self.call("batch_result_records_device", C.byref(p), C.byref(n))
        return p.value, n.value

    def batch_copy_records_device(self, d_dst_ptr, n_pairs):
        self.call("batch_copy_records_device", C.c_void_p(d_dst_ptr), int(n_pairs))

    # -- measurement
    def profiling(self, level=1):
        """0 off, 1 = HIP events around the frame stages + every 5th warp_residual launch, 2 = around every kernel, 3 = as 1 with every
        warp_residual launch. Resets the counters."""
        self.call("profiling", int(level))

    def kernel_stats(self):
        arr = (KernelStat * 32)()
        n = C.c_int()
        self.call("get_kernel_stats", arr, 32, C.byref(n))
        return [dict(name=arr[i].name.decode(), launches=arr[i].launches, total_ms=arr[i].total_ms, units=arr[i].units,
                     bytes_per_unit=arr[i].bytes_per_unit) for i in range(n.value)]

    def median_path_counts(self):
        a, b = C.c_uint64(), C.c_uint64()
        self.call("median_path_counts", C.byref(a), C.byref(b))
        return a.value, b.value

    def tscale_counts(self):
        """(runs of the Student-t scale stage, passes of its iteration) since the last counter reset (HIP library only)."""
        a, b = C.c_uint64(), C.c_uint64()
        self.call("tscale_counts", C.byref(a), C.byref(b))
        return a.value, b.value

    def fused_point_counts(self):
        """(fused, total) points linearised since the last counter reset (HIP library only)."""
        a, b = C.c_uint64(), C.c_uint64()
        self.call("fused_point_counts", C.byref(a), C.byref(b))
        return a.value, b.value

    def tap_cache_counts(self):
        """(hits, lookups, hits in the first 8 linearisations of a level, lookups there) since the last counter reset."""
        a = (C.c_uint64 * 4)()
        self.call("tap_cache_counts", a)
        return tuple(int(x) for x in a)

    def persistent_counts(self):
        """(pyramid levels run by the persistent single-launch GN kernel, 1 if such a launch ever gave up) (HIP library only)."""
        a, b = C.c_uint64(), C.c_int()
        self.call("persistent_counts", C.byref(a), C.byref(b))
        return a.value, b.value

    def upload_stats(self):
        """(seconds, bytes) of the upload pipeline of the last host-buffer batch_run (HIP library only)."""
        a, b = C.c_double(), C.c_uint64()
        self.call("upload_stats", C.byref(a), C.byref(b))
        return a.value, b.value

    def team_counts(self):
        """Batch estimates run by the team-persistent kernel since the context was created (HIP library only)."""
        a = C.c_uint64()
        self.call("team_counts", C.byref(a))
        return a.value

    def set_option(self, key, value):
        """bpvo_hip_set_option: per-context scheduling options (include/bpvo_hip/c_api.h)."""
        self.b.fn("set_option").argtypes = [C.c_void_p, C.c_char_p, C.c_double]
        self._ck(self.b.fn("set_option")(self.h, key.encode(), C.c_double(float(value))))

    def get_option(self, key):
        v = C.c_double(0.0)
        self.b.fn("get_option").argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_double)]
        self._ck(self.b.fn("get_option")(self.h, key.encode(), C.byref(v)))
        return v.value

    def set_max_lanes(self, n):
        """Cap (n >= 1) or uncap (n <= 0) the estimation lanes of later batch calls (HIP library only)."""
        self.call("set_max_lanes", int(n))

    def total_linearizations(self):
        n = C.c_uint64()
        self.call("total_linearizations", C.byref(n))
        return n.value
