/*
 * bpvo_hip/vo.hpp — header-only C++11 facade over the C ABI (c_api.h) with the reference's class names, argument
 * meaning and error behaviour, so that code written against bpvo/vo.h keeps compiling after swapping the include:
 *
 *   bpvo::VisualOdometry                (reference: bpvo/vo.h:31-105, bpvo/vo.cc:66-94)
 *   bpvo::VisualOdometryFrame           (reference: bpvo/vo_frame.h:21-90)
 *   bpvo::VisualOdometryPoseEstimator   (reference: bpvo/vo_pose_estimator.h:34-64)
 *   bpvo::VisualOdometrySequences       many independent VisualOdometry sequences in one context (no counterpart in the reference)
 *   bpvo::AlgorithmParameters, Result, OptimizerStatistics, PointWithInfo, PointCloud, Trajectory, ImageSize, enums
 *                                       (reference: bpvo/types.h:127-589, bpvo/point_cloud.h, bpvo/trajectory.h)
 *
 * Differences a caller sees:
 *   - no Eigen / OpenCV in the interface: Matrix33 / Matrix44 are row-major std::array<float,9|16>
 *     (an Eigen user maps them with Eigen::Map<const Eigen::Matrix<float,4,4,Eigen::RowMajor>>);
 *   - frames live on the GPU: VisualOdometryFrame is a handle (device context + slot), not a host container;
 *   - a non-zero C status becomes bpvo::Error (std::logic_error) exactly where the reference uses THROW_ERROR
 *     (bpvo/utils.h:211-220), e.g. null image/disparity pointers (bpvo/vo.cc:68-69).
 */
#ifndef BPVO_HIP_VO_HPP
#define BPVO_HIP_VO_HPP

#include <algorithm>
#include <array>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "c_api.h"

namespace bpvo {

struct Error : public std::logic_error {                       // bpvo/utils.h:205-209
  explicit Error(const std::string& what) : std::logic_error(what) {}
};

typedef std::array<float, 9> Matrix33;                          // row-major
typedef std::array<float, 16> Matrix44;                         // row-major
typedef Matrix44 Pose;
typedef std::array<float, 36> PoseCovariance;
typedef std::array<float, 4> Point;                             // (X, Y, Z, 1)  bpvo/types.h:84
typedef std::vector<Point> PointVector;
typedef std::vector<float> WeightsVector;

enum LossFunctionType { kHuber = BPVO_LOSS_HUBER, kTukey = BPVO_LOSS_TUKEY, kL2 = BPVO_LOSS_L2,
                        kStudentT = BPVO_LOSS_STUDENT_T /* an extension: c_api.h */ };
enum VerbosityType { kIteration = BPVO_VERB_ITERATION, kFinal, kSilent, kDebug };
/* all eight values of the reference (bpvo/types.h:142-152), all on the device path */
enum DescriptorType { kIntensity = BPVO_DESC_INTENSITY, kIntensityAndGradient, kDescriptorFieldsFirstOrder, kDescriptorFieldsSecondOrder,
                      kLatch, kCentralDifference, kLaplacian, kBitPlanes = BPVO_DESC_BITPLANES };
static_assert(kLaplacian + 1 == kBitPlanes, "DescriptorType numbering follows the reference");
enum GradientEstimationType { kCentralDifference_3 = BPVO_GRAD_CD3, kCentralDifference_5 = BPVO_GRAD_CD5 };
enum InterpolationType { kLinear = BPVO_INTERP_LINEAR, kCosine, kCubic, kCubicHermite };
enum PoseEstimationStatus { kParameterTolReached = BPVO_STATUS_PARAMETER_TOL, kFunctionTolReached, kGradientTolReached,
                            kMaxIterations, kSolverError };
enum KeyFramingReason { kLargeTranslation = BPVO_KF_LARGE_TRANSLATION, kLargeRotation, kSmallFracOfGoodPoints, kNoKeyFraming,
                        kFirstFrame };

struct ImageSize {                                              // bpvo/types.h:572-582
  int rows, cols;
  ImageSize(int r = 0, int c = 0) : rows(r), cols(c) {}
  int numel() const { return rows * cols; }
};

/* bpvo::AlgorithmParameters (bpvo/types.h:171-413): the same 35 fields; defaults = bpvo/types.cc:31-66 */
struct AlgorithmParameters : public bpvo_hip_params {
  AlgorithmParameters() { bpvo_hip_default_params(this); }
};

struct OptimizerStatistics {                                    // bpvo/types.h:444-482
  int numIterations;
  float finalError;
  float firstOrderOptimality;
  PoseEstimationStatus status;
  OptimizerStatistics() : numIterations(0), finalError(-1.0f), firstOrderOptimality(-1.0f), status(kSolverError) {}
  explicit OptimizerStatistics(const bpvo_hip_stats& s)
      : numIterations(s.numIterations), finalError(s.finalError), firstOrderOptimality(s.firstOrderOptimality),
        status(static_cast<PoseEstimationStatus>(s.status)) {}
};

typedef bpvo_hip_point_with_info PointWithInfo;                 // bpvo/point_cloud.h:30-62 (32-byte record)

class PointCloud {                                              // bpvo/point_cloud.h:67-120
 public:
  PointCloud() { setIdentity(); }
  const std::vector<PointWithInfo>& points() const { return _points; }
  std::vector<PointWithInfo>& points() { return _points; }
  size_t size() const { return _points.size(); }
  bool empty() const { return _points.empty(); }
  const Matrix44& pose() const { return _pose; }
  Matrix44& pose() { return _pose; }
 private:
  void setIdentity() { _pose.fill(0.0f); _pose[0] = _pose[5] = _pose[10] = _pose[15] = 1.0f; }
  std::vector<PointWithInfo> _points;
  Matrix44 _pose;
};

struct Result {                                                 // bpvo/types.h:489-563 (move-only)
  Pose pose;
  PoseCovariance covariance;
  std::vector<OptimizerStatistics> optimizerStatistics;
  bool isKeyFrame;
  KeyFramingReason keyFramingReason;
  std::unique_ptr<PointCloud> pointCloud;
  Result() : isKeyFrame(false), keyFramingReason(kNoKeyFraming) {}
  Result(Result&&) = default;
  Result& operator=(Result&&) = default;
  Result(const Result&) = delete;
  Result& operator=(const Result&) = delete;
};

/* The covariance of an estimated pose (c_api.h bpvo_hip_pose_covariances states the definition and its limits): `covariance` is that of eps in
 * T_true = pose * exp(eps), twist ordered (omega, v); `pose` is the estimate's pose against its key frame. */
/* the score of one candidate pose (c_api.h bpvo_hip_pose_score: cost_sum, score, n_valid, n_below) */
typedef bpvo_hip_pose_score PoseScore;

/* where the addFrame drivers start Gauss-Newton (c_api.h "start policy", an extension with no reference member): at the reference's start
 * (kKeyFramePose, the default), at the body's last motion or a hint (kConstantVelocity), or at the best-scoring of Identity, the last motion, the
 * last motion twice and the hints (kScored; tau in descriptor units, scoreLevel -1: the coarsest) */
struct StartPolicy : public bpvo_hip_start_policy {
  enum Mode { kKeyFramePose = BPVO_START_KEYFRAME_POSE, kConstantVelocity = BPVO_START_CONSTANT_VELOCITY, kScored = BPVO_START_SCORED };
  explicit StartPolicy(int mode_ = kKeyFramePose, float tau_ = 0.0f, int scoreLevel = -1) { mode = mode_; score_level = scoreLevel; tau = tau_; }
};
/* what an estimate of the last call started from (c_api.h bpvo_hip_start_info: n_candidates, chosen, kind, T_start, scores) */
typedef bpvo_hip_start_info StartInfo;
/* disparity fusion (c_api.h "disparity fusion", an extension with no reference member; off by default): a sequence carries a disparity and a
 * variance map, predicted into every new frame with the estimated motion and fused with the measured map in front of the template stage.  Units:
 * disparity pixels; gate in standard deviations; maxFillSigma 0: never fill.  No defaults are guessed: On(...) takes all four. */
struct DisparityFusion : public bpvo_hip_disparity_fusion {
  DisparityFusion() { mode = 0; measurement_sigma = process_sigma = gate = max_fill_sigma = 0.0f; }
  static DisparityFusion On(float measurementSigma, float processSigma, float gate_, float maxFillSigma)
  {
    DisparityFusion f;
    f.mode = 1; f.measurement_sigma = measurementSigma; f.process_sigma = processSigma; f.gate = gate_; f.max_fill_sigma = maxFillSigma;
    return f;
  }
};
/* the maps a sequence carries (row-major, the camera's size; variance < 0: the pixel carries nothing) */
struct FusedDisparity { ImageSize size; std::vector<float> disparity, variance; };
/* the last fusion of a sequence (c_api.h bpvo_hip_disparity_fusion_info: fused, replaced, measured, filled, none, predicted, slot, motion) */
typedef bpvo_hip_disparity_fusion_info DisparityFusionInfo;
/* measurement variance (c_api.h "measurement variance", an extension with no reference member; off by default): in the stereo addFrame calls of
 * a sequence that fuses its disparities, the measurement's variance comes per pixel from the matching cost of the rectified pair instead of the
 * constant measurement_sigma^2.  Units: noiseSigma in grey levels, minSigma / maxSigma in disparity pixels; radius 1 .. 7.  No defaults are
 * guessed: On(...) takes all four. */
struct MeasurementVariance : public bpvo_hip_measurement_variance {
  MeasurementVariance() { mode = 0; radius = 0; noise_sigma = min_sigma = max_sigma = 0.0f; }
  static MeasurementVariance On(int radius_, float noiseSigma, float minSigma, float maxSigma)
  {
    MeasurementVariance v;
    v.mode = 1; v.radius = radius_; v.noise_sigma = noiseSigma; v.min_sigma = minSigma; v.max_sigma = maxSigma;
    return v;
  }
};
/* the variance map of a sequence's last stereo frame (row-major, the camera's size) */
struct MeasurementVarianceMap { ImageSize size; std::vector<float> variance; };
/* its class counts (c_api.h bpvo_hip_measurement_variance_info: invalid, border, flat, floor, ceiling, model) */
typedef bpvo_hip_measurement_variance_info MeasurementVarianceInfo;
/* Motion stereo (an extension: no reference member; c_api.h bpvo_hip_set_motion_stereo).  mode 0: off, every call is what it was.  mode 1: in
 * a sequence that fuses its disparities, the prediction of every pixel is refined by a short search along its epipolar line in the key frame of
 * the call's last estimate.  Units: minGain in pixels per disparity pixel, noiseSigma in grey levels, minSigma / maxSigma in disparity pixels,
 * gate in standard deviations; radius 1 .. 3, steps 1 .. 8.  No defaults are guessed: On(...) takes all seven. */
struct MotionStereo : public bpvo_hip_motion_stereo {
  MotionStereo() { mode = 0; radius = steps = 0; min_gain = noise_sigma = min_sigma = max_sigma = gate = 0.0f; }
  static MotionStereo On(int radius_, int steps_, float minGain, float noiseSigma, float minSigma, float maxSigma, float gate_)
  {
    MotionStereo v;
    v.mode = 1; v.radius = radius_; v.steps = steps_; v.min_gain = minGain; v.noise_sigma = noiseSigma; v.min_sigma = minSigma; v.max_sigma = maxSigma;
    v.gate = gate_;
    return v;
  }
};
/* the last frame's class counts, whether a launch was made, the second view's slot and motion (c_api.h bpvo_hip_motion_stereo_info) */
typedef bpvo_hip_motion_stereo_info MotionStereoInfo;
inline std::vector<float> packPoses(const std::vector<Matrix44>& poses)
{
  std::vector<float> M(16 * poses.size());
  for(size_t i = 0; i < poses.size(); ++i) std::memcpy(&M[16 * i], poses[i].data(), 16 * sizeof(float));
  return M;
}

struct PoseCovarianceEstimate {
  enum Status { kOk = BPVO_COV_OK, kIndefinite = BPVO_COV_INDEFINITE, kDegenerate = BPVO_COV_DEGENERATE, kNone = BPVO_COV_NONE };
  Pose pose;
  PoseCovariance covariance;
  float sigma;
  int numValid, level;
  Status status;
  PoseCovarianceEstimate() : sigma(0.0f), numValid(0), level(-1), status(kNone) {}
  explicit PoseCovarianceEstimate(const bpvo_hip_pose_covariance& r) : sigma(r.sigma), numValid(r.num_valid), level(r.level), status((Status) r.status)
  {
    std::memcpy(pose.data(), r.T, sizeof(r.T));
    std::memcpy(covariance.data(), r.covariance, sizeof(r.covariance));
  }
};

class Trajectory {                                              // bpvo/trajectory.h
 public:
  size_t size() const { return _poses.size(); }
  const Matrix44& operator[](size_t i) const { return _poses[i]; }
  const Matrix44& back() const { return _poses.back(); }
  const std::vector<Matrix44>& poses() const { return _poses; }
  /* Trajectory::push_back (bpvo/trajectory.cc:29-50): appends back() * InvertPose(T) with InvertPose as written there,
   * R' = R^T, t' = -(R'^T) t = -R t.  VisualOdometry fills its trajectory on the device side with the same rule; this
   * member is for callers that assemble a trajectory themselves (apps/eval_kitti.cc:120-130). */
  void push_back(const Matrix44& T)
  {
    Matrix44 Ti;
    for(int i = 0; i < 3; ++i)
      for(int j = 0; j < 3; ++j) Ti[i * 4 + j] = T[j * 4 + i];
    for(int i = 0; i < 3; ++i) Ti[i * 4 + 3] = -((T[i * 4 + 0] * T[3] + T[i * 4 + 1] * T[7]) + T[i * 4 + 2] * T[11]);
    Ti[12] = Ti[13] = Ti[14] = 0.0f;
    Ti[15] = 1.0f;
    if(_poses.empty()) { _poses.push_back(Ti); return; }
    const Matrix44& A = _poses.back();
    Matrix44 C;
    for(int r = 0; r < 4; ++r)
      for(int c = 0; c < 4; ++c) {
        float acc = A[r * 4 + 0] * Ti[0 * 4 + c];
        for(int k = 1; k < 4; ++k) acc += A[r * 4 + k] * Ti[k * 4 + c];
        C[r * 4 + c] = acc;
      }
    _poses.push_back(C);
  }
 private:
  friend class VisualOdometry;
  friend class VisualOdometrySequences;
  friend class RigVisualOdometry;
  friend class RigsVisualOdometry;
  std::vector<Matrix44> _poses;
};

namespace detail {
/* owns one bpvo_hip_ctx; maps a non-zero status to bpvo::Error (THROW_ERROR, bpvo/utils.h:211-220) */
class Device {
 public:
  Device(const Matrix33& K, float baseline, ImageSize size, const AlgorithmParameters& p, int n_frames, int n_pairs, int device = 0)
      : _ctx(nullptr), _size(size)
  {
    const int rc = bpvo_hip_create(&_ctx, K.data(), baseline, size.rows, size.cols, &p, device, n_frames, n_pairs);
    if(rc != BPVO_OK) throw Error(std::string("bpvo_hip_create: ") + bpvo_hip_last_error(nullptr));
  }
  /* bpvo_hip_create_sequences: one camera per sequence; the context's size is the largest of theirs */
  Device(const std::vector<bpvo_hip_camera>& cams, const AlgorithmParameters& p, int device = 0) : _ctx(nullptr), _size()
  {
    const int rc = bpvo_hip_create_sequences(&_ctx, (int) cams.size(), cams.data(), &p, device);
    if(rc != BPVO_OK) throw Error(std::string("bpvo_hip_create_sequences: ") + bpvo_hip_last_error(nullptr));
    for(const bpvo_hip_camera& c : cams) { _size.rows = std::max(_size.rows, c.rows); _size.cols = std::max(_size.cols, c.cols); }
  }
  ~Device() { bpvo_hip_destroy(_ctx); }
  Device(const Device&) = delete;
  Device& operator=(const Device&) = delete;
  bpvo_hip_ctx* ctx() const { return _ctx; }
  ImageSize imageSize() const { return _size; }
  void check(int rc) const { if(rc != BPVO_OK) throw Error(bpvo_hip_last_error(_ctx)); }
  /* how the device schedules its work (c_api.h "Options"); no counterpart in the reference */
  void setOption(const std::string& name, double value) { check(bpvo_hip_set_option(_ctx, name.c_str(), value)); }
  double getOption(const std::string& name) const { double v = 0.0; check(bpvo_hip_get_option(_ctx, name.c_str(), &v)); return v; }
  /* the point budget (c_api.h bpvo_hip_set_point_budget; an extension, no counterpart in the reference): the context's, or sequence seq's own */
  void setPointBudget(const std::vector<int>& maxPoints) { check(bpvo_hip_set_point_budget(_ctx, maxPoints.data(), (int) maxPoints.size())); }
  void setPointBudget(int seq, const std::vector<int>& maxPoints) { check(bpvo_hip_seq_set_point_budget(_ctx, seq, maxPoints.data(), (int) maxPoints.size())); }
  /* normalised intensity (c_api.h bpvo_hip_set_intensity_normalization; an extension, no counterpart in the reference) */
  void setIntensityNormalization(int radius) { check(bpvo_hip_set_intensity_normalization(_ctx, radius)); }
  int intensityNormalization() const { int r = -1; check(bpvo_hip_get_intensity_normalization(_ctx, &r)); return r; }
  /* finestLevel points at level 0 and a quarter of the level below at every level above it, rounded down to a multiple of 16, never below 256 */
  std::vector<int> quarteredPointBudget(int finestLevel) const
  {
    std::vector<int> b((size_t) bpvo_hip_num_levels(_ctx));
    for(size_t l = 0; l < b.size(); ++l) b[l] = std::max(256, (int) ((long long) finestLevel >> (2 * l)) & ~15);
    return b;
  }
 private:
  bpvo_hip_ctx* _ctx;
  ImageSize _size;
};
}  // namespace detail

/* bpvo::VisualOdometryFrame (bpvo/vo_frame.h:21-90): a device-resident frame = slot of a Device */
class VisualOdometryFrame {
 public:
  VisualOdometryFrame(std::shared_ptr<detail::Device> dev, int slot) : _dev(dev), _slot(slot) {}
  void setData(const uint8_t* image, const float* disparity) { _dev->check(bpvo_hip_frame_set_data(_dev->ctx(), _slot, image, disparity)); }
  void setTemplate() { _dev->check(bpvo_hip_frame_set_template(_dev->ctx(), _slot)); }
  void clear() { _dev->check(bpvo_hip_frame_clear(_dev->ctx(), _slot)); }
  bool empty() const { int d = 0, t = 0; _dev->check(bpvo_hip_frame_state(_dev->ctx(), _slot, &d, &t)); return !d; }
  bool hasTemplate() const { int d = 0, t = 0; _dev->check(bpvo_hip_frame_state(_dev->ctx(), _slot, &d, &t)); return t != 0; }
  int numLevels() const { return bpvo_hip_num_levels(_dev->ctx()); }
  int numPointsAtLevel(int level) const { int n = 0; _dev->check(bpvo_hip_num_points(_dev->ctx(), _slot, level, &n)); return n; }
  /* The frame lives in device memory; what the reference hands out as references to host containers
   * (imagePointer, getDenseDescriptorAtLevel()->getChannel, getTemplateDataAtLevel()->{points, pixels, jacobians},
   * bpvo/vo_frame.h:62-80, bpvo/template_data.h:68-75) is copied out on request. */
  ImageSize levelSize(int level) const
  {
    int r = 0, c = 0;
    _dev->check(bpvo_hip_level_size(_dev->ctx(), level, &r, &c));
    return ImageSize(r, c);
  }
  int numChannels() const { return bpvo_hip_num_channels(_dev->ctx()); }
  std::vector<uint8_t> image(int level = 0) const
  {
    std::vector<uint8_t> v((size_t) levelSize(level).numel());
    _dev->check(bpvo_hip_get_image(_dev->ctx(), _slot, level, v.data()));
    return v;
  }
  std::vector<float> descriptorChannel(int level, int channel) const
  {
    std::vector<float> v((size_t) levelSize(level).numel());
    _dev->check(bpvo_hip_get_descriptor_channel(_dev->ctx(), _slot, level, channel, v.data()));
    return v;
  }
  PointVector points(int level) const
  {
    PointVector v((size_t) numPointsAtLevel(level));
    if(!v.empty()) _dev->check(bpvo_hip_get_points(_dev->ctx(), _slot, level, v[0].data()));
    return v;
  }
  std::vector<float> pixels(int level) const           // [channel][point], TemplateData::pixels()
  {
    std::vector<float> v((size_t) numPointsAtLevel(level) * numChannels());
    if(!v.empty()) _dev->check(bpvo_hip_get_pixels(_dev->ctx(), _slot, level, v.data()));
    return v;
  }
  std::vector<float> jacobians(int level) const        // [channel][point][6], TemplateData::jacobians()
  {
    std::vector<float> v((size_t) numPointsAtLevel(level) * numChannels() * 6);
    if(!v.empty()) _dev->check(bpvo_hip_get_jacobians(_dev->ctx(), _slot, level, v.data()));
    return v;
  }
  /* normalised intensity (an extension; c_api.h bpvo_hip_set_intensity_normalization): -1 off, 0 whole image, 1 .. 15 local; the frame's context's, while none of its frames holds data */
  void setIntensityNormalization(int radius) { _dev->setIntensityNormalization(radius); }
  int intensityNormalization() const { return _dev->intensityNormalization(); }
  int slot() const { return _slot; }
  const std::shared_ptr<detail::Device>& device() const { return _dev; }
 private:
  std::shared_ptr<detail::Device> _dev;
  int _slot;
};

/* bpvo::VisualOdometryPoseEstimator (bpvo/vo_pose_estimator.h:34-64) */
class VisualOdometryPoseEstimator {
 public:
  explicit VisualOdometryPoseEstimator(std::shared_ptr<detail::Device> dev, int workspace = 0) : _dev(dev), _ws(workspace) {}
  std::vector<OptimizerStatistics> estimatePose(const VisualOdometryFrame* ref_frame, const VisualOdometryFrame* cur_frame,
                                                const Matrix44& T_init, Matrix44& T_est)
  {
    std::vector<bpvo_hip_stats> st(bpvo_hip_num_levels(_dev->ctx()));
    _dev->check(bpvo_hip_estimate_pose(_dev->ctx(), _ws, ref_frame->slot(), cur_frame->slot(), T_init.data(), T_est.data(), st.data()));
    std::vector<OptimizerStatistics> ret;
    for(const auto& s : st) ret.push_back(OptimizerStatistics(s));
    return ret;
  }
  /* Pose scoring (c_api.h bpvo_hip_score_poses; no counterpart in the reference): the truncated-L1 score of every pose of `poses` at pyramid
   * level `level`, one launch for all of them; tau in descriptor units (about 0.5 for bit-planes, about 30 grey levels for intensity).  Touches
   * nothing of the estimator's state. */
  std::vector<PoseScore> scorePoses(const VisualOdometryFrame* ref_frame, const VisualOdometryFrame* cur_frame, int level,
                                    const std::vector<Matrix44>& poses, float tau) const
  {
    std::vector<float> T(poses.size() * 16);
    for(size_t i = 0; i < poses.size(); ++i) std::memcpy(&T[16 * i], poses[i].data(), 16 * sizeof(float));
    std::vector<PoseScore> out(poses.size());
    _dev->check(bpvo_hip_score_poses(_dev->ctx(), ref_frame->slot(), cur_frame->slot(), level, (int) poses.size(), T.data(), tau, out.data()));
    return out;
  }
  /* estimatePose from the best-scoring of the candidate starts (ties: the first; scoreLevel < 0: the coarsest level): exactly
   * estimatePose(T_init = candidates[chosen]).  chosen / scores: which start it was and every candidate's score, where asked for. */
  std::vector<OptimizerStatistics> estimatePoseFromBest(const VisualOdometryFrame* ref_frame, const VisualOdometryFrame* cur_frame,
                                                        const std::vector<Matrix44>& candidates, float tau, Matrix44& T_est, int* chosen = nullptr,
                                                        std::vector<PoseScore>* scores = nullptr, int scoreLevel = -1)
  {
    std::vector<float> T(candidates.size() * 16);
    for(size_t i = 0; i < candidates.size(); ++i) std::memcpy(&T[16 * i], candidates[i].data(), 16 * sizeof(float));
    std::vector<bpvo_hip_stats> st(bpvo_hip_num_levels(_dev->ctx()));
    if(scores) scores->resize(candidates.size());
    _dev->check(bpvo_hip_estimate_pose_best_start(_dev->ctx(), _ws, ref_frame->slot(), cur_frame->slot(), (int) candidates.size(), T.data(), scoreLevel, tau,
                                                  T_est.data(), st.data(), chosen, scores ? scores->data() : nullptr));
    std::vector<OptimizerStatistics> ret;
    for(const auto& s : st) ret.push_back(OptimizerStatistics(s));
    return ret;
  }
  /* normalised intensity (an extension; c_api.h bpvo_hip_set_intensity_normalization): -1 off, 0 whole image, 1 .. 15 local; the estimator's context's, while none of its frames holds data */
  void setIntensityNormalization(int radius) { _dev->setIntensityNormalization(radius); }
  int intensityNormalization() const { return _dev->intensityNormalization(); }
  float getFractionOfGoodPoints(float thresh) const
  {
    float f = 0.0f;
    _dev->check(bpvo_hip_fraction_good(_dev->ctx(), _ws, thresh, &f));
    return f;
  }
  const WeightsVector& getWeights() const
  {
    size_t n = 0;
    _dev->check(bpvo_hip_get_weights(_dev->ctx(), _ws, nullptr, &n));
    _weights.resize(n);
    if(n) _dev->check(bpvo_hip_get_weights(_dev->ctx(), _ws, _weights.data(), &n));
    return _weights;
  }
 private:
  std::shared_ptr<detail::Device> _dev;
  int _ws;
  mutable WeightsVector _weights;
};

/* Block-matching parameters of the reference's StereoAlgorithm (utils/stereo_algorithm.cc:63-82: the CvStereoBMState fields it sets,
 * with its defaults; numberOfDisparities "must be provided") */
struct StereoParameters : bpvo_hip_stereo_params {
  explicit StereoParameters(int number_of_disparities)
  {
    bpvo_hip_default_stereo_params(this);
    numberOfDisparities = number_of_disparities;
  }
  /* `StereoAlgorithm = SGM` (utils/stereo_algorithm.cc:42-59): the in-tree semi-global matcher with SgmStereo::Config() defaults
   * (utils/sgm.cc:47-56; the KITTI evaluation of the reference runs it: conf/kitti_eval.cfg:27) */
  static StereoParameters SemiGlobalMatching(int number_of_disparities = 128)
  {
    StereoParameters p(number_of_disparities);
    p.algorithm = BPVO_STEREO_SGM;
    return p;
  }
  /* `StereoAlgorithm = SGBM` (utils/stereo_algorithm.cc:27-40; conf/kitti_seq_0.cfg:6): cv::StereoSGBM as the reference's constructor call
   * builds it from the config KEYS (defaults of the cf.get calls) — nine positional arguments into a constructor of eleven, the keys land one
   * slot off (include/bpvo_hip/c_api.h).  Set the cv::StereoSGBM fields of the struct directly for the matcher as OpenCV documents it. */
  static StereoParameters SemiGlobalBlockMatching(int minDisparity, int numberOfDisparities, int SADWindowSize = 3, int P1 = 0, int P2 = 0,
                                                  int uniquenessRatio = 0, int speckleWindowSize = 0, int speckleRange = 0, int fullDP = 0)
  {
    StereoParameters p(numberOfDisparities);
    bpvo_hip_stereo_params_sgbm_from_config(&p, minDisparity, numberOfDisparities, SADWindowSize, P1, P2, uniquenessRatio, speckleWindowSize,
                                            speckleRange, fullDP);
    return p;
  }
};

/* bpvo::VisualOdometry (bpvo/vo.h:31-105).  The keyframe state machine of bpvo/vo.cc:125-224 runs inside the library
 * on three device-resident frames. */
class VisualOdometry {
 public:
  VisualOdometry(const Matrix33& K, float baseline, ImageSize image_size, const AlgorithmParameters& params = AlgorithmParameters(),
                 int device = 0)
      : _dev(std::make_shared<detail::Device>(K, baseline, image_size, params, 3, 1, device)), _max_test_level(params.maxTestLevel) {}

  /* reference: template <class CalibrationT> VisualOdometry(const CalibrationT&, ImageSize, const AlgorithmParameters&)
   * (bpvo/vo.h:49-52): any type with members K (Matrix33) and baseline */
  template <class CalibrationT>
  VisualOdometry(const CalibrationT& calib, ImageSize image_size, const AlgorithmParameters& params = AlgorithmParameters())
      : VisualOdometry(calib.K, calib.baseline, image_size, params) {}

  /* reference: template <class DataLoaderT> VisualOdometry(const DataLoaderT*, const AlgorithmParameters&) (bpvo/vo.h:57-60):
   * any type with calibration() and imageSize() — what apps/vo_perf.cc:56 calls with its Dataset */
  template <class DataLoaderT>
  VisualOdometry(const DataLoaderT* data_loader, const AlgorithmParameters& params = AlgorithmParameters())
      : VisualOdometry(data_loader->calibration(), data_loader->imageSize(), params) {}

  /* reference: template <class FramePointer> Result addFrame(const FramePointer&) (bpvo/vo.h:76-80): a (smart) pointer to a
   * frame whose image() / disparity() return matrices with a cv::Mat-style ptr<T>() (utils/dataset.h DatasetFrame) */
  template <class FramePointer>
  Result addFrame(const FramePointer& frame)
  {
    return this->addFrame(frame->image().template ptr<const uint8_t>(), frame->disparity().template ptr<const float>());
  }

  /* reference: Result addFrame(const uint8_t* image, const float* disparity) (bpvo/vo.h:71, bpvo/vo.cc:66-72) */
  Result addFrame(const uint8_t* image, const float* disparity)
  {
    if(image == nullptr || disparity == nullptr) throw Error("nullptr image/disparity");
    bpvo_hip_result r;
    _dev->check(bpvo_hip_add_frame(_dev->ctx(), image, disparity, &r));
    return makeResult(r);
  }

  /* The reference's apps compute the disparity with StereoAlgorithm::run(left, right, dmap) (utils/stereo_algorithm.h:24-30; block
   * matching by default) and pass it to addFrame.  Here both steps run on the device and the f32 map never crosses the bus. */
  Result addFrame(const uint8_t* left, const uint8_t* right, const StereoParameters& stereo)
  {
    if(left == nullptr || right == nullptr) throw Error("nullptr image");
    bpvo_hip_result r;
    _dev->check(bpvo_hip_add_frame_stereo(_dev->ctx(), left, right, &stereo, &r));
    return makeResult(r);
  }

  /* Raw (distorted, unrectified) pairs (an extension; c_api.h "rectification on the device"): the map of a side (0 left, 1 right) from a lens
   * or from the caller's f32 maps of the camera's size; addFrameRaw rectifies the pair on the device and runs the call above on the result,
   * which never visits the host. */
  void setRectification(int side, const bpvo_hip_lens& lens) { _dev->check(bpvo_hip_set_rectification(_dev->ctx(), side, &lens)); }
  void setRectificationMaps(int side, int rawRows, int rawCols, const float* mapx, const float* mapy)
  {
    _dev->check(bpvo_hip_set_rectification_maps(_dev->ctx(), side, rawRows, rawCols, mapx, mapy));
  }
  void clearRectification() { _dev->check(bpvo_hip_clear_rectification(_dev->ctx())); }
  Result addFrameRaw(const uint8_t* leftRaw, const uint8_t* rightRaw, const StereoParameters& stereo)
  {
    if(leftRaw == nullptr || rightRaw == nullptr) throw Error("nullptr image");
    bpvo_hip_result r;
    _dev->check(bpvo_hip_add_frame_stereo_raw(_dev->ctx(), leftRaw, rightRaw, &stereo, &r));
    return makeResult(r);
  }

  int numPointsAtLevel(int level = -1) const                     // bpvo/vo.h:86
  {
    int n = 0;
    _dev->check(bpvo_hip_vo_num_points_at_level(_dev->ctx(), level, &n));
    return n;
  }
  const PointVector& pointsAtLevel(int level = -1) const         // bpvo/vo.h:92
  {
    _points.resize(numPointsAtLevel(level));
    if(!_points.empty()) _dev->check(bpvo_hip_vo_points_at_level(_dev->ctx(), level, _points[0].data()));
    return _points;
  }
  const Trajectory& trajectory() const { return _trajectory; }   // bpvo/vo.h:98
  /* scheduling options of the device context (c_api.h "Options"; the reference has none) */
  void setOption(const std::string& name, double value) { _dev->setOption(name, value); }
  /* normalised intensity (an extension; c_api.h bpvo_hip_set_intensity_normalization): -1 off, 0 whole image, 1 .. 15 local; before the first frame */
  void setIntensityNormalization(int radius) { _dev->setIntensityNormalization(radius); }
  int intensityNormalization() const { return _dev->intensityNormalization(); }
  /* at most maxPoints[l] template points at level l, the most salient first (an extension; c_api.h bpvo_hip_set_point_budget); from the next key frame on */
  void setPointBudget(const std::vector<int>& maxPoints) { _dev->setPointBudget(maxPoints); }
  /* ... given for the finest level, a quarter of it per level above (multiples of 16, never below 256) */
  void setPointBudget(int finestLevelPoints) { _dev->setPointBudget(_dev->quarteredPointBudget(finestLevelPoints)); }
  double getOption(const std::string& name) const { return _dev->getOption(name); }
  /* where addFrame starts Gauss-Newton (an extension; c_api.h bpvo_hip_set_start_policy), the hints of the next estimate (frame-to-frame guesses in
   * Result::pose's convention), and what estimate `which` of the last addFrame started from (0: against the key frame, 1: the re-estimate) */
  void setStartPolicy(const StartPolicy& policy) { _dev->check(bpvo_hip_set_start_policy(_dev->ctx(), &policy)); }
  void setStartHints(const std::vector<Matrix44>& hints) { const std::vector<float> M = packPoses(hints); _dev->check(bpvo_hip_vo_set_start_hints(_dev->ctx(), (int) hints.size(), M.data())); }
  StartInfo startInfo(int which = 0) const { StartInfo r; _dev->check(bpvo_hip_vo_start_info(_dev->ctx(), which, &r)); return r; }
  /* disparity fusion (an extension; c_api.h bpvo_hip_set_disparity_fusion): the setting, the carried maps, the record of the last frame's fusion */
  void setDisparityFusion(const DisparityFusion& fusion) { _dev->check(bpvo_hip_set_disparity_fusion(_dev->ctx(), &fusion)); }
  FusedDisparity fusedDisparity() const
  {
    FusedDisparity r;
    r.size = _dev->imageSize();
    r.disparity.resize((size_t) r.size.rows * (size_t) r.size.cols);
    r.variance.resize(r.disparity.size());
    _dev->check(bpvo_hip_vo_get_fused_disparity(_dev->ctx(), r.disparity.data(), r.variance.data()));
    return r;
  }
  DisparityFusionInfo disparityFusionInfo() const { DisparityFusionInfo r; _dev->check(bpvo_hip_vo_disparity_fusion_info(_dev->ctx(), &r)); return r; }
  /* measurement variance (an extension; c_api.h bpvo_hip_set_measurement_variance): the setting, the last stereo frame's map and its class counts */
  void setMeasurementVariance(const MeasurementVariance& setting) { _dev->check(bpvo_hip_set_measurement_variance(_dev->ctx(), &setting)); }
  MeasurementVarianceMap measurementVariance() const
  {
    MeasurementVarianceMap r;
    r.size = _dev->imageSize();
    r.variance.resize((size_t) r.size.rows * r.size.cols);
    _dev->check(bpvo_hip_vo_get_measurement_variance(_dev->ctx(), r.variance.data()));
    return r;
  }
  MeasurementVarianceInfo measurementVarianceInfo() const { MeasurementVarianceInfo r; _dev->check(bpvo_hip_vo_measurement_variance_info(_dev->ctx(), &r)); return r; }
  /* motion stereo (an extension; c_api.h bpvo_hip_set_motion_stereo): the setting and the last frame's record */
  void setMotionStereo(const MotionStereo& setting) { _dev->check(bpvo_hip_set_motion_stereo(_dev->ctx(), &setting)); }
  MotionStereo motionStereo() const
  {
    MotionStereo r;
    _dev->check(bpvo_hip_get_motion_stereo(_dev->ctx(), &r));
    return r;
  }
  MotionStereoInfo motionStereoInfo() const { MotionStereoInfo r; _dev->check(bpvo_hip_vo_motion_stereo_info(_dev->ctx(), &r)); return r; }
  /* Result::covariance carries the covariance of the estimated pose (option "pose_covariance"); poseCovariance(): the last frame's record */
  void setPoseCovariance(bool on) { _dev->setOption("pose_covariance", on ? 1.0 : 0.0); }
  PoseCovarianceEstimate poseCovariance() const
  {
    bpvo_hip_pose_covariance r;
    _dev->check(bpvo_hip_vo_pose_covariance(_dev->ctx(), &r));
    return PoseCovarianceEstimate(r);
  }

 private:
  Result makeResult(const bpvo_hip_result& r)
  {
    Result ret;
    std::memcpy(ret.pose.data(), r.pose, sizeof(r.pose));
    std::memcpy(ret.covariance.data(), r.covariance, sizeof(r.covariance));
    for(int i = 0; i < r.numLevels; ++i) ret.optimizerStatistics.push_back(OptimizerStatistics(r.optimizerStatistics[i]));
    ret.isKeyFrame = r.isKeyFrame != 0;
    ret.keyFramingReason = static_cast<KeyFramingReason>(r.keyFramingReason);
    if(r.hasPointCloud) {
      size_t n = 0;
      _dev->check(bpvo_hip_get_point_cloud(_dev->ctx(), nullptr, &n, nullptr));
      ret.pointCloud.reset(new PointCloud);
      ret.pointCloud->points().resize(n);
      _dev->check(bpvo_hip_get_point_cloud(_dev->ctx(), ret.pointCloud->points().data(), &n, ret.pointCloud->pose().data()));
    }
    int nt = 0;
    _dev->check(bpvo_hip_trajectory_size(_dev->ctx(), &nt));
    _trajectory._poses.resize(nt);
    if(nt) _dev->check(bpvo_hip_get_trajectory(_dev->ctx(), _trajectory._poses[0].data()));
    return ret;
  }
  std::shared_ptr<detail::Device> _dev;
  int _max_test_level;
  Trajectory _trajectory;
  mutable PointVector _points;
};

/* Many independent VisualOdometry sequences (cameras of a rig, the sequences of an evaluation, a parameter sweep) advanced together by one
 * device context: addFrames runs addFrame for each of them, and every sequence's results equal, bit for bit, those of a VisualOdometry of
 * its own fed the same frames.  No counterpart in the reference. */
class VisualOdometrySequences {
 public:
  /* one calibration and image size of a sequence (bpvo_hip_camera) */
  struct Camera {
    Matrix33 K;
    float baseline;
    ImageSize size;
    Camera() : K(), baseline(0.0f), size() {}
    Camera(const Matrix33& K_, float b, ImageSize s) : K(K_), baseline(b), size(s) {}
  };

  VisualOdometrySequences(const Matrix33& K, float baseline, ImageSize image_size, int num_sequences,
                          const AlgorithmParameters& params = AlgorithmParameters(), int device = 0)
      : _dev(std::make_shared<detail::Device>(K, baseline, image_size, params, 3 * num_sequences, num_sequences, device)),
        _trajectories((size_t) (num_sequences > 0 ? num_sequences : 0)) {}
  /* sequence s with cameras[s] (bpvo_hip_create_sequences: the context's image size is the largest rows and cols among them) */
  VisualOdometrySequences(const std::vector<Camera>& cameras, const AlgorithmParameters& params = AlgorithmParameters(), int device = 0)
      : _dev(std::make_shared<detail::Device>(toC(cameras), params, device)), _trajectories(cameras.size()) {}
  /* ... and with parameters[s] (a parameter sweep): the context is created with parameters[0], which fixes the pyramid, the descriptor and the
   * other structural fields for all of them (setParameters) */
  VisualOdometrySequences(const std::vector<Camera>& cameras, const std::vector<AlgorithmParameters>& parameters, int device = 0)
      : _dev(std::make_shared<detail::Device>(toC(cameras), parameters.empty() ? AlgorithmParameters() : parameters[0], device)),
        _trajectories(cameras.size())
  {
    if(parameters.size() != cameras.size()) throw Error("one AlgorithmParameters per camera");
    for(size_t s = 1; s < parameters.size(); ++s) setParameters((int) s, parameters[s]);
  }

  int numSequences() const { int n = 0; _dev->check(bpvo_hip_seq_capacity(_dev->ctx(), &n)); return n; }

  /* the camera of sequence s, changed only while it holds no frame (new, or after reset(s)) and within the context's size */
  void setCamera(int s, const Camera& cam) { const bpvo_hip_camera c = toC(cam); _dev->check(bpvo_hip_seq_set_camera(_dev->ctx(), s, &c)); }
  Camera camera(int s) const
  {
    bpvo_hip_camera c;
    _dev->check(bpvo_hip_seq_get_camera(_dev->ctx(), s, &c));
    Camera r;
    std::memcpy(r.K.data(), c.K, sizeof(c.K));
    r.baseline = c.baseline;
    r.size = ImageSize(c.rows, c.cols);
    return r;
  }

  /* the algorithm parameters of sequence s (bpvo_hip_seq_set_params), changed only while it holds no frame: loss, iteration limit, tolerances,
   * key-framing thresholds, minSaliency and the disparity gate are the sequence's own; the structural fields (pyramid, descriptor, gradient,
   * interpolation, non-maximum suppression, maxTestLevel) must equal the context's */
  void setParameters(int s, const AlgorithmParameters& p) { _dev->check(bpvo_hip_seq_set_params(_dev->ctx(), s, &p)); }
  AlgorithmParameters parameters(int s) const
  {
    AlgorithmParameters p;
    _dev->check(bpvo_hip_seq_get_params(_dev->ctx(), s, &p));
    return p;
  }

  /* images / disparities: n frames back to back, frame i of its sequence's size (camera(seq[i]).size; one context-wide camera: rows * cols
   * pixels each); frame i is the next frame of sequence seq[i] (seq = nullptr: sequences 0 .. n-1; n = -1: every sequence).  Each Result
   * carries its point cloud, as VisualOdometry::addFrame's does. */
  std::vector<Result> addFrames(const uint8_t* images, const float* disparities, const int* seq = nullptr, int n = -1)
  {
    if(images == nullptr || disparities == nullptr) throw Error("nullptr image/disparity");
    if(n < 0) n = numSequences();
    std::vector<bpvo_hip_result> r((size_t) n);
    _dev->check(bpvo_hip_add_frames(_dev->ctx(), n, seq, images, disparities, 0, r.data()));
    std::vector<Result> ret;
    for(int i = 0; i < n; ++i) ret.push_back(makeResult(seq ? seq[i] : i, r[i]));
    return ret;
  }

  /* The same from rectified pairs, as the reference's apps feed every camera (apps/vo_app.cc: StereoAlgorithm::run(left, right), then
   * addFrame): left / right hold n images back to back, pair i of its sequence's size; the disparities are computed on the device in
   * each camera's own geometry and stay there (bpvo_hip_add_frames_stereo).  One StereoParameters serves the call. */
  std::vector<Result> addFrames(const uint8_t* left, const uint8_t* right, const StereoParameters& stereo, const int* seq = nullptr, int n = -1)
  {
    if(left == nullptr || right == nullptr) throw Error("nullptr image");
    if(n < 0) n = numSequences();
    std::vector<bpvo_hip_result> r((size_t) n);
    _dev->check(bpvo_hip_add_frames_stereo(_dev->ctx(), n, seq, left, right, 0, &stereo, r.data()));
    std::vector<Result> ret;
    for(int i = 0; i < n; ++i) ret.push_back(makeResult(seq ? seq[i] : i, r[i]));
    return ret;
  }

  /* ... and from raw (distorted, unrectified) pairs (an extension; c_api.h "rectification on the device"): the map of side `side` (0 left, 1
   * right) of sequence s from a lens or from the caller's f32 maps of the camera's size — setCamera(s, ...) clears both sides —; addFramesRaw
   * rectifies every pair of the call in one launch (pair i of the raw sizes of sequence seq[i]'s sides, the raw images back to back) and runs
   * the call above on the result, which never visits the host (bpvo_hip_add_frames_stereo_raw). */
  void setRectification(int s, int side, const bpvo_hip_lens& lens) { _dev->check(bpvo_hip_seq_set_rectification(_dev->ctx(), s, side, &lens)); }
  void setRectificationMaps(int s, int side, int rawRows, int rawCols, const float* mapx, const float* mapy)
  {
    _dev->check(bpvo_hip_seq_set_rectification_maps(_dev->ctx(), s, side, rawRows, rawCols, mapx, mapy));
  }
  void clearRectification(int s) { _dev->check(bpvo_hip_seq_clear_rectification(_dev->ctx(), s)); }
  std::vector<Result> addFramesRaw(const uint8_t* leftRaw, const uint8_t* rightRaw, const StereoParameters& stereo, const int* seq = nullptr, int n = -1)
  {
    if(leftRaw == nullptr || rightRaw == nullptr) throw Error("nullptr image");
    if(n < 0) n = numSequences();
    std::vector<bpvo_hip_result> r((size_t) n);
    _dev->check(bpvo_hip_add_frames_stereo_raw(_dev->ctx(), n, seq, leftRaw, rightRaw, 0, &stereo, r.data()));
    std::vector<Result> ret;
    for(int i = 0; i < n; ++i) ret.push_back(makeResult(seq ? seq[i] : i, r[i]));
    return ret;
  }

  const Trajectory& trajectory(int s) const { return _trajectories.at((size_t) s); }
  int numPointsAtLevel(int s, int level = -1) const
  {
    int n = 0;
    _dev->check(bpvo_hip_seq_num_points_at_level(_dev->ctx(), s, level, &n));
    return n;
  }
  /* the next frame of sequence s starts it again (a first frame: Result::keyFramingReason == KeyFramingReason::kFirstFrame) */
  void reset(int s)
  {
    _dev->check(bpvo_hip_seq_reset(_dev->ctx(), s));
    _trajectories.at((size_t) s)._poses.clear();
  }
  void setOption(const std::string& name, double value) { _dev->setOption(name, value); }
  /* normalised intensity (an extension; c_api.h bpvo_hip_set_intensity_normalization): -1 off, 0 whole image, 1 .. 15 local; before the first frame */
  void setIntensityNormalization(int radius) { _dev->setIntensityNormalization(radius); }
  int intensityNormalization() const { return _dev->intensityNormalization(); }
  /* at most maxPoints[l] template points at level l of sequence s, the most salient first (an extension; c_api.h bpvo_hip_seq_set_point_budget); an
   * empty list returns the sequence to the context's budget */
  void setPointBudget(int s, const std::vector<int>& maxPoints) { _dev->setPointBudget(s, maxPoints); }
  /* ... given for the finest level, a quarter of it per level above (multiples of 16, never below 256) */
  void setPointBudget(int s, int finestLevelPoints) { _dev->setPointBudget(s, _dev->quarteredPointBudget(finestLevelPoints)); }
  /* where the sequences start Gauss-Newton (an extension; c_api.h bpvo_hip_set_start_policy): every sequence's, or sequence s's own; the hints of
   * sequence s's next estimate; what estimate `which` of its last frame started from */
  void setStartPolicy(const StartPolicy& policy) { _dev->check(bpvo_hip_set_start_policy(_dev->ctx(), &policy)); }
  void setStartPolicy(int s, const StartPolicy& policy) { _dev->check(bpvo_hip_seq_set_start_policy(_dev->ctx(), s, &policy)); }
  void setStartHints(int s, const std::vector<Matrix44>& hints) { const std::vector<float> M = packPoses(hints); _dev->check(bpvo_hip_seq_set_start_hints(_dev->ctx(), s, (int) hints.size(), M.data())); }
  StartInfo startInfo(int s, int which = 0) const { StartInfo r; _dev->check(bpvo_hip_seq_start_info(_dev->ctx(), s, which, &r)); return r; }
  /* disparity fusion (an extension; c_api.h bpvo_hip_set_disparity_fusion): every sequence's setting, or sequence s's own; the maps sequence s
   * carries; the record of its last frame's fusion */
  void setDisparityFusion(const DisparityFusion& fusion) { _dev->check(bpvo_hip_set_disparity_fusion(_dev->ctx(), &fusion)); }
  void setDisparityFusion(int s, const DisparityFusion& fusion) { _dev->check(bpvo_hip_seq_set_disparity_fusion(_dev->ctx(), s, &fusion)); }
  FusedDisparity fusedDisparity(int s) const
  {
    bpvo_hip_camera c;
    _dev->check(bpvo_hip_seq_get_camera(_dev->ctx(), s, &c));
    FusedDisparity r;
    r.size = ImageSize(c.rows, c.cols);
    r.disparity.resize((size_t) c.rows * (size_t) c.cols);
    r.variance.resize(r.disparity.size());
    _dev->check(bpvo_hip_seq_get_fused_disparity(_dev->ctx(), s, r.disparity.data(), r.variance.data()));
    return r;
  }
  DisparityFusionInfo disparityFusionInfo(int s) const { DisparityFusionInfo r; _dev->check(bpvo_hip_seq_disparity_fusion_info(_dev->ctx(), s, &r)); return r; }
  /* measurement variance (an extension; c_api.h bpvo_hip_set_measurement_variance): every sequence's setting, or sequence s's own; the map of
   * sequence s's last stereo frame and its class counts */
  void setMeasurementVariance(const MeasurementVariance& setting) { _dev->check(bpvo_hip_set_measurement_variance(_dev->ctx(), &setting)); }
  void setMeasurementVariance(int s, const MeasurementVariance& setting) { _dev->check(bpvo_hip_seq_set_measurement_variance(_dev->ctx(), s, &setting)); }
  MeasurementVarianceMap measurementVariance(int s) const
  {
    bpvo_hip_camera c;
    _dev->check(bpvo_hip_seq_get_camera(_dev->ctx(), s, &c));
    MeasurementVarianceMap r;
    r.size = ImageSize(c.rows, c.cols);
    r.variance.resize((size_t) c.rows * c.cols);
    _dev->check(bpvo_hip_seq_get_measurement_variance_map(_dev->ctx(), s, r.variance.data()));
    return r;
  }
  MeasurementVarianceInfo measurementVarianceInfo(int s) const { MeasurementVarianceInfo r; _dev->check(bpvo_hip_seq_measurement_variance_info(_dev->ctx(), s, &r)); return r; }
  /* motion stereo (an extension; c_api.h bpvo_hip_set_motion_stereo): every sequence's setting, or sequence s's own; sequence s's last record */
  void setMotionStereo(const MotionStereo& setting) { _dev->check(bpvo_hip_set_motion_stereo(_dev->ctx(), &setting)); }
  void setMotionStereo(int s, const MotionStereo& setting) { _dev->check(bpvo_hip_seq_set_motion_stereo(_dev->ctx(), s, &setting)); }
  MotionStereo motionStereo(int s) const
  {
    MotionStereo r;
    _dev->check(bpvo_hip_seq_get_motion_stereo(_dev->ctx(), s, &r, nullptr));
    return r;
  }
  MotionStereoInfo motionStereoInfo(int s) const { MotionStereoInfo r; _dev->check(bpvo_hip_seq_motion_stereo_info(_dev->ctx(), s, &r)); return r; }
  double getOption(const std::string& name) const { return _dev->getOption(name); }
  /* Result::covariance of every sequence carries the covariance of its estimated pose (option "pose_covariance"); poseCovariance(s): sequence s's last record */
  void setPoseCovariance(bool on) { _dev->setOption("pose_covariance", on ? 1.0 : 0.0); }
  PoseCovarianceEstimate poseCovariance(int s) const
  {
    bpvo_hip_pose_covariance r;
    _dev->check(bpvo_hip_seq_pose_covariance(_dev->ctx(), s, &r));
    return PoseCovarianceEstimate(r);
  }

 private:
  static bpvo_hip_camera toC(const Camera& cam)
  {
    bpvo_hip_camera c;
    std::memcpy(c.K, cam.K.data(), sizeof(c.K));
    c.baseline = cam.baseline;
    c.rows = cam.size.rows; c.cols = cam.size.cols;
    return c;
  }
  static std::vector<bpvo_hip_camera> toC(const std::vector<Camera>& cams)
  {
    std::vector<bpvo_hip_camera> v;
    for(const Camera& c : cams) v.push_back(toC(c));
    return v;
  }
  Result makeResult(int s, const bpvo_hip_result& r)
  {
    Result ret;
    std::memcpy(ret.pose.data(), r.pose, sizeof(r.pose));
    std::memcpy(ret.covariance.data(), r.covariance, sizeof(r.covariance));
    for(int i = 0; i < r.numLevels; ++i) ret.optimizerStatistics.push_back(OptimizerStatistics(r.optimizerStatistics[i]));
    ret.isKeyFrame = r.isKeyFrame != 0;
    ret.keyFramingReason = static_cast<KeyFramingReason>(r.keyFramingReason);
    if(r.hasPointCloud) {
      size_t n = 0;
      _dev->check(bpvo_hip_seq_get_point_cloud(_dev->ctx(), s, nullptr, &n, nullptr));
      ret.pointCloud.reset(new PointCloud);
      ret.pointCloud->points().resize(n);
      _dev->check(bpvo_hip_seq_get_point_cloud(_dev->ctx(), s, ret.pointCloud->points().data(), &n, ret.pointCloud->pose().data()));
    }
    int nt = 0;
    _dev->check(bpvo_hip_seq_trajectory_size(_dev->ctx(), s, &nt));
    Trajectory& t = _trajectories.at((size_t) s);
    t._poses.resize(nt);
    if(nt) _dev->check(bpvo_hip_seq_get_trajectory(_dev->ctx(), s, t._poses[0].data()));
    return ret;
  }
  std::shared_ptr<detail::Device> _dev;
  std::vector<Trajectory> _trajectories;
};

/* The cameras of a rigid rig estimated as ONE body: addFrame takes the next frame of every camera and returns a single 6-DoF body pose, estimated
 * from all cameras' residuals at once, with one key-frame decision for the rig (bpvo_hip_add_frames_rig; the mathematics: c_api.h).  Camera p
 * sits at extrinsics[p], camera_from_body (x_cam = X_p x_body, rigid).  No counterpart in the reference, which is single-camera. */
class RigVisualOdometry {
 public:
  typedef VisualOdometrySequences::Camera Camera;

  RigVisualOdometry(const std::vector<Camera>& cameras, const std::vector<Matrix44>& extrinsics, const AlgorithmParameters& params = AlgorithmParameters(),
                    int device = 0)
      : _dev(std::make_shared<detail::Device>(toC(cameras), params, device)), _n((int) cameras.size())
  {
    if(extrinsics.size() != cameras.size()) throw Error("one extrinsic per camera");
    std::vector<float> X;
    for(const Matrix44& x : extrinsics) X.insert(X.end(), x.data(), x.data() + 16);
    _dev->check(bpvo_hip_rig_set(_dev->ctx(), _n, nullptr, X.data()));
  }

  int numCameras() const { return _n; }

  /* images / disparities: the cameras' frames back to back in camera order, each of its camera's size.  The Result is the body's: its pose maps the
   * previous body frame to this one, its covariance is the Identity unless setPoseCovariance(true); at a key frame the cameras' point clouds are fetched with pointCloud(camera)
   * (Result::pointCloud stays empty: there is one cloud per camera). */
  Result addFrame(const uint8_t* images, const float* disparities)
  {
    if(images == nullptr || disparities == nullptr) throw Error("nullptr image/disparity");
    bpvo_hip_result r;
    _dev->check(bpvo_hip_add_frames_rig(_dev->ctx(), images, disparities, 0, &r));
    Result ret;
    std::memcpy(ret.pose.data(), r.pose, sizeof(r.pose));
    std::memcpy(ret.covariance.data(), r.covariance, sizeof(r.covariance));
    for(int i = 0; i < r.numLevels; ++i) ret.optimizerStatistics.push_back(OptimizerStatistics(r.optimizerStatistics[i]));
    ret.isKeyFrame = r.isKeyFrame != 0;
    ret.keyFramingReason = static_cast<KeyFramingReason>(r.keyFramingReason);
    _hasPointClouds = r.hasPointCloud != 0;
    int nt = 0;
    _dev->check(bpvo_hip_rig_trajectory_size(_dev->ctx(), &nt));
    _trajectory._poses.resize(nt);
    if(nt) _dev->check(bpvo_hip_rig_get_trajectory(_dev->ctx(), _trajectory._poses[0].data()));
    return ret;
  }
  /* did the last addFrame leave point clouds (a key frame after the first)? */
  bool hasPointClouds() const { return _hasPointClouds; }
  /* the point cloud of a camera from the last addFrame (empty unless hasPointClouds()); its pose is world_from_camera, W_kf X_p^-1 */
  PointCloud pointCloud(int camera) const
  {
    PointCloud pc;
    size_t n = 0;
    _dev->check(bpvo_hip_seq_get_point_cloud(_dev->ctx(), camera, nullptr, &n, nullptr));
    pc.points().resize(n);
    _dev->check(bpvo_hip_seq_get_point_cloud(_dev->ctx(), camera, pc.points().data(), &n, pc.pose().data()));
    return pc;
  }
  /* the body's trajectory */
  const Trajectory& trajectory() const { return _trajectory; }
  int numPointsAtLevel(int camera, int level = -1) const
  {
    int n = 0;
    _dev->check(bpvo_hip_seq_num_points_at_level(_dev->ctx(), camera, level, &n));
    return n;
  }
  void setOption(const std::string& name, double value) { _dev->setOption(name, value); }
  /* normalised intensity (an extension; c_api.h bpvo_hip_set_intensity_normalization): -1 off, 0 whole image, 1 .. 15 local; before the first frame */
  void setIntensityNormalization(int radius) { _dev->setIntensityNormalization(radius); }
  int intensityNormalization() const { return _dev->intensityNormalization(); }
  /* at most maxPoints[l] template points at level l, the most salient first (an extension; c_api.h bpvo_hip_set_point_budget); from the next key frame on */
  void setPointBudget(const std::vector<int>& maxPoints) { _dev->setPointBudget(maxPoints); }
  /* ... given for the finest level, a quarter of it per level above (multiples of 16, never below 256) */
  void setPointBudget(int finestLevelPoints) { _dev->setPointBudget(_dev->quarteredPointBudget(finestLevelPoints)); }
  /* where the body starts Gauss-Newton (an extension; c_api.h bpvo_hip_rigs_set_start_policy on rig 0), the hints of its next estimate (body
   * motions), what estimate `which` of its last frame started from */
  void setStartPolicy(const StartPolicy& policy) { _dev->check(bpvo_hip_rigs_set_start_policy(_dev->ctx(), 0, &policy)); }
  void setStartHints(const std::vector<Matrix44>& hints) { const std::vector<float> M = packPoses(hints); _dev->check(bpvo_hip_rigs_set_start_hints(_dev->ctx(), 0, (int) hints.size(), M.data())); }
  StartInfo startInfo(int which = 0) const { StartInfo r; _dev->check(bpvo_hip_rigs_start_info(_dev->ctx(), 0, which, &r)); return r; }
  double getOption(const std::string& name) const { return _dev->getOption(name); }
  /* Result::covariance carries the covariance of the BODY pose, in the plain body twist (option "pose_covariance"); poseCovariance(): the last frame's record */
  void setPoseCovariance(bool on) { _dev->setOption("pose_covariance", on ? 1.0 : 0.0); }
  PoseCovarianceEstimate poseCovariance() const
  {
    bpvo_hip_pose_covariance r;
    _dev->check(bpvo_hip_rig_pose_covariance(_dev->ctx(), &r));
    return PoseCovarianceEstimate(r);
  }

 private:
  static std::vector<bpvo_hip_camera> toC(const std::vector<Camera>& cams)
  {
    std::vector<bpvo_hip_camera> v;
    for(const Camera& cam : cams) {
      bpvo_hip_camera c;
      std::memcpy(c.K, cam.K.data(), sizeof(c.K));
      c.baseline = cam.baseline;
      c.rows = cam.size.rows; c.cols = cam.size.cols;
      v.push_back(c);
    }
    return v;
  }
  std::shared_ptr<detail::Device> _dev;
  int _n;
  bool _hasPointClouds = false;
  Trajectory _trajectory;
};

/* Several rigid rigs in one context, advanced by one call (bpvo_hip_add_frames_rigs; c_api.h): a rig dataset's sequences, a fleet of identical
 * vehicles, a parameter sweep over recorded rig data.  Rig r has the cameras cameras[r] at extrinsics[r] (camera_from_body, as
 * RigVisualOdometry takes them) and, after setParameters(r, ...), its own algorithm parameters — the fields
 * VisualOdometrySequences::setParameters accepts.  Every rig's results are those of a RigVisualOdometry of its own with those parameters. */
class RigsVisualOdometry {
 public:
  typedef VisualOdometrySequences::Camera Camera;

  RigsVisualOdometry(const std::vector<std::vector<Camera> >& cameras, const std::vector<std::vector<Matrix44> >& extrinsics,
                     const AlgorithmParameters& params = AlgorithmParameters(), int device = 0)
      : _dev(std::make_shared<detail::Device>(toC(cameras), params, device))
  {
    if(extrinsics.size() != cameras.size()) throw Error("one set of extrinsics per rig");
    std::vector<float> X;
    int first = 0;
    for(size_t r = 0; r < cameras.size(); ++r) {
      if(extrinsics[r].size() != cameras[r].size()) throw Error("one extrinsic per camera");
      _count.push_back((int) cameras[r].size());
      _first.push_back(first);
      first += _count.back();
      for(const Matrix44& x : extrinsics[r]) X.insert(X.end(), x.data(), x.data() + 16);
    }
    _dev->check(bpvo_hip_rigs_set(_dev->ctx(), (int) _count.size(), _count.data(), nullptr, X.data()));
    _trajectories.resize(_count.size());
    _hasPointClouds.assign(_count.size(), false);
  }

  int numRigs() const { return (int) _count.size(); }
  int numCameras(int rig) const { return _count.at(rig); }
  /* only before the rig's first frame; a field that fixes the context's storage or kernels must equal the context's (Error names it) */
  void setParameters(int rig, const AlgorithmParameters& p) { _dev->check(bpvo_hip_rigs_set_params(_dev->ctx(), rig, &p)); }
  AlgorithmParameters parameters(int rig) const
  {
    AlgorithmParameters p;
    _dev->check(bpvo_hip_rigs_get_params(_dev->ctx(), rig, &p));
    return p;
  }

  /* The next frame of the n rigs rigs[0 .. n) (nullptr: every rig, in order): the frames of all their cameras back to back, rig after rig in call
   * order, camera order inside a rig, each of its camera's size.  Result i is the body's of rigs[i] (RigVisualOdometry::addFrame's). */
  std::vector<Result> addFrames(const uint8_t* images, const float* disparities, const int* rigs = nullptr, int n = -1)
  {
    if(images == nullptr || disparities == nullptr) throw Error("nullptr image/disparity");
    if(n < 0) n = numRigs();
    std::vector<bpvo_hip_result> r((size_t) (n > 0 ? n : 0));
    _dev->check(bpvo_hip_add_frames_rigs(_dev->ctx(), n, rigs, images, disparities, 0, r.data()));
    std::vector<Result> ret((size_t) n);
    for(int i = 0; i < n; ++i) {
      const int g = rigs ? rigs[i] : i;
      std::memcpy(ret[i].pose.data(), r[i].pose, sizeof(r[i].pose));
      std::memcpy(ret[i].covariance.data(), r[i].covariance, sizeof(r[i].covariance));
      for(int l = 0; l < r[i].numLevels; ++l) ret[i].optimizerStatistics.push_back(OptimizerStatistics(r[i].optimizerStatistics[l]));
      ret[i].isKeyFrame = r[i].isKeyFrame != 0;
      ret[i].keyFramingReason = static_cast<KeyFramingReason>(r[i].keyFramingReason);
      _hasPointClouds[g] = r[i].hasPointCloud != 0;
      int nt = 0;
      _dev->check(bpvo_hip_rigs_trajectory_size(_dev->ctx(), g, &nt));
      _trajectories[g]._poses.resize(nt);
      if(nt) _dev->check(bpvo_hip_rigs_get_trajectory(_dev->ctx(), g, _trajectories[g]._poses[0].data()));
    }
    return ret;
  }
  /* did the rig's last frame leave point clouds (a key frame after the first)? */
  bool hasPointClouds(int rig) const { return _hasPointClouds.at(rig); }
  /* the point cloud of a rig's camera from its last frame; its pose is world_from_camera, W_kf X_p^-1 */
  PointCloud pointCloud(int rig, int camera) const
  {
    PointCloud pc;
    size_t n = 0;
    const int s = _first.at(rig) + camera;
    _dev->check(bpvo_hip_seq_get_point_cloud(_dev->ctx(), s, nullptr, &n, nullptr));
    pc.points().resize(n);
    _dev->check(bpvo_hip_seq_get_point_cloud(_dev->ctx(), s, pc.points().data(), &n, pc.pose().data()));
    return pc;
  }
  /* the body's trajectory of a rig */
  const Trajectory& trajectory(int rig) const { return _trajectories.at(rig); }
  int numPointsAtLevel(int rig, int camera, int level = -1) const
  {
    int n = 0;
    _dev->check(bpvo_hip_seq_num_points_at_level(_dev->ctx(), _first.at(rig) + camera, level, &n));
    return n;
  }
  void setOption(const std::string& name, double value) { _dev->setOption(name, value); }
  /* normalised intensity (an extension; c_api.h bpvo_hip_set_intensity_normalization): -1 off, 0 whole image, 1 .. 15 local; before the first frame */
  void setIntensityNormalization(int radius) { _dev->setIntensityNormalization(radius); }
  int intensityNormalization() const { return _dev->intensityNormalization(); }
  /* at most maxPoints[l] template points at level l, the most salient first (an extension; c_api.h bpvo_hip_set_point_budget); from the next key frame on */
  void setPointBudget(const std::vector<int>& maxPoints) { _dev->setPointBudget(maxPoints); }
  /* ... given for the finest level, a quarter of it per level above (multiples of 16, never below 256) */
  void setPointBudget(int finestLevelPoints) { _dev->setPointBudget(_dev->quarteredPointBudget(finestLevelPoints)); }
  /* where the bodies start Gauss-Newton (an extension; c_api.h bpvo_hip_set_start_policy): every rig's, or rig `rig`'s own; the hints of its next
   * estimate (body motions); what estimate `which` of its last frame started from */
  void setStartPolicy(const StartPolicy& policy) { _dev->check(bpvo_hip_set_start_policy(_dev->ctx(), &policy)); }
  void setStartPolicy(int rig, const StartPolicy& policy) { _dev->check(bpvo_hip_rigs_set_start_policy(_dev->ctx(), rig, &policy)); }
  void setStartHints(int rig, const std::vector<Matrix44>& hints) { const std::vector<float> M = packPoses(hints); _dev->check(bpvo_hip_rigs_set_start_hints(_dev->ctx(), rig, (int) hints.size(), M.data())); }
  StartInfo startInfo(int rig, int which = 0) const { StartInfo r; _dev->check(bpvo_hip_rigs_start_info(_dev->ctx(), rig, which, &r)); return r; }
  double getOption(const std::string& name) const { return _dev->getOption(name); }
  void setPoseCovariance(bool on) { _dev->setOption("pose_covariance", on ? 1.0 : 0.0); }
  /* the record of the rig's last frame: the covariance of its BODY pose, in the plain body twist */
  PoseCovarianceEstimate poseCovariance(int rig) const
  {
    bpvo_hip_pose_covariance r;
    _dev->check(bpvo_hip_rigs_pose_covariance(_dev->ctx(), rig, &r));
    return PoseCovarianceEstimate(r);
  }

 private:
  static std::vector<bpvo_hip_camera> toC(const std::vector<std::vector<Camera> >& rigs)
  {
    std::vector<bpvo_hip_camera> v;
    for(const std::vector<Camera>& cams : rigs)
      for(const Camera& cam : cams) {
        bpvo_hip_camera c;
        std::memcpy(c.K, cam.K.data(), sizeof(c.K));
        c.baseline = cam.baseline;
        c.rows = cam.size.rows; c.cols = cam.size.cols;
        v.push_back(c);
      }
    return v;
  }
  std::shared_ptr<detail::Device> _dev;
  std::vector<int> _count, _first;
  std::vector<bool> _hasPointClouds;
  std::vector<Trajectory> _trajectories;
};

}  // namespace bpvo

#endif  // BPVO_HIP_VO_HPP
