// libbpvo_hip, host side: the stereo front-end — StereoAlgorithm::run of the reference (utils/stereo_algorithm.cc) for block matching, SGM and SGBM:
// the parameter checks, the front-end's buffers, the launches over the frames of a call (kernels_stereo.hip, kernels_sgm.hip, kernels_sgbm.hip), the
// stand-alone entry points bpvo_hip_stereo_bm / bpvo_hip_stereo_frames, and stereo_front: the front-end of an addFrame call (vo.hip), with the
// rectification in front of it (rectify.hip) when the call brings raw pairs.
#include "host_ctx.h"

using namespace bpvo_hip;
using namespace bpvo_hip_host;

namespace bpvo_hip_host {

// ---- stereo front-end (reference: utils/stereo_algorithm.cc:63-82,98-111 -> OpenCV 2.4 cvFindStereoCorrespondenceBM) ----
// the parameter fields of the semi-global matchers' launches for frames of rows x cols (pointers and frame counts: the caller's)
static SgbmLaunch sgbm_launch_of(const bpvo_hip_stereo_params& sp, int rows, int cols)
{
  SgbmLaunch g = {};
  g.rows = rows; g.cols = cols;
  g.min_disp = sp.minDisparity; g.ndisp = sp.numberOfDisparities; g.sad_window = sp.SADWindowSize; g.P1 = sp.P1; g.P2 = sp.P2;
  g.disp12_max_diff = sp.disp12MaxDiff; g.pre_filter_cap = sp.preFilterCap; g.uniqueness_ratio = sp.uniquenessRatio;
  g.speckle_window = sp.speckleWindowSize; g.speckle_range = sp.speckleRange; g.full_dp = sp.fullDP;
  return g;
}
static SgmLaunch sgm_launch_of(const bpvo_hip_stereo_params& sp, int rows, int cols)
{
  SgmLaunch g = {};
  g.rows = rows; g.cols = cols;
  g.ndisp = sp.numberOfDisparities; g.sobel_cap = sp.sobelCapValue; g.census_radius = sp.censusRadius; g.window_radius = sp.windowRadius;
  g.P1 = sp.smoothnessPenaltySmall; g.P2 = sp.smoothnessPenaltyLarge; g.consistency_threshold = sp.consistencyThreshold;
  g.disparity_factor = sp.disparityFactor; g.census_weight = sp.censusWeightFactor;
  return g;
}
// (rows x cols: the frame the parameters are checked for — the context's size, or a camera's)
static int stereo_check(bpvo_hip_ctx* c, const bpvo_hip_stereo_params* sp, int rows, int cols)
{
  // the argument checks of cvFindStereoCorrespondenceBM (stereobm.cpp) + what the kernel serves
  if(!sp) return fail(c, BPVO_ERR_INVALID_ARG, "nullptr stereo parameters");
  if(sp->algorithm == BPVO_STEREO_SGM) {
    // the checks of SgmStereo::compute / the SGMStereo setters (utils/sgm.cc:168-171,208-254)
    if(sp->numberOfDisparities <= 0 || sp->numberOfDisparities % 16) return fail(c, BPVO_ERR_INVALID_ARG, "numberOfDisparities must be a multiple of 16");
    if(sp->censusRadius < 1 || sp->censusRadius > 2) return fail(c, BPVO_ERR_INVALID_ARG, "window radius of Census transform must be 1 or 2");
    if(sp->censusWeightFactor < 0) return fail(c, BPVO_ERR_INVALID_ARG, "weight of Census transform must be positive");
    if(sp->smoothnessPenaltySmall < 0 || sp->smoothnessPenaltyLarge < 0) return fail(c, BPVO_ERR_INVALID_ARG, "smoothness penalty value is less than zero");
    if(sp->smoothnessPenaltySmall >= sp->smoothnessPenaltyLarge) return fail(c, BPVO_ERR_INVALID_ARG, "small value of smoothness penalty must be smaller than large penalty value");
    if(sp->consistencyThreshold < 0) return fail(c, BPVO_ERR_INVALID_ARG, "threshold for LR consistency must be positive");
    if(!(sp->disparityFactor > 0)) return fail(c, BPVO_ERR_INVALID_ARG, "disparity factor is less than zero");
    if(sp->numberOfDisparities > 256) return fail(c, BPVO_ERR_UNSUPPORTED, "SGM: numberOfDisparities <= 256 are on the device path");
    // (2r+1)^2 * 255 must stay below 2^15: the original's sliding sums are int16 saturating additions (_mm_adds_epi16) and the cost is read
    // back as int16; up to radius 5 (121 * 255 = 30855) nothing saturates and the plain integer sums of the device path are the same numbers
    if(sp->windowRadius < 0 || sp->windowRadius > 5 || rows <= sp->windowRadius) return fail(c, BPVO_ERR_UNSUPPORTED, "SGM: windowRadius 0..5 (and fewer than image rows) are on the device path");
    // int16 path costs: the sums of four paths stay clear of saturation for penalties below this (the original saturates silently)
    if(sp->smoothnessPenaltyLarge > 4000) return fail(c, BPVO_ERR_UNSUPPORTED, "SGM: smoothnessPenaltyLarge <= 4000 on the device path");
    return BPVO_OK;
  }
  if(sp->algorithm == BPVO_STEREO_SGBM) {
    if(sp->numberOfDisparities <= 0 || sp->numberOfDisparities % 16) return fail(c, BPVO_ERR_INVALID_ARG, "numberOfDisparities must be a positive multiple of 16");   // CV_Assert(D % 16 == 0)
    const char* why = nullptr;
    if(!sgbm_serves(sgbm_launch_of(*sp, rows, cols), &why)) return fail(c, BPVO_ERR_UNSUPPORTED, why);
    return BPVO_OK;
  }
  if(sp->algorithm != BPVO_STEREO_BLOCK_MATCHING) return fail(c, BPVO_ERR_UNSUPPORTED, "StereoAlgorithm: BlockMatching, SGM and SGBM are on the device path (RSGM is GPL-gated in the reference and not built)");
  if(sp->preFilterCap < 1 || sp->preFilterCap > 63) return fail(c, BPVO_ERR_INVALID_ARG, "preFilterCap must be within 1..63");
  if(sp->SADWindowSize < 5 || sp->SADWindowSize > 255 || sp->SADWindowSize % 2 == 0 || sp->SADWindowSize >= std::min(cols, rows))
    return fail(c, BPVO_ERR_INVALID_ARG, "SADWindowSize must be odd, be within 5..255 and be not larger than image width or height");
  if(sp->numberOfDisparities <= 0 || sp->numberOfDisparities % 16 != 0) return fail(c, BPVO_ERR_INVALID_ARG, "numberOfDisparities must be positive and divisble by 16");
  if(sp->textureThreshold < 0) return fail(c, BPVO_ERR_INVALID_ARG, "texture threshold must be non-negative");
  if(sp->uniquenessRatio < 0) return fail(c, BPVO_ERR_INVALID_ARG, "uniqueness ratio must be non-negative");
  if(sp->SADWindowSize > 21) return fail(c, BPVO_ERR_UNSUPPORTED, "SADWindowSize: 5..21 are on the device path");
  if(sp->minDisparity < 0 || sp->numberOfDisparities > 256) return fail(c, BPVO_ERR_UNSUPPORTED, "minDisparity >= 0 and numberOfDisparities <= 256 are on the device path");
  return BPVO_OK;
}
int stereo_reserve(bpvo_hip_ctx* c, size_t npix)      // npix: the pixels of a call, the sum over its frames
{
  if(npix <= c->st_pixels) return BPVO_OK;
  HIP_CK(c, hipStreamSynchronize(c->stream));
  DeviceBuf<uint8_t>* const u8[4] = {&c->st_left, &c->st_right, &c->st_left_pre, &c->st_right_pre};
  c->st_pixels = 0;
  for(auto* b : u8) b->reset();      // (all five go before the first comes back: the peak is one set)
  c->st_disp.reset();
  for(auto* b : u8) HIP_CK(c, b->alloc(npix));
  HIP_CK(c, c->st_disp.alloc(npix));
  if(int rc = variance_scratch_moved(c, npix)) return rc;      // (the measurement-variance maps, where the feature has run)
  c->st_pixels = npix;
  return BPVO_OK;
}
static int stereo_scratch(bpvo_hip_ctx* c, size_t need)      // the semi-global matchers' scratch, at least `need` bytes
{
  if(need <= c->st_sgm.size()) return BPVO_OK;
  HIP_CK(c, hipStreamSynchronize(c->stream));
  HIP_CK(c, c->st_sgm.reserve(need));
  return BPVO_OK;
}
static bool operator==(const StereoSize& a, const StereoSize& b) { return a.rows == b.rows && a.cols == b.cols; }
// The checks of a call's stereo stage, once per size among its frames; nothing is touched.  ids: null (the context's own size: stereo_run), or the
// sequence of each frame — a failure names the first frame's whose size fails.
static int stereo_check_sizes(bpvo_hip_ctx* c, int n, const StereoSize* sz, const bpvo_hip_stereo_params* sp, const int* ids)
{
  if(!sp) return fail(c, BPVO_ERR_INVALID_ARG, "nullptr stereo parameters");
  for(int i = 0; i < n; ++i) {
    bool seen = false;
    for(int k = 0; k < i && !seen; ++k) seen = sz[k] == sz[i];
    if(seen) continue;
    const int rc = stereo_check(c, sp, sz[i].rows, sz[i].cols);
    if(rc && ids) c->err = "sequence " + std::to_string(ids[i]) + ": " + c->err;
    if(rc) return rc;
  }
  return BPVO_OK;
}
// SGM frames of one size per launch (option "stereo_frames_per_launch"): as many as a third of the free device memory holds — the rule of
// the 4x4 tap cache (estimate.hip) —, the free memory read once per context, when the scratch is first needed; never fewer than one (whose
// allocation is then attempted as before).
static int sgm_frames_per_launch(bpvo_hip_ctx* c, size_t per_frame, int count)
{
  if(c->stereo_frames_per_launch == 1 || count <= 1) return 1;
  if(c->st_sgm_budget == 0) {
    size_t free_b = 0, total_b = 0;
    if(hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void) hipGetLastError(); free_b = 0; }
    c->st_free_seen = free_b + c->st_sgm.size();      // (a scratch this context already holds is given back before a larger one is taken)
    c->st_sgm_budget = std::max<size_t>(1, c->st_free_seen / 3);
  }
  int F = (int) std::min<size_t>((size_t) count, std::max<size_t>(1, c->st_sgm_budget / per_frame));
  if(c->stereo_frames_per_launch > 1) F = std::min(F, c->stereo_frames_per_launch);
  return F;
}
// Disparities of n rectified pairs into c->st_disp (device), pair i of sz[i].rows x sz[i].cols pixels, images and maps back to back in call
// order; d_left: where the left images are on the device afterwards.  The caller has run stereo_check_sizes.
// Block matching takes all the frames in one launch per stage: the launch-wide kernels where they share one size, the table forms
// otherwise.  The semi-global matchers' kernels take launch-wide sizes: they serve runs of neighbouring frames of one size (neighbours in
// the call lie back to back in memory), SGM in chunks of sgm_frames_per_launch frames per launch, SGBM frame after frame.
static int stereo_run_sizes(bpvo_hip_ctx* c, int n, const StereoSize* sz, const uint8_t* left, const uint8_t* right, bool on_device,
                            const bpvo_hip_stereo_params* sp, const uint8_t** d_left)
{
  if(n <= 0 || !left || !right) return fail(c, BPVO_ERR_INVALID_ARG, "nullptr image");
  size_t npix = 0;
  bool uniform = true;
  int max_rows = 0, max_cols = 0;
  for(int i = 0; i < n; ++i) {
    npix += (size_t) sz[i].rows * sz[i].cols;
    uniform = uniform && sz[i] == sz[0];
    max_rows = std::max(max_rows, sz[i].rows); max_cols = std::max(max_cols, sz[i].cols);
  }
  int rc = stereo_reserve(c, npix);
  if(rc) return rc;
  const uint8_t* dl = left;
  const uint8_t* dr = right;
  if(!on_device) {
    HIP_CK(c, hipMemcpyAsync(c->st_left, left, npix, hipMemcpyHostToDevice, c->stream));
    HIP_CK(c, hipMemcpyAsync(c->st_right, right, npix, hipMemcpyHostToDevice, c->stream));
    dl = c->st_left; dr = c->st_right;
  }
  if(d_left) *d_left = dl;
  if(sp->algorithm == BPVO_STEREO_SGM || sp->algorithm == BPVO_STEREO_SGBM) {
    const bool sgm = sp->algorithm == BPVO_STEREO_SGM;
    // runs of neighbouring frames of one size: [first, first + count) at pixel offset `at`; the scratch is sized for the largest need of the call
    struct Run { int first, count, per_launch; size_t at; };
    std::vector<Run> runs;
    size_t at = 0, need = 0;
    for(int i = 0; i < n;) {
      int k = i + 1;
      while(k < n && sz[k] == sz[i]) ++k;
      const size_t per = sgm ? sgm_scratch_bytes(sz[i].rows, sz[i].cols, sp->numberOfDisparities)
                             : sgbm_scratch_bytes(sz[i].rows, sz[i].cols, sp->minDisparity, sp->numberOfDisparities);
      const int F = sgm ? sgm_frames_per_launch(c, per, k - i) : 1;
      need = std::max(need, per * (size_t) F);
      runs.push_back(Run{i, k - i, F, at});
      at += (size_t) (k - i) * sz[i].rows * sz[i].cols;
      i = k;
    }
    rc = stereo_scratch(c, need);
    if(rc) return rc;
    for(const Run& r : runs) {
      const StereoSize& q = sz[r.first];
      if(sgm) {
        SgmLaunch g = sgm_launch_of(*sp, q.rows, q.cols);
        g.left = dl + r.at; g.right = dr + r.at; g.disp = c->st_disp + r.at; g.scratch = c->st_sgm;
        g.nframes = r.count; g.frames_per_launch = r.per_launch;
        c->st_frames_per_launch_seen = r.per_launch;
        if(!launch_stereo_sgm(c->stream, g)) return fail(c, BPVO_ERR_UNSUPPORTED, "semi-global matching: disparity range not served by the kernels");
      } else {
        SgbmLaunch g = sgbm_launch_of(*sp, q.rows, q.cols);
        g.left = dl + r.at; g.right = dr + r.at; g.disp = c->st_disp + r.at; g.scratch = c->st_sgm;
        g.nframes = r.count;
        if(!launch_stereo_sgbm(c->stream, g)) return fail(c, BPVO_ERR_UNSUPPORTED, "semi-global block matching: parameters not served by the kernels");
      }
      HIP_CK(c, hipGetLastError());
    }
    return BPVO_OK;
  }
  StereoLaunch g;
  g.left_pre = c->st_left_pre; g.right_pre = c->st_right_pre; g.disp = c->st_disp;
  g.rows = max_rows; g.cols = max_cols; g.nframes = n;
  g.wsz = sp->SADWindowSize; g.ndisp = sp->numberOfDisparities; g.mindisp = sp->minDisparity; g.cap = sp->preFilterCap;
  g.texture_threshold = sp->textureThreshold; g.uniqueness_ratio = sp->uniquenessRatio;
  if(uniform) {
    launch_stereo_prefilter(c->stream, dl, c->st_left_pre, max_rows, max_cols, sp->preFilterCap, n);
    launch_stereo_prefilter(c->stream, dr, c->st_right_pre, max_rows, max_cols, sp->preFilterCap, n);
  } else {
    if((size_t) n > c->h_st_frames.size()) {      // (the pinned table comes last: its size says that both are there)
      HIP_CK(c, hipStreamSynchronize(c->stream));
      c->d_st_frames.reset(); c->h_st_frames.reset();
      const size_t cap = (size_t) std::max(n, seq_capacity(c));
      HIP_CK(c, c->d_st_frames.alloc(cap));
      HIP_CK(c, c->h_st_frames.alloc(cap));
    }
    if(!c->st_tab_ev) HIP_CK(c, c->st_tab_ev.create(hipEventDisableTiming));
    else HIP_CK(c, hipEventSynchronize(c->st_tab_ev));      // (the last call's copy has read the pinned rows)
    size_t at = 0;
    for(int i = 0; i < n; ++i) {
      c->h_st_frames[i] = StereoFrame{sz[i].rows, sz[i].cols, at};
      at += (size_t) sz[i].rows * sz[i].cols;
    }
    HIP_CK(c, hipMemcpyAsync(c->d_st_frames, c->h_st_frames, (size_t) n * sizeof(StereoFrame), hipMemcpyHostToDevice, c->stream));
    HIP_CK(c, hipEventRecord(c->st_tab_ev, c->stream));
    launch_stereo_prefilter_frames(c->stream, dl, c->st_left_pre, c->d_st_frames, max_rows, max_cols, sp->preFilterCap, n);
    launch_stereo_prefilter_frames(c->stream, dr, c->st_right_pre, c->d_st_frames, max_rows, max_cols, sp->preFilterCap, n);
    g.frames = c->d_st_frames; g.total_pixels = npix;
  }
  if(!launch_stereo_bm(c->stream, g)) return fail(c, BPVO_ERR_UNSUPPORTED, "stereo block matching: window / disparity range not served by the kernel");
  HIP_CK(c, hipGetLastError());
  return BPVO_OK;
}
// `count` pairs of the context's size: the sized path's uniform case (the parameters are held against the size before the images are looked at)
static int stereo_run(bpvo_hip_ctx* c, int count, const uint8_t* left, const uint8_t* right, bool on_device, const bpvo_hip_stereo_params* sp,
                      const uint8_t** d_left)
{
  const StereoSize size{c->rows, c->cols};
  const int rc = stereo_check_sizes(c, 1, &size, sp, nullptr);
  if(rc) return rc;
  const std::vector<StereoSize> sz((size_t) std::max(count, 0), size);
  return stereo_run_sizes(c, count, sz.data(), left, right, on_device, sp, d_left);
}

// ---- the front-end of an addFrame call (host_ctx.h states the contract): the order of the checks is the entry points' own ----
static int rect_side_missing(bpvo_hip_ctx* c, int seq, int side)
{
  c->err = (seq < 0 ? std::string() : "sequence " + std::to_string(seq) + ": ") + (side ? "no rectification of the right side" : "no rectification of the left side");
  return BPVO_ERR_NO_DATA;
}
int stereo_front(bpvo_hip_ctx* c, int n, const StereoSize* sz, const int* ids, const uint8_t* left, const uint8_t* right, bool raw, bool on_device,
                 const bpvo_hip_stereo_params* sp, const uint8_t** d_left)
{
  if(raw)
    for(int i = 0; i < n; ++i)
      for(int side = 0; side < 2; ++side)
        if(!rect_map_of(c, ids ? ids[i] : -1, side)) return rect_side_missing(c, ids ? ids[i] : -1, side);
  int rc = stereo_check_sizes(c, n, sz, sp, ids);
  if(rc) return rc;
  (void) hipSetDevice(c->device);
  if(raw) {
    // the raw pairs become the rectified pairs in the front-end's own image buffers — one launch for both sides, no host synchronisation, no
    // copy —, which the front-end then reads where they lie
    size_t npix = 0;
    for(int i = 0; i < n; ++i) npix += (size_t) sz[i].rows * sz[i].cols;
    rc = stereo_reserve(c, npix);
    if(rc) return rc;
    const RectSide sides[2] = {{0, left, c->st_left}, {1, right, c->st_right}};
    rc = rectify_queue(c, n, ids, 2, sides, on_device);
    if(rc) { (void) hipStreamSynchronize(c->stream); return rc; }
    left = c->st_left; right = c->st_right; on_device = true;
  }
  const uint8_t* dl = nullptr;
  rc = stereo_run_sizes(c, n, sz, left, right, on_device, sp, &dl);
  if(d_left) *d_left = dl;
  // option measurement variance (c_api.h; disparity_variance.hip): the variance maps of the frames that will be fused with one, behind the matcher
  if(rc == BPVO_OK) rc = variance_front(c, n, sz, ids, dl, on_device ? right : c->st_right.get());
  if(rc) (void) hipStreamSynchronize(c->stream);
  return rc;
}

}  // namespace bpvo_hip_host

extern "C" {

void bpvo_hip_default_stereo_params(bpvo_hip_stereo_params* p)   // utils/stereo_algorithm.cc:63-82 (numberOfDisparities has no default there)
{
  std::memset(p, 0, sizeof(*p));
  p->preFilterCap = 31; p->SADWindowSize = 15; p->minDisparity = 0; p->numberOfDisparities = 64; p->textureThreshold = 10; p->uniquenessRatio = 15;
  // SgmStereo::Config() (utils/sgm.cc:47-56); algorithm: "BlockMatching" is the config file's default (utils/stereo_algorithm.cc:25)
  p->algorithm = BPVO_STEREO_BLOCK_MATCHING;
  p->sobelCapValue = 15; p->censusRadius = 2; p->windowRadius = 2; p->smoothnessPenaltySmall = 100; p->smoothnessPenaltyLarge = 1600;
  p->consistencyThreshold = 1; p->disparityFactor = 256.0; p->censusWeightFactor = 1.0 / 6.0;
}
void bpvo_hip_stereo_params_sgbm_from_config(bpvo_hip_stereo_params* p, int minDisparity, int numberOfDisparities, int SADWindowSize, int P1, int P2,
                                             int uniquenessRatio, int speckleWindowSize, int speckleRange, int fullDP)
{
  // make_unique<cv::StereoSGBM>(minDisparity, numberOfDisparities, SADWindowSize, P1, P2, uniquenessRatio, speckleWindowSize, speckleRange,
  // (bool) fullDP) against StereoSGBM(minDisparity, numDisparities, SADWindowSize, P1, P2, disp12MaxDiff, preFilterCap, uniquenessRatio,
  // speckleWindowSize, speckleRange = 0, fullDP = false)  (utils/stereo_algorithm.cc:30-39)
  bpvo_hip_default_stereo_params(p);
  p->algorithm = BPVO_STEREO_SGBM;
  p->minDisparity = minDisparity; p->numberOfDisparities = numberOfDisparities; p->SADWindowSize = SADWindowSize; p->P1 = P1; p->P2 = P2;
  p->disp12MaxDiff = uniquenessRatio;
  p->preFilterCap = speckleWindowSize;
  p->uniquenessRatio = speckleRange;
  p->speckleWindowSize = fullDP ? 1 : 0;
  p->speckleRange = 0;
  p->fullDP = 0;
  p->textureThreshold = 0;
}
int bpvo_hip_stereo_bm(bpvo_hip_ctx* c, int count, const uint8_t* left, const uint8_t* right, int on_device, const bpvo_hip_stereo_params* sp,
                       float* disparity, int disparity_on_device)
{
  CHECK_CTX(c);
  if(!disparity) return fail(c, BPVO_ERR_INVALID_ARG, "nullptr disparity");
  (void) hipSetDevice(c->device);
  int rc = stereo_run(c, count, left, right, on_device != 0, sp, nullptr);
  if(rc) return rc;
  HIP_CK(c, hipMemcpyAsync(disparity, c->st_disp, c->geom[0].npix * (size_t) count * sizeof(float),
                           disparity_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, c->stream));
  HIP_CK(c, hipStreamSynchronize(c->stream));
  return BPVO_OK;
}
int bpvo_hip_stereo_frames(bpvo_hip_ctx* c, int n, const bpvo_hip_camera* cams, const uint8_t* left, const uint8_t* right, int on_device,
                           const bpvo_hip_stereo_params* sp, float* disparity, int disparity_on_device)
{
  CHECK_CTX(c);
  if(!disparity) return fail(c, BPVO_ERR_INVALID_ARG, "nullptr disparity");
  if(n < 1 || !cams) return fail(c, BPVO_ERR_INVALID_ARG, "stereo_frames: n >= 1 cameras");
  if(!left || !right) return fail(c, BPVO_ERR_INVALID_ARG, "nullptr image");
  std::vector<StereoSize> sz((size_t) n);
  std::vector<int> ids((size_t) n);
  size_t npix = 0;
  for(int i = 0; i < n; ++i) {
    ids[i] = i;
    sz[i] = StereoSize{cams[i].rows, cams[i].cols};
    if(sz[i].rows < 1 || sz[i].cols < 1) return seq_fail(c, BPVO_ERR_INVALID_ARG, i, "camera: image size out of range");
    if(sz[i].rows > c->rows || sz[i].cols > c->cols) return camera_too_large(c, i, sz[i].rows, sz[i].cols);
    npix += (size_t) sz[i].rows * sz[i].cols;
  }
  int rc = stereo_check_sizes(c, n, sz.data(), sp, ids.data());
  if(rc) return rc;
  for(int i = 0; i < n; ++i)      // (what bpvo_hip_create admits, after the parameters have been held against every size)
    if(sz[i].rows < 8 || sz[i].cols < 8) return seq_fail(c, BPVO_ERR_INVALID_ARG, i, "camera: image size out of range (at least 8 rows and cols)");
  (void) hipSetDevice(c->device);
  rc = stereo_run_sizes(c, n, sz.data(), left, right, on_device != 0, sp, nullptr);
  if(rc) { (void) hipStreamSynchronize(c->stream); return rc; }
  HIP_CK(c, hipMemcpyAsync(disparity, c->st_disp, npix * sizeof(float), disparity_on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, c->stream));
  HIP_CK(c, hipStreamSynchronize(c->stream));
  return BPVO_OK;
}

}  // extern "C"
