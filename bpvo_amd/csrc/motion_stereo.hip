// libbpvo_hip, host side: motion stereo (include/bpvo_hip/c_api.h; the rule: motion_stereo_math.h; the kernel: kernels_motion_stereo.hip).  A
// fusion stage (disparity_fusion.hip fusion_stage) calls motion_stereo_stage between its splat and its update: ONE launch over a table of jobs
// for the frames of the stage whose sequence has the feature in mode 1, on the z-buffer words the splat left.  bpvo_hip_motion_stereo_frames
// runs the same launch for a caller's image pairs and prior maps.  With mode 0 everywhere, or without fusion, no existing call launches,
// allocates or reads anything of this file.
#include "host_ctx.h"
#include "motion_stereo_math.h"

namespace bpvo_hip_host {

static const bpvo_hip_motion_stereo& ms_setting(const bpvo_hip_ctx* c, int seq)
{
  const MotionStereoState& S = c->motion_stereo;
  return (size_t) seq < S.seq.size() && S.seq[(size_t) seq].own ? S.seq[(size_t) seq].prm : S.prm;
}
bool motion_stereo_on(const bpvo_hip_ctx* c, int seq) { return c->motion_stereo.n_on > 0 && ms_setting(c, seq).mode == 1; }

static void ms_recount(bpvo_hip_ctx* c)
{
  MotionStereoState& S = c->motion_stereo;
  S.n_on = 0;
  for(size_t s = 0; s < S.seq.size(); ++s) S.n_on += ms_setting(c, (int) s).mode == 1 ? 1 : 0;
}
static void ms_states(bpvo_hip_ctx* c)
{
  if(c->motion_stereo.seq.empty()) c->motion_stereo.seq.resize((size_t) std::max(1, seq_capacity(c)));
}
// the counters of the last launch, once they have landed: the classes into the records of its sequences and the totals, the tiles into the totals
static int ms_resolve(bpvo_hip_ctx* c)
{
  MotionStereoState& S = c->motion_stereo;
  if(S.pending.empty()) return BPVO_OK;
  HIP_CK(c, hipEventSynchronize(S.done_ev));
  for(size_t k = 0; k < S.pending.size(); ++k) {
    const unsigned* cnt = S.h_counts + kMotionStereoCounters * k;
    for(int t = 0; t < 3; ++t) S.tiles[t] += cnt[MS_CLASSES + t];
    for(int t = 0; t < MS_CLASSES; ++t) S.classes[t] += cnt[t];
    if(S.pending[k] < 0) continue;
    bpvo_hip_motion_stereo_info& info = S.seq[(size_t) S.pending[k]].info;
    info.no_prior = cnt[MS_NO_PRIOR]; info.low_parallax = cnt[MS_LOW_PARALLAX]; info.border = cnt[MS_BORDER]; info.edge = cnt[MS_EDGE];
    info.flat = cnt[MS_FLAT]; info.rejected = cnt[MS_REJECTED]; info.fused = cnt[MS_FUSED];
  }
  S.pending.clear();
  return BPVO_OK;
}
void motion_stereo_seq_reset(bpvo_hip_ctx* c, int seq)
{
  MotionStereoState& S = c->motion_stereo;
  if((size_t) seq >= S.seq.size()) return;
  (void) ms_resolve(c);
  S.seq[(size_t) seq].info = bpvo_hip_motion_stereo_info{};
}

// ms_tables: the job table and the counters for m jobs, free to be written.  ms_launch: the launch for the m rows the caller has put into
// S.h_jobs (but for the counters' address), the counters on their way back; owners[k]: the sequence of job k, or -1.
static int ms_tables(bpvo_hip_ctx* c, size_t m)
{
  MotionStereoState& S = c->motion_stereo;
  if(int rc = ms_resolve(c)) return rc;      // (and the last launch's copy has read the pinned rows)
  if(m > S.h_counts.size() / kMotionStereoCounters) {      // (the pinned counters come last: they say that all four are there)
    HIP_CK(c, hipStreamSynchronize(c->stream));
    S.d_jobs.reset(); S.h_jobs.reset(); S.d_counts.reset(); S.h_counts.reset();
    const size_t cap = std::max(m, (size_t) std::max(1, seq_capacity(c)));
    HIP_CK(c, S.d_jobs.alloc(cap));
    HIP_CK(c, S.h_jobs.alloc(cap));
    HIP_CK(c, S.d_counts.alloc(cap * kMotionStereoCounters));
    HIP_CK(c, S.h_counts.alloc(cap * kMotionStereoCounters));
  }
  if(!S.done_ev) HIP_CK(c, S.done_ev.create(hipEventDisableTiming));
  return BPVO_OK;
}
static int ms_launch(bpvo_hip_ctx* c, size_t m, const std::vector<int>& owners)
{
  MotionStereoState& S = c->motion_stereo;
  int max_tiles = 0;
  size_t pixels = 0;
  for(size_t k = 0; k < m; ++k) {
    MotionStereoJob& j = S.h_jobs[k];
    j.counts = S.d_counts + kMotionStereoCounters * k;
    max_tiles = std::max(max_tiles, motion_stereo_tiles(j.rows, j.cols));
    pixels += (size_t) j.rows * (size_t) j.cols;
  }
  HIP_CK(c, hipMemcpyAsync(S.d_jobs, S.h_jobs, sizeof(MotionStereoJob) * m, hipMemcpyHostToDevice, c->stream));
  HIP_CK(c, hipMemsetAsync(S.d_counts, 0, sizeof(unsigned) * kMotionStereoCounters * m, c->stream));
  S.timed = false;
  if(c->profiling) {      // (measurement: scripts/motion_stereo_bench.py)
    if(!S.t0) HIP_CK(c, S.t0.create());
    if(!S.t1) HIP_CK(c, S.t1.create());
    HIP_CK(c, hipEventRecord(S.t0, c->stream));
  }
  launch_motion_stereo(c->stream, S.d_jobs, (int) m, max_tiles);
  HIP_CK(c, hipGetLastError());
  if(c->profiling) {
    HIP_CK(c, hipEventRecord(S.t1, c->stream));
    S.timed = true;
  }
  HIP_CK(c, hipMemcpyAsync(S.h_counts, S.d_counts, sizeof(unsigned) * kMotionStereoCounters * m, hipMemcpyDeviceToHost, c->stream));
  HIP_CK(c, hipEventRecord(S.done_ev, c->stream));
  S.pending = owners;
  S.launches += 1;
  S.pixels += pixels;
  return BPVO_OK;
}
// the rule's numbers of a job: the setting, the gate, the camera and the motion Q ([16] row-major, X_K = Q X_C)
static void ms_job_rule(MotionStereoJob& j, const bpvo_hip_motion_stereo& prm, const DfCamera& cam, const float* Q)
{
  const MsRule r = ms_rule(prm.radius, prm.steps, prm.min_gain, prm.noise_sigma, prm.min_sigma, prm.max_sigma, prm.gate);
  const MsGeometry g = ms_geometry(cam, Q);
  j.rows = cam.rows; j.cols = cam.cols; j.radius = r.radius; j.steps = r.steps;
  j.lo = cam.lo; j.hi = cam.hi; j.min_gain = r.min_gain; j.noise2 = r.noise2; j.min2 = r.min2; j.max2 = r.max2; j.gate = r.gate;
  j.fx = g.fx; j.fy = g.fy; j.cx = g.cx; j.cy = g.cy;
  std::memcpy(j.R, g.R, sizeof(j.R));
  std::memcpy(j.e, g.e, sizeof(j.e));
}

int motion_stereo_stage(bpvo_hip_ctx* c, int n, const MotionStereoView* views, bool* launched)
{
  MotionStereoState& S = c->motion_stereo;
  *launched = false;
  if(S.n_on == 0) return BPVO_OK;
  std::vector<int> owners;
  std::vector<M44> Qs;
  std::vector<const MotionStereoView*> act;
  for(int i = 0; i < n; ++i) {
    const MotionStereoView& v = views[i];
    if(!motion_stereo_on(c, v.seq)) continue;
    if(!S.pending.empty())
      if(int rc = ms_resolve(c)) return rc;      // (before the record of a sequence of the last launch is rewritten)
    bpvo_hip_motion_stereo_info& info = S.seq[(size_t) v.seq].info;
    info = bpvo_hip_motion_stereo_info{};
    info.view_slot = -1;
    std::memcpy(info.motion, m44_identity().m, 64);
    if(v.view_slot < 0 || !v.T || !df_motion_ok(v.T)) continue;
    M44 T;
    std::memcpy(T.m, v.T, 64);
    const M44 Q = m44_inverse(T);
    if(!df_motion_ok(Q.m)) continue;      // (a singular estimate)
    info.launched = 1;
    info.view_slot = v.view_slot;
    std::memcpy(info.motion, Q.m, 64);
    act.push_back(&v);
    Qs.push_back(Q);
    owners.push_back(v.seq);
  }
  if(act.empty()) return BPVO_OK;
  const size_t m = act.size();
  if(int rc = ms_tables(c, m)) return rc;
  for(size_t k = 0; k < m; ++k) {
    const MotionStereoView& v = *act[k];
    const FrameSlot& f = c->frames[v.slot];
    const FrameSlot& kf = c->frames[v.view_slot];
    const LevelGeom& g = slot_geom(c, f, 0);
    const bpvo_hip_params& sp = f.seq_params ? *f.seq_params : c->params;
    MotionStereoJob& j = S.h_jobs[k];
    j = MotionStereoJob{};
    j.C = f.img[0]; j.K = kf.img[0]; j.zbuf = v.zbuf;
    const DfCamera cam{g.K[0], g.K[4], g.K[2], g.K[5], g.b, sp.minValidDisparity, sp.maxValidDisparity, g.rows, g.cols};
    ms_job_rule(j, ms_setting(c, v.seq), cam, Qs[k].m);
  }
  if(int rc = ms_launch(c, m, owners)) return rc;
  *launched = true;
  return BPVO_OK;
}

double motion_stereo_last_ms(bpvo_hip_ctx* c)
{
  MotionStereoState& S = c->motion_stereo;
  float ms = -1.0f;
  if(!S.timed || hipEventSynchronize(S.t1) != hipSuccess) return -1.0;
  if(hipEventElapsedTime(&ms, S.t0, S.t1) != hipSuccess) return -1.0;
  return (double) ms;
}

static int ms_check_setting(bpvo_hip_ctx* c, const bpvo_hip_motion_stereo* v)
{
  if(v->mode != 0 && v->mode != 1) return fail(c, BPVO_ERR_INVALID_ARG, "motion stereo: mode must be 0 (off) or 1 (on)");
  if(v->mode == 0) return BPVO_OK;
  if(const char* why = ms_refusal(v->radius, v->steps, v->min_gain, v->noise_sigma, v->min_sigma, v->max_sigma, v->gate)) return fail(c, BPVO_ERR_INVALID_ARG, why);
  if(!c->rigs.empty()) return fail(c, BPVO_ERR_UNSUPPORTED, "motion stereo: a context that declares a rig does not serve mode 1");
  return BPVO_OK;
}
static int ms_get_info(bpvo_hip_ctx* c, int seq, bpvo_hip_motion_stereo_info* info)
{
  if(!info) return fail(c, BPVO_ERR_INVALID_ARG, "nullptr motion stereo info");
  if(int rc = ms_resolve(c)) return rc;
  if((size_t) seq < c->motion_stereo.seq.size()) *info = c->motion_stereo.seq[(size_t) seq].info;
  else *info = bpvo_hip_motion_stereo_info{};
  return BPVO_OK;
}

}  // namespace bpvo_hip_host

extern "C" {

#define CHECK_SEQ(c, s) if((s) < 0 || (s) >= seq_capacity(c)) return seq_fail(c, BPVO_ERR_INVALID_ARG, s, "no such sequence")

int bpvo_hip_set_motion_stereo(bpvo_hip_ctx* c, const bpvo_hip_motion_stereo* setting)
{
  CHECK_CTX(c);
  if(!setting) return fail(c, BPVO_ERR_INVALID_ARG, "nullptr motion stereo");
  if(int rc = ms_check_setting(c, setting)) return rc;
  if(setting->mode == 1) ms_states(c);
  c->motion_stereo.prm = *setting;
  ms_recount(c);
  return BPVO_OK;
}
int bpvo_hip_get_motion_stereo(const bpvo_hip_ctx* c, bpvo_hip_motion_stereo* setting)
{
  if(!c || !setting) return BPVO_ERR_INVALID_ARG;
  *setting = c->motion_stereo.prm;
  return BPVO_OK;
}
int bpvo_hip_seq_set_motion_stereo(bpvo_hip_ctx* c, int seq, const bpvo_hip_motion_stereo* setting)
{
  CHECK_CTX(c); CHECK_SEQ(c, seq);
  if(setting)
    if(int rc = ms_check_setting(c, setting)) return rc;
  if(!setting && c->motion_stereo.seq.empty()) return BPVO_OK;
  ms_states(c);
  MotionStereoSeq& q = c->motion_stereo.seq[(size_t) seq];
  q.own = setting != nullptr;
  if(setting) q.prm = *setting;
  ms_recount(c);
  return BPVO_OK;
}
int bpvo_hip_seq_get_motion_stereo(const bpvo_hip_ctx* c, int seq, bpvo_hip_motion_stereo* setting, int* own)
{
  if(!c || !setting || seq < 0 || seq >= seq_capacity(c)) return BPVO_ERR_INVALID_ARG;
  *setting = ms_setting(c, seq);
  if(own) *own = (size_t) seq < c->motion_stereo.seq.size() && c->motion_stereo.seq[(size_t) seq].own ? 1 : 0;
  return BPVO_OK;
}
int bpvo_hip_vo_motion_stereo_info(bpvo_hip_ctx* c, bpvo_hip_motion_stereo_info* info)
{
  CHECK_CTX(c);
  return ms_get_info(c, 0, info);
}
int bpvo_hip_seq_motion_stereo_info(bpvo_hip_ctx* c, int seq, bpvo_hip_motion_stereo_info* info)
{
  CHECK_CTX(c); CHECK_SEQ(c, seq);
  return ms_get_info(c, seq, info);
}
int bpvo_hip_motion_stereo_frames(bpvo_hip_ctx* c, int n, const bpvo_hip_camera* cams, const uint8_t* first, const uint8_t* second,
                                  const float* motions, const float* prior_disparity, const float* prior_variance, int on_device,
                                  float* out_disparity, float* out_variance, uint8_t* out_class)
{
  CHECK_CTX(c);
  if(n < 1 || !cams) return fail(c, BPVO_ERR_INVALID_ARG, "motion_stereo_frames: n >= 1 cameras");
  if(!first || !second || !motions || !prior_disparity || !prior_variance) return fail(c, BPVO_ERR_INVALID_ARG, "nullptr image/motion/prior");
  MotionStereoState& S = c->motion_stereo;
  if(S.prm.mode != 1) return fail(c, BPVO_ERR_INVALID_ARG, "motion_stereo_frames: the context's setting is not in mode 1 (bpvo_hip_set_motion_stereo)");
  size_t npix = 0;
  for(int i = 0; i < n; ++i) {
    if(cams[i].rows < 1 || cams[i].cols < 1 || cams[i].rows > kRectMaxRaw || cams[i].cols > kRectMaxRaw) return seq_fail(c, BPVO_ERR_INVALID_ARG, i, "camera: image size out of range");
    if(!(cams[i].K[0] > 0.0f) || !(cams[i].K[4] > 0.0f) || !(cams[i].baseline > 0.0f) || !std::isfinite(cams[i].K[0]) || !std::isfinite(cams[i].K[4]) ||
       !std::isfinite(cams[i].K[2]) || !std::isfinite(cams[i].K[5]) || !std::isfinite(cams[i].baseline))
      return seq_fail(c, BPVO_ERR_INVALID_ARG, i, "camera: fx, fy and the baseline must be positive, the intrinsics finite");
    npix += (size_t) cams[i].rows * cams[i].cols;
  }
  (void) hipSetDevice(c->device);
  const uint8_t* dc = first;
  const uint8_t* dk = second;
  const float* dpd = prior_disparity;
  const float* dpv = prior_variance;
  float* dd = out_disparity;
  float* dv = out_variance;
  uint8_t* dcl = out_class;
  const size_t npad = (npix + 3) / 4 * 4;
  if(!on_device) {      // [pd][pv][first][second] in, [D][V][class] out: buffers of the feature's own
    if(npad * 10 > S.frames_in.size() || npad * 9 > S.frames_out.size()) {
      HIP_CK(c, hipStreamSynchronize(c->stream));
      HIP_CK(c, S.frames_in.reserve(npad * 10));
      HIP_CK(c, S.frames_out.reserve(npad * 9));
    }
    float* in_f = reinterpret_cast<float*>(S.frames_in.get());
    uint8_t* in_b = S.frames_in.get() + npad * 8;
    HIP_CK(c, hipMemcpyAsync(in_f, prior_disparity, npix * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIP_CK(c, hipMemcpyAsync(in_f + npad, prior_variance, npix * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIP_CK(c, hipMemcpyAsync(in_b, first, npix, hipMemcpyHostToDevice, c->stream));
    HIP_CK(c, hipMemcpyAsync(in_b + npad, second, npix, hipMemcpyHostToDevice, c->stream));
    dpd = in_f; dpv = in_f + npad; dc = in_b; dk = in_b + npad;
    float* out_f = reinterpret_cast<float*>(S.frames_out.get());
    dd = out_disparity ? out_f : nullptr;
    dv = out_variance ? out_f + npad : nullptr;
    dcl = out_class ? S.frames_out.get() + npad * 8 : nullptr;
  }
  if(int rc = ms_tables(c, (size_t) n)) return rc;
  size_t at = 0;
  for(int i = 0; i < n; ++i) {
    MotionStereoJob& j = S.h_jobs[i];
    j = MotionStereoJob{};
    j.C = dc + at; j.K = dk + at; j.pd = dpd + at; j.pv = dpv + at;
    j.out_d = dd ? dd + at : nullptr; j.out_v = dv ? dv + at : nullptr; j.out_c = dcl ? dcl + at : nullptr;
    const DfCamera cam{cams[i].K[0], cams[i].K[4], cams[i].K[2], cams[i].K[5], cams[i].baseline, c->params.minValidDisparity, c->params.maxValidDisparity,
                       cams[i].rows, cams[i].cols};
    ms_job_rule(j, S.prm, cam, motions + 16 * (size_t) i);
    at += (size_t) cams[i].rows * cams[i].cols;
  }
  int rc = ms_launch(c, (size_t) n, std::vector<int>((size_t) n, -1));
  if(rc) { (void) hipStreamSynchronize(c->stream); return rc; }
  if(!on_device) {
    if(out_disparity) HIP_CK(c, hipMemcpyAsync(out_disparity, dd, npix * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    if(out_variance) HIP_CK(c, hipMemcpyAsync(out_variance, dv, npix * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    if(out_class) HIP_CK(c, hipMemcpyAsync(out_class, dcl, npix, hipMemcpyDeviceToHost, c->stream));
  }
  HIP_CK(c, hipStreamSynchronize(c->stream));
  return ms_resolve(c);
}
int bpvo_hip_motion_stereo_counts(bpvo_hip_ctx* c, uint64_t* launches, uint64_t* pixels, uint64_t* tiles, uint64_t* classes)
{
  CHECK_CTX(c);
  if(tiles || classes)
    if(int rc = ms_resolve(c)) return rc;
  if(launches) *launches = c->motion_stereo.launches;
  if(pixels) *pixels = c->motion_stereo.pixels;
  for(int t = 0; tiles && t < 3; ++t) tiles[t] = c->motion_stereo.tiles[t];
  for(int t = 0; classes && t < 7; ++t) classes[t] = c->motion_stereo.classes[t];
  return BPVO_OK;
}
#undef CHECK_SEQ

}  // extern "C"
