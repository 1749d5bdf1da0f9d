// libbpvo_hip, host side: the measurement variance (include/bpvo_hip/c_api.h; the rule: disparity_variance_math.h; the kernel:
// kernels_disparity_variance.hip).  The stereo front-end (stereo.hip stereo_front) calls variance_front behind the matcher: ONE launch over a
// table of jobs for the pairs of the call whose sequence fuses its disparities with a per-pixel measurement variance, into c->st_var; the fusion
// items of those frames (vo.hip) carry the pointer.  bpvo_hip_disparity_variance_frames runs the same launch for a caller's pairs.  With mode 0
// everywhere, or without fusion, no existing call launches, allocates or reads anything of this file.
#include "host_ctx.h"
#include "disparity_variance_math.h"

namespace bpvo_hip_host {

static const bpvo_hip_measurement_variance& variance_setting(const bpvo_hip_ctx* c, int seq)
{
  const VarianceState& S = c->variance;
  return (size_t) seq < S.seq.size() && S.seq[(size_t) seq].own ? S.seq[(size_t) seq].prm : S.prm;
}
static bool variance_on(const bpvo_hip_ctx* c, int seq) { return c->variance.n_on > 0 && variance_setting(c, seq).mode == 1 && fusion_on(c, seq); }

static void variance_recount(bpvo_hip_ctx* c)
{
  VarianceState& S = c->variance;
  S.n_on = 0;
  for(size_t s = 0; s < S.seq.size(); ++s) S.n_on += variance_setting(c, (int) s).mode == 1 ? 1 : 0;
}
static void variance_states(bpvo_hip_ctx* c)
{
  if(c->variance.seq.empty()) c->variance.seq.resize((size_t) std::max(1, seq_capacity(c)));
}
// the counters of the last launch, once they have landed: the classes into the records of its sequences, the tiles into the totals
static int variance_resolve(bpvo_hip_ctx* c)
{
  VarianceState& S = c->variance;
  if(S.pending.empty()) return BPVO_OK;
  HIP_CK(c, hipEventSynchronize(S.done_ev));
  for(size_t k = 0; k < S.pending.size(); ++k) {
    const unsigned* cnt = S.h_counts + kVarianceCounters * k;
    for(int t = 0; t < 3; ++t) S.tiles[t] += cnt[DV_CLASSES + t];
    if(S.pending[k] < 0) continue;
    bpvo_hip_measurement_variance_info& info = S.seq[(size_t) S.pending[k]].info;
    info.invalid = cnt[DV_INVALID]; info.border = cnt[DV_BORDER]; info.flat = cnt[DV_FLAT];
    info.floor = cnt[DV_FLOOR]; info.ceiling = cnt[DV_CEILING]; info.model = cnt[DV_MODEL];
  }
  S.pending.clear();
  return BPVO_OK;
}
void variance_seq_reset(bpvo_hip_ctx* c, int seq)
{
  VarianceState& S = c->variance;
  if((size_t) seq >= S.seq.size()) return;
  (void) variance_resolve(c);
  S.seq[(size_t) seq].has = false;
  S.seq[(size_t) seq].info = bpvo_hip_measurement_variance_info{};
}
int variance_scratch_moved(bpvo_hip_ctx* c, size_t npix)
{
  c->variance.serial += 1;      // (whatever lay in c->st_var is gone, or is about to be rewritten by a larger call)
  if(!c->st_var) return BPVO_OK;
  c->st_var.reset();
  HIP_CK(c, c->st_var.alloc(npix));
  return BPVO_OK;
}
const float* variance_map_of(const bpvo_hip_ctx* c, int seq)
{
  const VarianceState& S = c->variance;
  if(!S.live || (size_t) seq >= S.seq.size()) return nullptr;
  const VarianceSeq& q = S.seq[(size_t) seq];
  return q.has && q.serial == S.serial ? c->st_var + q.offset : nullptr;
}

// variance_tables: the job table and the counters for m jobs, free to be written.  variance_launch: the launch for the m rows the caller has put
// into S.h_jobs (but for the counters' address), the counters on their way back; owners[k]: the sequence of job k, or -1.
static int variance_tables(bpvo_hip_ctx* c, size_t m)
{
  VarianceState& S = c->variance;
  if(int rc = variance_resolve(c)) return rc;      // (and the last launch's copy has read the pinned rows)
  if(m > S.h_counts.size() / kVarianceCounters) {      // (the pinned counters come last: they say that all four are there)
    HIP_CK(c, hipStreamSynchronize(c->stream));
    S.d_jobs.reset(); S.h_jobs.reset(); S.d_counts.reset(); S.h_counts.reset();
    const size_t cap = std::max(m, (size_t) std::max(1, seq_capacity(c)));
    HIP_CK(c, S.d_jobs.alloc(cap));
    HIP_CK(c, S.h_jobs.alloc(cap));
    HIP_CK(c, S.d_counts.alloc(cap * kVarianceCounters));
    HIP_CK(c, S.h_counts.alloc(cap * kVarianceCounters));
  }
  if(!S.done_ev) HIP_CK(c, S.done_ev.create(hipEventDisableTiming));
  return BPVO_OK;
}
static int variance_launch(bpvo_hip_ctx* c, size_t m, const std::vector<int>& owners)
{
  VarianceState& S = c->variance;
  int max_tiles = 0;
  size_t pixels = 0;
  for(size_t k = 0; k < m; ++k) {
    VarianceJob& j = S.h_jobs[k];
    j.counts = S.d_counts + kVarianceCounters * k;
    max_tiles = std::max(max_tiles, disparity_variance_tiles(j.rows, j.cols));
    pixels += (size_t) j.rows * (size_t) j.cols;
  }
  HIP_CK(c, hipMemcpyAsync(S.d_jobs, S.h_jobs, sizeof(VarianceJob) * m, hipMemcpyHostToDevice, c->stream));
  HIP_CK(c, hipMemsetAsync(S.d_counts, 0, sizeof(unsigned) * kVarianceCounters * m, c->stream));
  S.timed = false;
  if(c->profiling) {      // (measurement: scripts/disparity_variance_bench.py)
    if(!S.t0) HIP_CK(c, S.t0.create());
    if(!S.t1) HIP_CK(c, S.t1.create());
    HIP_CK(c, hipEventRecord(S.t0, c->stream));
  }
  launch_disparity_variance(c->stream, S.d_jobs, (int) m, max_tiles);
  HIP_CK(c, hipGetLastError());
  if(c->profiling) {
    HIP_CK(c, hipEventRecord(S.t1, c->stream));
    S.timed = true;
  }
  HIP_CK(c, hipMemcpyAsync(S.h_counts, S.d_counts, sizeof(unsigned) * kVarianceCounters * m, hipMemcpyDeviceToHost, c->stream));
  HIP_CK(c, hipEventRecord(S.done_ev, c->stream));
  S.pending = owners;
  S.launches += 1;
  S.pixels += pixels;
  return BPVO_OK;
}
static void variance_job_rule(VarianceJob& j, const bpvo_hip_measurement_variance& prm, float lo, float hi)
{
  const DvRule r = dv_rule(prm.radius, prm.noise_sigma, prm.min_sigma, prm.max_sigma);
  j.radius = r.radius; j.noise2 = r.noise2; j.min2 = r.min2; j.max2 = r.max2;
  j.lo = lo; j.hi = hi;
}

int variance_front(bpvo_hip_ctx* c, int n, const StereoSize* sz, const int* ids, const uint8_t* d_left, const uint8_t* d_right)
{
  VarianceState& S = c->variance;
  S.live = false;
  if(S.n_on == 0 || c->fusion.n_on == 0) return BPVO_OK;
  std::vector<int> owners;
  for(int i = 0; i < n; ++i)
    if(variance_on(c, ids ? ids[i] : 0)) owners.push_back(ids ? ids[i] : 0);
  if(owners.empty()) return BPVO_OK;
  if(!c->st_var) HIP_CK(c, c->st_var.alloc(c->st_pixels));      // (the front-end's scratch holds at least this call's pixels: stereo_reserve)
  const size_t m = owners.size();
  if(int rc = variance_tables(c, m)) return rc;
  S.serial += 1;
  size_t at = 0, k = 0;
  for(int i = 0; i < n; ++i) {
    const size_t npix = (size_t) sz[i].rows * sz[i].cols;
    const int s = ids ? ids[i] : 0;
    if(variance_on(c, s)) {
      // the gate of the sequence's parameters, as its fusion and its template stage read it
      const bpvo_hip_params& sp = ids && c->frames[3 * s].seq_params ? *c->frames[3 * s].seq_params : c->params;
      VarianceJob& j = S.h_jobs[k++];
      j = VarianceJob{};
      j.L = d_left + at; j.R = d_right + at; j.M = c->st_disp + at; j.out = c->st_var + at;
      j.rows = sz[i].rows; j.cols = sz[i].cols;
      variance_job_rule(j, variance_setting(c, s), sp.minValidDisparity, sp.maxValidDisparity);
      VarianceSeq& q = S.seq[(size_t) s];
      q.has = true; q.offset = at; q.npix = npix; q.serial = S.serial;
      q.info = bpvo_hip_measurement_variance_info{};
    }
    at += npix;
  }
  if(int rc = variance_launch(c, m, owners)) return rc;
  S.live = true;
  return BPVO_OK;
}

double variance_last_ms(bpvo_hip_ctx* c)
{
  VarianceState& S = c->variance;
  float ms = -1.0f;
  if(!S.timed || hipEventSynchronize(S.t1) != hipSuccess) return -1.0;
  if(hipEventElapsedTime(&ms, S.t0, S.t1) != hipSuccess) return -1.0;
  return (double) ms;
}

static int variance_check_setting(bpvo_hip_ctx* c, const bpvo_hip_measurement_variance* v)
{
  if(v->mode != 0 && v->mode != 1) return fail(c, BPVO_ERR_INVALID_ARG, "measurement variance: mode must be 0 (off) or 1 (on)");
  if(v->mode == 0) return BPVO_OK;
  if(const char* why = dv_refusal(v->radius, v->noise_sigma, v->min_sigma, v->max_sigma)) return fail(c, BPVO_ERR_INVALID_ARG, why);
  return BPVO_OK;
}
static int variance_get_map(bpvo_hip_ctx* c, int seq, float* variance)
{
  VarianceState& S = c->variance;
  if(!variance) return fail(c, BPVO_ERR_INVALID_ARG, "nullptr variance map");
  if((size_t) seq >= S.seq.size() || !S.seq[(size_t) seq].has) return seq_fail(c, BPVO_ERR_NO_DATA, seq, "has no measurement variance map (no stereo call has made one)");
  const VarianceSeq& q = S.seq[(size_t) seq];
  if(q.serial != S.serial) return seq_fail(c, BPVO_ERR_NO_DATA, seq, "measurement variance map: a later call has reused the front-end's scratch");
  (void) hipSetDevice(c->device);
  HIP_CK(c, hipMemcpyAsync(variance, c->st_var + q.offset, q.npix * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  HIP_CK(c, hipStreamSynchronize(c->stream));
  return BPVO_OK;
}
static int variance_get_info(bpvo_hip_ctx* c, int seq, bpvo_hip_measurement_variance_info* info)
{
  if(!info) return fail(c, BPVO_ERR_INVALID_ARG, "nullptr measurement variance info");
  if(int rc = variance_resolve(c)) return rc;
  if((size_t) seq >= c->variance.seq.size() || !c->variance.seq[(size_t) seq].has)
    return seq_fail(c, BPVO_ERR_NO_DATA, seq, "has no measurement variance map (no stereo call has made one)");
  *info = c->variance.seq[(size_t) seq].info;
  return BPVO_OK;
}

}  // namespace bpvo_hip_host

extern "C" {

#define CHECK_SEQ(c, s) if((s) < 0 || (s) >= seq_capacity(c)) return seq_fail(c, BPVO_ERR_INVALID_ARG, s, "no such sequence")

int bpvo_hip_set_measurement_variance(bpvo_hip_ctx* c, const bpvo_hip_measurement_variance* setting)
{
  CHECK_CTX(c);
  if(!setting) return fail(c, BPVO_ERR_INVALID_ARG, "nullptr measurement variance");
  if(int rc = variance_check_setting(c, setting)) return rc;
  if(setting->mode == 1) variance_states(c);
  c->variance.prm = *setting;
  variance_recount(c);
  return BPVO_OK;
}
int bpvo_hip_get_measurement_variance(const bpvo_hip_ctx* c, bpvo_hip_measurement_variance* setting)
{
  if(!c || !setting) return BPVO_ERR_INVALID_ARG;
  *setting = c->variance.prm;
  return BPVO_OK;
}
int bpvo_hip_seq_set_measurement_variance(bpvo_hip_ctx* c, int seq, const bpvo_hip_measurement_variance* setting)
{
  CHECK_CTX(c); CHECK_SEQ(c, seq);
  if(setting)
    if(int rc = variance_check_setting(c, setting)) return rc;
  if(!setting && c->variance.seq.empty()) return BPVO_OK;
  variance_states(c);
  VarianceSeq& q = c->variance.seq[(size_t) seq];
  q.own = setting != nullptr;
  if(setting) q.prm = *setting;
  variance_recount(c);
  return BPVO_OK;
}
int bpvo_hip_seq_get_measurement_variance(const bpvo_hip_ctx* c, int seq, bpvo_hip_measurement_variance* setting, int* own)
{
  if(!c || !setting || seq < 0 || seq >= seq_capacity(c)) return BPVO_ERR_INVALID_ARG;
  *setting = variance_setting(c, seq);
  if(own) *own = (size_t) seq < c->variance.seq.size() && c->variance.seq[(size_t) seq].own ? 1 : 0;
  return BPVO_OK;
}
int bpvo_hip_vo_get_measurement_variance(bpvo_hip_ctx* c, float* variance)
{
  CHECK_CTX(c);
  return variance_get_map(c, 0, variance);
}
int bpvo_hip_seq_get_measurement_variance_map(bpvo_hip_ctx* c, int seq, float* variance)
{
  CHECK_CTX(c); CHECK_SEQ(c, seq);
  return variance_get_map(c, seq, variance);
}
int bpvo_hip_vo_measurement_variance_info(bpvo_hip_ctx* c, bpvo_hip_measurement_variance_info* info)
{
  CHECK_CTX(c);
  return variance_get_info(c, 0, info);
}
int bpvo_hip_seq_measurement_variance_info(bpvo_hip_ctx* c, int seq, bpvo_hip_measurement_variance_info* info)
{
  CHECK_CTX(c); CHECK_SEQ(c, seq);
  return variance_get_info(c, seq, info);
}
int bpvo_hip_disparity_variance_frames(bpvo_hip_ctx* c, int n, const bpvo_hip_camera* cams, const uint8_t* left, const uint8_t* right,
                                       const float* disparity, int on_device, float lo, float hi, const bpvo_hip_measurement_variance* setting,
                                       float* variance_out, int variance_on_device, uint32_t* counts_out)
{
  CHECK_CTX(c);
  if(n < 1 || !cams) return fail(c, BPVO_ERR_INVALID_ARG, "disparity_variance_frames: n >= 1 cameras");
  if(!left || !right || !disparity || !variance_out) return fail(c, BPVO_ERR_INVALID_ARG, "nullptr image/disparity/variance");
  if(!setting || setting->mode != 1) return fail(c, BPVO_ERR_INVALID_ARG, "disparity_variance_frames: needs a setting in mode 1");
  if(int rc = variance_check_setting(c, setting)) return rc;
  size_t npix = 0;
  for(int i = 0; i < n; ++i) {
    if(cams[i].rows < 1 || cams[i].cols < 1) return seq_fail(c, BPVO_ERR_INVALID_ARG, i, "camera: image size out of range");
    npix += (size_t) cams[i].rows * cams[i].cols;
  }
  (void) hipSetDevice(c->device);
  VarianceState& S = c->variance;
  const uint8_t* dl = left;
  const uint8_t* dr = right;
  const float* dm = disparity;
  float* dv = variance_out;
  if(!on_device || !variance_on_device) {      // (the front-end's scratch, as bpvo_hip_stereo_frames takes it)
    if(int rc = stereo_reserve(c, npix)) return rc;
    if(!variance_on_device && !c->st_var) HIP_CK(c, c->st_var.alloc(c->st_pixels));
  }
  if(!on_device) {
    HIP_CK(c, hipMemcpyAsync(c->st_left, left, npix, hipMemcpyHostToDevice, c->stream));
    HIP_CK(c, hipMemcpyAsync(c->st_right, right, npix, hipMemcpyHostToDevice, c->stream));
    HIP_CK(c, hipMemcpyAsync(c->st_disp, disparity, npix * sizeof(float), hipMemcpyHostToDevice, c->stream));
    dl = c->st_left; dr = c->st_right; dm = c->st_disp;
  }
  if(!variance_on_device) { dv = c->st_var; S.serial += 1; }      // (the sequences' maps in it are gone)
  if(int rc = variance_tables(c, (size_t) n)) return rc;
  size_t at = 0;
  for(int i = 0; i < n; ++i) {
    VarianceJob& j = S.h_jobs[i];
    j = VarianceJob{};
    j.L = dl + at; j.R = dr + at; j.M = dm + at; j.out = dv + at;
    j.rows = cams[i].rows; j.cols = cams[i].cols;
    variance_job_rule(j, *setting, lo, hi);
    at += (size_t) cams[i].rows * cams[i].cols;
  }
  int rc = variance_launch(c, (size_t) n, std::vector<int>((size_t) n, -1));
  if(rc) { (void) hipStreamSynchronize(c->stream); return rc; }
  if(!variance_on_device) HIP_CK(c, hipMemcpyAsync(variance_out, c->st_var, npix * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  HIP_CK(c, hipStreamSynchronize(c->stream));
  if(counts_out)
    for(int i = 0; i < n; ++i)
      for(int k = 0; k < DV_CLASSES; ++k) counts_out[DV_CLASSES * i + k] = S.h_counts[kVarianceCounters * (size_t) i + k];
  return variance_resolve(c);
}
int bpvo_hip_fuse_disparities_var(bpvo_hip_ctx* c, int n, const int* seq, const float* disparities, const float* variances, int on_device,
                                  const float* poses)
{
  CHECK_CTX(c);
  if(!variances) return fail(c, BPVO_ERR_INVALID_ARG, "nullptr variances");
  return fuse_disparities_impl(c, n, seq, disparities, variances, on_device, poses);
}
int bpvo_hip_measurement_variance_counts(bpvo_hip_ctx* c, uint64_t* launches, uint64_t* pixels, uint64_t* tiles)
{
  CHECK_CTX(c);
  if(tiles)
    if(int rc = variance_resolve(c)) return rc;
  if(launches) *launches = c->variance.launches;
  if(pixels) *pixels = c->variance.pixels;
  for(int t = 0; tiles && t < 3; ++t) tiles[t] = c->variance.tiles[t];
  return BPVO_OK;
}
#undef CHECK_SEQ

}  // extern "C"
