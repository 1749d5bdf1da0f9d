// libbpvo_hip, host side: disparity fusion (include/bpvo_hip/c_api.h; the rule: disparity_fusion_math.h; the kernels: kernels_disparity_fusion.hip).
// A sequence in mode 1 carries a disparity and a variance map outside its frame slots; a stage (fusion_stage) predicts the carried maps of all
// the sequences it is given into their new frames and fuses them with the slots' measured maps, in two launches over a table of jobs.  The
// addFrame drivers (vo.hip) queue the stage in front of the template stage; bpvo_hip_fuse_disparities runs it for a caller's own motions.  With
// mode 0 everywhere no existing call launches, allocates or reads anything of this file.
#include "host_ctx.h"
#include "disparity_fusion_math.h"

namespace bpvo_hip_host {

static const bpvo_hip_disparity_fusion& fusion_setting(const bpvo_hip_ctx* c, int seq)
{
  const FusionState& F = c->fusion;
  return (size_t) seq < F.seq.size() && F.seq[(size_t) seq].own ? F.seq[(size_t) seq].prm : F.prm;
}
bool fusion_on(const bpvo_hip_ctx* c, int seq) { return c->fusion.n_on > 0 && fusion_setting(c, seq).mode == 1; }

static void fusion_recount(bpvo_hip_ctx* c)
{
  FusionState& F = c->fusion;
  F.n_on = 0;
  for(size_t s = 0; s < F.seq.size(); ++s) F.n_on += fusion_setting(c, (int) s).mode == 1 ? 1 : 0;
}
// the counters of the last stage, once they have landed, into the records of its sequences
static int fusion_resolve(bpvo_hip_ctx* c)
{
  FusionState& F = c->fusion;
  if(F.pending.empty()) return BPVO_OK;
  HIP_CK(c, hipEventSynchronize(F.done_ev));
  for(size_t k = 0; k < F.pending.size(); ++k) {
    bpvo_hip_disparity_fusion_info& info = F.seq[(size_t) F.pending[k]].info;
    const unsigned* cnt = F.h_counts + DF_CLASSES * k;
    info.fused = cnt[DF_FUSED]; info.replaced = cnt[DF_REPLACED]; info.measured = cnt[DF_MEASURED]; info.filled = cnt[DF_FILLED]; info.none = cnt[DF_NONE];
  }
  F.pending.clear();
  return BPVO_OK;
}
void fusion_seq_reset(bpvo_hip_ctx* c, int seq)
{
  FusionState& F = c->fusion;
  if((size_t) seq >= F.seq.size()) return;
  (void) fusion_resolve(c);
  F.seq[(size_t) seq].carried = false;
  F.seq[(size_t) seq].info = bpvo_hip_disparity_fusion_info{};
}

// the slab of a sequence for a camera of npix pixels (a z-buffer is zeroed here, once, and left all zero by every stage)
static int fusion_storage(bpvo_hip_ctx* c, FusionSeq& q, size_t npix)
{
  if(q.slab && q.npix == npix) return BPVO_OK;
  if(q.slab) HIP_CK(c, hipStreamSynchronize(c->stream));
  q.slab.reset();
  q.carried = false;
  const size_t npad = (npix + 3) / 4 * 4;
  HIP_CK(c, q.slab.alloc(npad * 8 + npix * 8));
  q.npix = npix;
  q.Dc = reinterpret_cast<float*>(q.slab.get());
  q.Vc = q.Dc + npad;
  q.zbuf = reinterpret_cast<unsigned long long*>(q.slab.get() + npad * 8);
  HIP_CK(c, hipMemsetAsync(q.zbuf, 0, npix * 8, c->stream));
  return BPVO_OK;
}

int fusion_stage(bpvo_hip_ctx* c, int n, const FusionItem* items)
{
  FusionState& F = c->fusion;
  if(F.n_on == 0) return BPVO_OK;
  std::vector<const FusionItem*> act;
  for(int i = 0; i < n; ++i)
    if(fusion_on(c, items[i].seq)) act.push_back(&items[i]);
  if(act.empty()) return BPVO_OK;
  if(int rc = fusion_resolve(c)) return rc;      // (and the last stage's copy has read the pinned rows)
  const size_t cap = F.seq.size();
  if(!F.h_counts) {      // (the pinned counters come last: they say that all four are there)
    if(!F.d_jobs) HIP_CK(c, F.d_jobs.alloc(cap));
    if(!F.h_jobs) HIP_CK(c, F.h_jobs.alloc(cap));
    if(!F.d_counts) HIP_CK(c, F.d_counts.alloc(cap * DF_CLASSES));
    if(!F.done_ev) HIP_CK(c, F.done_ev.create(hipEventDisableTiming));
    HIP_CK(c, F.h_counts.alloc(cap * DF_CLASSES));
  }
  const size_t m = act.size();
  size_t max_pixels = 0, pixels = 0;
  bool any_predict = false;
  std::vector<MotionStereoView> views;      // (motion stereo, motion_stereo.hip: the jobs' second views; stays empty unless a sequence has it on)
  for(size_t k = 0; k < m; ++k) {
    const FusionItem& it = *act[k];
    FusionSeq& q = F.seq[(size_t) it.seq];
    const FrameSlot& f = c->frames[it.slot];
    const LevelGeom& g = slot_geom(c, f, 0);
    if(int rc = fusion_storage(c, q, g.npix)) return rc;
    const bpvo_hip_params& sp = f.seq_params ? *f.seq_params : c->params;
    const bpvo_hip_disparity_fusion& prm = fusion_setting(c, it.seq);
    const DfRule rule = df_rule(prm.measurement_sigma, prm.process_sigma, prm.gate, prm.max_fill_sigma);
    FusionJob& j = F.h_jobs[k];
    j = FusionJob{};
    j.rows = g.rows; j.cols = g.cols;
    j.predict = (it.P && q.carried && df_motion_ok(it.P)) ? 1 : 0;
    j.fx = g.K[0]; j.fy = g.K[4]; j.cx = g.K[2]; j.cy = g.K[5]; j.b = g.b;
    j.lo = sp.minValidDisparity; j.hi = sp.maxValidDisparity;
    j.r2 = rule.r2; j.q2 = rule.q2; j.gate = rule.gate; j.fill2 = rule.fill2;
    if(it.P) std::memcpy(j.P, it.P, sizeof(j.P));
    j.slot = f.disp; j.Dc = q.Dc; j.Vc = q.Vc; j.zbuf = q.zbuf; j.counts = F.d_counts + DF_CLASSES * k;
    j.R = it.R;
    any_predict = any_predict || j.predict;
    if(c->motion_stereo.n_on > 0) views.push_back(MotionStereoView{it.seq, it.slot, j.predict ? it.view_slot : -1, it.T_view, q.zbuf});
    max_pixels = std::max(max_pixels, g.npix);
    pixels += g.npix;
    q.info = bpvo_hip_disparity_fusion_info{};
    q.info.predicted = j.predict;
    q.info.slot = it.slot;
    if(it.P) std::memcpy(q.info.motion, it.P, 64);
    else std::memcpy(q.info.motion, m44_identity().m, 64);
    q.carried = true;
  }
  HIP_CK(c, hipMemcpyAsync(F.d_jobs, F.h_jobs, sizeof(FusionJob) * m, hipMemcpyHostToDevice, c->stream));
  HIP_CK(c, hipMemsetAsync(F.d_counts, 0, sizeof(unsigned) * DF_CLASSES * m, c->stream));
  F.timed = false;
  if(c->profiling) {      // (measurement: scripts/disparity_fusion_bench.py)
    if(!F.t0) HIP_CK(c, F.t0.create());
    if(!F.t1) HIP_CK(c, F.t1.create());
    if(!F.t2) HIP_CK(c, F.t2.create());
    HIP_CK(c, hipEventRecord(F.t0, c->stream));
  }
  if(any_predict) launch_fusion_splat(c->stream, F.d_jobs, (int) m, max_pixels);
  // motion stereo: the predictions of the sequences that have it on, refined in place before the update reads them (one launch, or none; while
  // profiling its duration counts into the splat's, and is its own option besides).  A failure there is returned behind the update: the update
  // is what leaves the z-buffers all zero again.
  bool refined = false;
  const int refine_rc = views.empty() ? BPVO_OK : motion_stereo_stage(c, (int) views.size(), views.data(), &refined);
  if(c->profiling) HIP_CK(c, hipEventRecord(F.t1, c->stream));
  launch_fusion_update(c->stream, F.d_jobs, (int) m, max_pixels);
  HIP_CK(c, hipGetLastError());
  if(c->profiling) {
    HIP_CK(c, hipEventRecord(F.t2, c->stream));
    F.timed = true;
  }
  HIP_CK(c, hipMemcpyAsync(F.h_counts, F.d_counts, sizeof(unsigned) * DF_CLASSES * m, hipMemcpyDeviceToHost, c->stream));
  HIP_CK(c, hipEventRecord(F.done_ev, c->stream));
  for(size_t k = 0; k < m; ++k) F.pending.push_back(act[k]->seq);
  F.launches += any_predict ? 2 : 1;
  F.pixels += pixels;
  return refine_rc;
}

double fusion_last_ms(bpvo_hip_ctx* c, int which)
{
  FusionState& F = c->fusion;
  float ms = -1.0f;
  if(!F.timed || hipEventSynchronize(F.t2) != hipSuccess) return -1.0;
  if(hipEventElapsedTime(&ms, which == 0 ? F.t0 : F.t1, which == 0 ? F.t1 : F.t2) != hipSuccess) return -1.0;
  return (double) ms;
}

// the slot a sequence's next frame goes to: where bpvo_hip_fuse_disparities leaves the fused map
static int fusion_cur_slot(const bpvo_hip_ctx* c, int seq)
{
  if(c->vo_mode == 1) return c->vo.cur;
  return c->seqs.empty() ? 3 * seq + 1 : c->seqs[(size_t) seq].cur;
}
static int fusion_check_setting(bpvo_hip_ctx* c, const bpvo_hip_disparity_fusion* f)
{
  if(f->mode != 0 && f->mode != 1) return fail(c, BPVO_ERR_INVALID_ARG, "disparity fusion: mode must be 0 (off) or 1 (on)");
  if(f->mode == 0) return BPVO_OK;
  if(const char* why = df_refusal(f->measurement_sigma, f->process_sigma, f->gate, f->max_fill_sigma)) return fail(c, BPVO_ERR_INVALID_ARG, why);
  if(!c->rigs.empty()) return fail(c, BPVO_ERR_UNSUPPORTED, "disparity fusion: a context that declares a rig does not serve mode 1");
  if(seq_capacity(c) < 1) return fail(c, BPVO_ERR_INVALID_ARG, "disparity fusion: needs a ctx with n_frames >= 3 and n_pairs >= 1");
  return BPVO_OK;
}
static void fusion_states(bpvo_hip_ctx* c)
{
  if(c->fusion.seq.empty()) c->fusion.seq.resize((size_t) std::max(1, seq_capacity(c)));
}
static int fusion_get_maps(bpvo_hip_ctx* c, int seq, float* disparity, float* variance)
{
  FusionState& F = c->fusion;
  if((size_t) seq >= F.seq.size() || !F.seq[(size_t) seq].carried) return seq_fail(c, BPVO_ERR_NO_DATA, seq, "carries no fused disparity");
  const FusionSeq& q = F.seq[(size_t) seq];
  (void) hipSetDevice(c->device);
  if(disparity) HIP_CK(c, hipMemcpyAsync(disparity, q.Dc, q.npix * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  if(variance) HIP_CK(c, hipMemcpyAsync(variance, q.Vc, q.npix * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  HIP_CK(c, hipStreamSynchronize(c->stream));
  return BPVO_OK;
}
static int fusion_get_info(bpvo_hip_ctx* c, int seq, bpvo_hip_disparity_fusion_info* info)
{
  if(!info) return fail(c, BPVO_ERR_INVALID_ARG, "nullptr fusion info");
  if(int rc = fusion_resolve(c)) return rc;
  if((size_t) seq < c->fusion.seq.size()) *info = c->fusion.seq[(size_t) seq].info;
  else *info = bpvo_hip_disparity_fusion_info{};
  return BPVO_OK;
}

int fuse_disparities_impl(bpvo_hip_ctx* c, int n, const int* seq, const float* disparities, const float* variances, int on_device, const float* poses)
{
  const int limit = seq_capacity(c);
  if(n < 1 || n > limit) return fail(c, BPVO_ERR_INVALID_ARG, "fuse_disparities: n must be within 1 .. the sequence capacity");
  if(c->vo_mode == 1 && n != 1) return fail(c, BPVO_ERR_INVALID_ARG, "fuse_disparities: a context that runs bpvo_hip_add_frame has one sequence");
  if(!disparities || !poses) return fail(c, BPVO_ERR_INVALID_ARG, "nullptr disparity/pose");
  std::vector<FusionItem> items((size_t) n);
  std::vector<char> seen((size_t) limit, 0);
  for(int i = 0; i < n; ++i) {
    const int s = seq ? seq[i] : i;
    if(s < 0 || s >= limit) return seq_fail(c, BPVO_ERR_INVALID_ARG, s, "no such sequence");
    if(seen[(size_t) s]) return seq_fail(c, BPVO_ERR_INVALID_ARG, s, "appears twice in one call");
    seen[(size_t) s] = 1;
    if(!fusion_on(c, s)) return seq_fail(c, BPVO_ERR_INVALID_ARG, s, "fuse_disparities: the sequence is not in mode 1 (bpvo_hip_set_disparity_fusion)");
    items[(size_t) i] = FusionItem{s, fusion_cur_slot(c, s), poses + 16 * (size_t) i};
  }
  (void) hipSetDevice(c->device);
  size_t total = 0;
  for(int i = 0; i < n; ++i) total += slot_geom(c, c->frames[items[(size_t) i].slot], 0).npix;
  const float* d_var = variances;      // the caller's variance maps on the device (host maps: uploaded into a buffer of the feature's own)
  if(variances && !on_device) {
    DeviceBuf<float>& buf = c->variance.fuse_var;
    if(total > buf.size()) {
      HIP_CK(c, hipStreamSynchronize(c->stream));
      HIP_CK(c, buf.reserve(total));
    }
    HIP_CK(c, hipMemcpyAsync(buf, variances, total * sizeof(float), hipMemcpyHostToDevice, c->stream));
    d_var = buf;
  }
  size_t at = 0;
  for(int i = 0; i < n; ++i) {
    const FrameSlot& f = c->frames[items[(size_t) i].slot];
    const size_t npix = slot_geom(c, f, 0).npix;
    HIP_CK(c, hipMemcpyAsync(f.disp, disparities + at, npix * sizeof(float), on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c->stream));
    if(d_var) items[(size_t) i].R = d_var + at;
    at += npix;
  }
  const int rc = fusion_stage(c, n, items.data());
  HIP_CK(c, hipStreamSynchronize(c->stream));
  return rc;
}

}  // namespace bpvo_hip_host

extern "C" {

#define CHECK_SEQ(c, s) if((s) < 0 || (s) >= seq_capacity(c)) return seq_fail(c, BPVO_ERR_INVALID_ARG, s, "no such sequence")

int bpvo_hip_set_disparity_fusion(bpvo_hip_ctx* c, const bpvo_hip_disparity_fusion* fusion)
{
  CHECK_CTX(c);
  if(!fusion) return fail(c, BPVO_ERR_INVALID_ARG, "nullptr disparity fusion");
  if(int rc = fusion_check_setting(c, fusion)) return rc;
  if(fusion->mode == 1) fusion_states(c);
  c->fusion.prm = *fusion;
  fusion_recount(c);
  return BPVO_OK;
}
int bpvo_hip_get_disparity_fusion(const bpvo_hip_ctx* c, bpvo_hip_disparity_fusion* fusion)
{
  if(!c || !fusion) return BPVO_ERR_INVALID_ARG;
  *fusion = c->fusion.prm;
  return BPVO_OK;
}
int bpvo_hip_seq_set_disparity_fusion(bpvo_hip_ctx* c, int seq, const bpvo_hip_disparity_fusion* fusion)
{
  CHECK_CTX(c); CHECK_SEQ(c, seq);
  if(fusion)
    if(int rc = fusion_check_setting(c, fusion)) return rc;
  if(!fusion && c->fusion.seq.empty()) return BPVO_OK;
  fusion_states(c);
  FusionSeq& q = c->fusion.seq[(size_t) seq];
  q.own = fusion != nullptr;
  if(fusion) q.prm = *fusion;
  fusion_recount(c);
  return BPVO_OK;
}
int bpvo_hip_seq_get_disparity_fusion(const bpvo_hip_ctx* c, int seq, bpvo_hip_disparity_fusion* fusion, int* own)
{
  if(!c || !fusion || seq < 0 || seq >= seq_capacity(c)) return BPVO_ERR_INVALID_ARG;
  *fusion = fusion_setting(c, seq);
  if(own) *own = (size_t) seq < c->fusion.seq.size() && c->fusion.seq[(size_t) seq].own ? 1 : 0;
  return BPVO_OK;
}
int bpvo_hip_vo_get_fused_disparity(bpvo_hip_ctx* c, float* disparity, float* variance)
{
  CHECK_CTX(c);
  return fusion_get_maps(c, 0, disparity, variance);
}
int bpvo_hip_seq_get_fused_disparity(bpvo_hip_ctx* c, int seq, float* disparity, float* variance)
{
  CHECK_CTX(c); CHECK_SEQ(c, seq);
  return fusion_get_maps(c, seq, disparity, variance);
}
int bpvo_hip_vo_disparity_fusion_info(bpvo_hip_ctx* c, bpvo_hip_disparity_fusion_info* info)
{
  CHECK_CTX(c);
  return fusion_get_info(c, 0, info);
}
int bpvo_hip_seq_disparity_fusion_info(bpvo_hip_ctx* c, int seq, bpvo_hip_disparity_fusion_info* info)
{
  CHECK_CTX(c); CHECK_SEQ(c, seq);
  return fusion_get_info(c, seq, info);
}
int bpvo_hip_fuse_disparities(bpvo_hip_ctx* c, int n, const int* seq, const float* disparities, int on_device, const float* poses)
{
  CHECK_CTX(c);
  return fuse_disparities_impl(c, n, seq, disparities, nullptr, on_device, poses);
}
int bpvo_hip_get_disparity(bpvo_hip_ctx* c, int slot, float* out)
{
  CHECK_CTX(c); CHECK_SLOT(c, slot);
  if(!out) return fail(c, BPVO_ERR_INVALID_ARG, "nullptr output");
  const FrameSlot& f = c->frames[slot];
  (void) hipSetDevice(c->device);
  HIP_CK(c, hipMemcpyAsync(out, f.disp, slot_geom(c, f, 0).npix * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  HIP_CK(c, hipStreamSynchronize(c->stream));
  return BPVO_OK;
}
int bpvo_hip_disparity_fusion_counts(bpvo_hip_ctx* c, uint64_t* launches, uint64_t* pixels)
{
  CHECK_CTX(c);
  if(launches) *launches = c->fusion.launches;
  if(pixels) *pixels = c->fusion.pixels;
  return BPVO_OK;
}
#undef CHECK_SEQ

}  // extern "C"
