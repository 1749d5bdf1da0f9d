// libbpvo_hip, host side: the per-frame stages — VisualOdometryFrame::setData (pyramid, descriptors) and setTemplate (saliency, selection, points,
// normalisation, template pixels and gradients) for batches of frames — and the accessors of their results.
#include "host_ctx.h"
#include "intensity_norm_math.h"

using namespace bpvo_hip;
using namespace bpvo_hip_host;

namespace bpvo_hip_host {

FrameRun ctx_run(bpvo_hip_ctx* c) { return FrameRun{c->stream, &c->lanes[0], 0, false, nullptr, nullptr}; }

// which: 0 = table of the setData stage, 1 = table of the setTemplate stage (two tables, so that queueing the template stage does not
// have to wait for the descriptor kernels that still read the first).  Returns the device table through *tab (row fr.tab of level 0).
int upload_frame_jobs(bpvo_hip_ctx* c, const int* slots, int count, const FrameRun& fr, int which, const FrameJob** tab)
{
  const size_t table = (size_t) which * c->L * c->n_frames;
  FR_CK(c, fr, hipEventSynchronize(fr.ln->staging_ev[which]));   // the pinned rows may still feed the copy of an earlier call
  for(int l = 0; l < c->L; ++l) {
    FrameJob* row = c->h_fjobs + table + (size_t) l * c->n_frames + fr.tab;
    for(int i = 0; i < count; ++i) row[i] = make_frame_job(c, c->frames[slots[i]], l);
  }
  // rows [tab, tab + count) of every level in one copy
  const size_t pitch = sizeof(FrameJob) * (size_t) c->n_frames;
  static_assert(sizeof(FrameJob) % 8 == 0 && sizeof(PairJob) % 8 == 0, "copy_rows_kernel moves 8-byte words");
  // (small tables too — up to 512 frames, 0.4 MB: a 2-D copy of a few KB is a 20 us stop of the stream, the kernel 5 — what a stage of one or two frames notices)
  if(c->ctl_by_kernel.load() || count <= 512)
    launch_copy_rows(fr.stream, c->d_fjobs + table + fr.tab, c->h_fjobs + table + fr.tab, pitch, sizeof(FrameJob) * (size_t) count, c->L);
  else
    FR_CK(c, fr, hipMemcpy2DAsync(c->d_fjobs + table + fr.tab, pitch, c->h_fjobs + table + fr.tab, pitch, sizeof(FrameJob) * (size_t) count, (size_t) c->L,
                                  hipMemcpyHostToDevice, fr.stream));
  FR_CK(c, fr, hipEventRecord(fr.ln->staging_ev[which], fr.stream));
  *tab = c->d_fjobs + table + fr.tab;
  return BPVO_OK;
}
std::vector<int> strided_slots(int first, int stride, int count)
{
  std::vector<int> v((size_t) std::max(count, 0));
  for(int i = 0; i < count; ++i) v[i] = first + i * stride;
  return v;
}
// the launch-wide sizes of a stage: those of its slots (the context's, or one camera size of bpvo_hip_add_frames), which must all agree
static const LevelGeom* stage_geom(bpvo_hip_ctx* c, const int* slots, int count)
{
  const LevelGeom* geom = c->frames[slots[0]].own_geom ? c->frames[slots[0]].geom : c->geom;
  for(int i = 1; i < count; ++i)
    if(slot_geom(c, c->frames[slots[i]], 0).rows != geom[0].rows || slot_geom(c, c->frames[slots[i]], 0).cols != geom[0].cols) {
      fail(c, BPVO_ERR_INVALID_ARG, "frame stage over slots of different sizes");
      return nullptr;
    }
  return geom;
}

// VisualOdometryFrame::setData (reference: bpvo/vo_frame.cc:48-55) for `count` frames at once
// skip_odd_disp: the frames are the (A, B) frames of pairs, in that order: B (odd i) only ever serves as the CURRENT frame of its pair,
// whose disparity nothing reads (the reference copies what it is handed, bpvo/vo_frame.cc:50-51; estimatePose never looks at it) — it is
// neither uploaded nor copied: 40 % of a pair's input bytes
// (2: as 1, with the device-resident disparities packed for the even frames only — the staging area of the upload pipeline)
int frames_set_data_slots(bpvo_hip_ctx* c, const int* slots, int count, const uint8_t* images, const float* disps, bool on_device,
                          const FrameRun& fr, int skip_odd_disp, const size_t* offsets)
{
  if(count <= 0) return BPVO_OK;
  const LevelGeom* geom = stage_geom(c, slots, count);
  if(!geom) return BPVO_ERR_INVALID_ARG;
  const size_t npix = geom[0].npix;
  const bpvo_hip_params& p = c->params;
  const DescriptorForm form = descriptor_form(p, c->C, c->inorm_radius);
  hipStream_t s = fr.stream;
  if(!on_device) {
    for(int i = 0; i < count; ++i) {
      FrameSlot& f = c->frames[slots[i]];
      const size_t at = offsets ? offsets[i] : (size_t) i * npix;
      FR_CK(c, fr, hipMemcpyAsync(f.img[0], images + at, npix, hipMemcpyHostToDevice, s));
      if(!(skip_odd_disp && (i & 1)) && !fr.skip_disparity_upload)
        FR_CK(c, fr, hipMemcpyAsync(f.disp, disps + at, npix * sizeof(float), hipMemcpyHostToDevice, s));
    }
  }
  // pair batches: the compact channel-0 plane serves the saliency map of TEMPLATE frames only; the current frames' descriptor kernel
  // skips its store (the selection reads channel 0 from the records should such a frame be made a template later)
  // (FrameSlot::ch0_valid, set with the lazy flags below)
  // ... and the TEMPLATE frames (A, even) of a pair batch keep no records at the NMS levels (FrameSlot::lazy): bit-planes with the census
  // fused into the blur kernel, CD3 gradients.  Every other frame, and every frame set through the frame API, is dense.
  const bool lazy_ok = skip_odd_disp != 0 && c->lazy_template && form == DF_BITPLANES_FUSED && p.gradientEstimation == BPVO_GRAD_CD3;
  // ... and not even channel 0 where the tiled selection (NMS radius 1) forms it from the census bytes (option lazy_template_saliency):
  // census_templates_kernel writes those, and the blur below runs over the dense tile columns of such a level only
  const bool census_only_ok = lazy_ok && c->lazy_saliency;
  bool census_only[kMaxLevels] = {};
  bool any_census_only = false;
  for(int l = p.maxTestLevel; l < c->L; ++l) any_census_only |= census_only[l] = census_only_ok && geom[l].nms_radius == 1;
  for(int i = 0; i < count; ++i) {
    FrameSlot& f = c->frames[slots[i]];
    f.ch0_valid = !(skip_odd_disp && (i & 1));
    for(int l = 0; l < c->L; ++l) {
      f.lazy[l] = (lazy_ok && !(i & 1) && geom[l].nms_radius > 0) ? (census_only[l] ? 2 : 1) : 0;
      // a saliency map that would have been formed on demand from the data replaced here can no longer be (until the next template)
      if(f.sal_state[l] == FrameSlot::SAL_ON_DEMAND) f.sal_state[l] = FrameSlot::SAL_GONE;
    }
  }
  const FrameJob* tab = nullptr;
  int rc = upload_frame_jobs(c, slots, count, fr, 0, &tab);
  if(rc) return rc;
  const int NF = c->n_frames;
  if(on_device && offsets) {
    // (entries at arbitrary places of the packed inputs: their offsets travel in rows [tab, tab + count) of the sequences' offset table)
    size_t* h_off = c->h_seq_off + fr.tab;
    for(int i = 0; i < count; ++i) h_off[i] = offsets[i];
    FR_CK(c, fr, hipMemcpyAsync(c->d_seq_off + fr.tab, h_off, sizeof(size_t) * (size_t) count, hipMemcpyHostToDevice, s));
    launch_ingest_at(s, tab, images, disps, c->d_seq_off + fr.tab, npix, count);
  } else if(on_device) {
    launch_ingest(s, tab, images, disps, npix, count, skip_odd_disp);   // one launch instead of 2 copies per frame
  }
  {
    double px = 0;
    for(int l = 1; l < c->L; ++l) px += (double) geom[l].npix * count;
    ScopedTimer t(c, KC_PYRAMID, px, fr.ln);
    // ImagePyramid::compute (bpvo/image_pyramid.cc:43-50).  Few frames: up to three levels per launch (kernels_frame.hip pyramid_levels_kernel)
    bool grouped = count <= c->merge_levels_max_frames;
    for(int l = 0; l < c->L; ++l) grouped = grouped && geom[l].cols >= 8 && geom[l].rows >= 8;
    for(int l = 1; l < c->L;) {
      const int steps = grouped ? std::min(3, c->L - l) : 0;
      if(steps >= 2) {
        launch_pyramid_levels(s, tab + (size_t) (l - 1) * NF, NF, steps, geom[l + steps - 1].cols, geom[l + steps - 1].rows, count);
        l += steps;
      } else {
        launch_pyrdown(s, tab + (size_t) (l - 1) * NF, tab + (size_t) l * NF, geom[l].cols, geom[l].rows, count);
        l += 1;
      }
    }
  }
  {
    const int tested = c->L - p.maxTestLevel;
    double px = 0;
    for(int l = p.maxTestLevel; l < c->L; ++l) px += (double) geom[l].npix * count;
    ScopedTimer t(c, KC_DESCRIPTOR, px, fr.ln);
    // DenseDescriptorPyramid::init (dense_descriptor_pyramid.cc:67-71): the levels in one launch (frame_plan.h) or level by level
    for(const LevelSpan& sp : level_spans(c->L, p.maxTestLevel, merge_descriptor_levels(count, c->merge_levels_max_frames, tested, form))) {
      const FrameLaunch f = frame_launch(c, tab, geom, sp, count);
      switch(form) {
        case DF_BITPLANES_FUSED:
          // census-only levels of a pair batch's template frames: their census bytes, then — level by level — the current frames over every tile and
          // the template frames over the dense tile columns only; in one launch the blur kernel runs over all frames and leaves the lazy tiles itself
          if(sp.count > 1 ? any_census_only : census_only[sp.first]) launch_census_templates(s, f);
          if(sp.count == 1 && census_only[sp.first]) launch_bitplanes_pairs(s, f, c->gauss_k);
          else launch_bitplanes(s, f, p.sigmaBitPlanes, c->gauss_k, 1);
          break;
        case DF_BITPLANES_SMOOTHED_CENSUS:      // (conf/perf_bitplanes.cfg: two launches)
        case DF_BITPLANES_UNSMOOTHED:
          launch_census(s, f, p.sigmaPriorToCensusTransform > 0.0f ? c->census_taps : nullptr);
          launch_bitplanes(s, f, p.sigmaBitPlanes, c->gauss_k, 0);
          break;
        case DF_INTENSITY: launch_intensity(s, f); break;
        case DF_INTENSITY_NORM: launch_intensity_norm(s, f, c->inorm_radius); break;
        case DF_LAPLACIAN: launch_laplacian(s, f.jobs, f.W, f.R, count, p.laplacianKernelSize); break;
        case DF_GRADIENT: launch_gradient_descriptor(s, f.jobs, f.W, f.R, count, c->grad_pre); break;
        case DF_FIELDS_1ST:
        case DF_FIELDS_2ND: launch_descriptor_fields(s, f.jobs, f.W, f.R, count, form == DF_FIELDS_2ND, c->df_g1, c->df_g2); break;
        case DF_CENTRAL_DIFFERENCE: launch_central_difference(s, f.jobs, f.W, f.R, count, p.centralDifferenceRadius, c->cd_before, c->cd_after); break;
        case DF_LATCH:
          launch_latch(s, f.jobs, f.W, f.R, count, p.latchNumBytes, p.latchHalfSsdSize, c->d_latch_off, c->latch_taps[0], c->latch_taps[1], c->latch_after);
          break;
      }
    }
  }
  FR_CK(c, fr, hipGetLastError());
  for(int i = 0; i < count; ++i) {
    FrameSlot& f = c->frames[slots[i]];
    f.has_data = true;
    f.has_disp = !(skip_odd_disp && (i & 1));
  }
  return BPVO_OK;
}
// the disparity of a slot whose data stage ran with FrameRun::skip_disparity_upload, from the caller's host buffer, on the context's copy stream; the
// context's stream waits for it (whatever is queued there later sees the disparity).  A copy from pageable memory holds the host until it is done
// (1.2 MB of a 640x480 disparity: 90 us): addFrame calls this with the estimate queued, so that the GPU works meanwhile.
int upload_disparity(bpvo_hip_ctx* c, int slot, const float* disparity)
{
  if(!c->copy_stream) {
    HIP_CK(c, c->copy_stream.create());
    HIP_CK(c, c->copy_ev.create(hipEventDisableTiming));
  }
  HIP_CK(c, hipMemcpyAsync(c->frames[slot].disp, disparity, slot_geom(c, c->frames[slot], 0).npix * sizeof(float), hipMemcpyHostToDevice, c->copy_stream));
  HIP_CK(c, hipEventRecord(c->copy_ev, c->copy_stream));
  HIP_CK(c, hipStreamWaitEvent(c->stream, c->copy_ev, 0));
  return BPVO_OK;
}
int frames_set_data(bpvo_hip_ctx* c, int first, int stride, int count, const uint8_t* images, const float* disps, bool on_device, int skip_odd_disp)
{
  if(count <= 0) return BPVO_OK;
  if(first < 0 || stride < 1 || first + (count - 1) * stride >= c->n_frames) return fail(c, BPVO_ERR_INVALID_ARG, "bad frame slot range");
  if(!images || !disps) return fail(c, BPVO_ERR_INVALID_ARG, "nullptr image/disparity");
  return frames_set_data_slots(c, strided_slots(first, stride, count).data(), count, images, disps, on_device, ctx_run(c), skip_odd_disp);
}

// VisualOdometryFrame::setTemplate (reference: bpvo/vo_frame.cc:61-93 -> bpvo/template_data.cc:37-142) for `count` frames
int frames_set_template_slots(bpvo_hip_ctx* c, const int* slots, int count, const FrameRun& fr)
{
  if(count <= 0) return BPVO_OK;
  const LevelGeom* geom = stage_geom(c, slots, count);      // (storage: the context's)
  if(!geom) return BPVO_ERR_INVALID_ARG;
  hipStream_t s = fr.stream;
  for(int i = 0; i < count; ++i) FR_CK(c, fr, ensure_template_storage(c, c->frames[slots[i]], s));
  // the point budgets of the stage: what each slot's levels run with (bpvo_hip_get_selection_info), and which levels have one in any slot
  bool budget_at[kMaxLevels] = {};
  for(int i = 0; i < count; ++i) {
    FrameSlot& f = c->frames[slots[i]];
    f.min_saliency_used = (f.seq_params ? f.seq_params : &c->params)->minSaliency;
    for(int l = 0; l < c->L; ++l) {
      f.budget_used[l] = l >= c->params.maxTestLevel ? slot_budget(c, f, l) : 0;
      if(f.budget_used[l] > 0) budget_at[l] = true;
      // the saliency map of a census-only level is not stored: whoever reads it has it formed first (ensure_saliency)
      // (... but it is stored for a level with a point budget: the budget's threshold is read from the map)
      f.sal_state[l] = (f.lazy[l] == 2 && slot_budget(c, f, l) <= 0) ? FrameSlot::SAL_ON_DEMAND : FrameSlot::SAL_STORED;
    }
  }
  const FrameJob* tab = nullptr;
  int rc = upload_frame_jobs(c, slots, count, fr, 1, &tab);
  if(rc) return rc;
  const int NF = c->n_frames;
  int* const h_ints = c->h_ints + (size_t) fr.tab * kMaxLevels;
  int* const d_ints = c->d_ints + (size_t) fr.tab * kMaxLevels;
  const bpvo_hip_params& p = c->params;
  const int border = std::max(p.nonMaxSuppRadius, 3);   // template_data.cc:51
  const int tested = c->L - p.maxTestLevel;
  bool tiled = true;
  for(int l = p.maxTestLevel; l < c->L; ++l) tiled = tiled && geom[l].nms_radius <= 1;
  hipEvent_t counts_ev = fr.ln ? fr.ln->round_ev[0] : nullptr;      // (the lane's round events are idle outside its estimation)
  // The normalisation — sequential sums in the reference's order, a latency chain of one workgroup per (frame, level): 0.2 ms whatever the
  // batch — is read by the Gauss-Newton kernels only (the Jacobian rows are rebuilt there; template_build stores pixels and gradients).
  // A stage that runs alone on the context's stream (single frames, batches on one lane) puts it on a stream of its own — forked right
  // behind the selection, next to the read-back of the point counts, the host's round trip for them and template_build — and joins
  // the two before it returns; lanes of a fanned-out batch keep it in line.
  const bool side = c->nrm_side_stream && !fr.own_thread && fr.ln == &c->lanes[0] && counts_ev;
  if(side && !c->side_stream) {
    FR_CK(c, fr, c->side_stream.create());
    FR_CK(c, fr, c->side_stream2.create());
    for(auto& e : c->side_ev) FR_CK(c, fr, e.create(hipEventDisableTiming));
  }
  // ... and when the estimation follows on this stream within the same call (fr.defer_finest_nrm: a batch on one lane), only the COARSEST
  // level's sums are joined here: the others — the longest is the first level without non-maximum suppression, 100 k points of a
  // 1241x376 frame, 0.17 ms — are needed when the Gauss-Newton iterations leave the coarsest level: ctx->nrm_pending, waited for by the
  // estimation just before its second level (estimate.hip).  Which launches, streams and events that makes: normalization_plan (frame_plan.h)
  const int with_nrm = c->dspace ? 0 : p.withNormalization;      // DisparitySpaceWarp::setNormalization is a no-op (bpvo/disparity_space_warp.h:87-90)
  const bool defer = fr.defer_finest_nrm && c->nrm_defer && !c->nrm_pending && !c->nrm_pending_finest;
  const NrmPlan nrm = normalization_plan(c->L, p.maxTestLevel, side, defer, templates_may_be_dense(c));
  // (on a side stream it is timed like the in-line form, with events there: they are resolved once this stream — which the side stream joins — is synchronised)
  auto run_normalization = [&]() -> int {
    if(side) FR_CK(c, fr, hipEventRecord(c->side_ev[0], s));
    for(int k = 0; k < nrm.n; ++k) {
      const NrmPart& q = nrm.part[k];
      hipStream_t on = q.stream == NRM_INLINE ? s : (q.stream == NRM_SIDE ? c->side_stream : c->side_stream2);
      if(on != s && (k == 0 || q.stream != nrm.part[k - 1].stream)) FR_CK(c, fr, hipStreamWaitEvent(on, c->side_ev[0], 0));
      { ScopedTimer t(c, KC_NORMALIZATION, 0.0, fr.ln, true, on == s ? nullptr : on); launch_normalization(on, tab, NF, count, q.first_level, q.end_level, with_nrm, c->nrm_dpp_asm); }
      if(q.event >= 0) FR_CK(c, fr, hipEventRecord(c->side_ev[q.event], on));
    }
    if(nrm.pending_finest_event >= 0) c->nrm_pending_finest = c->side_ev[nrm.pending_finest_event];
    if(nrm.pending_event >= 0) c->nrm_pending = c->side_ev[nrm.pending_event];
    return BPVO_OK;
  };
  // the selection: the levels in one launch of each of its kernels, or level by level.  A span with a point budget: the budget's kernel between
  // the candidates and their scan (units: the pixels it may visit)
  for(const LevelSpan& sp : level_spans(c->L, p.maxTestLevel, merge_selection_levels(count, c->merge_levels_max_frames, tested, tiled))) {
    const FrameLaunch f = frame_launch(c, tab, geom, sp, count);
    const int radius = geom[sp.first].nms_radius;      // (several levels: every one of them tiled)
    double px = 0, budget_px = 0;
    for(int l = sp.first; l < sp.first + sp.count; ++l) {
      px += (double) geom[l].npix * count;
      if(budget_at[l]) budget_px += (double) geom[l].npix * count;
    }
    const bool budget = budget_px > 0;
    {
      ScopedTimer t(c, KC_SALIENCY_SELECT, px, fr.ln);
      launch_saliency_select(s, f, c->C, radius, border, c->gauss_k, budget ? SELECT_CANDIDATES : SELECT_ALL);
    }
    if(!budget) continue;
    {
      ScopedTimer t(c, KC_POINT_BUDGET, budget_px, fr.ln);
      launch_point_budget(s, f, radius);
    }
    ScopedTimer t(c, KC_SALIENCY_SELECT, 0.0, fr.ln);
    launch_saliency_select(s, f, c->C, radius, border, c->gauss_k, SELECT_COMPACT);
  }
  if(!nrm.behind_readback)
    if(int rcn = run_normalization()) return rcn;
  // one read-back of the point counts: the host needs them to size the template-build and GN grids.  Queued AHEAD of an in-line normalisation
  // and waited for through an event of its own: the host's round trip (~30 us) then runs under the normalisation's sequential sums
  // instead of behind them.
  launch_gather_counts(s, tab, NF, count, p.maxTestLevel, c->L, d_ints);
  FR_CK(c, fr, hipMemcpyAsync(h_ints, d_ints, sizeof(int) * kMaxLevels * (size_t) count, hipMemcpyDeviceToHost, s));
  if(counts_ev) FR_CK(c, fr, hipEventRecord(counts_ev, s));
  if(fr.selected_ev) FR_CK(c, fr, hipEventRecord(fr.selected_ev, s));
  if(fr.on_selected) fr.on_selected();
  if(nrm.behind_readback)
    if(int rcn = run_normalization()) return rcn;
  if(counts_ev) FR_CK(c, fr, hipEventSynchronize(counts_ev));
  else FR_CK(c, fr, hipStreamSynchronize(s));
  int max_n[kMaxLevels] = {};
  double pts = 0;
  for(int i = 0; i < count; ++i) {
    FrameSlot& f = c->frames[slots[i]];
    for(int l = 0; l < c->L; ++l) {
      f.n_host[l] = (l >= p.maxTestLevel) ? h_ints[(size_t) i * kMaxLevels + l] : 0;
      max_n[l] = std::max(max_n[l], f.n_host[l]);
      pts += f.n_host[l];
    }
  }
  if(c->profiling) {
    std::lock_guard<std::mutex> lk(c->units_mu);
    c->kc_units[KC_TEMPLATE] += pts;
    c->kc_units[KC_NORMALIZATION] += pts;
  }
  for(const LevelSpan& sp : level_spans(c->L, p.maxTestLevel, merge_template_levels(count, c->merge_levels_max_frames, tested))) {
    ScopedTimer t(c, KC_TEMPLATE, 0.0, fr.ln);
    const int most = *std::max_element(max_n + sp.first, max_n + sp.first + sp.count);
    launch_template_build(s, frame_launch(c, tab, geom, sp, count), c->C, most, p.gradientEstimation == BPVO_GRAD_CD5, c->gauss_k);
  }
  if(nrm.join_event >= 0) FR_CK(c, fr, hipStreamWaitEvent(s, c->side_ev[nrm.join_event], 0));      // the normalisation joins here: whatever follows on this stream sees it
  if(!fr.own_thread && !fr.no_final_sync) {      // (a lane thread goes straight on to its estimation on the same stream)
    FR_CK(c, fr, hipStreamSynchronize(s));
    FR_CK(c, fr, hipGetLastError());
    resolve_events(c);
  }
  for(int i = 0; i < count; ++i) c->frames[slots[i]].has_template = true;
  return BPVO_OK;
}
int frames_set_template(bpvo_hip_ctx* c, int first, int stride, int count)
{
  if(count <= 0) return BPVO_OK;
  if(first < 0 || stride < 1 || first + (count - 1) * stride >= c->n_frames) return fail(c, BPVO_ERR_INVALID_ARG, "bad frame slot range");
  for(int i = 0; i < count; ++i) {
    if(!c->frames[first + i * stride].has_data) return fail(c, BPVO_ERR_NO_DATA, "no data in frame");   // vo_frame.cc:63
    if(!c->frames[first + i * stride].has_disp) return fail(c, BPVO_ERR_NO_DATA, "no disparity in frame (the current frame of a pair batch)");
  }
  return frames_set_template_slots(c, strided_slots(first, stride, count).data(), count, ctx_run(c));
}

// The full records of a slot's lazy levels, from the image the slot still holds: the descriptor kernel again, for this frame alone,
// with the flag cleared (accessors; a template frame of a batch used as the current frame of a later estimate).
int ensure_dense_descriptor(bpvo_hip_ctx* c, int slot)
{
  FrameSlot& f = c->frames[slot];
  bool any = false;
  for(int l = 0; l < c->L; ++l) any = any || f.lazy[l];
  if(!any) return BPVO_OK;
  // The job table is built from the flags, so they are cleared for it and put back if anything fails: the slot counts as dense
  // only once the kernels that fill its records have run.
  uint8_t was[kMaxLevels];
  for(int l = 0; l < c->L; ++l) { was[l] = f.lazy[l]; f.lazy[l] = 0; }
  auto restore = [&]() { for(int l = 0; l < c->L; ++l) f.lazy[l] = was[l]; };
  const FrameRun fr = ctx_run(c);
  const FrameJob* tab = nullptr;
  const int rc = upload_frame_jobs(c, &slot, 1, fr, 0, &tab);
  if(rc) { restore(); return rc; }
  for(const LevelSpan& sp : level_spans(c->L, c->params.maxTestLevel, false))      // (lazy levels: DF_BITPLANES_FUSED only, frames_set_data_slots)
    launch_bitplanes(c->stream, frame_launch(c, tab, c->geom, sp, 1), c->params.sigmaBitPlanes, c->gauss_k, 1);
  if(hipGetLastError() != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) {
    restore();
    return fail(c, BPVO_ERR_DEVICE, "ensure_dense_descriptor: descriptor kernels failed");
  }
  return BPVO_OK;
}


// The saliency map of a level whose selection did not store it (FrameSlot::sal_state; template frames of a pair batch): the slot's dense
// records first, then the saliency kernel of the untiled selection — the closed form the tiles evaluate, value for value.
int ensure_saliency(bpvo_hip_ctx* c, int slot, int level)
{
  FrameSlot& f = c->frames[slot];
  if(f.sal_state[level] == FrameSlot::SAL_STORED) return BPVO_OK;
  if(f.sal_state[level] == FrameSlot::SAL_GONE)
    return fail(c, BPVO_ERR_NO_DATA, "the saliency map of a pair batch's template frame is formed on demand from the frame's data, which has been replaced");
  if(int rc = ensure_dense_descriptor(c, slot)) return rc;
  f.sal_state[level] = FrameSlot::SAL_STORED;      // (the job table is built from the state: the job carries the map's address)
  const FrameRun fr = ctx_run(c);
  const FrameJob* tab = nullptr;
  int rc = upload_frame_jobs(c, &slot, 1, fr, 1, &tab);
  if(rc == BPVO_OK) {
    launch_saliency(c->stream, frame_launch(c, tab, &slot_geom(c, f, 0), LevelSpan{level, 1}, 1), c->C);
    if(hipGetLastError() != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) rc = fail(c, BPVO_ERR_DEVICE, "ensure_saliency: saliency kernel failed");
  }
  if(rc) f.sal_state[level] = FrameSlot::SAL_ON_DEMAND;
  return rc;
}

int check_point_budget(bpvo_hip_ctx* c, const int* max_points, int n_levels)
{
  if(n_levels < 0 || n_levels > c->L) return fail(c, BPVO_ERR_INVALID_ARG, "point budget: more levels than the context has");
  if(n_levels > 0 && !max_points) return fail(c, BPVO_ERR_INVALID_ARG, "point budget: nullptr");
  for(int l = 0; l < n_levels; ++l) {
    if(max_points[l] < 0) return fail(c, BPVO_ERR_INVALID_ARG, "point budget: negative");
    if(max_points[l] > 0 && max_points[l] < 16) return fail(c, BPVO_ERR_INVALID_ARG, "point budget: 1 .. 15 points would always give an empty template (templates are cut to a multiple of 16)");
  }
  return BPVO_OK;
}

}  // namespace bpvo_hip_host

extern "C" {

// ---- normalised intensity (an extension: no reference member) ----------------------------------------------------------
int bpvo_hip_set_intensity_normalization(bpvo_hip_ctx* c, int radius)
{
  CHECK_CTX(c);
  if(descriptor_form(c->params, c->C) != DF_INTENSITY)
    return fail(c, BPVO_ERR_UNSUPPORTED, "intensity normalization: a mode of the Intensity descriptor, this context has another");
  if(radius < kInormOff || radius > kInormMaxRadius)
    return fail(c, BPVO_ERR_INVALID_ARG, "intensity normalization: radius -1 (off), 0 (whole image) or 1 .. 15 (local)");
  // the setting fixes what the stored planes mean: not while any holds data (frame slots, and through them every sequence and rig member)
  for(const FrameSlot& f : c->frames)
    if(f.has_data || f.has_template)
      return fail(c, BPVO_ERR_INVALID_ARG, "intensity normalization: a frame slot holds data; set it before the first frame or once every slot is cleared");
  (void) hipSetDevice(c->device);
  if(radius == 0 && !c->d_inorm) {
    // bins and tickets are zero between stages: once here, by the kernels from then on
    const size_t n = (size_t) c->n_frames * c->L;
    HIP_CK(c, c->d_inorm.alloc(n));
    HIP_CK(c, hipMemsetAsync(c->d_inorm, 0, n * sizeof(InormScratch), c->stream));
    HIP_CK(c, hipStreamSynchronize(c->stream));
  } else if(radius != 0 && c->d_inorm) {
    HIP_CK(c, hipStreamSynchronize(c->stream));
    c->d_inorm.reset();
  }
  c->inorm_radius = radius;
  return BPVO_OK;
}
int bpvo_hip_get_intensity_normalization(const bpvo_hip_ctx* c, int* radius)
{
  if(!c || !radius) return BPVO_ERR_INVALID_ARG;
  *radius = c->inorm_radius;
  return BPVO_OK;
}

// ---- point budget (an extension: no reference member) -----------------------------------------------------------------
int bpvo_hip_set_point_budget(bpvo_hip_ctx* c, const int* max_points, int n_levels)
{
  CHECK_CTX(c);
  if(int rc = check_point_budget(c, max_points, n_levels)) return rc;
  for(int l = 0; l < kMaxLevels; ++l) c->point_budget[l] = l < n_levels ? max_points[l] : 0;
  return BPVO_OK;
}
int bpvo_hip_get_point_budget(const bpvo_hip_ctx* c, int* max_points)
{
  if(!c || !max_points) return BPVO_ERR_INVALID_ARG;
  for(int l = 0; l < kMaxLevels; ++l) max_points[l] = c->point_budget[l];
  return BPVO_OK;
}
int bpvo_hip_get_selection_info(bpvo_hip_ctx* c, int slot, int level, int* n_candidates, float* threshold, int* n_ties_kept)
{
  CHECK_CTX(c); CHECK_SLOT(c, slot); CHECK_LEVEL(c, level);
  FrameSlot& f = c->frames[slot];
  if(!f.has_template) return fail(c, BPVO_ERR_NO_TEMPLATE, "no template");
  (void) hipSetDevice(c->device);
  int info[4] = {0, 0, 0, 0};
  float thr = f.min_saliency_used;
  if(f.budget_used[level] > 0) {
    // the record the budget's kernel left: {candidates, bits of the threshold, ties kept, 1 if the budget bound}
    HIP_CK(c, hipMemcpyAsync(info, f.sel_info + 4 * level, sizeof(info), hipMemcpyDeviceToHost, c->stream));
    HIP_CK(c, hipStreamSynchronize(c->stream));
    if(info[3]) std::memcpy(&thr, &info[1], sizeof(float));
    else info[2] = 0;
  } else {
    // no budget ran: the candidates are still all there, as bits (tiled selection) or flag bytes
    const LevelGeom& g = slot_geom(c, f, level);
    if(g.nms_radius <= 1) {
      std::vector<unsigned long long> w((size_t) g.rows * ((g.cols + 63) / 64));
      HIP_CK(c, hipMemcpyAsync(w.data(), f.flag[level], w.size() * 8, hipMemcpyDeviceToHost, c->stream));
      HIP_CK(c, hipStreamSynchronize(c->stream));
      for(unsigned long long v : w) info[0] += __builtin_popcountll(v);
    } else {
      std::vector<uint8_t> fl(g.npix);
      HIP_CK(c, hipMemcpyAsync(fl.data(), f.flag[level], fl.size(), hipMemcpyDeviceToHost, c->stream));
      HIP_CK(c, hipStreamSynchronize(c->stream));
      for(uint8_t v : fl) info[0] += v ? 1 : 0;
    }
  }
  if(n_candidates) *n_candidates = info[0];
  if(threshold) *threshold = thr;
  if(n_ties_kept) *n_ties_kept = info[2];
  return BPVO_OK;
}

int bpvo_hip_frames_set_data(bpvo_hip_ctx* c, int first_slot, int slot_stride, int count, const uint8_t* images,
                             const float* disparities, int on_device)
{
  CHECK_CTX(c);
  (void) hipSetDevice(c->device);
  int rc = frames_set_data(c, first_slot, slot_stride, count, images, disparities, on_device != 0);
  if(rc) return rc;
  HIP_CK(c, hipStreamSynchronize(c->stream));   // the caller may reuse its buffers on return (vo_frame.cc:50-51)
  resolve_events(c);
  return BPVO_OK;
}
int bpvo_hip_frame_set_data(bpvo_hip_ctx* c, int slot, const uint8_t* image, const float* disparity)
{
  CHECK_CTX(c); CHECK_SLOT(c, slot);
  return bpvo_hip_frames_set_data(c, slot, 1, 1, image, disparity, 0);
}
int bpvo_hip_frame_set_data_device(bpvo_hip_ctx* c, int slot, const uint8_t* d_image, const float* d_disparity)
{
  CHECK_CTX(c); CHECK_SLOT(c, slot);
  return bpvo_hip_frames_set_data(c, slot, 1, 1, d_image, d_disparity, 1);
}
int bpvo_hip_frame_set_template(bpvo_hip_ctx* c, int slot)
{
  CHECK_CTX(c); CHECK_SLOT(c, slot);
  (void) hipSetDevice(c->device);
  return frames_set_template(c, slot, 1, 1);
}
int bpvo_hip_frames_set_template(bpvo_hip_ctx* c, int first_slot, int slot_stride, int count)
{
  CHECK_CTX(c);
  (void) hipSetDevice(c->device);
  return frames_set_template(c, first_slot, slot_stride, count);
}
int bpvo_hip_frame_clear(bpvo_hip_ctx* c, int slot)
{
  CHECK_CTX(c); CHECK_SLOT(c, slot);
  c->frames[slot].has_data = false;
  c->frames[slot].has_template = false;
  return BPVO_OK;
}
int bpvo_hip_frame_state(const bpvo_hip_ctx* c, int slot, int* has_data, int* has_template)
{
  if(!c || slot < 0 || slot >= c->n_frames) return BPVO_ERR_INVALID_ARG;
  *has_data = c->frames[slot].has_data;
  *has_template = c->frames[slot].has_template;
  return BPVO_OK;
}

// ---- accessors ------------------------------------------------------------------------------------------------------
int bpvo_hip_get_image(bpvo_hip_ctx* c, int slot, int level, uint8_t* out)
{
  CHECK_CTX(c); CHECK_SLOT(c, slot);
  if(level < 0 || level >= c->L) return fail(c, BPVO_ERR_INVALID_ARG, "bad level");
  if(!c->frames[slot].has_data) return fail(c, BPVO_ERR_NO_DATA, "no data in frame");
  (void) hipSetDevice(c->device);
  HIP_CK(c, hipMemcpyAsync(out, c->frames[slot].img[level], c->geom[level].npix, hipMemcpyDeviceToHost, c->stream));
  HIP_CK(c, hipStreamSynchronize(c->stream));
  return BPVO_OK;
}
int bpvo_hip_get_descriptor_channel(bpvo_hip_ctx* c, int slot, int level, int channel, float* out)
{
  CHECK_CTX(c); CHECK_SLOT(c, slot); CHECK_LEVEL(c, level);
  if(channel < 0 || channel >= c->C) return fail(c, BPVO_ERR_INVALID_ARG, "bad channel");
  if(!c->frames[slot].has_data) return fail(c, BPVO_ERR_NO_DATA, "no data in frame");
  (void) hipSetDevice(c->device);
  if(int rc = ensure_dense_descriptor(c, slot)) return rc;      // (a template frame of a pair batch: its NMS levels kept no records)
  const size_t npix = c->geom[level].npix;
  // de-interleave one channel: 2-D copy with a source pitch of C floats
  HIP_CK(c, hipMemcpy2DAsync(out, sizeof(float), c->frames[slot].desc[level] + channel, sizeof(float) * c->C, sizeof(float), npix,
                             hipMemcpyDeviceToHost, c->stream));
  HIP_CK(c, hipStreamSynchronize(c->stream));
  return BPVO_OK;
}
int bpvo_hip_get_saliency(bpvo_hip_ctx* c, int slot, int level, float* out)
{
  CHECK_CTX(c); CHECK_SLOT(c, slot); CHECK_LEVEL(c, level);
  if(!c->frames[slot].has_template) return fail(c, BPVO_ERR_NO_TEMPLATE, "no template");
  (void) hipSetDevice(c->device);
  if(int rc = ensure_saliency(c, slot, level)) return rc;      // (a template frame of a pair batch: its selection stored no map)
  HIP_CK(c, hipMemcpyAsync(out, c->frames[slot].sal[level], c->geom[level].npix * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  HIP_CK(c, hipStreamSynchronize(c->stream));
  return BPVO_OK;
}
#define TMPL(c, slot, level)                                                                    \
  CHECK_CTX(c); CHECK_SLOT(c, slot); CHECK_LEVEL(c, level);                                     \
  if(!(c)->frames[slot].has_template) return fail(c, BPVO_ERR_NO_TEMPLATE, "no template");      \
  (void) hipSetDevice((c)->device);                                                             \
  FrameSlot& f = (c)->frames[slot];                                                             \
  const int n = f.n_host[level]

int bpvo_hip_num_points(bpvo_hip_ctx* c, int slot, int level, int* n_out) { TMPL(c, slot, level); *n_out = n; return BPVO_OK; }
int bpvo_hip_get_points(bpvo_hip_ctx* c, int slot, int level, float* xyzw)
{
  TMPL(c, slot, level);
  if(n && c->points_from_compact) {      // debug: the points as the Gauss-Newton kernels rebuild them from the 8-byte records (load_point)
    DeviceBuf<float4> d_out;
    HIP_CK(c, d_out.alloc((size_t) n));
    launch_rebuild_points(c->stream, make_pair_job(c, 0, slot, slot, level), d_out);
    HIP_CK(c, hipMemcpyAsync(xyzw, d_out, sizeof(float4) * n, hipMemcpyDeviceToHost, c->stream));
    HIP_CK(c, hipStreamSynchronize(c->stream));
    return BPVO_OK;
  }
  if(n) HIP_CK(c, hipMemcpyAsync(xyzw, f.pts[level], sizeof(float4) * n, hipMemcpyDeviceToHost, c->stream));
  HIP_CK(c, hipStreamSynchronize(c->stream));
  return BPVO_OK;
}
int bpvo_hip_get_point_indices(bpvo_hip_ctx* c, int slot, int level, int* inds)
{
  TMPL(c, slot, level);
  if(n) HIP_CK(c, hipMemcpyAsync(inds, f.inds[level], sizeof(int) * n, hipMemcpyDeviceToHost, c->stream));
  HIP_CK(c, hipStreamSynchronize(c->stream));
  return BPVO_OK;
}
int bpvo_hip_get_pixels(bpvo_hip_ctx* c, int slot, int level, float* pixels)
{
  TMPL(c, slot, level);
  const int C = c->C;
  std::vector<float> t(tiled_floats(n, C));
  if(n) HIP_CK(c, hipMemcpyAsync(t.data(), f.pix[level], t.size() * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  HIP_CK(c, hipStreamSynchronize(c->stream));
  detile_to_channel_major(t.data(), n, C, 1, C == 8 ? 4 : C, pixels);
  return BPVO_OK;
}
int bpvo_hip_get_jacobians(bpvo_hip_ctx* c, int slot, int level, float* J)
{
  TMPL(c, slot, level);
  if(n == 0) return BPVO_OK;
  // the rows are not stored: evaluate them on the device from (point, Ix, Iy) exactly like irls_reduce does
  const size_t floats = 6 * (size_t) n * c->C;
  DeviceBuf<float> d_out;
  HIP_CK(c, d_out.alloc(floats));
  HIP_CK(c, hipStreamSynchronize(c->stream));
  c->h_fjobs[0] = make_frame_job(c, f, level);
  HIP_CK(c, hipMemcpyAsync(c->d_fjobs, c->h_fjobs, sizeof(FrameJob), hipMemcpyHostToDevice, c->stream));
  launch_export_jacobians(c->stream, c->d_fjobs, c->C, n, d_out);
  HIP_CK(c, hipMemcpyAsync(J, d_out, sizeof(float) * floats, hipMemcpyDeviceToHost, c->stream));
  HIP_CK(c, hipStreamSynchronize(c->stream));
  return BPVO_OK;
}
int bpvo_hip_get_normalization(bpvo_hip_ctx* c, int slot, int level, float T[16], float T_inv[16])
{
  TMPL(c, slot, level);
  M44 t = m44_identity(), ti = m44_identity();
  // no normalisation was set (withNormalization off, an empty level, or DisparitySpaceWarp, whose setNormalization is a
  // no-op): the warp keeps the Identity it was constructed with (bpvo/rigid_body_warp.cc:27-28), not [1, -1 * 0]
  if(!c->params.withNormalization || c->dspace || n == 0) {
    std::memcpy(T, t.m, 64);
    std::memcpy(T_inv, ti.m, 64);
    return BPVO_OK;
  }
  float nrm[4];
  HIP_CK(c, hipMemcpyAsync(nrm, f.nrm + 4 * level, sizeof(nrm), hipMemcpyDeviceToHost, c->stream));
  HIP_CK(c, hipStreamSynchronize(c->stream));
  t.m[0] = t.m[5] = t.m[10] = nrm[0];
  t.m[3] = -nrm[0] * nrm[1]; t.m[7] = -nrm[0] * nrm[2]; t.m[11] = -nrm[0] * nrm[3];
  ti.m[0] = ti.m[5] = ti.m[10] = 1.0f / nrm[0];
  ti.m[3] = nrm[1]; ti.m[7] = nrm[2]; ti.m[11] = nrm[3];
  std::memcpy(T, t.m, 64);
  std::memcpy(T_inv, ti.m, 64);
  return BPVO_OK;
}

}  // extern "C"
