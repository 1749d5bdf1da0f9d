// libbpvo_hip, host side: rectification on the device (include/bpvo_hip/c_api.h; the rule: rectify_math.h; the kernel: kernels_rectify.hip).
// A set call builds the map of one camera side on the host — 467 k entries for a KITTI frame, once — and uploads it; a call rectifies all its
// frames, both sides, in one launch from a table of frames (rectify_queue), which stereo_front (stereo.hip) puts in front of the stereo
// front-end.  No existing call launches, allocates or reads anything of this file.
#include "host_ctx.h"
#include "rectify_math.h"

#include "../../include/bpvo_hip/c_api.h"

namespace bpvo_hip_host {

static_assert(sizeof(RectEntry) == sizeof(int2), "a map entry is an int2 on the device");

static int rect_fail(bpvo_hip_ctx* c, int code, int seq, const std::string& what)
{
  c->err = seq < 0 ? what : "sequence " + std::to_string(seq) + ": " + what;
  return code;
}
static RectMap* rect_slot(bpvo_hip_ctx* c, int seq, int side)
{
  if(seq < 0) return &c->rect.own[side];
  return (size_t) (2 * seq + side) < c->rect.seq.size() ? &c->rect.seq[(size_t) (2 * seq + side)] : nullptr;
}
const RectMap* rect_map_of(const bpvo_hip_ctx* c, int seq, int side)
{
  const RectMap* m = rect_slot(const_cast<bpvo_hip_ctx*>(c), seq, side);
  return m && m->d_map ? m : nullptr;
}
// the camera a side's map is made for: the sequence's (its first frame slot's geometry), or the context's own
static const LevelGeom& rect_camera(const bpvo_hip_ctx* c, int seq) { return seq < 0 ? c->geom[0] : slot_geom(c, c->frames[3 * seq], 0); }

int rect_clear(bpvo_hip_ctx* c, int seq)
{
  RectMap* m[2] = {rect_slot(c, seq, 0), rect_slot(c, seq, 1)};
  if(!(m[0] && m[0]->d_map) && !(m[1] && m[1]->d_map)) return BPVO_OK;
  (void) hipSetDevice(c->device);
  HIP_CK(c, hipStreamSynchronize(c->stream));      // (a launch may still read the tables)
  for(RectMap* q : m)
    if(q) *q = RectMap();
  return BPVO_OK;
}

// the checks every set call makes of its target and of the raw size; the camera's skew
static int rect_check_target(bpvo_hip_ctx* c, int seq, int side, int raw_rows, int raw_cols)
{
  if(seq >= seq_capacity(c)) return rect_fail(c, BPVO_ERR_INVALID_ARG, seq, "no such sequence");
  if(side != 0 && side != 1) return rect_fail(c, BPVO_ERR_INVALID_ARG, seq, "rectification: side must be 0 (left) or 1 (right)");
  if(raw_rows < 2 || raw_cols < 2) return rect_fail(c, BPVO_ERR_INVALID_ARG, seq, "rectification: a raw image has at least 2 rows and 2 cols");
  if(raw_rows > kRectMaxRaw || raw_cols > kRectMaxRaw) return rect_fail(c, BPVO_ERR_UNSUPPORTED, seq, "rectification: a raw image has at most 32767 rows and cols");
  if(rect_camera(c, seq).K[1] != 0.0f) return rect_fail(c, BPVO_ERR_UNSUPPORTED, seq, "rectification: a camera with skew (K[1] != 0) is not served");
  return BPVO_OK;
}
// the map of (seq, side) becomes `entries` ([rows][cols] of the camera): a table the device may still read is waited for first
static int rect_install(bpvo_hip_ctx* c, int seq, int side, int raw_rows, int raw_cols, const std::vector<RectEntry>& entries)
{
  const LevelGeom& g = rect_camera(c, seq);
  uint64_t outside = 0;
  for(const RectEntry& e : entries) outside += rectify_outside(raw_rows, raw_cols, e.xq, e.yq) ? 1u : 0u;
  (void) hipSetDevice(c->device);
  if(seq >= 0 && c->rect.seq.empty()) c->rect.seq.resize((size_t) 2 * (size_t) seq_capacity(c));
  RectMap* m = rect_slot(c, seq, side);
  if(m->d_map) {
    HIP_CK(c, hipStreamSynchronize(c->stream));
    *m = RectMap();
  }
  HIP_CK(c, m->d_map.alloc(entries.size()));
  const hipError_t e = hipMemcpy(m->d_map, entries.data(), entries.size() * sizeof(RectEntry), hipMemcpyHostToDevice);
  if(e != hipSuccess) {
    *m = RectMap();
    c->err = std::string("rectification: map upload: ") + hipGetErrorString(e);
    return BPVO_ERR_DEVICE;
  }
  m->rows = g.rows; m->cols = g.cols; m->raw_rows = raw_rows; m->raw_cols = raw_cols; m->outside = outside;
  return BPVO_OK;
}
static int rect_set_lens(bpvo_hip_ctx* c, int seq, int side, const bpvo_hip_lens* lens)
{
  if(!lens) return rect_fail(c, BPVO_ERR_INVALID_ARG, seq, "nullptr lens");
  RectLens q;
  q.fx = lens->fx; q.fy = lens->fy; q.cx = lens->cx; q.cy = lens->cy;
  for(int k = 0; k < 8; ++k) q.dist[k] = lens->dist[k];
  for(int k = 0; k < 9; ++k) q.R[k] = lens->R[k];
  bool finite = std::isfinite(q.fx) && std::isfinite(q.fy) && std::isfinite(q.cx) && std::isfinite(q.cy);
  for(int k = 0; k < 8; ++k) finite = finite && std::isfinite(q.dist[k]);
  for(int k = 0; k < 9; ++k) finite = finite && std::isfinite(q.R[k]);
  if(!finite) return rect_fail(c, BPVO_ERR_INVALID_ARG, seq, "rectification: the lens values must be finite");
  if(!(q.fx > 0.0) || !(q.fy > 0.0)) return rect_fail(c, BPVO_ERR_INVALID_ARG, seq, "rectification: fx and fy must be positive");
  if(!(rect_orthonormal_error(q.R) <= 1e-6)) return rect_fail(c, BPVO_ERR_INVALID_ARG, seq, "rectification: R must be orthonormal (max |R^T R - I| <= 1e-6)");
  if(int rc = rect_check_target(c, seq, side, lens->raw_rows, lens->raw_cols)) return rc;
  const LevelGeom& g = rect_camera(c, seq);
  const double fxn = (double) g.K[0], fyn = (double) g.K[4], cxn = (double) g.K[2], cyn = (double) g.K[5];
  std::vector<RectEntry> entries((size_t) g.rows * (size_t) g.cols);
  for(int v = 0; v < g.rows; ++v)
    for(int u = 0; u < g.cols; ++u) entries[(size_t) v * g.cols + u] = rect_lens_entry(q, fxn, fyn, cxn, cyn, u, v);
  return rect_install(c, seq, side, lens->raw_rows, lens->raw_cols, entries);
}
static int rect_set_maps(bpvo_hip_ctx* c, int seq, int side, int raw_rows, int raw_cols, const float* mapx, const float* mapy)
{
  if(!mapx || !mapy) return rect_fail(c, BPVO_ERR_INVALID_ARG, seq, "nullptr map");
  if(int rc = rect_check_target(c, seq, side, raw_rows, raw_cols)) return rc;
  const LevelGeom& g = rect_camera(c, seq);
  std::vector<RectEntry> entries((size_t) g.rows * (size_t) g.cols);
  for(size_t i = 0; i < entries.size(); ++i) entries[i] = rect_quantise((double) mapx[i], (double) mapy[i]);
  return rect_install(c, seq, side, raw_rows, raw_cols, entries);
}
static int rect_info(bpvo_hip_ctx* c, int seq, int side, int* raw_rows, int* raw_cols, uint64_t* outside_pixels)
{
  if(seq >= seq_capacity(c)) return rect_fail(c, BPVO_ERR_INVALID_ARG, seq, "no such sequence");
  if(side != 0 && side != 1) return rect_fail(c, BPVO_ERR_INVALID_ARG, seq, "rectification: side must be 0 (left) or 1 (right)");
  const RectMap* m = rect_map_of(c, seq, side);
  if(!m) return rect_fail(c, BPVO_ERR_NO_DATA, seq, side ? "no rectification of the right side" : "no rectification of the left side");
  if(raw_rows) *raw_rows = m->raw_rows;
  if(raw_cols) *raw_cols = m->raw_cols;
  if(outside_pixels) *outside_pixels = m->outside;
  return BPVO_OK;
}

int rectify_queue(bpvo_hip_ctx* c, int n, const int* seq, int n_sides, const RectSide* sides, bool on_device)
{
  RectState& R = c->rect;
  const size_t rows_needed = (size_t) n * (size_t) n_sides;
  if(rows_needed > R.h_tab.size()) {      // (the pinned table comes last: its size says that both are there)
    HIP_CK(c, hipStreamSynchronize(c->stream));
    R.d_tab.reset(); R.h_tab.reset();
    const size_t cap = std::max(rows_needed, (size_t) 2 * (size_t) std::max(1, seq_capacity(c)));
    HIP_CK(c, R.d_tab.alloc(cap));
    HIP_CK(c, R.h_tab.alloc(cap));
  }
  if(!R.tab_ev) HIP_CK(c, R.tab_ev.create(hipEventDisableTiming));
  else HIP_CK(c, hipEventSynchronize(R.tab_ev));      // (the last call's copy has read the pinned rows)
  int max_rows = 0, max_cols = 0;
  uint64_t pixels = 0;
  for(int k = 0; k < n_sides; ++k) {
    size_t raw_bytes = 0;
    for(int i = 0; i < n; ++i) {
      const RectMap* m = rect_map_of(c, seq ? seq[i] : -1, sides[k].side);
      raw_bytes += (size_t) m->raw_rows * (size_t) m->raw_cols;
    }
    const uint8_t* src = sides[k].raw;
    if(!on_device) {
      if(raw_bytes > R.raw[k].size()) {
        HIP_CK(c, hipStreamSynchronize(c->stream));
        HIP_CK(c, R.raw[k].reserve(raw_bytes));
      }
      HIP_CK(c, hipMemcpyAsync(R.raw[k], sides[k].raw, raw_bytes, hipMemcpyHostToDevice, c->stream));
      src = R.raw[k];
    }
    size_t raw_at = 0, dst_at = 0;
    for(int i = 0; i < n; ++i) {
      const RectMap* m = rect_map_of(c, seq ? seq[i] : -1, sides[k].side);
      R.h_tab[(size_t) k * n + i] = RectifyFrame{m->rows, m->cols, m->raw_rows, m->raw_cols, m->d_map, src + raw_at, sides[k].dst + dst_at};
      raw_at += (size_t) m->raw_rows * (size_t) m->raw_cols;
      dst_at += (size_t) m->rows * (size_t) m->cols;
      max_rows = std::max(max_rows, m->rows); max_cols = std::max(max_cols, m->cols);
      pixels += (uint64_t) m->rows * (uint64_t) m->cols;
    }
  }
  HIP_CK(c, hipMemcpyAsync(R.d_tab, R.h_tab, rows_needed * sizeof(RectifyFrame), hipMemcpyHostToDevice, c->stream));
  HIP_CK(c, hipEventRecord(R.tab_ev, c->stream));
  R.timed = false;
  if(c->profiling) {      // (measurement: scripts/rectify_bench.py)
    if(!R.t0) HIP_CK(c, R.t0.create());
    if(!R.t1) HIP_CK(c, R.t1.create());
    HIP_CK(c, hipEventRecord(R.t0, c->stream));
  }
  launch_rectify_frames(c->stream, R.d_tab, (int) rows_needed, max_rows, max_cols);
  HIP_CK(c, hipGetLastError());
  if(c->profiling) {
    HIP_CK(c, hipEventRecord(R.t1, c->stream));
    R.timed = true;
  }
  R.launches += 1;
  R.pixels += pixels;
  return BPVO_OK;
}

}  // namespace bpvo_hip_host

extern "C" {

int bpvo_hip_seq_set_rectification(bpvo_hip_ctx* c, int seq, int side, const bpvo_hip_lens* lens)
{
  CHECK_CTX(c);
  if(seq < 0) return rect_fail(c, BPVO_ERR_INVALID_ARG, seq, "sequence " + std::to_string(seq) + ": no such sequence");
  return rect_set_lens(c, seq, side, lens);
}
int bpvo_hip_seq_set_rectification_maps(bpvo_hip_ctx* c, int seq, int side, int raw_rows, int raw_cols, const float* mapx, const float* mapy)
{
  CHECK_CTX(c);
  if(seq < 0) return rect_fail(c, BPVO_ERR_INVALID_ARG, seq, "sequence " + std::to_string(seq) + ": no such sequence");
  return rect_set_maps(c, seq, side, raw_rows, raw_cols, mapx, mapy);
}
int bpvo_hip_seq_clear_rectification(bpvo_hip_ctx* c, int seq)
{
  CHECK_CTX(c);
  if(seq < 0 || seq >= seq_capacity(c)) return rect_fail(c, BPVO_ERR_INVALID_ARG, -1, "sequence " + std::to_string(seq) + ": no such sequence");
  return rect_clear(c, seq);
}
int bpvo_hip_seq_rectification_info(bpvo_hip_ctx* c, int seq, int side, int* raw_rows, int* raw_cols, uint64_t* outside_pixels)
{
  CHECK_CTX(c);
  if(seq < 0) return rect_fail(c, BPVO_ERR_INVALID_ARG, seq, "sequence " + std::to_string(seq) + ": no such sequence");
  return rect_info(c, seq, side, raw_rows, raw_cols, outside_pixels);
}
int bpvo_hip_set_rectification(bpvo_hip_ctx* c, int side, const bpvo_hip_lens* lens)
{
  CHECK_CTX(c);
  return rect_set_lens(c, -1, side, lens);
}
int bpvo_hip_set_rectification_maps(bpvo_hip_ctx* c, int side, int raw_rows, int raw_cols, const float* mapx, const float* mapy)
{
  CHECK_CTX(c);
  return rect_set_maps(c, -1, side, raw_rows, raw_cols, mapx, mapy);
}
int bpvo_hip_clear_rectification(bpvo_hip_ctx* c)
{
  CHECK_CTX(c);
  return rect_clear(c, -1);
}
int bpvo_hip_rectification_info(bpvo_hip_ctx* c, int side, int* raw_rows, int* raw_cols, uint64_t* outside_pixels)
{
  CHECK_CTX(c);
  return rect_info(c, -1, side, raw_rows, raw_cols, outside_pixels);
}
int bpvo_hip_rectify_counts(bpvo_hip_ctx* c, uint64_t* launches, uint64_t* pixels)
{
  CHECK_CTX(c);
  if(launches) *launches = c->rect.launches;
  if(pixels) *pixels = c->rect.pixels;
  return BPVO_OK;
}
int bpvo_hip_rectify_frames(bpvo_hip_ctx* c, int n, const int* seq, int side, const uint8_t* raw, int on_device, uint8_t* out, int out_on_device)
{
  CHECK_CTX(c);
  if(n < 1 || n > 32767) return fail(c, BPVO_ERR_INVALID_ARG, "rectify_frames: n must be within 1 .. 32767");
  if(side != 0 && side != 1) return fail(c, BPVO_ERR_INVALID_ARG, "rectification: side must be 0 (left) or 1 (right)");
  if(!raw || !out) return fail(c, BPVO_ERR_INVALID_ARG, "nullptr image");
  size_t out_bytes = 0;
  for(int i = 0; i < n; ++i) {
    const int s = seq ? seq[i] : -1;
    if(seq && (s < 0 || s >= seq_capacity(c))) return rect_fail(c, BPVO_ERR_INVALID_ARG, -1, "sequence " + std::to_string(s) + ": no such sequence");
    const RectMap* m = rect_map_of(c, s, side);
    if(!m) return rect_fail(c, BPVO_ERR_NO_DATA, s, side ? "no rectification of the right side" : "no rectification of the left side");
    out_bytes += (size_t) m->rows * (size_t) m->cols;
  }
  (void) hipSetDevice(c->device);
  uint8_t* dst = out;
  if(!out_on_device) {
    if(out_bytes > c->rect.out.size()) {
      HIP_CK(c, hipStreamSynchronize(c->stream));
      HIP_CK(c, c->rect.out.reserve(out_bytes));
    }
    dst = c->rect.out;
  }
  const RectSide one{side, raw, dst};
  const int rc = rectify_queue(c, n, seq, 1, &one, on_device != 0);
  if(rc) { (void) hipStreamSynchronize(c->stream); return rc; }
  if(!out_on_device) HIP_CK(c, hipMemcpyAsync(out, dst, out_bytes, hipMemcpyDeviceToHost, c->stream));
  HIP_CK(c, hipStreamSynchronize(c->stream));
  return BPVO_OK;
}

}  // extern "C"
