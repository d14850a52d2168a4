// recon_kernel.hip -- hevcdl_recon_kernel: the unfiltered reconstruction of intra pictures from CTU records on gfx950, and its host entry points.
//
// The arithmetic and the walk over a CTU are csrc/recon_core.h, one source for this kernel and for hevcdl_reconstruct_frames_host (one "lane" on the CPU: what the
// kernel's index logic is checked with where there is no GPU).  Here: how the rows of a batch are dealt and how a row waits for the one above.
//   * A workgroup is ONE wave (64 lanes over the samples of a transform block); it rebuilds whole CTU rows.
//   * Rows are claimed in increasing (picture, row) order from one atomic ticket.  A CTU reads reconstructed samples of its left neighbour (its own wave) and of the three
//     CTUs above it, so CTU x of a row waits until the row above has finished min(x + 2, width) CTUs: a per-row finished count in HBM, written with a release store behind
//     the row's samples and read with agent-scope acquire loads, s_sleep between them.  The row waited for has a smaller ticket, so it was claimed by a wave that is
//     already running (or done): no launch can deadlock, whatever its residency.  The wait is bounded all the same (SPIN_LIMIT): past it the wave sets the error word and
//     goes on, the host returns HEVCDL_ERR_HIP -- a shared device is never left with a wave that spins for ever.
//   * 8- and 10-bit samples are the two instantiations of one template.
// The kernel is launched only on records that passed hevcdl_validate_records (the host-buffer entry points check; the device form takes the caller's word, and
// recon_core.h clamps and masks every index all the same).
#include <hip/hip_runtime.h>
#include <atomic>
#include <cstring>
#include <type_traits>
#include <vector>
#include "hevcdl.h"
#include "hevcdl_dev.h"
#include "recon_launch.h"
#include "hevcdl_parse.h"
#include "recon_core.h"

using namespace hevcdl_rc;

namespace {
enum { SPIN_LIMIT = 1 << 22, RC_MAX_GROUPS = 2048 };
struct RcLaunch {
  RcPic pic;                     // picture 0: recs, out; the kernel steps both per picture
  const int32_t *qps;            // [n_frames] in HBM, or null: pic.qp for every picture
  uint32_t *sync;                // [0] ticket, [1] error word, [2 + picture * ctus_y + row] finished CTUs of the row; zeroed before the launch
  size_t frame_bytes;
  int n_frames, ctus;
};

struct RcLaunchQp {              // RcLaunch with a QP map instead of per-picture QPs: pic.qp_map is picture 0's, stepped per picture like recs
  RcPicQp pic; uint32_t *sync; size_t frame_bytes; int n_frames, ctus;
};

struct RcLaunchSl {              // RcLaunchQp with the scaling factors: pic.factor is the stream's block, the same for every picture
  RcPicSl pic; uint32_t *sync; size_t frame_bytes; int n_frames, ctus;
};

// LAUNCH RcLaunchSl: the instantiation with scaling lists on top of the QP map (recon_core.h: RcPicSl); the factors are read from HBM where a block is dequantised.
// LAUNCH RcLaunch: the constant-QP form, as it ever was.  LAUNCH RcLaunchQp: the instantiation with a QP per CU and the PPS chroma offsets (recon_core.h: RcPicQp)
template <typename PEL, typename LAUNCH = RcLaunch>
__global__ __launch_bounds__(64) void hevcdl_recon_kernel(LAUNCH L)
{
  __shared__ RcWork w;
  __shared__ int ticket;
  const int lane = (int)threadIdx.x, rows = L.pic.ctus_y, total = L.n_frames * rows;
  for (int it = 0; it <= total; it++) {
    if (lane == 0) ticket = (int)atomicAdd(L.sync, 1u);
    __syncthreads();
    const int t = ticket;
    __syncthreads();
    if (t >= total) return;
    const int f = t / rows, cy = t - f * rows;
    auto p = L.pic;
    p.recs = L.pic.recs + (size_t)f * L.ctus; p.out = (unsigned char *)L.pic.out + (size_t)f * L.frame_bytes;
    if constexpr (std::is_same<LAUNCH, RcLaunch>::value) { if (L.qps) p.qp = L.qps[f]; }
    else p.qp_map = L.pic.qp_map + (size_t)f * L.ctus * 256;
    uint32_t *fin = L.sync + 2 + (size_t)f * rows;
    for (int cx = 0; cx < p.ctus_x; cx++) {
      if (cy > 0) {
        const uint32_t need = (uint32_t)(cx + 2 < p.ctus_x ? cx + 2 : p.ctus_x);
        if (lane == 0) {
          int spins = 0;
          if (__hip_atomic_load(L.sync + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) spins = SPIN_LIMIT;      // a wait has run out already: nobody waits again
          while (__hip_atomic_load(fin + cy - 1, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) < need && spins < SPIN_LIMIT) { __builtin_amdgcn_s_sleep(16); spins++; }
          if (spins >= SPIN_LIMIT) __hip_atomic_store(L.sync + 1, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        __syncthreads();
      }
      rc_ctu<PEL>(p, w, lane, 64, cx, cy);
      __threadfence();
      __syncthreads();
      if (lane == 0) __hip_atomic_store(fin + cy, (uint32_t)(cx + 1), __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

std::atomic<unsigned long long> g_launches{0};

#define RC_REFUSE(st, ...) do { hevcdl_parse::set_error(__VA_ARGS__); return st; } while (0)

// cfg and layout -> the picture's geometry and the unit (slice, tile) of every CTU
hevcdl_status rc_setup(const hevcdl_stream_config *cfg, const hevcdl_slice_layout *sl, RcPic &p, std::vector<uint32_t> &unit)
{
  if (!cfg || cfg->struct_size != sizeof *cfg) RC_REFUSE(HEVCDL_ERR_INVALID_ARG, "null configuration, or one of another size");
  if (cfg->width < 8 || cfg->height < 8 || (cfg->width & 7) || (cfg->height & 7) || cfg->width > 16384 || cfg->height > 16384) RC_REFUSE(HEVCDL_ERR_INVALID_ARG, "picture size %d x %d", cfg->width, cfg->height);
  if (cfg->bit_depth != 8 && cfg->bit_depth != 10) RC_REFUSE(HEVCDL_ERR_UNSUPPORTED, "bit depth %d: 8 and 10 are reconstructed", cfg->bit_depth);
  if (cfg->qp < 0 || cfg->qp > 51) RC_REFUSE(HEVCDL_ERR_INVALID_ARG, "QP %d", cfg->qp);
  p.W = cfg->width; p.H = cfg->height; p.ctus_x = (p.W + 63) >> 6; p.ctus_y = (p.H + 63) >> 6; p.bit_depth = cfg->bit_depth; p.qp = cfg->qp;
  p.strong = (cfg->tools & HEVCDL_TOOL_STRONG_INTRA) != 0;
  int col_bd[21], row_bd[23];
  const int tc = cfg->tile_columns, tr = cfg->tile_rows;
  if (tc < 1 || tr < 1 || tc > 20 || tr > 22 || hevcdl_tile_bounds(p.ctus_x, tc, cfg->tile_uniform_spacing != 0, cfg->tile_column_width, 1, col_bd) ||
      hevcdl_tile_bounds(p.ctus_y, tr, cfg->tile_uniform_spacing != 0, cfg->tile_row_height, 1, row_bd)) RC_REFUSE(HEVCDL_ERR_INVALID_ARG, "the tile grid does not fit the picture");
  const int mode = sl ? sl->mode : 0;
  if (mode != 0 && mode != 1 && mode != 3) RC_REFUSE(HEVCDL_ERR_UNSUPPORTED, "SliceMode %d", mode);
  if (mode == 1 && (sl->argument < 1 || sl->argument % p.ctus_x != 0 || tc * tr > 1)) RC_REFUSE(HEVCDL_ERR_UNSUPPORTED, "SliceMode 1 needs whole CTU rows and no tiles");
  if (mode == 3 && sl->argument < 1) RC_REFUSE(HEVCDL_ERR_INVALID_ARG, "SliceMode 3 needs at least one tile a slice");
  unit.assign((size_t)p.ctus_x * p.ctus_y, 0);
  for (int y = 0; y < p.ctus_y; y++) for (int x = 0; x < p.ctus_x; x++) {
    int tx = 0, ty = 0;
    while (tx + 1 < tc && x >= col_bd[tx + 1]) tx++;
    while (ty + 1 < tr && y >= row_bd[ty + 1]) ty++;
    const int tile = ty * tc + tx, slice = mode == 1 ? y / (sl->argument / p.ctus_x) : (mode == 3 ? tile / sl->argument : 0);
    unit[(size_t)y * p.ctus_x + x] = (uint32_t)slice * 1024u + (uint32_t)tile;
  }
  return HEVCDL_OK;
}
hevcdl_status rc_check_qps(const int32_t *qps, int n)
{
  if (qps) for (int i = 0; i < n; i++) if (qps[i] < 0 || qps[i] > 51) RC_REFUSE(HEVCDL_ERR_INVALID_ARG, "QP %d of picture %d", qps[i], i);
  return HEVCDL_OK;
}
#define HIPOK(call) do { if ((call) != hipSuccess) { (void)hipGetLastError(); RC_REFUSE(HEVCDL_ERR_HIP, "%s failed", #call); } } while (0)
hevcdl_status rc_check_qp_info(const hevcdl_qp_info *q, const void *map)
{
  if (!q || !map) RC_REFUSE(HEVCDL_ERR_INVALID_ARG, "null QP map or hevcdl_qp_info");
  if (q->cb_qp_offset < -12 || q->cb_qp_offset > 12 || q->cr_qp_offset < -12 || q->cr_qp_offset > 12) RC_REFUSE(HEVCDL_ERR_INVALID_ARG, "chroma QP offsets %d / %d", q->cb_qp_offset, q->cr_qp_offset);
  return HEVCDL_OK;
}
hevcdl_status rc_check_scaling(const hevcdl_scaling_info *s)
{
  if (!s) RC_REFUSE(HEVCDL_ERR_INVALID_ARG, "null hevcdl_scaling_info");
  for (int i = 0; i < HEVCDL_SCALING_FACTOR_BYTES; i++) if (!s->factor[i]) RC_REFUSE(HEVCDL_ERR_INVALID_ARG, "scaling factor %d is 0", i);
  return HEVCDL_OK;
}

// ---- one host path for the three instantiations --------------------------------------------------------------------------------------------------------------------
// The forms are named by their launch struct: RcLaunch (a QP per picture), RcLaunchQp (hevcdl_parse_stream_qp's QP map and the PPS chroma offsets), RcLaunchSl (the
// scaling factors of hevcdl_parse_stream_sl on top of the map).  RcQuant is what a form dequantises with, as its entry points are given it: qps (null: cfg->qp for every
// picture) for RcLaunch; info and map for the other two, map in host or device memory as the records of the same call are; for RcLaunchSl also the factors -- `scaling`
// on the host, d_factor where a launch reads them.  What differs between the forms is said where it differs, with if constexpr.
struct RcQuant { const int32_t *qps; const hevcdl_qp_info *info; const void *map; const hevcdl_scaling_info *scaling; const void *d_factor; };
template <typename LAUNCH> constexpr bool rc_has_map = !std::is_same<LAUNCH, RcLaunch>::value;
template <typename LAUNCH> constexpr bool rc_has_factor = std::is_same<LAUNCH, RcLaunchSl>::value;
std::atomic<unsigned long long> g_qp_launches{0}, g_sl_launches{0};      // g_launches counts every launch, these two only their own form's

// the form's check of what it dequantises with, behind the pointers and in front of the sizes: the per-picture QPs, or the PPS offsets and the map
template <typename LAUNCH>
hevcdl_status rc_check_quant(const RcQuant &q, int n_frames)
{
  if constexpr (rc_has_map<LAUNCH>) return rc_check_qp_info(q.info, q.map); else return rc_check_qps(q.qps, n_frames);
}

// what the CPU form and the host-buffer form refuse, in this order, before either does anything
template <typename LAUNCH>
hevcdl_status rc_check_host(const hevcdl_stream_config *cfg, const hevcdl_slice_layout *slices_opt, const RcQuant &q, const hevcdl_ctu_record *records, int n_frames, const void *recon,
                            RcPic &p, std::vector<uint32_t> &unit)
{
  hevcdl_status st = rc_setup(cfg, slices_opt, p, unit);
  if (st != HEVCDL_OK) return st;
  if (!records || !recon || n_frames < 0) RC_REFUSE(HEVCDL_ERR_INVALID_ARG, "null records or pictures");
  if ((st = rc_check_quant<LAUNCH>(q, n_frames)) != HEVCDL_OK) return st;
  if constexpr (rc_has_factor<LAUNCH>) { if ((st = rc_check_scaling(q.scaling)) != HEVCDL_OK) return st; }
  return hevcdl_validate_records(cfg, records, n_frames);      // nothing is allocated, copied or launched on QPs or records that are refused
}

// the *_host forms: rc_ctu as one "lane" over every CTU of every picture
template <typename LAUNCH>
hevcdl_status rc_host(const hevcdl_stream_config *cfg, const hevcdl_slice_layout *slices_opt, const RcQuant &q, const hevcdl_ctu_record *records, int n_frames, void *recon)
{
  decltype(LAUNCH::pic) p; std::vector<uint32_t> unit;
  const hevcdl_status st = rc_check_host<LAUNCH>(cfg, slices_opt, q, records, n_frames, recon, p, unit);
  if (st != HEVCDL_OK) return st;
  const size_t ctus = unit.size(), fb = hevcdl_frame_bytes_bd(p.W, p.H, p.bit_depth);
  std::vector<RcWork> w(1);
  p.unit = unit.data();
  if constexpr (rc_has_map<LAUNCH>) { p.cb_off = q.info->cb_qp_offset; p.cr_off = q.info->cr_qp_offset; }
  if constexpr (rc_has_factor<LAUNCH>) p.factor = q.scaling->factor;
  for (int f = 0; f < n_frames; f++) {
    p.recs = records + (size_t)f * ctus; p.out = (unsigned char *)recon + (size_t)f * fb;
    if constexpr (rc_has_map<LAUNCH>) p.qp_map = (const int8_t *)q.map + (size_t)f * ctus * 256; else p.qp = q.qps ? q.qps[f] : cfg->qp;
    for (int cy = 0; cy < p.ctus_y; cy++) for (int cx = 0; cx < p.ctus_x; cx++) {
      if (p.bit_depth == 8) rc_ctu<uint8_t>(p, w[0], 0, 1, cx, cy); else rc_ctu<uint16_t>(p, w[0], 0, 1, cx, cy);
    }
  }
  return HEVCDL_OK;
}

// The launch alone, on work memory the caller owns (hevcdl_decode_stream: a buffer of the context, sized once by hevcdl_recon_work_bytes): nothing is allocated, freed or
// waited for.  `keep` receives the host copy of what is uploaded (units, QPs) and must live until the stream has passed the copies; *d_error is the error word in the
// work memory, to be fetched with the batch's other results: non-zero = a row waited past the limit.  The device is the caller's current one.  The work memory is laid
// out alike for the three forms -- units, a QP per picture, ticket and error word, row counts -- and the forms with a map leave the QPs' room unused.
template <typename LAUNCH>
hevcdl_status rc_enqueue(const hevcdl_stream_config *cfg, const hevcdl_slice_layout *slices_opt, const RcQuant &q, const void *d_records, int n_frames,
                         void *d_recon, void *d_work, size_t work_bytes, void *stream, std::vector<uint32_t> &keep, const uint32_t **d_error)
{
  LAUNCH L;
  memset(&L, 0, sizeof L);
  hevcdl_status st = rc_setup(cfg, slices_opt, L.pic, keep);
  if (st != HEVCDL_OK) return st;
  if (!d_records || !d_recon || !d_work || !d_error || (rc_has_factor<LAUNCH> && !q.d_factor) || n_frames < 1 || n_frames > (1 << 16)) RC_REFUSE(HEVCDL_ERR_INVALID_ARG, "null device pointer, or a picture count outside 1 .. 65536");
  if ((st = rc_check_quant<LAUNCH>(q, n_frames)) != HEVCDL_OK) return st;
  if (work_bytes < hevcdl_recon_work_bytes(cfg->width, cfg->height, n_frames)) RC_REFUSE(HEVCDL_ERR_INVALID_ARG, "work memory smaller than hevcdl_recon_work_bytes");
  hipStream_t s = (hipStream_t)stream;
  const size_t ctus = keep.size(), rows = (size_t)n_frames * L.pic.ctus_y;
  const size_t b_unit = ctus * 4, b_qp = (size_t)n_frames * 4, b_sync = (2 + rows) * 4;
  if constexpr (!rc_has_map<LAUNCH>) { if (q.qps) keep.insert(keep.end(), (const uint32_t *)q.qps, (const uint32_t *)q.qps + n_frames); }
  unsigned char *d = (unsigned char *)d_work;
  HIPOK(hipMemcpyAsync(d, keep.data(), keep.size() * 4, hipMemcpyHostToDevice, s));
  HIPOK(hipMemsetAsync(d + b_unit + b_qp, 0, b_sync, s));
  L.pic.unit = (const uint32_t *)d; L.pic.recs = (const hevcdl_ctu_record *)d_records; L.pic.out = d_recon;
  if constexpr (rc_has_map<LAUNCH>) { L.pic.qp_map = (const int8_t *)q.map; L.pic.cb_off = q.info->cb_qp_offset; L.pic.cr_off = q.info->cr_qp_offset; }
  else L.qps = q.qps ? (const int32_t *)(d + b_unit) : nullptr;
  if constexpr (rc_has_factor<LAUNCH>) L.pic.factor = (const uint8_t *)q.d_factor;
  L.sync = (uint32_t *)(d + b_unit + b_qp);
  L.frame_bytes = hevcdl_frame_bytes_bd(L.pic.W, L.pic.H, L.pic.bit_depth); L.n_frames = n_frames; L.ctus = (int)ctus;
  const unsigned groups = (unsigned)(rows < RC_MAX_GROUPS ? rows : RC_MAX_GROUPS);
  g_launches.fetch_add(1);
  if (std::is_same<LAUNCH, RcLaunchQp>::value) g_qp_launches.fetch_add(1);
  if (rc_has_factor<LAUNCH>) g_sl_launches.fetch_add(1);
  if (L.pic.bit_depth == 8) hipLaunchKernelGGL((hevcdl_recon_kernel<uint8_t, LAUNCH>), dim3(groups), dim3(64), 0, s, L);
  else hipLaunchKernelGGL((hevcdl_recon_kernel<uint16_t, LAUNCH>), dim3(groups), dim3(64), 0, s, L);
  HIPOK(hipGetLastError());
  *d_error = L.sync + 1;
  return HEVCDL_OK;
}

// The stand-alone device forms: their own work memory, allocated and freed by the call, which therefore waits for the stream (a pipeline uses rc_enqueue).  The
// scaling-list form checks its factors before it asks for the device, and carries them behind the work memory, rounded up to 16 bytes, to be freed with it.
template <typename LAUNCH>
hevcdl_status rc_run_dev(int device, const hevcdl_stream_config *cfg, const hevcdl_slice_layout *slices_opt, RcQuant q, const void *d_records, int n_frames, void *d_recon, void *stream)
{
  if constexpr (rc_has_map<LAUNCH>) { if (!cfg || n_frames < 1) RC_REFUSE(HEVCDL_ERR_INVALID_ARG, "null configuration or no picture"); }
  else { // the constant-QP form takes no picture for a question about the configuration
    if (n_frames == 0 && cfg) { RcPic p; std::vector<uint32_t> u; return rc_setup(cfg, slices_opt, p, u); }
    if (!cfg || n_frames < 0) RC_REFUSE(HEVCDL_ERR_INVALID_ARG, "null configuration or a negative picture count");
  }
  if constexpr (rc_has_factor<LAUNCH>) { const hevcdl_status st = rc_check_scaling(q.scaling); if (st != HEVCDL_OK) return st; }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) { (void)hipGetLastError(); RC_REFUSE(HEVCDL_ERR_NO_DEVICE, "no such device"); }
  HIPOK(hipSetDevice(device));
  const size_t need = hevcdl_recon_work_bytes(cfg->width, cfg->height, n_frames), work = rc_has_factor<LAUNCH> ? (need + 15) & ~(size_t)15 : need;
  unsigned char *d = nullptr;
  if (hipMalloc(&d, work + (rc_has_factor<LAUNCH> ? HEVCDL_SCALING_FACTOR_BYTES : 0)) != hipSuccess) { (void)hipGetLastError(); RC_REFUSE(HEVCDL_ERR_OOM, "no device memory for the row counts"); }
  std::vector<uint32_t> keep; const uint32_t *d_err = nullptr; uint32_t err = 0;
  hevcdl_status out = HEVCDL_OK;
  if constexpr (rc_has_factor<LAUNCH>) {
    q.d_factor = d + work;
    if (hipMemcpyAsync(d + work, q.scaling->factor, HEVCDL_SCALING_FACTOR_BYTES, hipMemcpyHostToDevice, (hipStream_t)stream) != hipSuccess) { (void)hipGetLastError(); hevcdl_parse::set_error("upload failed"); out = HEVCDL_ERR_HIP; }
  }
  if (out == HEVCDL_OK) out = rc_enqueue<LAUNCH>(cfg, slices_opt, q, d_records, n_frames, d_recon, d, work, stream, keep, &d_err);
  if (out == HEVCDL_OK && (hipMemcpyAsync(&err, d_err, 4, hipMemcpyDeviceToHost, (hipStream_t)stream) != hipSuccess || hipStreamSynchronize((hipStream_t)stream) != hipSuccess)) {
    (void)hipGetLastError(); hevcdl_parse::set_error("a HIP call of the reconstruction failed"); out = HEVCDL_ERR_HIP;
  }
  if (out == HEVCDL_OK && err) { hevcdl_parse::set_error("a CTU row waited for the row above longer than the limit"); out = HEVCDL_ERR_HIP; }
  if (out != HEVCDL_OK) (void)hipStreamSynchronize((hipStream_t)stream);      // nothing may still read the work memory when it is freed
  (void)hipFree(d);
  return out;
}

// The host-buffer forms: records, pictures and (with a map) the map behind them in one allocation, uploaded, run by the device form, the pictures downloaded.
template <typename LAUNCH>
hevcdl_status rc_run_host_buffers(int device, const hevcdl_stream_config *cfg, const hevcdl_slice_layout *slices_opt, RcQuant q, const hevcdl_ctu_record *records, int n_frames, void *recon)
{
  RcPic p; std::vector<uint32_t> unit;
  hevcdl_status st = rc_check_host<LAUNCH>(cfg, slices_opt, q, records, n_frames, recon, p, unit);
  if (st != HEVCDL_OK) return st;
  if (n_frames == 0) return HEVCDL_OK;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) { (void)hipGetLastError(); RC_REFUSE(HEVCDL_ERR_NO_DEVICE, "no such device"); }
  HIPOK(hipSetDevice(device));
  const size_t b_rec = sizeof(hevcdl_ctu_record) * unit.size() * (size_t)n_frames, b_pic = hevcdl_frame_bytes_bd(p.W, p.H, p.bit_depth) * (size_t)n_frames;
  const size_t b_map = rc_has_map<LAUNCH> ? unit.size() * 256 * (size_t)n_frames : 0;
  unsigned char *d = nullptr;
  if (hipMalloc(&d, b_rec + b_pic + b_map) != hipSuccess) { (void)hipGetLastError(); RC_REFUSE(HEVCDL_ERR_OOM, "no device memory for %d pictures", n_frames); }
  if (hipMemcpy(d, records, b_rec, hipMemcpyHostToDevice) != hipSuccess || hipMemset(d + b_rec, 0, b_pic) != hipSuccess ||
      (rc_has_map<LAUNCH> && hipMemcpy(d + b_rec + b_pic, q.map, b_map, hipMemcpyHostToDevice) != hipSuccess)) { (void)hipGetLastError(); hevcdl_parse::set_error("upload failed"); st = HEVCDL_ERR_HIP; }
  if (rc_has_map<LAUNCH>) q.map = d + b_rec + b_pic;
  if (st == HEVCDL_OK) st = rc_run_dev<LAUNCH>(device, cfg, slices_opt, q, d, n_frames, d + b_rec, nullptr);
  if (st == HEVCDL_OK && hipMemcpy(recon, d + b_rec, b_pic, hipMemcpyDeviceToHost) != hipSuccess) { (void)hipGetLastError(); hevcdl_parse::set_error("download failed"); st = HEVCDL_ERR_HIP; }
  (void)hipFree(d);
  return st;
}
} // namespace

extern "C" size_t hevcdl_recon_work_bytes(int width, int height, int n_frames)
{
  const size_t cx = (size_t)((width + 63) >> 6), cy = (size_t)((height + 63) >> 6), n = (size_t)(n_frames > 0 ? n_frames : 0);
  return cx * cy * 4 + n * 4 + (2 + n * cy) * 4;
}

// ---- the entry points: per form the CPU loop, the launch (recon_launch.h), the stand-alone device form, the host-buffer form and a launch counter ------------------------
extern "C" unsigned long long hevcdl_recon_launches(void) { return g_launches.load(); }
extern "C" hevcdl_status hevcdl_reconstruct_frames_host(const hevcdl_stream_config *cfg, const hevcdl_slice_layout *slices_opt, const int32_t *qps_opt,
                                                       const hevcdl_ctu_record *records, int n_frames, void *recon)
{
  return rc_host<RcLaunch>(cfg, slices_opt, { qps_opt, nullptr, nullptr, nullptr, nullptr }, records, n_frames, recon);
}
hevcdl_status hevcdl_recon_enqueue(const hevcdl_stream_config *cfg, const hevcdl_slice_layout *slices_opt, const int32_t *qps_opt, const void *d_records, int n_frames,
                                   void *d_recon, void *d_work, size_t work_bytes, void *stream, std::vector<uint32_t> &keep, const uint32_t **d_error)
{
  return rc_enqueue<RcLaunch>(cfg, slices_opt, { qps_opt, nullptr, nullptr, nullptr, nullptr }, d_records, n_frames, d_recon, d_work, work_bytes, stream, keep, d_error);
}
extern "C" hevcdl_status hevcdl_reconstruct_frames_dev(int device, const hevcdl_stream_config *cfg, const hevcdl_slice_layout *slices_opt, const int32_t *qps_opt,
                                                      const void *d_records, int n_frames, void *d_recon, void *stream)
{
  return rc_run_dev<RcLaunch>(device, cfg, slices_opt, { qps_opt, nullptr, nullptr, nullptr, nullptr }, d_records, n_frames, d_recon, stream);
}
extern "C" hevcdl_status hevcdl_reconstruct_frames(int device, const hevcdl_stream_config *cfg, const hevcdl_slice_layout *slices_opt, const int32_t *qps_opt,
                                                  const hevcdl_ctu_record *records, int n_frames, void *recon)
{
  return rc_run_host_buffers<RcLaunch>(device, cfg, slices_opt, { qps_opt, nullptr, nullptr, nullptr, nullptr }, records, n_frames, recon);
}

// with a QP map (hevcdl_parse_stream_qp) and the PPS chroma offsets: the QP-map instantiation of hevcdl_recon_kernel
extern "C" unsigned long long hevcdl_recon_qp_launches(void) { return g_qp_launches.load(); }
extern "C" hevcdl_status hevcdl_reconstruct_frames_qp_host(const hevcdl_stream_config *cfg, const hevcdl_slice_layout *slices_opt, const hevcdl_qp_info *qp_info,
                                                          const int8_t *qp_map, const hevcdl_ctu_record *records, int n_frames, void *recon)
{
  return rc_host<RcLaunchQp>(cfg, slices_opt, { nullptr, qp_info, qp_map, nullptr, nullptr }, records, n_frames, recon);
}
hevcdl_status hevcdl_recon_enqueue_qp(const hevcdl_stream_config *cfg, const hevcdl_slice_layout *slices_opt, const hevcdl_qp_info *qp_info, const void *d_qp_map, const void *d_records,
                                      int n_frames, void *d_recon, void *d_work, size_t work_bytes, void *stream, std::vector<uint32_t> &keep, const uint32_t **d_error)
{
  return rc_enqueue<RcLaunchQp>(cfg, slices_opt, { nullptr, qp_info, d_qp_map, nullptr, nullptr }, d_records, n_frames, d_recon, d_work, work_bytes, stream, keep, d_error);
}
extern "C" hevcdl_status hevcdl_reconstruct_frames_qp_dev(int device, const hevcdl_stream_config *cfg, const hevcdl_slice_layout *slices_opt, const hevcdl_qp_info *qp_info,
                                                         const void *d_qp_map, const void *d_records, int n_frames, void *d_recon, void *stream)
{
  return rc_run_dev<RcLaunchQp>(device, cfg, slices_opt, { nullptr, qp_info, d_qp_map, nullptr, nullptr }, d_records, n_frames, d_recon, stream);
}
extern "C" hevcdl_status hevcdl_reconstruct_frames_qp(int device, const hevcdl_stream_config *cfg, const hevcdl_slice_layout *slices_opt, const hevcdl_qp_info *qp_info,
                                                     const int8_t *qp_map, const hevcdl_ctu_record *records, int n_frames, void *recon)
{
  return rc_run_host_buffers<RcLaunchQp>(device, cfg, slices_opt, { nullptr, qp_info, qp_map, nullptr, nullptr }, records, n_frames, recon);
}

// with scaling factors on top of the QP map (hevcdl_parse_stream_sl): the scaling-list instantiation of hevcdl_recon_kernel
extern "C" unsigned long long hevcdl_recon_sl_launches(void) { return g_sl_launches.load(); }
extern "C" hevcdl_status hevcdl_reconstruct_frames_sl_host(const hevcdl_stream_config *cfg, const hevcdl_slice_layout *slices_opt, const hevcdl_qp_info *qp_info,
                                                          const int8_t *qp_map, const hevcdl_scaling_info *scaling, const hevcdl_ctu_record *records, int n_frames, void *recon)
{
  return rc_host<RcLaunchSl>(cfg, slices_opt, { nullptr, qp_info, qp_map, scaling, nullptr }, records, n_frames, recon);
}
// d_factor: HEVCDL_SCALING_FACTOR_BYTES in device memory, non-zero bytes (the caller has checked them: hevcdl_parse_stream_sl's are by construction)
hevcdl_status hevcdl_recon_enqueue_sl(const hevcdl_stream_config *cfg, const hevcdl_slice_layout *slices_opt, const hevcdl_qp_info *qp_info, const void *d_qp_map, const void *d_factor,
                                      const void *d_records, int n_frames, void *d_recon, void *d_work, size_t work_bytes, void *stream, std::vector<uint32_t> &keep, const uint32_t **d_error)
{
  return rc_enqueue<RcLaunchSl>(cfg, slices_opt, { nullptr, qp_info, d_qp_map, nullptr, d_factor }, d_records, n_frames, d_recon, d_work, work_bytes, stream, keep, d_error);
}
extern "C" hevcdl_status hevcdl_reconstruct_frames_sl_dev(int device, const hevcdl_stream_config *cfg, const hevcdl_slice_layout *slices_opt, const hevcdl_qp_info *qp_info,
                                                         const void *d_qp_map, const hevcdl_scaling_info *scaling, const void *d_records, int n_frames, void *d_recon, void *stream)
{
  return rc_run_dev<RcLaunchSl>(device, cfg, slices_opt, { nullptr, qp_info, d_qp_map, scaling, nullptr }, d_records, n_frames, d_recon, stream);
}
extern "C" hevcdl_status hevcdl_reconstruct_frames_sl(int device, const hevcdl_stream_config *cfg, const hevcdl_slice_layout *slices_opt, const hevcdl_qp_info *qp_info,
                                                     const int8_t *qp_map, const hevcdl_scaling_info *scaling, const hevcdl_ctu_record *records, int n_frames, void *recon)
{
  return rc_run_host_buffers<RcLaunchSl>(device, cfg, slices_opt, { nullptr, qp_info, qp_map, scaling, nullptr }, records, n_frames, recon);
}
