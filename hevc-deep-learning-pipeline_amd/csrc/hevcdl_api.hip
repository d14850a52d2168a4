// hevcdl_api.hip -- host side of the C ABI declared in include/hevcdl.h (compiled by hipcc for gfx950).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <string.h>
#include <algorithm>
#include <vector>
#include "hevcdl.h"
#include "hevcdl_dev.h"
#include "recon_launch.h"
#include "dbk_select.h"
#include "entropy_coder.h"
#include "picture_hash_core.h"
#include "source_core.h"
#include "rd_launch_plan.h"
#include "slice_grid.h"
#include "qp_rd.h"
#include "frame_qp.h"
#include "slice_decode_units.h"

enum { LABELS_PER_CTU = 16, LOGITS_PER_CTU = 64, CTU_RGB_BYTES = 64 * 64 * 3 };      // of a CTU: its 16x16 cells, four logits a cell, the RGB input of hevcdl_predict_depth_rgb

extern "C" __global__ void hevcdl_cnn_ctu_kernel(hevcdl_cnn_params p);
extern "C" __global__ void hevcdl_fc_kernel(hevcdl_fc_params p);          // fc_kernel.hip: fully connected head + labels, 16 CTUs per workgroup
// the decision kernel's builds: rd_kernel.hip (its hevcdl_rd_smem_bytes / _scratch_bytes / _waves_per_group: hevcdl_dev.h), and the same kernel for uint16 samples
// (rd_kernel_bd10.hip), with more wavefronts per workgroup (rd_kernel_wide.hip) and with the cfg's tool switches read at run time (rd_kernel_tools.hip)
extern "C" __global__ void hevcdl_rd_frame_kernel(hevcdl_rd_params p);
#define RD_BUILD_DECL(sfx) extern "C" __global__ void hevcdl_rd_frame_kernel##sfx(hevcdl_rd_params p); extern "C" size_t hevcdl_rd_smem_bytes##sfx(void); \
                           extern "C" size_t hevcdl_rd_scratch_bytes##sfx(void); extern "C" int hevcdl_rd_waves_per_group##sfx(void);
RD_BUILD_DECL(_bd10) RD_BUILD_DECL(_wide) RD_BUILD_DECL(_tools)

// The decision kernel's four builds.  Whatever depends on which of them a launch runs is read from its row (rd_launch_plan.h picks the row and holds the names).
struct RdBuild { const void *kernel; size_t (*smem_bytes)(void); size_t (*scratch_bytes)(void); int (*waves_per_group)(void); };      // scratch_bytes: per wave
#define RD_BUILD_ROW(sfx) { (const void *)hevcdl_rd_frame_kernel##sfx, hevcdl_rd_smem_bytes##sfx, hevcdl_rd_scratch_bytes##sfx, hevcdl_rd_waves_per_group##sfx }
static const RdBuild rd_builds[RD_BUILDS] = { RD_BUILD_ROW(), RD_BUILD_ROW(_wide), RD_BUILD_ROW(_tools), RD_BUILD_ROW(_bd10) };      // in the order of rd_launch_plan.h's RD_*

// 10-bit samples -> the 8-bit planes the CNN stage reads (the reference's label producer works on 8-bit frames: gen_frames.py)
__global__ void hevcdl_narrow_samples_kernel(const uint16_t *src, uint8_t *dst, size_t n, int shift)
{
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) dst[i] = (uint8_t)(src[i] >> shift);
}

// Boundary policy HEVCDL_BOUNDARY_CLAMP applied to caller-supplied labels (the label files of the reference's use_model.py are unclamped):
// every cell is raised to the smallest depth whose CU lies inside the picture, then the quadtree is made consistent again (a split CTU has
// no depth-0 cell, a split 32x32 quadrant no depth-1 cell) -- the same rule the label stage of fc_kernel.hip applies to its own output.
// Labels above 3 are a caller error: *bad is set.  One thread per CTU.
__global__ void hevcdl_clamp_labels_kernel(uint8_t *labels, int n_ctus, int ctus_per_frame, int ctus_x, int width, int height, int *bad)
{
  const int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n_ctus) return;
  const int addr = g % ctus_per_frame, x0 = (addr % ctus_x) * 64, y0 = (addr / ctus_x) * 64;
  uint8_t *lab = labels + (size_t)g * 16;
  uint8_t l[16];
  for (int c = 0; c < 16; c++) { l[c] = lab[c]; if (l[c] > 3) { *bad = 1; l[c] = 3; } }
  hevcdl_clamp_ctu_labels(l, x0, y0, width, height);
  for (int c = 0; c < 16; c++) lab[c] = (uint8_t)l[c];
}

// the window's SSE of the reconstruction before the in-loop filters into the statistics of a padded picture (hevcdl_set_source_format): one thread per (picture, plane)
__global__ void hevcdl_stats_sse_kernel(const hevcdl_quality *q, hevcdl_frame_stats *stats, int n_frames)
{
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t < 3 * n_frames) stats[t / 3].sse[t % 3] = q[t / 3].sse[t % 3];
}

// Owners: a handle that is released in the destructor and in reset(), moves but does not copy, and converts to the handle.  Everything a context holds on the device
// is one of these, so releasing a feature is assigning a fresh sub-struct and hevcdl_destroy is `delete`.
template <class H, class Release> struct Owned {
  H p = H();
  Owned() = default;
  Owned(Owned &&o) noexcept : p(o.p) { o.p = H(); }      // (a move constructor: no copies)
  Owned &operator=(Owned &&o) noexcept { if (this != &o) { reset(); p = o.p; o.p = H(); } return *this; }
  ~Owned() { reset(); }
  void reset() { if (p) Release()(p); p = H(); }
  operator H() const { return p; }
};
struct ReleaseDev { void operator()(void *p) const { hipFree(p); } };
struct ReleaseHost { void operator()(void *p) const { hipHostFree(p); } };
struct ReleaseEvent { void operator()(hipEvent_t e) const { hipEventDestroy(e); } };
struct ReleaseStream { void operator()(hipStream_t s) const { hipStreamDestroy(s); } };
template <class T> using DevBuf = Owned<T *, ReleaseDev>;      // hipMalloc'ed
using HostBuf = Owned<unsigned char *, ReleaseHost>;           // page-locked
using Event = Owned<hipEvent_t, ReleaseEvent>;
using Stream = Owned<hipStream_t, ReleaseStream>;

// The context's buffers, grouped by who allocates them (and who gives them back).
struct Staging {      // staging buffers for the host-pointer entry points: the first six by ensure_staging (all or nothing), the rest by the first call that needs them
  DevBuf<uint8_t> d_yuv, d_labels, d_recon; DevBuf<unsigned char> d_records, d_stats; DevBuf<float> d_logits;
  DevBuf<uint8_t> d_yuv8;               // 8-bit copy of 10-bit input for the CNN stage
  DevBuf<unsigned char> d_wide;         // 16-bit staging of hevcdl_*_planes with sample_bytes 2 on an 8-bit context
  DevBuf<uint8_t> d_picture;            // final pictures of hevcdl_encode_pictures (SAO output)
  HostBuf h_chunk[2]; size_t h_chunk_bytes = 0; Stream copy_stream; Event copy_ev[2];   // hevcdl_encode_pictures_chunked: two page-locked chunk buffers
};
struct SaoWorkspace { DevBuf<unsigned char> d_sao_stats, d_sao_recon, d_sao_params, d_sao_cand; std::vector<hevcdl_sao_blk> given; };
struct Decoder { DevBuf<unsigned char> d_work; std::vector<uint32_t> keep; };      // hevcdl_decode_stream: the reconstruction's units, QPs and row counts (cfg.max_frames), by the first call      // SAO workspace: by the first call that needs each
// slice data DECODED on the device (slice_decode_kernel.hip): everything below is allocated by hevcdl_enable_device_parse(ctx, 1), sized for cfg.max_frames pictures, and
// freed by (ctx, 0); the three that hold a batch's bytes and tables are given back and allocated larger when a batch needs more.  A context that never turns the switch
// on allocates and launches none of it
// a QP per CU (hevcdl_enable_cu_qp): the map of a batch in HBM beside the records -- uploaded behind a host parse, written by the kernel with device parse --, allocated
// by the first stream that needs it.  active / info: the batch in work, read by the deblocking launch (null outside hevcdl_decode_stream and hevcdl_deblock_frames_map)
struct CuQp { bool on = false; DevBuf<signed char> d_map; const signed char *active = nullptr; hevcdl_qp_info info = { 0, 0, 0, 0 }; };
// scaling lists (hevcdl_enable_scaling_lists): the factor block of the stream in work in HBM, allocated by the first stream that has lists; such a stream also uses cuqp.d_map
struct ScalingLists { bool on = false; DevBuf<unsigned char> d_factor; };
struct DeviceParse {
  bool on = false;
  DevBuf<unsigned char> d_tables, d_rbsp, d_sao; DevBuf<hevcdl_sd::SdSub> d_subs; DevBuf<hevcdl_sd::SdUnit> d_units; DevBuf<hevcdl_sd::SdResult> d_results;
  size_t rbsp_bytes = 0, n_subs = 0, n_units = 0;      // what the three hold
  std::vector<hevcdl_sao_blk> h_sao; std::vector<hevcdl_sd::SdResult> h_results; std::vector<hevcdl_sd::SdUnit> h_units;      // the batch in work
};
// picture quality (quality_kernel.hip): the workspace is allocated by hevcdl_enable_quality(ctx, 1), or by the first hevcdl_picture_quality* call of a context
// with the switch off, and freed by hevcdl_enable_quality(ctx, 0); d_q_out by the switch or by hevcdl_picture_quality (host buffers).  A context that uses neither allocates none of it
struct Quality {
  bool quality_on = false;                 // hevcdl_enable_quality: the picture pipeline also measures its output pictures
  DevBuf<unsigned char> d_q_pyr, d_q_partial, d_q_weights, d_q_out; int q_group = 0;      // workspace of q_group pictures; d_q_out: [max_frames] hevcdl_quality of the pipeline
  std::vector<hevcdl_quality> h_quality;   // the pipeline's last batch (hevcdl_get_quality)
};
// picture report (report_kernel.hip): the workspace -- records, CRC / checksum partials and the SSE launch's output for max_frames pictures, a few KB a picture -- is
// allocated by hevcdl_enable_picture_report(ctx, 1, method), or by the first hevcdl_picture_report* call of a context with the switch off, and freed by (ctx, 0, 0)
struct Report {
  bool report_on = false; int report_method = 0;
  DevBuf<unsigned char> d_rp_out, d_rp_sse; DevBuf<uint32_t> d_rp_partials;
  std::vector<hevcdl_picture_report_t> h_report;      // the pipeline's last batch (hevcdl_get_picture_report)
};
// slice data on the device (entropy_kernel.hip): everything below is allocated by hevcdl_enable_device_entropy(ctx, 1) and freed by (ctx, 0); a context that never
// turns the switch on allocates and launches none of it
struct Entropy {
  bool entropy_on = false;
  int ec_units = 0, ec_pass_frames = 0; size_t ec_frame_stride = 0;        // sub-streams of a picture, pictures the workspace holds, bytes of a picture's regions
  DevBuf<unsigned char> d_ec_tables, d_ec_ws, d_ec_packed, d_ec_sync;
  DevBuf<uint32_t> d_ec_off, d_ec_cap, d_ec_sizes, d_ec_ovf; DevBuf<unsigned long long> d_ec_dst;
  std::vector<uint32_t> ec_off, ec_cap;
  std::vector<uint8_t> h_slice; std::vector<uint32_t> h_slice_sizes; std::vector<size_t> h_slice_at;      // the last batch: packed sub-streams, [picture][unit] lengths, start of every picture (+ the end)
  int ec_fallbacks = 0;                    // pictures of the last batch the host coded (a sub-stream overflowed its region)
};
// source format (source_kernel.hip): everything below is allocated by hevcdl_set_source_format(ctx, fmt) and freed by (ctx, NULL); a context without one allocates
// and launches none of it.  d_src: max_frames frames of the larger of the source and the output format (the picture pipeline's upload; staging of the host entry
// points).  With padding (source_windowed) also the window crops at the internal depth of originals and pictures, and the SSE words of the statistics.
struct Source {
  bool source_on = false, source_windowed = false; hevcdl_source_format src_fmt = {};
  DevBuf<unsigned char> d_src, d_win_org, d_win_pic, d_win_sse;
  const uint8_t *d_last_final = nullptr; int last_frames = 0;      // output pictures of the last picture pipeline call, still in HBM (hevcdl_get_output_frames)
};
// per-picture deblocking parameters: the parameter rows of a batch in HBM and the metric's sums, allocated by the first call that needs them; the choices of the picture
// pipeline's last batch (hevcdl_get_dbk_choice)
struct DbkSelect {
  DevBuf<int> d_frame_params; DevBuf<unsigned long long> d_sums;      // d_sums: [max_frames][49] words (the metric uses two a picture)
  std::vector<int> h_frame_params; std::vector<unsigned long long> h_sums; std::vector<hevcdl_dbk_choice> h_choice;
  hevcdl_dbk_walk_state walk = { 0, 0, 0, 0 };      // DeblockingFilterMetric 2: the reference's m_DBParam[0], advanced picture by picture across calls (hevcdl_dbk_select_reset)
};
// per-CTU session (hevcdl_begin_frames / hevcdl_compress_ctu): coder state after the last CTU of every frame, next CTU expected
struct Session { DevBuf<unsigned char> d_cabac; std::vector<int> next_ctu; int session_frames = 0; };
// the decision kernel's workspace and scheduling areas
struct RdWorkspace {
  RdPlanContext plan;                    // what rd_launch_plan reads of this context (rd_launch_plan.h)
  DevBuf<unsigned char> d_scratch;       // one block per wave of every workgroup of a launch; allocated by the first launch that needs it, grown when a later one needs more (ensure_scratch)
  size_t scratch_bytes = 0, scratch_per_wave = 0;      // scratch_per_wave: the largest of the builds this context can run
  int wpp_ring = 0; size_t wpp_state_bytes = 0;
  DevBuf<unsigned char> d_wpp;           // WaveFrontSynchro: [max_frames][ctus_y] 256 bytes (the contexts behind a row's second CTU, the row's finished-CTU count: rd_kernel.hip)
  DevBuf<unsigned char> d_sched;         // hand-over of units between workgroups (finished counter, per-workgroup unit counts, mailboxes)
};
// DeltaQpRD (qp_rd_kernel.hip, qp_rd.h): the candidate table of the configuration; the trial set -- outputs of the candidates behind the first, for max_frames pictures --
// and the rows, allocated by the first decision call of a context with the key (or hevcdl_reserve_workspace); the per-picture QP table of the stages behind the
// decisions.  A context without the key (n == 0) allocates and launches none of it.
struct QpRd {
  int n = 0, count = 1;                  // cfg.delta_qp_rd, 2 n + 1
  hevcdl_qp_rd_candidate cand[HEVCDL_QP_RD_MAX_CANDIDATES]; double frame_lambda = 0;
  DevBuf<unsigned char> d_records, d_recon, d_stats; DevBuf<hevcdl_qp_rd_row> d_rows;
  DevBuf<hevcdl_frame_qp> d_frame_qp; std::vector<hevcdl_frame_qp> h_frame_qp;      // what SAO and the entropy coder read per picture (staged like the deblocking rows)
  size_t trial_bytes = 0; unsigned long long launches = 0;
  std::vector<Event> ev_sum, ev_keep;    // with hevcdl_profile_enable: start / stop pairs round the sum and keep launches of the last search (hevcdl_get_qp_rd_info)
  int last_frames = 0;                   // pictures of the last decision call: their rows are in d_rows
  std::vector<int32_t> h_idx;            // the picture pipeline's last batch: the candidate every picture was coded with
  std::vector<hevcdl_qp_rd_row> h_rows;  // ... and its rows, fetched once (hevcdl_get_qp_rd then copies from here, also inside a chunk callback); empty behind a *_dev call
};

// A QP per picture (hevcdl_set_frame_qps, hevcdl_set_lambda_modifier; frame_qp.h, frame_permute_kernel.hip): the list and the modifier as set; the QPs of the last decision
// call; the two sorted sets -- originals and labels the gather fills, records / reconstruction / statistics the decision launches fill and the scatter empties -- for
// max_frames pictures, all or nothing, by the first call whose list is not contiguous runs (or hevcdl_reserve_workspace).  A context that never sets a list or a modifier
// allocates and launches none of it.  Not DeltaQpRD's trial set: the two keys exclude each other.
struct FrameQp {
  std::vector<int> list; double lambda_modifier = 1.0;
  bool active() const { return !list.empty() || lambda_modifier != 1.0; }
  std::vector<int> used;                 // the QP of every picture of the last decision call
  std::vector<int> perm;                 // of the last permuted call: sorted place -> picture; the host copy the upload reads (it lives until the next call)
  DevBuf<uint8_t> d_yuv, d_labels, d_recon; DevBuf<unsigned char> d_records, d_stats; DevBuf<int> d_perm;      // d_perm: [max_frames], read by the gather and (as its inverse) by the scatter
  size_t set_bytes = 0; int rd_launches = 0, permute_launches = 0;
  std::vector<Event> ev_permute;         // with hevcdl_profile_enable: start / stop pairs round the gather and the scatter launch of the last call
};

struct hevcdl_ctx {
  char last_rd[160] = { 0 };           // which build and launch form the last decision launch took (hevcdl_last_rd_launch)
  hevcdl_config cfg = {};              // as created -- but with slices its tile fields hold the grid the context RUNS (hevcdl_create): a column of row slices for SliceMode 1
  hevcdl_slice_layout slices = { 0, 0, 1 };      // what the caller's slice keys say; the stream is written from this, never from the grid
  hevcdl_segment_layout segments = { 0, 0 };     // the caller's SliceSegmentMode / SliceSegmentArgument: the stream's alone -- ctx->cfg does not hold them (slice_grid.h)
  int stream_lf_across_tiles = 1;      // the caller's lf_across_tiles (cfg's is the effective one: in SliceMode 3 combined with lf_across_slices)
  int ctus_x = 0, ctus_y = 0, ctus = 0, n_cus = 0; size_t frame_bytes = 0;
  int col_bd[21] = { 0 }, row_bd[23] = { 0 };    // tile boundaries in CTUs
  DevBuf<float> d_weights, d_a3; size_t a3_ctus = 0;   // d_a3: conv3 outputs of one chunk of CTUs (32 KB per CTU): the hand-over from the conv kernel to the head kernel
  DevBuf<int> d_flag;                  // device-side error flag of the label check
  Staging stage; SaoWorkspace sao; Decoder dec; DeviceParse dp; CuQp cuqp; ScalingLists sclist; Quality q; Report rp; Entropy ec; Source src; Session ses; RdWorkspace rd; DbkSelect dbk; QpRd qprd; FrameQp fqp;
  int ec_capacity_per_ctu = 0;         // hevcdl_set_entropy_capacity (tests): 0 = the default; outlives the entropy switch
  bool profile = false;
  std::vector<Event> ev_cnn, ev_rd, ev_conv;       // start/stop pairs (ev_conv: the convolution kernel alone, one pair per chunk of CTUs)
  Event rp_ev[4]; double rp_ms[3] = { 0, 0, 0 };      // with `profile`: HIP-event times of the last report launches (SSE, partial or MD5, finish)
  double ec_ms[3] = { 0, 0, 0 };       // with `profile`: HIP-event times of the last entropy batch (phase 1, coding, pack)
  char err[256] = { 0 };
  // sizes of a batch of n frames
  size_t records_bytes(size_t n) const { return (size_t)ctus * sizeof(hevcdl_ctu_record) * n; }
  size_t labels_bytes(size_t n) const { return (size_t)ctus * LABELS_PER_CTU * n; }
  size_t logits_bytes(size_t n) const { return (size_t)ctus * LOGITS_PER_CTU * sizeof(float) * n; }
  size_t sao_bytes(size_t n) const { return (size_t)ctus * sizeof(hevcdl_sao_blk) * n; }
};

// (CHROMA_SCALE_420 and the quantiser scales of TComRom.cpp: csrc/qp_rd.h, beside the lambda family that reads them)

static hevcdl_status fail(hevcdl_ctx *c, hevcdl_status s, const char *what, hipError_t e = hipSuccess)
{
  if (c) snprintf(c->err, sizeof c->err, "%s%s%s", what, e != hipSuccess ? ": " : "", e != hipSuccess ? hipGetErrorString(e) : "");
  return s;
}
#define HIPCHK(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) return fail(ctx, HEVCDL_ERR_HIP, #call, e_); } while (0)

// The one mapping of a HIP error to a status, and the one way an allocation (or the upload that fills it) fails: the sticky error is cleared, the message is `what`.
static hevcdl_status hip_status(hipError_t e) { return e == hipErrorOutOfMemory ? HEVCDL_ERR_OOM : HEVCDL_ERR_HIP; }
static hevcdl_status hip_fail(hevcdl_ctx *c, const char *what, hipError_t e) { (void)hipGetLastError(); return fail(c, hip_status(e), what, e); }
struct AllocItem { void **slot; size_t bytes; };
template <class T> static AllocItem want(DevBuf<T> &b, size_t bytes) { return { (void **)&b.p, bytes }; }
// A set of (empty) buffers, all or nothing: a partial set would let later calls run on null buffers (records alone are 63 GB at 2048 frames of 2160p)
static hevcdl_status alloc_all(hevcdl_ctx *c, std::initializer_list<AllocItem> items, const char *what)
{
  for (const AllocItem &it : items) {
    const hipError_t e = hipMalloc(it.slot, it.bytes);
    if (e == hipSuccess) continue;
    for (const AllocItem &u : items) { if (&u == &it) break; hipFree(*u.slot); *u.slot = nullptr; }
    *it.slot = nullptr;
    return hip_fail(c, what, e);
  }
  return HEVCDL_OK;
}
// a buffer allocated by the first call that needs it
template <class T> static hevcdl_status lazy_alloc(hevcdl_ctx *c, DevBuf<T> &b, size_t bytes, const char *what)
{
  if (b) return HEVCDL_OK;
  const hipError_t e = hipMalloc(&b.p, bytes);
  return e == hipSuccess ? HEVCDL_OK : hip_fail(c, what, e);
}
#define TRY(call) do { hevcdl_status st_ = (call); if (st_) return st_; } while (0)
// the device of the entries that take no context
static hevcdl_status select_device(int device)
{
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device < 0 || device >= n) { (void)hipGetLastError(); return HEVCDL_ERR_NO_DEVICE; }
  if (hipSetDevice(device) != hipSuccess) { (void)hipGetLastError(); return HEVCDL_ERR_HIP; }
  return HEVCDL_OK;
}
// the error of the launches just made, if any
static hevcdl_status launch_status(hevcdl_ctx *ctx) { HIPCHK(hipGetLastError()); return HEVCDL_OK; }
// the context's device, idle: behind the launches of a host wrapper, in front of giving buffers back
static hevcdl_status sync_or_fail(hevcdl_ctx *ctx, const char *what)
{
  hipError_t e = hipSetDevice(ctx->cfg.device); if (e == hipSuccess) e = hipDeviceSynchronize();
  return e == hipSuccess ? HEVCDL_OK : fail(ctx, HEVCDL_ERR_HIP, what, e);
}

extern "C" int hevcdl_ctus_per_frame(int w, int h) { return ((w + 63) >> 6) * ((h + 63) >> 6); }
extern "C" size_t hevcdl_frame_bytes(int w, int h) { return (size_t)w * h * 3 / 2; }
extern "C" size_t hevcdl_frame_bytes_bd(int w, int h, int bit_depth) { return (size_t)w * h * 3 / 2 * (bit_depth > 8 ? 2 : 1); }

extern "C" hevcdl_status hevcdl_config_default(hevcdl_config *cfg, int width, int height, int qp)
{
  return hevcdl_config_default_bd(cfg, width, height, qp, 8);
}

extern "C" hevcdl_status hevcdl_config_default_bd(hevcdl_config *cfg, int width, int height, int qp, int bit_depth)
{
  if (bit_depth != 8 && bit_depth != 10) return HEVCDL_ERR_UNSUPPORTED;
  if (!cfg || width <= 0 || height <= 0 || (width & 7) || (height & 7) || qp < 0 || qp > 51) return HEVCDL_ERR_INVALID_ARG;
  memset(cfg, 0, sizeof *cfg);
  cfg->struct_size = sizeof *cfg;
  cfg->width = width; cfg->height = height; cfg->bit_depth = bit_depth; cfg->chroma_format = 420; cfg->qp = qp;
  cfg->ctu_size = 64; cfg->max_partition_depth = 4; cfg->tu_log2_min = 2; cfg->tu_log2_max = 5; cfg->tu_max_depth_intra = 3;
  cfg->tools = HEVCDL_TOOLS_REFERENCE; cfg->bn_mode = HEVCDL_BN_REFERENCE; cfg->boundary_policy = HEVCDL_BOUNDARY_CLAMP;
  cfg->cnn_input = HEVCDL_CNN_INPUT_RGB601; cfg->device = 0; cfg->max_frames = 1; cfg->tile_columns = 1; cfg->tile_rows = 1; cfg->tile_uniform_spacing = 1; cfg->lf_across_tiles = 1; cfg->lf_offset_in_pps = 1; cfg->lf_across_slices = 1;
  // TEncSlice::calculateLambda (TEncSlice.cpp:433-527) for an all-intra GOP of 1, then setUpLambda (:112-140) and the quantiser's tables: csrc/qp_rd.h, the code every
  // candidate of the QP search (delta_qp_rd) is computed by as well
  hevcdl_qp_rd_candidate f;
  hevcdl_lambda_family_of(qp, qp, bit_depth, &f);
  cfg->lambda = f.lambda; cfg->sqrt_lambda = f.sqrt_lambda; cfg->chroma_weight = f.chroma_weight; cfg->lambda_chroma = f.lambda_chroma; cfg->qp_chroma = f.qp_chroma;
  memcpy(cfg->err_scale, f.err_scale, sizeof cfg->err_scale); cfg->sbh_rd_factor[0] = f.sbh_rd_factor[0]; cfg->sbh_rd_factor[1] = f.sbh_rd_factor[1];
  return HEVCDL_OK;
}

// state_dict order of the reference checkpoint (fp32 tensors): offsets in floats
enum { B_C1W = 0, B_C1B = 1200, B_C1G = 1216, B_C1BE = 1232, B_C2W = 1280, B_C2B = 19712, B_C2G = 19776, B_C2BE = 19840,
       B_C3W = 20032, B_C3B = 93760, B_C3G = 93888, B_C3BE = 94016, B_F1W = 94400, B_F1B = 618688, B_F2W = 618944, B_F2B = 635328,
       B_F3W = 635392, B_F3B = 636416, B_C64W = 636432, B_C64B = 637632, B_C64G = 637648, B_C64BE = 637664 };

// f32 -> IEEE half, round to nearest even (weights are small: no overflow handling beyond saturation to the largest finite half)
static uint16_t f32_to_f16(float f)
{
  uint32_t x; memcpy(&x, &f, 4);
  const uint32_t sign = (x >> 16) & 0x8000u; x &= 0x7fffffffu;
  if (x >= 0x477ff000u) return (uint16_t)(sign | 0x7bffu);
  if (x < 0x38800000u) { // subnormal half (or zero)
    if (x < 0x33000000u) return (uint16_t)sign;
    const int shift = 113 - (int)(x >> 23);
    uint32_t m = (x & 0x7fffffu) | 0x800000u;
    const uint32_t r = m >> (shift + 13), rem = m & ((1u << (shift + 13)) - 1u), half = 1u << (shift + 12);
    return (uint16_t)(sign | (r + ((rem > half || (rem == half && (r & 1u))) ? 1u : 0u)));
  }
  const uint32_t r = ((x - 0x38000000u) >> 13), rem = x & 0x1fffu;
  return (uint16_t)(sign | (r + ((rem > 0x1000u || (rem == 0x1000u && (r & 1u))) ? 1u : 0u)));
}
static float f16_to_f32(uint16_t h)
{
  const uint32_t sign = (uint32_t)(h & 0x8000u) << 16, e = (h >> 10) & 31u, m = h & 0x3ffu;
  uint32_t x;
  if (e == 0) { if (!m) x = sign; else { int sh = 0; uint32_t mm = m; while (!(mm & 0x400u)) { mm <<= 1; sh++; } x = sign | ((uint32_t)(113 - sh) << 23) | ((mm & 0x3ffu) << 13); } }
  else x = sign | ((e + 112u) << 23) | (m << 13);
  float f; memcpy(&f, &x, 4); return f;
}
// conv2 / conv3 on v_mfma_f32_16x16x32_f16 with SPLIT operands (cnn_kernel.hip): a weight w is the pair hi = half(w), lo = half(w - hi).  B-operand packing:
// lane l supplies B[k = 8 * (l >> 4) + j][n = l & 15], j = 0..7, and k-value (l >> 4, j) of k-step s stands for half j & 1 of the channel PAIR 16 s + 4 (j >> 1) + (l >> 4)
// of the kernel's activation maps (a word of a map holds the hi -- or the lo -- halves of two channels: four words are an operand as they lie in LDS).  Layout: [oc/16 N-tiles][9 taps][ic/32 k-steps][hi | lo][64 lanes][8 halves],
// then bias, gamma, beta as floats -- the same number of bytes as the f32 packing it replaces.
// the 5x5 convolutions (3 input channels, 16 output channels = one N-tile): the 75 taps (c * 5 + ky) * 5 + kx in the order of hevcdl_conv5_slot_tap, 5 k-steps of 16.
// The A operand of a step is four raw split words (hi, lo, hi, lo, ...): B1 carries the weight's hi half against both halves, B2 its lo half against the hi half only.
// weight scale of a layer (hevcdl_dev.h HEVCDL_ACT_SCALE): the largest power of two that keeps max |w| * scale below 2^15 (f16 holds 65504), at most 2^24
static float layer_scale(const float *w, size_t n)
{
  float m = 0.f;
  for (size_t i = 0; i < n; i++) { const float a = fabsf(w[i]); if (a > m && a <= 3.0e38f) m = a; }
  float sc = 1.f;
  if (m > 0.f) while (sc < 16777216.f && m * sc * 2.f < 32768.f) sc *= 2.f;
  return sc;
}
// sc: the layer's weight scale; the bias enters the accumulator, which holds sc * HEVCDL_ACT_SCALE times the layer's output
static void pack_conv5(const float *w, const float *b, const float *g, const float *be, float *dst, float sc)
{
  uint16_t *d16 = (uint16_t *)dst;
  for (int s = 0; s < 5; s++) for (int l = 0; l < 64; l++) for (int e = 0; e < 8; e++) {
    const int k = hevcdl_conv5_slot_tap(16 * s + 4 * (l >> 4) + (e >> 1)), oc = l & 15;
    const float v = (k >= 0 ? w[oc * 75 + k] : 0.f) * sc;
    const uint16_t hi = f32_to_f16(v), lo = f32_to_f16(v - f16_to_f32(hi));
    d16[(size_t)(s * 2) * 512 + (size_t)l * 8 + e] = hi; d16[(size_t)(s * 2 + 1) * 512 + (size_t)l * 8 + e] = (e & 1) ? (uint16_t)0 : lo;
  }
  for (int c = 0; c < 16; c++) dst[HEVCDL_W_C5 + c] = b[c] * sc * HEVCDL_ACT_SCALE;
  memcpy(dst + HEVCDL_W_C5 + 16, g, 16 * sizeof(float)); memcpy(dst + HEVCDL_W_C5 + 32, be, 16 * sizeof(float));
}
static void pack_conv3(const float *w, const float *b, const float *g, const float *be, int oc, int ic, float *dst, float sc)
{
  uint16_t *d16 = (uint16_t *)dst;
  const int ks = ic / 32;
  for (int nt = 0; nt < oc / 16; nt++) for (int tap = 0; tap < 9; tap++) for (int s = 0; s < ks; s++) for (int l = 0; l < 64; l++) for (int j = 0; j < 8; j++) {
    // element j of lane group g = l >> 4: half j & 1 of the map's channel PAIR m = 16 s + 4 (j >> 1) + g (cnn_kernel.hip: the operand is four words of a plane of pairs).
    // conv2's input (32 channels): pair m = channels 2m | 2m + 1;  conv3's input (64): pairs 0..15 = channels m | m + 16, pairs 16..31 = 16 + m | 32 + m
    const int m = 16 * s + 4 * (j >> 1) + (l >> 4), hf = j & 1;
    const int c = ic == 32 ? 2 * m + hf : (m < 16 ? m + 16 * hf : 16 + m + 16 * hf), o = nt * 16 + (l & 15);
    const float v = w[((size_t)o * ic + c) * 9 + tap] * sc;
    const uint16_t hi = f32_to_f16(v), lo = f32_to_f16(v - f16_to_f32(hi));
    const size_t base = ((((size_t)nt * 9 + tap) * ks + s) * 2) * 512;        // halves: 64 lanes x 8 per operand
    d16[base + (size_t)l * 8 + j] = hi; d16[base + 512 + (size_t)l * 8 + j] = lo;
  }
  float *t = dst + (size_t)9 * ic * oc;
  for (int c = 0; c < oc; c++) t[c] = b[c] * sc * HEVCDL_ACT_SCALE;
  memcpy(t + oc, g, oc * sizeof(float)); memcpy(t + 2 * oc, be, oc * sizeof(float));
}
// HEVCDL_BN_EVAL: BatchNorm with the checkpoint's running statistics (model.eval()) is the fixed affine map y = x * alpha + beta' with
// alpha = gamma / sqrt(running_var + eps), beta' = beta - running_mean * alpha; the kernels find the pair in the gamma / beta slots of the
// packed layer (state_dict order: weight, bias, running_mean, running_var follow each other, `oc` floats each).
// The map is applied to the accumulator (in_sc = weight scale * HEVCDL_ACT_SCALE times the layer's output) and writes activations scaled by HEVCDL_ACT_SCALE.
static void fold_bn_eval(const float *g, const float *be, int oc, float *dst_g, float *dst_be, float in_sc)
{
  const float *rm = be + oc, *rv = be + 2 * oc;
  for (int c = 0; c < oc; c++) {
    const double a = (double)g[c] / sqrt((double)rv[c] + 1e-5);
    dst_g[c] = (float)(a / (double)in_sc * (double)HEVCDL_ACT_SCALE); dst_be[c] = (float)(((double)be[c] - (double)rm[c] * a) * (double)HEVCDL_ACT_SCALE);
  }
}
// fc1 (2048 -> 256) for the split-f16 MFMA of fc_kernel.hip: [k-step of 32][N-tile of 16][hi | lo][64 lanes][8 halves], lane l element j <-> k = 32 * step + 8 * (l >> 4) + j,
// n = 16 * tile + (l & 15); the pairs take exactly the bytes of the f32 matrix, the bias follows as before
static void pack_fc1(const float *w, const float *b, float *dst, float sc)
{
  uint16_t *d16 = (uint16_t *)dst;
  for (int ks = 0; ks < 64; ks++) for (int nt = 0; nt < 16; nt++) for (int l = 0; l < 64; l++) for (int j = 0; j < 8; j++) {
    const int k = 32 * ks + 8 * (l >> 4) + j, n = nt * 16 + (l & 15);
    const float v = w[(size_t)n * 2048 + k] * sc;
    const uint16_t hi = f32_to_f16(v), lo = f32_to_f16(v - f16_to_f32(hi));
    const size_t base = (((size_t)ks * 16 + nt) * 2) * 512;
    d16[base + (size_t)l * 8 + j] = hi; d16[base + 512 + (size_t)l * 8 + j] = lo;
  }
  memcpy(dst + (size_t)2048 * 256, b, 256 * sizeof(float));
}
static void pack_fc(const float *w, const float *b, int out, int in, float *dst)
{ for (int j = 0; j < out; j++) for (int k = 0; k < in; k++) dst[(size_t)k * out + j] = w[(size_t)j * in + k]; memcpy(dst + (size_t)in * out, b, out * sizeof(float)); }

// hevcdl_create has no context to leave a message in: the calling thread's last refusal
static thread_local const char *g_create_error = "";
static hevcdl_status refuse(hevcdl_status s, const char *why) { g_create_error = why; return s; }
extern "C" const char *hevcdl_create_error(void) { return g_create_error; }

extern "C" hevcdl_status hevcdl_create(const hevcdl_config *cfg, const float *weights, size_t n_floats, hevcdl_ctx **out)
{
  g_create_error = "";
  if (!cfg || !out || !weights || cfg->struct_size != sizeof(hevcdl_config)) return HEVCDL_ERR_INVALID_ARG;
  if (n_floats != HEVCDL_WEIGHT_FLOATS) return HEVCDL_ERR_INVALID_ARG;
  if (cfg->width <= 0 || cfg->height <= 0 || (cfg->width & 7) || (cfg->height & 7) || cfg->qp < 0 || cfg->qp > 51 || cfg->max_frames < 1) return HEVCDL_ERR_INVALID_ARG;
  // keys that would change the path are rejected, not ignored
  if ((cfg->bit_depth != 8 && cfg->bit_depth != 10) || cfg->chroma_format != 420 || cfg->ctu_size != 64 || cfg->max_partition_depth != 4 || cfg->tu_log2_min != 2 ||
      cfg->tu_log2_max != 5 || cfg->tu_max_depth_intra != 3 || !HEVCDL_TOOLS_SUPPORTED(cfg->tools) || cfg->lf_beta_offset_div2 < -6 || cfg->lf_beta_offset_div2 > 6 || cfg->lf_tc_offset_div2 < -6 || cfg->lf_tc_offset_div2 > 6 || (cfg->bn_mode != HEVCDL_BN_REFERENCE && cfg->bn_mode != HEVCDL_BN_EVAL) ||
      cfg->boundary_policy != HEVCDL_BOUNDARY_CLAMP || (cfg->cnn_input != HEVCDL_CNN_INPUT_RGB601 && cfg->cnn_input != HEVCDL_CNN_INPUT_LUMA) ||
      (cfg->exec_flags & ~(HEVCDL_EXEC_NO_UNIT_HANDOVER | HEVCDL_EXEC_RD_WIDE | HEVCDL_EXEC_RD_NARROW)) ||
      ((cfg->exec_flags & HEVCDL_EXEC_RD_WIDE) && (cfg->exec_flags & HEVCDL_EXEC_RD_NARROW)))
    return HEVCDL_ERR_UNSUPPORTED;
  { // tiles: uniform spacing, every column at least 4 CTUs wide and every row 1 CTU high (TComPicSym.cpp:380-392), at most 20 x 22 (level 6.2)
    const int cx = (cfg->width + 63) >> 6, cy = (cfg->height + 63) >> 6;
    int cb[21], rb[23];
    if (cfg->tile_columns < 1 || cfg->tile_rows < 1 || cfg->tile_columns > 20 || cfg->tile_rows > 22) return HEVCDL_ERR_INVALID_ARG;
    const int tiled = cfg->tile_columns > 1 || cfg->tile_rows > 1;
    if (hevcdl_tile_bounds(cx, cfg->tile_columns, cfg->tile_uniform_spacing, cfg->tile_column_width, tiled ? 4 : 1, cb) ||
        hevcdl_tile_bounds(cy, cfg->tile_rows, cfg->tile_uniform_spacing, cfg->tile_row_height, 1, rb)) return HEVCDL_ERR_INVALID_ARG;
  }
  if (cfg->wavefront != 0 && cfg->wavefront != 1) return HEVCDL_ERR_INVALID_ARG;
  if (cfg->wavefront && cfg->tile_columns * cfg->tile_rows > 1) return HEVCDL_ERR_UNSUPPORTED;      // as the reference (TAppEncCfg.cpp xCheckParameter: only the high-throughput profile has both)
  // per-picture deblocking parameters: the reference's own condition (TAppEncCfg.cpp:2143) -- that the filter is on is the caller's word at every picture pipeline call
  // (its `deblock` argument), checked there -- and the metric's assert (TEncGOP.cpp:3198-3199)
  if (cfg->deblocking_metric < 0 || cfg->deblocking_metric > 2 || (cfg->lf_offset_in_pps != 0 && cfg->lf_offset_in_pps != 1)) return refuse(HEVCDL_ERR_INVALID_ARG, "deblocking_metric is 0, 1 or 2 and lf_offset_in_pps 0 or 1");
  if (cfg->deblocking_metric != 0 && cfg->lf_offset_in_pps != 0) return refuse(HEVCDL_ERR_INVALID_ARG, "If DeblockingFilterMetric is non-zero then both LoopFilterDisable and LoopFilterOffsetInPPS must be 0");
  if (cfg->deblocking_metric == 1 && (hevcdl_dbk_metric_edges(cfg->width) < 1 || hevcdl_dbk_metric_edges(cfg->height) < 1))
    return refuse(HEVCDL_ERR_INVALID_ARG, "DeblockingFilterMetric 1 needs a coded picture of at least 64 luma samples in either direction (the reference asserts noCol > 1 && noRows > 1)");
  // Slices: the grid the context runs (slice_grid.h) -- a column of row slices for SliceMode 1, the cfg's tiles otherwise; the segment keys are checked there and left out of it
  hevcdl_config grid;
  { const char *why = ""; const hevcdl_status gs = hevcdl_slice_grid(cfg, &grid, &why); if (gs != HEVCDL_OK) return refuse(gs, why); }
  // DeltaQpRD: what the key is refused with (qp_rd.h), in its words
  { const char *why = ""; const hevcdl_status qs = hevcdl_qp_rd_keys(cfg, &why); if (qs != HEVCDL_OK) return refuse(qs, why); }
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || cfg->device >= ndev) return HEVCDL_ERR_NO_DEVICE;
  hevcdl_ctx *ctx = new (std::nothrow) hevcdl_ctx();
  if (!ctx) return HEVCDL_ERR_OOM;
  ctx->cfg = grid; ctx->stream_lf_across_tiles = cfg->lf_across_tiles;
  ctx->slices.mode = cfg->slice_mode; ctx->slices.argument = cfg->slice_mode ? cfg->slice_argument : 0; ctx->slices.lf_across_slices = cfg->slice_mode ? cfg->lf_across_slices != 0 : 1;
  ctx->segments.mode = cfg->slice_segment_mode; ctx->segments.argument = cfg->slice_segment_mode ? cfg->slice_segment_argument : 0;
  cfg = &ctx->cfg;      // the one place the grid comes from
  { // the candidates' constants (hevcdl_qp_rd_candidates gives the same table; one candidate without the key): with the key the cfg's own lambda fields are not read
    ctx->qprd.n = cfg->delta_qp_rd;
    ctx->qprd.count = hevcdl_qp_rd_table(cfg->qp, cfg->delta_qp_rd, cfg->bit_depth, ctx->qprd.cand, &ctx->qprd.frame_lambda);
    if (ctx->qprd.count < 1) { delete ctx; return refuse(HEVCDL_ERR_INVALID_ARG, "DeltaQpRD: no candidate table for this QP and bit depth"); }
  }
  ctx->ctus_x = (cfg->width + 63) >> 6; ctx->ctus_y = (cfg->height + 63) >> 6; ctx->ctus = ctx->ctus_x * ctx->ctus_y;
  ctx->frame_bytes = hevcdl_frame_bytes_bd(cfg->width, cfg->height, cfg->bit_depth);
  hevcdl_tile_bounds(ctx->ctus_x, cfg->tile_columns, cfg->tile_uniform_spacing, cfg->tile_column_width, 1, ctx->col_bd);
  hevcdl_tile_bounds(ctx->ctus_y, cfg->tile_rows, cfg->tile_uniform_spacing, cfg->tile_row_height, 1, ctx->row_bd);
  hipError_t e;
#define CK(call) if ((e = (call)) != hipSuccess) { hevcdl_status s_ = hip_status(e); hevcdl_destroy(ctx); return s_; }
  CK(hipSetDevice(cfg->device));
  { hipDeviceProp_t prop; CK(hipGetDeviceProperties(&prop, cfg->device)); ctx->n_cus = prop.multiProcessorCount; }
  std::vector<float> pk(HEVCDL_W_TOTAL);
  // operand scales (hevcdl_dev.h HEVCDL_ACT_SCALE): weights of a layer by a power of two, activations by HEVCDL_ACT_SCALE; the kernels find 1 / (their product) behind the weights
  const float sc1 = layer_scale(weights + B_C1W, 1200), sc64 = layer_scale(weights + B_C64W, 1200), sc2 = layer_scale(weights + B_C2W, 9 * 32 * 64),
              sc3 = layer_scale(weights + B_C3W, 9 * 64 * 128), scf = layer_scale(weights + B_F1W, 2048 * 256);
  { const float scs[5] = { sc1, sc64, sc2, sc3, scf }; for (int i = 0; i < 8; i++) pk[HEVCDL_W_SCALES + i] = i < 5 ? 1.0f / (scs[i] * HEVCDL_ACT_SCALE) : 0.f; }
  pack_conv5(weights + B_C1W, weights + B_C1B, weights + B_C1G, weights + B_C1BE, pk.data() + HEVCDL_W_C1, sc1);
  pack_conv5(weights + B_C64W, weights + B_C64B, weights + B_C64G, weights + B_C64BE, pk.data() + HEVCDL_W_C64, sc64);
  pack_conv3(weights + B_C2W, weights + B_C2B, weights + B_C2G, weights + B_C2BE, 64, 32, pk.data() + HEVCDL_W_C2, sc2);
  pack_conv3(weights + B_C3W, weights + B_C3B, weights + B_C3G, weights + B_C3BE, 128, 64, pk.data() + HEVCDL_W_C3, sc3);
  if (cfg->bn_mode == HEVCDL_BN_EVAL) {
    fold_bn_eval(weights + B_C1G, weights + B_C1BE, 16, pk.data() + HEVCDL_W_C1 + HEVCDL_W_C5 + 16, pk.data() + HEVCDL_W_C1 + HEVCDL_W_C5 + 32, sc1 * HEVCDL_ACT_SCALE);
    fold_bn_eval(weights + B_C64G, weights + B_C64BE, 16, pk.data() + HEVCDL_W_C64 + HEVCDL_W_C5 + 16, pk.data() + HEVCDL_W_C64 + HEVCDL_W_C5 + 32, sc64 * HEVCDL_ACT_SCALE);
    fold_bn_eval(weights + B_C2G, weights + B_C2BE, 64, pk.data() + HEVCDL_W_C2 + 9 * 32 * 64 + 64, pk.data() + HEVCDL_W_C2 + 9 * 32 * 64 + 128, sc2 * HEVCDL_ACT_SCALE);
    fold_bn_eval(weights + B_C3G, weights + B_C3BE, 128, pk.data() + HEVCDL_W_C3 + 9 * 64 * 128 + 128, pk.data() + HEVCDL_W_C3 + 9 * 64 * 128 + 256, sc3 * HEVCDL_ACT_SCALE);
  }
  pack_fc1(weights + B_F1W, weights + B_F1B, pk.data() + HEVCDL_W_FC1, scf);
  pack_fc(weights + B_F2W, weights + B_F2B, 64, 256, pk.data() + HEVCDL_W_FC2);
  pack_fc(weights + B_F3W, weights + B_F3B, 16, 64, pk.data() + HEVCDL_W_FC3);
  CK(hipMalloc(&ctx->d_flag.p, sizeof(int)));
  CK(hipMalloc(&ctx->rd.d_sched.p, 8192 + 1024 * 192));
  if (cfg->wavefront) { // per (frame, row) 256 bytes, then the queue of claimable rows: 1024 bytes of counters + a ring of one int per frame (rounded up to a power of two)
    ctx->rd.wpp_ring = 64; while (ctx->rd.wpp_ring < cfg->max_frames) ctx->rd.wpp_ring <<= 1;
    ctx->rd.wpp_state_bytes = (size_t)256 * ctx->ctus_y * cfg->max_frames;
    CK(hipMalloc(&ctx->rd.d_wpp.p, ctx->rd.wpp_state_bytes + 1024 + (size_t)4 * ctx->rd.wpp_ring));
  }
  if (cfg->bit_depth > 8) CK(hipMalloc(&ctx->stage.d_yuv8.p, hevcdl_frame_bytes(cfg->width, cfg->height) * (size_t)cfg->max_frames));    // the CNN stage's 8-bit copy
  CK(hipMalloc(&ctx->d_weights.p, sizeof(float) * HEVCDL_W_TOTAL));
  CK(hipMemcpy(ctx->d_weights, pk.data(), sizeof(float) * HEVCDL_W_TOTAL, hipMemcpyHostToDevice));
  for (int b = 0; b < RD_BUILDS; b++)       // the largest of the builds this context can run: the three 8-bit ones, or the 10-bit one
    if ((b == RD_BD10) == (cfg->bit_depth != 8)) ctx->rd.scratch_per_wave = std::max(ctx->rd.scratch_per_wave, rd_builds[b].scratch_bytes());
  { int waves[RD_BUILDS];                  // what the launch plan reads (rd_launch_plan.h)
    for (int b = 0; b < RD_BUILDS; b++) waves[b] = rd_builds[b].waves_per_group();
    ctx->rd.plan = rd_plan_context_of(*cfg, ctx->n_cus, waves); }
  // (the workspace itself -- 1.6 MB per wave -- is sized by the launches: a context that only ever codes a frame or two in the independent form holds a few MB, not the
  // several GB a launch on every CU needs)
  CK(hipFuncSetAttribute((const void *)hevcdl_cnn_ctu_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)hevcdl_cnn_smem_bytes()));
  CK(hipFuncSetAttribute((const void *)hevcdl_fc_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)hevcdl_fc_smem_bytes()));
  { // conv -> head hand-over buffer for one chunk of CTUs, allocated up front so that no step pays for it
    const size_t chunk = (size_t)std::min<long long>((long long)cfg->max_frames * ctx->ctus, 131072);
    CK(hipMalloc(&ctx->d_a3.p, chunk * 4 * 2048 * sizeof(float))); ctx->a3_ctus = chunk;
  }
  for (const RdBuild &b : rd_builds) CK(hipFuncSetAttribute(b.kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)b.smem_bytes()));
#undef CK
  *out = ctx;
  return HEVCDL_OK;
}

extern "C" void hevcdl_destroy(hevcdl_ctx *ctx)
{
  if (!ctx) return;
  hipSetDevice(ctx->cfg.device);
  hipDeviceSynchronize();
  delete ctx;
}

extern "C" const char *hevcdl_last_error(const hevcdl_ctx *ctx) { return ctx ? ctx->err : "null ctx"; }

extern "C" hevcdl_status hevcdl_device_memory(int device, size_t *free_bytes, size_t *total_bytes)
{
  if (!free_bytes || !total_bytes) return HEVCDL_ERR_INVALID_ARG;
  TRY(select_device(device));
  if (hipMemGetInfo(free_bytes, total_bytes) != hipSuccess) { (void)hipGetLastError(); return HEVCDL_ERR_HIP; }
  return HEVCDL_OK;
}
// page-locked host memory for the buffers of the host-pointer entry points (optional: any host memory works, pinned memory copies faster)
extern "C" void *hevcdl_host_alloc(size_t bytes) { void *p = nullptr; return hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocDefault) == hipSuccess ? p : nullptr; }
extern "C" void hevcdl_host_free(void *p) { if (p) hipHostFree(p); }

static hevcdl_status ensure_staging(hevcdl_ctx *ctx)
{
  if (ctx->stage.d_yuv) return HEVCDL_OK;
  const size_t nf = (size_t)ctx->cfg.max_frames;
  Staging &g = ctx->stage;
  return alloc_all(ctx, { want(g.d_recon, ctx->frame_bytes * nf), want(g.d_labels, ctx->labels_bytes(nf)), want(g.d_logits, ctx->logits_bytes(nf)), want(g.d_records, ctx->records_bytes(nf)),
                          want(g.d_stats, sizeof(hevcdl_frame_stats) * nf), want(g.d_yuv, ctx->frame_bytes * nf) }, "staging buffers (cfg.max_frames)");
}

static void prof_begin(hevcdl_ctx *ctx, std::vector<Event> &v, hipStream_t s)
{
  if (!ctx->profile) return;
  Event a, b; hipEventCreate(&a.p); hipEventCreate(&b.p);
  hipEventRecord(a, s); v.push_back(std::move(a)); v.push_back(std::move(b));
}
static void prof_end(hevcdl_ctx *ctx, std::vector<Event> &v, hipStream_t s) { if (ctx->profile) hipEventRecord(v.back(), s); }

static hevcdl_status launch_cnn(hevcdl_ctx *ctx, const void *d_in, int mode, int n_ctus, int clamp, void *d_labels, void *d_logits, hipStream_t s)
{
  hevcdl_cnn_params p;
  p.input = (const uint8_t *)d_in; p.weights = ctx->d_weights; p.labels = (uint8_t *)d_labels; p.logits = (float *)d_logits;
  p.input_mode = mode; p.width = ctx->cfg.width; p.height = ctx->cfg.height; p.ctus_x = ctx->ctus_x; p.ctus_per_frame = ctx->ctus; p.clamp = clamp;
  if (mode == HEVCDL_DEV_INPUT_RGB_CTU) { p.ctus_per_frame = n_ctus > 0 ? n_ctus : 1; p.ctus_x = p.ctus_per_frame; }
  // convolutions per CTU (one workgroup each) -> 32 KB of conv3 output per CTU in HBM -> the fully connected head batched over 16 CTUs
  // per workgroup.  The hand-over buffer holds one chunk of CTUs (<= 4 GiB); larger batches go through it chunk by chunk.
  const size_t chunk = (size_t)std::min<long long>(n_ctus, 131072);
  if (ctx->a3_ctus < chunk) { ctx->d_a3.reset(); ctx->a3_ctus = 0; HIPCHK(hipMalloc(&ctx->d_a3.p, chunk * 4 * 2048 * sizeof(float))); ctx->a3_ctus = chunk; }
  p.a3 = ctx->d_a3; p.n_cus = ctx->n_cus; p.bn_eval = ctx->cfg.bn_mode == HEVCDL_BN_EVAL;
  hevcdl_fc_params f;
  f.logits_in = nullptr;
  f.a3 = ctx->d_a3; f.weights = ctx->d_weights; f.width = p.width; f.height = p.height; f.ctus_x = p.ctus_x; f.ctus_per_frame = p.ctus_per_frame; f.clamp = clamp;
  prof_begin(ctx, ctx->ev_cnn, s);
  for (size_t base = 0; base < (size_t)n_ctus; base += chunk) {
    const int n = (int)std::min<size_t>(chunk, (size_t)n_ctus - base);
    p.ctu_base = (int)base;
    prof_begin(ctx, ctx->ev_conv, s);
    hipLaunchKernelGGL(hevcdl_cnn_ctu_kernel, dim3(n), dim3(256), hevcdl_cnn_smem_bytes(), s, p);
    prof_end(ctx, ctx->ev_conv, s);
    f.n_ctus = n; f.ctu_base = (int)base; f.labels = (uint8_t *)d_labels + base * 16;
    f.logits = d_logits ? (float *)d_logits + base * 64 : nullptr;
#ifdef HEVCDL_CNN_PROF
    f.logits = nullptr;              // the profiling build returns the conv kernel's phase timers through the logits buffer
#endif
    hipLaunchKernelGGL(hevcdl_fc_kernel, dim3((n + 15) / 16), dim3(256), hevcdl_fc_smem_bytes(), s, f);
  }
  prof_end(ctx, ctx->ev_cnn, s);
  return launch_status(ctx);
}

#ifdef HEVCDL_STAGE_TRACE
static unsigned int *g_stage_log = nullptr;
static const size_t STAGE_LOG_WORDS = (12u << 20) + 8;       // rd_kernel.hip STAGE_CAP + header
// words of the log of the last launch (header excluded), copied to dst up to cap_words; returns the number of words the kernel wanted to write
extern "C" size_t hevcdl_stage_trace_fetch(unsigned int *dst, size_t cap_words)
{
  if (!g_stage_log) return 0;
  unsigned int used = 0;
  hipDeviceSynchronize();
  hipMemcpy(&used, g_stage_log, 4, hipMemcpyDeviceToHost);
  size_t n = used; if (n > (size_t)(12u << 20)) n = (size_t)(12u << 20); if (n > cap_words) n = cap_words;
  if (n) hipMemcpy(dst, g_stage_log + 2, n * 4, hipMemcpyDeviceToHost);
  return used;
}
#endif

// the decision kernel's workspace: grown to `need` bytes (a launch's one block per wave of every workgroup, or hevcdl_reserve_workspace's largest); what: the message of a refusal
static hevcdl_status ensure_scratch(hevcdl_ctx *ctx, size_t need, hipStream_t s, const char *what)
{
  RdWorkspace &w = ctx->rd;
  if (need <= w.scratch_bytes) return HEVCDL_OK;
  if (w.d_scratch) { HIPCHK(hipStreamSynchronize(s)); w.d_scratch.reset(); w.scratch_bytes = 0; }
  const hipError_t e = hipMalloc(&w.d_scratch.p, need);
  if (e != hipSuccess) { (void)hipGetLastError(); return fail(ctx, HEVCDL_ERR_OOM, what, e); }
  w.scratch_bytes = need;
  return HEVCDL_OK;
}

// One decision launch: the plan (rd_launch_plan.h: build, form, workgroups), the areas it wants cleared and seeded, the workspace, the launch, the report.
static hevcdl_status launch_rd(hevcdl_ctx *ctx, const void *d_yuv, int n_frames, const void *d_labels, void *d_records, void *d_recon, void *d_stats, hipStream_t s,
                               int ctu_begin = 0, int ctu_end = -1, const void *d_cabac_in = nullptr, void *d_cabac_out = nullptr,
                               int tile_begin = 0, int tile_count = -1, int session_frame = -1, const hevcdl_qp_rd_candidate *cand = nullptr)
{
  RdWorkspace &w = ctx->rd;
  const RdLaunchArgs a = { n_frames, ctu_begin, ctu_end, d_cabac_in != nullptr, d_cabac_out != nullptr, tile_begin, tile_count, session_frame };
  RdLaunchPlan pl = rd_launch_plan(w.plan, a);
  if (pl.status) return fail(ctx, pl.status, "WaveFrontSynchro: whole-frame launches or the per-CTU session (no tile range, no CTU range of several frames)");
  hevcdl_rd_params p;
  memset(&p, 0, sizeof p);
  p.ctu_begin = ctu_begin; p.ctu_end = ctu_end < 0 ? ctx->ctus : ctu_end; p.cabac_in = (const unsigned char *)d_cabac_in; p.cabac_out = (unsigned char *)d_cabac_out;
  p.yuv = (const uint8_t *)d_yuv; p.labels = (const uint8_t *)d_labels; p.records = (unsigned char *)d_records; p.recon = (uint8_t *)d_recon;
  p.stats = (unsigned char *)d_stats; p.scratch_per_wave = w.scratch_per_wave;
  p.width = ctx->cfg.width; p.height = ctx->cfg.height; p.ctus_x = ctx->ctus_x; p.ctus_y = ctx->ctus_y; p.n_frames = n_frames;
  p.tile_cols = ctx->cfg.tile_columns; p.tile_rows = ctx->cfg.tile_rows;
  memcpy(p.col_bd, ctx->col_bd, sizeof p.col_bd); memcpy(p.row_bd, ctx->row_bd, sizeof p.row_bd);
  p.tile_begin = tile_begin; p.tile_count = pl.tile_count;
  p.wpp = pl.wpp; p.wpp_masters = pl.wpp_masters; p.master_groups = pl.master_groups; p.migrate = pl.migrate; p.remote = pl.remote; p.sched = w.d_sched;
  if (pl.wpp) { // the rows' contexts and the queue of claimable rows: the session's stay from call to call, a whole-frame launch starts from cleared ones
    p.wpp_state = pl.wpp_session ? w.d_wpp + (size_t)256 * ctx->ctus_y * session_frame : w.d_wpp.p; p.wpp_queue = w.d_wpp + w.wpp_state_bytes; p.wpp_ring = w.wpp_ring;
    if (!pl.wpp_session) {
      HIPCHK(hipMemsetAsync(w.d_wpp, 0, (size_t)256 * ctx->ctus_y * n_frames, s));
      HIPCHK(hipMemsetAsync(p.wpp_queue, 0, 1024 + (size_t)4 * w.wpp_ring, s));
    }
  }
  if (d_stats) HIPCHK(hipMemsetAsync(d_stats, 0, sizeof(hevcdl_frame_stats) * (size_t)n_frames, s));     // the tile waves of a frame add into its entry
  p.k.lambda = ctx->cfg.lambda; p.k.sqrt_lambda = ctx->cfg.sqrt_lambda; p.k.chroma_weight = ctx->cfg.chroma_weight; p.k.lambda_chroma = ctx->cfg.lambda_chroma;
  memcpy(p.k.err_scale, ctx->cfg.err_scale, sizeof p.k.err_scale);
  p.k.sbh_rd_factor[0] = ctx->cfg.sbh_rd_factor[0]; p.k.sbh_rd_factor[1] = ctx->cfg.sbh_rd_factor[1];
  p.k.qp = ctx->cfg.qp; p.k.qp_chroma = ctx->cfg.qp_chroma; p.k.tools = (int)ctx->cfg.tools;
  if (cand) { // DeltaQpRD: this launch codes one candidate of the QP search -- its constants in the cfg's place (setUpLambda(lambda[idx], iQP[idx]), TEncSlice.cpp:632)
    p.k.lambda = cand->lambda; p.k.sqrt_lambda = cand->sqrt_lambda; p.k.chroma_weight = cand->chroma_weight; p.k.lambda_chroma = cand->lambda_chroma;
    memcpy(p.k.err_scale, cand->err_scale, sizeof p.k.err_scale);
    p.k.sbh_rd_factor[0] = cand->sbh_rd_factor[0]; p.k.sbh_rd_factor[1] = cand->sbh_rd_factor[1]; p.k.qp = cand->qp; p.k.qp_chroma = cand->qp_chroma;
  }
#ifdef HEVCDL_STAGE_TRACE
  // stage-trace build (tests/test_rd_gpu.py, lib/libhevcdl_hip_trace.so): the kernel logs its search events here; hevcdl_stage_trace_fetch reads them
  if (!g_stage_log) HIPCHK(hipMalloc(&g_stage_log, STAGE_LOG_WORDS * 4));
  HIPCHK(hipMemsetAsync(g_stage_log, 0, 8, s)); p.dbgbuf = g_stage_log;
#endif
#if defined(HEVCDL_KERNEL_PROF) || defined(HEVCDL_KERNEL_DEBUG)
  unsigned int *d_dbg = nullptr;               // instrumented builds only (tools/phase_profile.py): in-kernel timers / traces come back through this buffer
  HIPCHK(hipMalloc(&d_dbg, 8004 * 4)); HIPCHK(hipMemset(d_dbg, 0, 8004 * 4)); p.dbgbuf = d_dbg;
#endif
  if (pl.sched_clear) HIPCHK(hipMemsetAsync(w.d_sched, 0, pl.sched_clear, s));
  if (pl.migrate) { // unit hand-over: every workgroup's share of the units behind the counters
    std::vector<int> init(16 + pl.groups, 0);
    const int groups = pl.groups, base = pl.n_units / groups, extra = pl.n_units % groups;
    for (int g = 0; g < groups; g++) { const int e = (g * extra + groups - 1) / groups; init[16 + g] = base + ((e < extra && (e * groups) / extra == g) ? 1 : 0); }    // the kernel's dealing
    HIPCHK(hipMemcpyAsync(w.d_sched, init.data(), init.size() * sizeof(int), hipMemcpyHostToDevice, s));      // pageable source: the copy is staged before the call returns
  }
  const RdBuild &rd = rd_builds[pl.build];
  TRY(ensure_scratch(ctx, w.scratch_per_wave * pl.scratch_blocks(), s, "decision-kernel workspace (1.6 MB per wave of the launch)"));
  p.scratch = w.d_scratch;
  const int threads = 64 * pl.waves;
  const size_t smem = rd.smem_bytes();
  prof_begin(ctx, ctx->ev_rd, s);
  bool launched = false;
  void *args[] = { &p };
  if (pl.cooperative()) { // workgroups that wait for each other: a cooperative launch, which the runtime only accepts when the whole grid can be resident at once
    if (hipLaunchCooperativeKernel(rd.kernel, dim3(pl.grid), dim3(threads), args, smem, s) == hipSuccess) launched = true;
    else {
      (void)hipGetLastError(); p.migrate = pl.migrate = 0; p.remote = pl.remote = 0; pl.grid = pl.groups;
      if (pl.wpp == 1) { prof_end(ctx, ctx->ev_rd, s); ctx->cfg.exec_flags |= HEVCDL_EXEC_NO_UNIT_HANDOVER; w.plan.exec_flags = ctx->cfg.exec_flags;      // rows on waves of their own need co-residency: this context walks a frame's rows on one wave from now on
                         return launch_rd(ctx, d_yuv, n_frames, d_labels, d_records, d_recon, d_stats, s, ctu_begin, ctu_end, d_cabac_in, d_cabac_out, tile_begin, tile_count, -1, cand); }
    }
  }
  if (!launched) (void)hipLaunchKernel(rd.kernel, dim3(pl.groups), dim3(threads), args, smem, s);      // (an error is picked up below, as after every launch)
  prof_end(ctx, ctx->ev_rd, s);
  HIPCHK(hipGetLastError());
  rd_launch_report(pl, ctx->last_rd, sizeof ctx->last_rd);
#if defined(HEVCDL_KERNEL_PROF) || defined(HEVCDL_KERNEL_DEBUG)
  {
    std::vector<unsigned int> hb(8004); hipDeviceSynchronize(); hipMemcpy(hb.data(), d_dbg, 8004 * 4, hipMemcpyDeviceToHost);
#ifdef HEVCDL_KERNEL_PROF
    for (unsigned i = 0; i < hb[0] && i < 64; i++) { // accumulators of the kernel's timers: cycles in the low 40 bits, calls above -> kilocycles, calls
      const unsigned long long v = (unsigned long long)hb[2 + 2 * i] | ((unsigned long long)hb[3 + 2 * i] << 32);
      printf("DBGV %u %u\n", (unsigned)((v & 0xffffffffffull) >> 10), (unsigned)(v >> 40));
    }
#else
    for (unsigned i = 0; i < hb[0] && i < 3990; i++) printf("DBGV %u %u\n", hb[1 + 2 * i], hb[2 + 2 * i]);
#endif
    fflush(stdout); hipFree(d_dbg);
  }
#endif
  return HEVCDL_OK;
}

static hevcdl_status check_frames(hevcdl_ctx *ctx, int n_frames)
{
  if (!ctx) return HEVCDL_ERR_INVALID_ARG;
  if (n_frames < 0 || n_frames > ctx->cfg.max_frames) return fail(ctx, HEVCDL_ERR_INVALID_ARG, "n_frames out of range (cfg.max_frames)");
  hipError_t e = hipSetDevice(ctx->cfg.device);
  if (e != hipSuccess) return fail(ctx, HEVCDL_ERR_HIP, "hipSetDevice", e);
  return HEVCDL_OK;
}

// the opening of an entry that takes n_frames pictures: a bad context or count is its status, no pictures are nothing to do
#define FRAMES_OR_RETURN(ctx, n) do { TRY(check_frames(ctx, n)); if ((n) == 0) return HEVCDL_OK; } while (0)

// ---- DeltaQpRD: TEncSlice::precompressSlice (TEncSlice.cpp:572-661) for a batch of pictures ----------------------------------------------------------------------------
// the trial set and the rows, all or nothing, for max_frames pictures
static hevcdl_status ensure_qp_rd_trial(hevcdl_ctx *ctx)
{
  QpRd &g = ctx->qprd;
  if (g.d_rows) return HEVCDL_OK;
  const size_t nf = (size_t)ctx->cfg.max_frames, bytes = ctx->records_bytes(nf) + ctx->frame_bytes * nf + sizeof(hevcdl_frame_stats) * nf + sizeof(hevcdl_qp_rd_row) * nf;
  TRY(alloc_all(ctx, { want(g.d_records, ctx->records_bytes(nf)), want(g.d_recon, ctx->frame_bytes * nf), want(g.d_stats, sizeof(hevcdl_frame_stats) * nf), want(g.d_rows, sizeof(hevcdl_qp_rd_row) * nf) },
                "DeltaQpRD trial set (records, reconstruction and statistics of cfg.max_frames pictures)"));
  g.trial_bytes = bytes;
  return HEVCDL_OK;
}

// 2N+1 decision launches over the same frames and labels, each followed by the sum launch and (behind the first) the keep launch, all in order on `s`.  Our search is
// deterministic: the trial that wins is what the reference's final compressSlice at the winning QP (TEncGOP.cpp, behind precompressSlice) would produce again, so it is kept.
static hevcdl_status qp_rd_search(hevcdl_ctx *ctx, const void *d_yuv, int n_frames, const void *d_labels, void *d_records, void *d_recon, void *d_stats, hipStream_t s)
{
  QpRd &g = ctx->qprd;
  if (((uintptr_t)d_records & 15) || ((uintptr_t)d_recon & 15) || ((uintptr_t)d_stats & 7)) return fail(ctx, HEVCDL_ERR_INVALID_ARG, "DeltaQpRD: records and reconstruction must be 16-byte aligned, statistics 8-byte aligned");
  TRY(ensure_qp_rd_trial(ctx));
  g.last_frames = 0; g.h_rows.clear(); g.ev_sum.clear(); g.ev_keep.clear();
  hevcdl_qp_rd_sum_params sp; memset(&sp, 0, sizeof sp);
  sp.rows = g.d_rows; sp.ctus_per_frame = ctx->ctus; sp.n_frames = n_frames; sp.frame_lambda = g.frame_lambda;
  hevcdl_qp_rd_keep_params kp; memset(&kp, 0, sizeof kp);
  kp.src_records = g.d_records; kp.src_recon = g.d_recon; kp.src_stats = d_stats ? g.d_stats.p : nullptr;
  kp.dst_records = (unsigned char *)d_records; kp.dst_recon = (unsigned char *)d_recon; kp.dst_stats = (unsigned char *)d_stats;
  kp.rows = g.d_rows; kp.rec16 = ctx->records_bytes(1) / 16; kp.pic16 = kp.rec16 + ctx->frame_bytes / 16; kp.n_frames = n_frames;
  for (int idx = 0; idx < g.count; idx++) {
    const bool own = idx == 0;      // candidate 0 writes into the call's own buffers, the others into the trial set
    TRY(launch_rd(ctx, d_yuv, n_frames, d_labels, own ? d_records : (void *)g.d_records.p, own ? d_recon : (void *)g.d_recon.p, d_stats ? (own ? d_stats : (void *)g.d_stats.p) : nullptr, s,
                  0, -1, nullptr, nullptr, 0, -1, -1, &g.cand[idx]));
    sp.records = own ? (const unsigned char *)d_records : g.d_records.p; sp.idx = idx;
    prof_begin(ctx, g.ev_sum, s); hevcdl_launch_qp_rd_sum(&sp, s); prof_end(ctx, g.ev_sum, s); g.launches++;
    if (!own) { prof_begin(ctx, g.ev_keep, s); hevcdl_launch_qp_rd_keep(&kp, s); prof_end(ctx, g.ev_keep, s); g.launches++; }
    HIPCHK(hipGetLastError());
  }
  g.last_frames = n_frames;
  return HEVCDL_OK;
}

// ---- a QP per picture: one decision launch per run of equal QP (frame_qp.h) ----------------------------------------------------------------------------------------------
// the two sorted sets and the permutations, all or nothing, for max_frames pictures
static hevcdl_status ensure_frame_qp_sets(hevcdl_ctx *ctx)
{
  FrameQp &g = ctx->fqp;
  if (g.d_perm) return HEVCDL_OK;
  const size_t nf = (size_t)ctx->cfg.max_frames;
  TRY(alloc_all(ctx, { want(g.d_records, ctx->records_bytes(nf)), want(g.d_yuv, ctx->frame_bytes * nf), want(g.d_recon, ctx->frame_bytes * nf), want(g.d_labels, ctx->labels_bytes(nf)),
                       want(g.d_stats, sizeof(hevcdl_frame_stats) * nf), want(g.d_perm, sizeof(int) * nf) },
                "sorted picture sets of a QP per picture (originals, labels, records, reconstruction and statistics of cfg.max_frames pictures)"));
  g.set_bytes = ctx->records_bytes(nf) + 2 * ctx->frame_bytes * nf + ctx->labels_bytes(nf) + sizeof(hevcdl_frame_stats) * nf + sizeof(int) * nf;
  return HEVCDL_OK;
}

// the QP of picture i of a call: the list's, past its end the context's
static int frame_qp_at(const hevcdl_ctx *ctx, int i) { return i < (int)ctx->fqp.list.size() ? ctx->fqp.list[(size_t)i] : ctx->cfg.qp; }

static hevcdl_status frame_qp_decide(hevcdl_ctx *ctx, const void *d_yuv, int n_frames, const void *d_labels, void *d_records, void *d_recon, void *d_stats, hipStream_t s)
{
  FrameQp &g = ctx->fqp;
  g.used.resize((size_t)n_frames);
  for (int i = 0; i < n_frames; i++) g.used[(size_t)i] = frame_qp_at(ctx, i);
  g.rd_launches = 0; g.permute_launches = 0; g.ev_permute.clear();
  std::vector<hevcdl_qp_run> runs((size_t)std::min(n_frames, 52));
  int n_runs = hevcdl_frame_qp_contiguous_runs(g.used.data(), n_frames, runs.data());
  if (n_runs < 0) return fail(ctx, HEVCDL_ERR_INVALID_ARG, HEVCDL_FRAME_QP_REFUSE_RANGE);
  const bool permuted = n_runs == 0;
  const unsigned char *yuv = (const unsigned char *)d_yuv, *labels = (const unsigned char *)d_labels;
  unsigned char *records = (unsigned char *)d_records, *recon = (unsigned char *)d_recon, *stats = (unsigned char *)d_stats;
  hevcdl_frame_permute_params pp; memset(&pp, 0, sizeof pp);
  if (permuted) { // bring the pictures together by QP: the runs are those of the sorted order, the launches read and write the sorted sets
    TRY(ensure_frame_qp_sets(ctx));
    g.perm.resize((size_t)n_frames);
    n_runs = hevcdl_frame_qp_group(g.used.data(), n_frames, g.perm.data(), runs.data(), nullptr);
    HIPCHK(hipMemcpyAsync(g.d_perm, g.perm.data(), sizeof(int) * (size_t)n_frames, hipMemcpyHostToDevice, s));
    pp.perm = g.d_perm; pp.n_frames = n_frames; pp.scatter = 0; pp.n_ranges = 2;
    pp.r[0].src = yuv; pp.r[0].dst = g.d_yuv; pp.r[0].bytes = ctx->frame_bytes;
    pp.r[1].src = labels; pp.r[1].dst = g.d_labels; pp.r[1].bytes = ctx->labels_bytes(1);
    prof_begin(ctx, g.ev_permute, s); hevcdl_launch_frame_permute(&pp, s); prof_end(ctx, g.ev_permute, s); g.permute_launches++;
    HIPCHK(hipGetLastError());
    yuv = g.d_yuv; labels = g.d_labels; records = g.d_records; recon = g.d_recon; stats = d_stats ? g.d_stats.p : nullptr;
  }
  for (int r = 0; r < n_runs; r++) { // the plan of every launch is rd_launch_plan's for the run's frame count; its constants are the run's lambda family
    hevcdl_qp_rd_candidate fam;
    hevcdl_frame_qp_family(runs[(size_t)r].qp, ctx->cfg.bit_depth, g.lambda_modifier, &fam);
    const size_t f0 = (size_t)runs[(size_t)r].first;
    TRY(launch_rd(ctx, yuv + ctx->frame_bytes * f0, runs[(size_t)r].count, labels + ctx->labels_bytes(f0), records + ctx->records_bytes(f0), recon + ctx->frame_bytes * f0,
                  stats ? stats + sizeof(hevcdl_frame_stats) * f0 : nullptr, s, 0, -1, nullptr, nullptr, 0, -1, -1, &fam));
    g.rd_launches++;
  }
  if (permuted) { // back to picture order: sorted place i goes to picture perm[i]
    pp.scatter = 1; pp.n_ranges = d_stats ? 3 : 2;
    pp.r[0].src = g.d_records; pp.r[0].dst = (unsigned char *)d_records; pp.r[0].bytes = ctx->records_bytes(1);
    pp.r[1].src = g.d_recon; pp.r[1].dst = (unsigned char *)d_recon; pp.r[1].bytes = ctx->frame_bytes;
    pp.r[2].src = g.d_stats; pp.r[2].dst = (unsigned char *)d_stats; pp.r[2].bytes = sizeof(hevcdl_frame_stats);
    prof_begin(ctx, g.ev_permute, s); hevcdl_launch_frame_permute(&pp, s); prof_end(ctx, g.ev_permute, s); g.permute_launches++;
    HIPCHK(hipGetLastError());
  }
  return HEVCDL_OK;
}

// caller-supplied labels (device copy): boundary clamp + quadtree consistency in place; labels above 3 -> HEVCDL_ERR_INVALID_ARG
extern "C" hevcdl_status hevcdl_clamp_labels_dev(hevcdl_ctx *ctx, void *d_labels, int n_frames, void *stream)
{
  FRAMES_OR_RETURN(ctx, n_frames);
  if (!d_labels) return fail(ctx, HEVCDL_ERR_INVALID_ARG, "null device pointer");
  const int n = n_frames * ctx->ctus;
  HIPCHK(hipMemsetAsync(ctx->d_flag, 0, sizeof(int), (hipStream_t)stream));
  hipLaunchKernelGGL(hevcdl_clamp_labels_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, (uint8_t *)d_labels, n, ctx->ctus, ctx->ctus_x, ctx->cfg.width, ctx->cfg.height, ctx->d_flag.p);
  int bad = 0;
  HIPCHK(hipMemcpyAsync(&bad, ctx->d_flag, sizeof(int), hipMemcpyDeviceToHost, (hipStream_t)stream));
  HIPCHK(hipStreamSynchronize((hipStream_t)stream));
  if (bad) return fail(ctx, HEVCDL_ERR_INVALID_ARG, "labels: depth above 3");
  return HEVCDL_OK;
}

extern "C" hevcdl_status hevcdl_predict_depth_dev(hevcdl_ctx *ctx, const void *d_yuv, int n_frames, void *d_labels, void *d_logits_opt, void *stream)
{
  FRAMES_OR_RETURN(ctx, n_frames);
  if (!d_yuv || !d_labels) return fail(ctx, HEVCDL_ERR_INVALID_ARG, "null device pointer");
  if (ctx->cfg.bit_depth > 8) { // the CNN stage is defined on 8-bit pictures: the top 8 bits of every sample
    TRY(lazy_alloc(ctx, ctx->stage.d_yuv8, hevcdl_frame_bytes(ctx->cfg.width, ctx->cfg.height) * (size_t)ctx->cfg.max_frames, "8-bit pictures of the CNN stage (cfg.max_frames)"));
    const size_t n = hevcdl_frame_bytes(ctx->cfg.width, ctx->cfg.height) * (size_t)n_frames;
    hipLaunchKernelGGL(hevcdl_narrow_samples_kernel, dim3(2048), dim3(256), 0, (hipStream_t)stream, (const uint16_t *)d_yuv, ctx->stage.d_yuv8.p, n, ctx->cfg.bit_depth - 8);
    d_yuv = ctx->stage.d_yuv8.p;
  }
  return launch_cnn(ctx, d_yuv, ctx->cfg.cnn_input == HEVCDL_CNN_INPUT_LUMA ? HEVCDL_DEV_INPUT_LUMA : HEVCDL_DEV_INPUT_RGB601,
                    n_frames * ctx->ctus, 1, d_labels, d_logits_opt, (hipStream_t)stream);
}

extern "C" hevcdl_status hevcdl_compress_frames_dev(hevcdl_ctx *ctx, const void *d_yuv, int n_frames, const void *d_labels,
                                                    void *d_records, void *d_recon, void *d_stats, void *stream)
{
  FRAMES_OR_RETURN(ctx, n_frames);
  if (!d_yuv || !d_labels || !d_records || !d_recon) return fail(ctx, HEVCDL_ERR_INVALID_ARG, "null device pointer");
  if (ctx->qprd.n) return qp_rd_search(ctx, d_yuv, n_frames, d_labels, d_records, d_recon, d_stats, (hipStream_t)stream);
  if (ctx->fqp.active()) return frame_qp_decide(ctx, d_yuv, n_frames, d_labels, d_records, d_recon, d_stats, (hipStream_t)stream);
  ctx->fqp.used.assign((size_t)n_frames, ctx->cfg.qp); ctx->fqp.rd_launches = 1; ctx->fqp.permute_launches = 0;
  return launch_rd(ctx, d_yuv, n_frames, d_labels, d_records, d_recon, d_stats, (hipStream_t)stream);
}

extern "C" hevcdl_status hevcdl_compress_tiles_dev(hevcdl_ctx *ctx, const void *d_yuv, int n_frames, const void *d_labels, void *d_records, void *d_recon, void *d_stats,
                                                   int tile_begin, int tile_count, void *stream)
{
  TRY(check_frames(ctx, n_frames));
  if (ctx->qprd.n) return fail(ctx, HEVCDL_ERR_UNSUPPORTED, "compress_tiles: DeltaQpRD picks a QP per picture from the sums of ALL its tiles; a range of tiles cannot (use hevcdl_compress_frames_dev)");
  if (ctx->fqp.active()) return fail(ctx, HEVCDL_ERR_UNSUPPORTED, HEVCDL_FRAME_QP_REFUSE_TILES);
  if (tile_begin < 0 || tile_count < 0 || tile_begin + tile_count > ctx->cfg.tile_columns * ctx->cfg.tile_rows) return fail(ctx, HEVCDL_ERR_INVALID_ARG, "tile range outside the tile grid");
  if (n_frames == 0 || tile_count == 0) return HEVCDL_OK;
  if (!d_yuv || !d_labels || !d_records || !d_recon) return fail(ctx, HEVCDL_ERR_INVALID_ARG, "null device pointer");
  return launch_rd(ctx, d_yuv, n_frames, d_labels, d_records, d_recon, d_stats, (hipStream_t)stream, 0, -1, nullptr, nullptr, tile_begin, tile_count);
}

extern "C" hevcdl_status hevcdl_encode_frames_dev(hevcdl_ctx *ctx, const void *d_yuv, int n_frames, void *d_labels,
                                                  void *d_records, void *d_recon, void *d_stats, void *stream)
{
  TRY(hevcdl_predict_depth_dev(ctx, d_yuv, n_frames, d_labels, nullptr, stream));
  return hevcdl_compress_frames_dev(ctx, d_yuv, n_frames, d_labels, d_records, d_recon, d_stats, stream);
}

// hevcdl_planes -> the packed planar frames of the staging buffer (row by row: hipMemcpy2D; 8-bit samples in 16-bit containers are narrowed on the device)
static hevcdl_status upload_planes(hevcdl_ctx *ctx, const hevcdl_planes *src, int n_frames)
{
  if (!src || !src->plane[0] || !src->plane[1] || !src->plane[2]) return fail(ctx, HEVCDL_ERR_INVALID_ARG, "null plane pointer");
  const int native = ctx->cfg.bit_depth > 8 ? 2 : 1, sb = src->sample_bytes;
  if (sb != native && !(sb == 2 && native == 1)) return fail(ctx, HEVCDL_ERR_INVALID_ARG, "sample_bytes does not fit the context's bit depth");
  const int w = ctx->cfg.width, h = ctx->cfg.height;
  for (int c = 0; c < 3; c++) if (src->row_stride[c] < (size_t)(c ? w / 2 : w) * sb) return fail(ctx, HEVCDL_ERR_INVALID_ARG, "row stride smaller than a row");
  unsigned char *dst = (unsigned char *)ctx->stage.d_yuv;
  if (sb != native) {
    TRY(lazy_alloc(ctx, ctx->stage.d_wide, 2 * ctx->frame_bytes * (size_t)ctx->cfg.max_frames, "16-bit staging of the planes (cfg.max_frames)"));
    dst = ctx->stage.d_wide;
  }
  const size_t fb = ctx->frame_bytes / native * sb, off[3] = { 0, (size_t)w * h * sb, (size_t)w * h * sb + (size_t)(w / 2) * (h / 2) * sb };
  for (int f = 0; f < n_frames; f++) for (int c = 0; c < 3; c++) {
    const size_t rw = (size_t)(c ? w / 2 : w) * sb; const int rows = c ? h / 2 : h;
    HIPCHK(hipMemcpy2D(dst + (size_t)f * fb + off[c], rw, (const unsigned char *)src->plane[c] + (size_t)f * src->frame_stride[c], src->row_stride[c], rw, rows, hipMemcpyHostToDevice));
  }
  if (sb != native) {
    hipLaunchKernelGGL(hevcdl_narrow_samples_kernel, dim3(2048), dim3(256), 0, (hipStream_t)nullptr, (const uint16_t *)ctx->stage.d_wide.p, ctx->stage.d_yuv.p, ctx->frame_bytes * (size_t)n_frames, 0);
    HIPCHK(hipGetLastError());
  }
  return HEVCDL_OK;
}

static hevcdl_status predict_depth_staged(hevcdl_ctx *ctx, int n_frames, uint8_t *labels, float *logits_opt);
extern "C" hevcdl_status hevcdl_predict_depth(hevcdl_ctx *ctx, const uint8_t *yuv, int n_frames, uint8_t *labels, float *logits_opt)
{
  FRAMES_OR_RETURN(ctx, n_frames);
  if (!yuv || !labels) return fail(ctx, HEVCDL_ERR_INVALID_ARG, "null pointer");
  TRY(ensure_staging(ctx));
  HIPCHK(hipMemcpy(ctx->stage.d_yuv, yuv, ctx->frame_bytes * n_frames, hipMemcpyHostToDevice));
  return predict_depth_staged(ctx, n_frames, labels, logits_opt);
}
extern "C" hevcdl_status hevcdl_predict_depth_planes(hevcdl_ctx *ctx, const hevcdl_planes *src, int n_frames, uint8_t *labels, float *logits_opt)
{
  FRAMES_OR_RETURN(ctx, n_frames);
  if (!labels) return fail(ctx, HEVCDL_ERR_INVALID_ARG, "null pointer");
  TRY(ensure_staging(ctx));
  TRY(upload_planes(ctx, src, n_frames));
  return predict_depth_staged(ctx, n_frames, labels, logits_opt);
}
static hevcdl_status predict_depth_staged(hevcdl_ctx *ctx, int n_frames, uint8_t *labels, float *logits_opt)
{
  TRY(hevcdl_predict_depth_dev(ctx, ctx->stage.d_yuv, n_frames, ctx->stage.d_labels, logits_opt ? ctx->stage.d_logits.p : nullptr, nullptr));
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(hipMemcpy(labels, ctx->stage.d_labels, ctx->labels_bytes(n_frames), hipMemcpyDeviceToHost));
  if (logits_opt) HIPCHK(hipMemcpy(logits_opt, ctx->stage.d_logits, ctx->logits_bytes(n_frames), hipMemcpyDeviceToHost));
  return HEVCDL_OK;
}

extern "C" hevcdl_status hevcdl_predict_depth_rgb(hevcdl_ctx *ctx, const uint8_t *ctu_rgb, int n_ctus, uint8_t *labels, float *logits_opt)
{
  if (!ctx) return HEVCDL_ERR_INVALID_ARG;
  if (n_ctus < 0) return fail(ctx, HEVCDL_ERR_INVALID_ARG, "n_ctus < 0");
  if (n_ctus == 0) return HEVCDL_OK;
  if (!ctu_rgb || !labels) return fail(ctx, HEVCDL_ERR_INVALID_ARG, "null pointer");
  HIPCHK(hipSetDevice(ctx->cfg.device));
  const size_t n = (size_t)n_ctus;
  DevBuf<uint8_t> d_in, d_lab; DevBuf<float> d_lg;
  TRY(alloc_all(ctx, { want(d_in, n * CTU_RGB_BYTES), want(d_lab, n * LABELS_PER_CTU), want(d_lg, n * LOGITS_PER_CTU * sizeof(float)) }, "predict_depth_rgb buffers"));
  const hipError_t e0 = hipMemcpy(d_in, ctu_rgb, n * CTU_RGB_BYTES, hipMemcpyHostToDevice);
  if (e0 != hipSuccess) return hip_fail(ctx, "predict_depth_rgb buffers", e0);
  TRY(launch_cnn(ctx, d_in, HEVCDL_DEV_INPUT_RGB_CTU, n_ctus, 0, d_lab, d_lg, nullptr));
  TRY(sync_or_fail(ctx, "cnn kernel"));
  hipMemcpy(labels, d_lab, n * LABELS_PER_CTU, hipMemcpyDeviceToHost);
  if (logits_opt) hipMemcpy(logits_opt, d_lg, n * LOGITS_PER_CTU * sizeof(float), hipMemcpyDeviceToHost);
  return HEVCDL_OK;
}

extern "C" const char *hevcdl_last_rd_launch(const hevcdl_ctx *ctx) { return ctx ? ctx->last_rd : ""; }

// The decision kernel's workspace (1.6 MB per wave of a launch) is allocated by the first launch that needs it and grown when a later one needs more: a context that
// only ever codes a frame in the independent form holds megabytes, a launch on every CU 3.4 GB (4.3 GB for the ten-wave build).  A caller that wants to learn
// about a lack of device memory BEFORE its first pictures are in flight reserves the largest workspace any launch of this context can ask for -- launches of 1 ..
// max_frames frames, as the launch plan sizes them (rd_launch_plan.h, rd_largest_scratch_blocks) -- and gets HEVCDL_ERR_OOM here.
extern "C" hevcdl_status hevcdl_reserve_workspace(hevcdl_ctx *ctx)
{
  if (!ctx) return HEVCDL_ERR_INVALID_ARG;
  HIPCHK(hipSetDevice(ctx->cfg.device));
  if (ctx->qprd.n) TRY(ensure_qp_rd_trial(ctx));      // DeltaQpRD: the trial set is part of what the decisions need
  if (!ctx->fqp.list.empty()) TRY(ensure_frame_qp_sets(ctx));      // a QP per picture: so are the sorted sets (a list that is contiguous runs never touches them)
  const size_t need = ctx->rd.scratch_per_wave * rd_largest_scratch_blocks(ctx->rd.plan);
  if (need <= ctx->rd.scratch_bytes) return HEVCDL_OK;
  HIPCHK(hipDeviceSynchronize());
  return ensure_scratch(ctx, need, nullptr, "decision-kernel workspace (1.6 MB per wave of the largest launch)");
}

extern "C" hevcdl_status hevcdl_labels_from_logits(hevcdl_ctx *ctx, const float *logits, int n_ctus, int clamp, uint8_t *labels)
{
  if (!ctx) return HEVCDL_ERR_INVALID_ARG;
  if (n_ctus < 0) return fail(ctx, HEVCDL_ERR_INVALID_ARG, "n_ctus < 0");
  if (n_ctus == 0) return HEVCDL_OK;
  if (!logits || !labels) return fail(ctx, HEVCDL_ERR_INVALID_ARG, "null pointer");
  HIPCHK(hipSetDevice(ctx->cfg.device));
  const size_t n = (size_t)n_ctus;
  DevBuf<uint8_t> d_lab; DevBuf<float> d_lg;
  TRY(alloc_all(ctx, { want(d_lab, n * LABELS_PER_CTU), want(d_lg, n * LOGITS_PER_CTU * sizeof(float)) }, "labels_from_logits buffers"));
  const hipError_t e0 = hipMemcpy(d_lg, logits, n * LOGITS_PER_CTU * sizeof(float), hipMemcpyHostToDevice);
  if (e0 != hipSuccess) return hip_fail(ctx, "labels_from_logits buffers", e0);
  hevcdl_fc_params f;
  f.a3 = nullptr; f.weights = ctx->d_weights; f.labels = d_lab; f.logits = nullptr; f.logits_in = d_lg;
  f.n_ctus = n_ctus; f.ctu_base = 0; f.width = ctx->cfg.width; f.height = ctx->cfg.height; f.ctus_x = ctx->ctus_x; f.ctus_per_frame = ctx->ctus; f.clamp = clamp ? 1 : 0;
  hipLaunchKernelGGL(hevcdl_fc_kernel, dim3((n_ctus + 15) / 16), dim3(256), hevcdl_fc_smem_bytes(), nullptr, f);
  TRY(sync_or_fail(ctx, "label kernel"));
  hipMemcpy(labels, d_lab, n * LABELS_PER_CTU, hipMemcpyDeviceToHost);
  return HEVCDL_OK;
}

// the labels of n_frames staged pictures into the staging buffer: the caller's (uploaded, boundary policy applied) or the CNN stage's
static hevcdl_status stage_labels(hevcdl_ctx *ctx, const uint8_t *labels_opt, int n_frames)
{
  if (!labels_opt) return hevcdl_predict_depth_dev(ctx, ctx->stage.d_yuv, n_frames, ctx->stage.d_labels, nullptr, nullptr);
  HIPCHK(hipMemcpy(ctx->stage.d_labels, labels_opt, ctx->labels_bytes(n_frames), hipMemcpyHostToDevice));
  return hevcdl_clamp_labels_dev(ctx, ctx->stage.d_labels, n_frames, nullptr);
}

static hevcdl_status compress_frames_staged(hevcdl_ctx *ctx, int n_frames, const uint8_t *labels_opt, hevcdl_ctu_record *records, uint8_t *recon_opt, hevcdl_frame_stats *stats_opt);
extern "C" hevcdl_status hevcdl_compress_frames(hevcdl_ctx *ctx, const uint8_t *yuv, int n_frames, const uint8_t *labels_opt,
                                                hevcdl_ctu_record *records, uint8_t *recon_opt, hevcdl_frame_stats *stats_opt)
{
  FRAMES_OR_RETURN(ctx, n_frames);
  if (!yuv || !records) return fail(ctx, HEVCDL_ERR_INVALID_ARG, "null pointer");
  TRY(ensure_staging(ctx));
  HIPCHK(hipMemcpy(ctx->stage.d_yuv, yuv, ctx->frame_bytes * n_frames, hipMemcpyHostToDevice));
  return compress_frames_staged(ctx, n_frames, labels_opt, records, recon_opt, stats_opt);
}
extern "C" hevcdl_status hevcdl_compress_frames_planes(hevcdl_ctx *ctx, const hevcdl_planes *src, int n_frames, const uint8_t *labels_opt,
                                                       hevcdl_ctu_record *records, uint8_t *recon_opt, hevcdl_frame_stats *stats_opt)
{
  FRAMES_OR_RETURN(ctx, n_frames);
  if (!records) return fail(ctx, HEVCDL_ERR_INVALID_ARG, "null pointer");
  TRY(ensure_staging(ctx));
  TRY(upload_planes(ctx, src, n_frames));
  return compress_frames_staged(ctx, n_frames, labels_opt, records, recon_opt, stats_opt);
}
static hevcdl_status compress_frames_staged(hevcdl_ctx *ctx, int n_frames, const uint8_t *labels_opt, hevcdl_ctu_record *records, uint8_t *recon_opt, hevcdl_frame_stats *stats_opt)
{
  TRY(stage_labels(ctx, labels_opt, n_frames));
  TRY(hevcdl_compress_frames_dev(ctx, ctx->stage.d_yuv, n_frames, ctx->stage.d_labels, ctx->stage.d_records, ctx->stage.d_recon, ctx->stage.d_stats, nullptr));
  TRY(sync_or_fail(ctx, "rd kernel"));
  HIPCHK(hipMemcpy(records, ctx->stage.d_records, ctx->records_bytes(n_frames), hipMemcpyDeviceToHost));
  if (recon_opt) HIPCHK(hipMemcpy(recon_opt, ctx->stage.d_recon, ctx->frame_bytes * n_frames, hipMemcpyDeviceToHost));
  if (stats_opt) HIPCHK(hipMemcpy(stats_opt, ctx->stage.d_stats, sizeof(hevcdl_frame_stats) * n_frames, hipMemcpyDeviceToHost));
  return HEVCDL_OK;
}

// ---- deblocking (row f-2, first half): TComLoopFilter::loopFilterPic, TComLoopFilter.cpp:130, called at TEncGOP.cpp:1742 ----
// tc / beta / chroma tc of a picture filtered with (beta_offset_div2, tc_offset_div2): TComLoopFilter.cpp:59-67 (the tables: csrc/dbk_select.h), :623-624, 782-804, Bs 2
// qp: the picture's slice QP (the cfg's, or with DeltaQpRD the one the picture was coded with)
static void dbk_triple(const hevcdl_ctx *ctx, int qp, int beta_offset_div2, int tc_offset_div2, int *tc, int *beta, int *tc_c)
{
  const int qpc = HEVCDL_CHROMA_SCALE_420[qp < 0 ? 0 : (qp > 57 ? 57 : qp)];      // TComLoopFilter.cpp:782-797, cQpOffset 0
  const int bd_scale = 1 << (ctx->cfg.bit_depth - 8);                                       // iBitdepthScale, TComLoopFilter.cpp:596, 770
  const int tco = 2 * tc_offset_div2, bo = 2 * beta_offset_div2;   // slice_tc_offset_div2 / slice_beta_offset_div2 << 1 (TComLoopFilter.cpp:623-624, 804), Bs 2
  auto clipi = [](int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); };
  *tc = HEVCDL_DBK_TC[clipi(qp + 2 + tco, 53)] * bd_scale; *beta = HEVCDL_DBK_BETA[clipi(qp + bo, 51)] * bd_scale; *tc_c = HEVCDL_DBK_TC[clipi(qpc + 2 + tco, 53)] * bd_scale;
}

// idx: NULL, or the candidate of the QP search every picture was coded with (DeltaQpRD)
static hevcdl_status check_qp_rd_idx(hevcdl_ctx *ctx, const int32_t *idx, int n_frames)
{
  for (int i = 0; idx && i < n_frames; i++) if (idx[i] < 0 || idx[i] >= ctx->qprd.count) return fail(ctx, HEVCDL_ERR_INVALID_ARG, "a picture's candidate index lies outside the context's table (0 .. 2 DeltaQpRD)");
  return HEVCDL_OK;
}

extern "C" hevcdl_status hevcdl_deblock_frames_choice_dev(hevcdl_ctx *ctx, const void *d_recon, int n_frames, const void *d_records, const hevcdl_dbk_choice *choices, void *d_out, void *stream)
{
  return hevcdl_deblock_frames_qp_dev(ctx, d_recon, n_frames, d_records, choices, nullptr, d_out, stream);
}

extern "C" hevcdl_status hevcdl_deblock_frames_qp_dev(hevcdl_ctx *ctx, const void *d_recon, int n_frames, const void *d_records, const hevcdl_dbk_choice *choices, const int32_t *idx, void *d_out, void *stream)
{
  FRAMES_OR_RETURN(ctx, n_frames);
  TRY(check_qp_rd_idx(ctx, idx, n_frames));
  if (!d_recon || !d_records || !d_out) return fail(ctx, HEVCDL_ERR_INVALID_ARG, "null device pointer");
  hevcdl_dbk_params p;
  p.in = (const uint8_t *)d_recon; p.out = (uint8_t *)d_out; p.records = (const unsigned char *)d_records;
  p.width = ctx->cfg.width; p.height = ctx->cfg.height; p.ctus_x = ctx->ctus_x; p.ctus_per_frame = ctx->ctus; p.n_frames = n_frames;
  dbk_triple(ctx, ctx->cfg.qp, ctx->cfg.lf_beta_offset_div2, ctx->cfg.lf_tc_offset_div2, &p.tc, &p.beta, &p.tc_c);
  p.pel_max = (1 << ctx->cfg.bit_depth) - 1;
  p.lf_across_tiles = ctx->cfg.lf_across_tiles != 0; p.tile_cols = ctx->cfg.tile_columns; p.tile_rows = ctx->cfg.tile_rows;
  memcpy(p.col_bd, ctx->col_bd, sizeof p.col_bd); memcpy(p.row_bd, ctx->row_bd, sizeof p.row_bd);
  p.frame_params = nullptr; p.qp_map = nullptr; p.cb_qp_offset = p.cr_qp_offset = 0;
  if (ctx->cuqp.active) { // a QP per edge: the rows are (2 tc_offset_div2, 2 beta_offset_div2, -, disabled), the map and the PPS chroma offsets go with them
    if (idx) return fail(ctx, HEVCDL_ERR_INVALID_ARG, "a QP map does not go with candidate indices");
    for (int i = 0; choices && i < n_frames; i++)
      if (choices[i].beta_offset_div2 < -6 || choices[i].beta_offset_div2 > 6 || choices[i].tc_offset_div2 < -6 || choices[i].tc_offset_div2 > 6) return fail(ctx, HEVCDL_ERR_INVALID_ARG, "a picture's deblocking offsets are out of range (-6 .. 6)");
    TRY(lazy_alloc(ctx, ctx->dbk.d_frame_params, sizeof(int) * 4 * (size_t)ctx->cfg.max_frames, "per-picture deblocking parameters (cfg.max_frames)"));
    std::vector<int> &h = ctx->dbk.h_frame_params;
    h.assign((size_t)4 * n_frames, 0);
    for (int i = 0; i < n_frames; i++) {
      h[4 * i] = 2 * (choices ? choices[i].tc_offset_div2 : ctx->cfg.lf_tc_offset_div2); h[4 * i + 1] = 2 * (choices ? choices[i].beta_offset_div2 : ctx->cfg.lf_beta_offset_div2);
      h[4 * i + 3] = choices && choices[i].disabled != 0;
    }
    HIPCHK(hipMemcpyAsync(ctx->dbk.d_frame_params, h.data(), sizeof(int) * h.size(), hipMemcpyHostToDevice, (hipStream_t)stream));
    p.frame_params = ctx->dbk.d_frame_params; p.qp_map = ctx->cuqp.active; p.cb_qp_offset = ctx->cuqp.info.cb_qp_offset; p.cr_qp_offset = ctx->cuqp.info.cr_qp_offset;
  } else
  if (choices || idx || !ctx->fqp.list.empty()) { // a row of (tc, beta, tc_c, disabled) per picture, uploaded in front of the launch on its stream (the host copy lives in the context until the next call)
    for (int i = 0; choices && i < n_frames; i++)
      if (choices[i].beta_offset_div2 < -6 || choices[i].beta_offset_div2 > 6 || choices[i].tc_offset_div2 < -6 || choices[i].tc_offset_div2 > 6) return fail(ctx, HEVCDL_ERR_INVALID_ARG, "a picture's deblocking offsets are out of range (-6 .. 6)");
    TRY(lazy_alloc(ctx, ctx->dbk.d_frame_params, sizeof(int) * 4 * (size_t)ctx->cfg.max_frames, "per-picture deblocking parameters (cfg.max_frames)"));
    std::vector<int> &h = ctx->dbk.h_frame_params;
    h.assign((size_t)4 * n_frames, 0);
    for (int i = 0; i < n_frames; i++) {
      const int qp = idx ? ctx->qprd.cand[idx[i]].qp : frame_qp_at(ctx, i);      // a candidate's (DeltaQpRD), the list's (hevcdl_set_frame_qps) or the context's
      dbk_triple(ctx, qp, choices ? choices[i].beta_offset_div2 : ctx->cfg.lf_beta_offset_div2, choices ? choices[i].tc_offset_div2 : ctx->cfg.lf_tc_offset_div2, &h[4 * i], &h[4 * i + 1], &h[4 * i + 2]);
      h[4 * i + 3] = choices && choices[i].disabled != 0;
    }
    HIPCHK(hipMemcpyAsync(ctx->dbk.d_frame_params, h.data(), sizeof(int) * h.size(), hipMemcpyHostToDevice, (hipStream_t)stream));
    p.frame_params = ctx->dbk.d_frame_params;
  }
  hevcdl_launch_deblock(&p, stream);
  return launch_status(ctx);
}

extern "C" hevcdl_status hevcdl_deblock_frames_dev(hevcdl_ctx *ctx, const void *d_recon, int n_frames, const void *d_records, void *d_out, void *stream)
{
  return hevcdl_deblock_frames_choice_dev(ctx, d_recon, n_frames, d_records, nullptr, d_out, stream);
}

extern "C" hevcdl_status hevcdl_deblock_frames(hevcdl_ctx *ctx, const uint8_t *recon, int n_frames, const hevcdl_ctu_record *records, uint8_t *out)
{
  return hevcdl_deblock_frames_choice(ctx, recon, n_frames, records, nullptr, out);
}

extern "C" hevcdl_status hevcdl_deblock_frames_choice(hevcdl_ctx *ctx, const uint8_t *recon, int n_frames, const hevcdl_ctu_record *records, const hevcdl_dbk_choice *choices, uint8_t *out)
{
  return hevcdl_deblock_frames_qp(ctx, recon, n_frames, records, choices, nullptr, out);
}

extern "C" hevcdl_status hevcdl_deblock_frames_qp(hevcdl_ctx *ctx, const uint8_t *recon, int n_frames, const hevcdl_ctu_record *records, const hevcdl_dbk_choice *choices, const int32_t *idx, uint8_t *out)
{
  FRAMES_OR_RETURN(ctx, n_frames);
  if (!recon || !records || !out) return fail(ctx, HEVCDL_ERR_INVALID_ARG, "null pointer");
  TRY(ensure_staging(ctx));
  HIPCHK(hipMemcpy(ctx->stage.d_recon, recon, ctx->frame_bytes * n_frames, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(ctx->stage.d_records, records, ctx->records_bytes(n_frames), hipMemcpyHostToDevice));
  TRY(hevcdl_deblock_frames_qp_dev(ctx, ctx->stage.d_recon, n_frames, ctx->stage.d_records, choices, idx, ctx->stage.d_yuv, nullptr));   // d_yuv: free staging plane set
  TRY(sync_or_fail(ctx, "deblock kernels"));
  HIPCHK(hipMemcpy(out, ctx->stage.d_yuv, ctx->frame_bytes * n_frames, hipMemcpyDeviceToHost));
  return HEVCDL_OK;
}

// the filter with a QP per edge on host buffers (TEST AND DIAGNOSTIC: the decoder keeps the map in HBM): qp_map [n_frames][ctus][256]
namespace { struct CuQpActive { hevcdl_ctx *c; ~CuQpActive() { c->cuqp.active = nullptr; } }; }
static hevcdl_status ensure_qp_map(hevcdl_ctx *ctx) { return lazy_alloc(ctx, ctx->cuqp.d_map, (size_t)256 * ctx->ctus * (size_t)ctx->cfg.max_frames, "QP map (cfg.max_frames)"); }
extern "C" hevcdl_status hevcdl_deblock_frames_map(hevcdl_ctx *ctx, const void *recon, int n_frames, const hevcdl_ctu_record *records, const hevcdl_dbk_choice *choices_opt,
                                                  const hevcdl_qp_info *qp_info, const int8_t *qp_map, void *out)
{
  FRAMES_OR_RETURN(ctx, n_frames);
  if (!recon || !records || !out || !qp_info || !qp_map) return fail(ctx, HEVCDL_ERR_INVALID_ARG, "null pointer");
  if (qp_info->cb_qp_offset < -12 || qp_info->cb_qp_offset > 12 || qp_info->cr_qp_offset < -12 || qp_info->cr_qp_offset > 12) return fail(ctx, HEVCDL_ERR_INVALID_ARG, "chroma QP offsets out of range (-12 .. 12)");
  TRY(ensure_staging(ctx));
  TRY(ensure_qp_map(ctx));
  HIPCHK(hipMemcpy(ctx->stage.d_recon, recon, ctx->frame_bytes * n_frames, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(ctx->stage.d_records, records, ctx->records_bytes(n_frames), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(ctx->cuqp.d_map, qp_map, (size_t)256 * ctx->ctus * (size_t)n_frames, hipMemcpyHostToDevice));
  CuQpActive guard{ ctx };
  ctx->cuqp.active = ctx->cuqp.d_map; ctx->cuqp.info = *qp_info;
  TRY(hevcdl_deblock_frames_qp_dev(ctx, ctx->stage.d_recon, n_frames, ctx->stage.d_records, choices_opt, nullptr, ctx->stage.d_yuv, nullptr));
  TRY(sync_or_fail(ctx, "deblock kernels"));
  HIPCHK(hipMemcpy(out, ctx->stage.d_yuv, ctx->frame_bytes * n_frames, hipMemcpyDeviceToHost));
  return HEVCDL_OK;
}

extern "C" hevcdl_status hevcdl_enable_cu_qp(hevcdl_ctx *ctx, int on)
{
  if (!ctx) return HEVCDL_ERR_INVALID_ARG;
  if (!on && ctx->cuqp.on) { TRY(sync_or_fail(ctx, "hevcdl_enable_cu_qp")); ctx->cuqp = CuQp(); }
  ctx->cuqp.on = on != 0;
  return HEVCDL_OK;
}

extern "C" hevcdl_status hevcdl_enable_scaling_lists(hevcdl_ctx *ctx, int on)
{
  if (!ctx) return HEVCDL_ERR_INVALID_ARG;
  if (!on && ctx->sclist.on) { TRY(sync_or_fail(ctx, "hevcdl_enable_scaling_lists")); ctx->sclist = ScalingLists(); }
  ctx->sclist.on = on != 0;
  return HEVCDL_OK;
}

// ---- per-picture deblocking parameters: DeblockingFilterMetric 1 (dbk_select_kernel.hip, dbk_select.h), TEncGOP::applyDeblockingFilterMetric, called at TEncGOP.cpp:1739 ----
extern "C" hevcdl_status hevcdl_dbk_metric_frames_dev(hevcdl_ctx *ctx, const void *d_recon, int n_frames, void *d_sums, void *stream)
{
  FRAMES_OR_RETURN(ctx, n_frames);
  if (!d_recon || !d_sums) return fail(ctx, HEVCDL_ERR_INVALID_ARG, "null device pointer");
  hevcdl_dbk_metric_params p;
  p.recon = d_recon; p.sums = d_sums; p.width = ctx->cfg.width; p.height = ctx->cfg.height; p.n_frames = n_frames; p.sample_bytes = ctx->cfg.bit_depth > 8 ? 2 : 1;
  p.edges_x = hevcdl_dbk_metric_edges(p.width); p.edges_y = hevcdl_dbk_metric_edges(p.height);
  if (p.edges_x < 1 || p.edges_y < 1) return fail(ctx, HEVCDL_ERR_INVALID_ARG, "the deblocking metric needs a picture of at least 64 luma samples in either direction");
  hevcdl_dbk_metric_thresholds(ctx->cfg.qp, ctx->cfg.bit_depth, &p.thr1, &p.thr2);
  HIPCHK(hipMemsetAsync(d_sums, 0, sizeof(unsigned long long) * 2 * (size_t)n_frames, (hipStream_t)stream));
  hevcdl_launch_dbk_metric(&p, stream);
  return launch_status(ctx);
}

extern "C" hevcdl_status hevcdl_dbk_metric_frames(hevcdl_ctx *ctx, const void *recon, int n_frames, uint64_t *sums)
{
  FRAMES_OR_RETURN(ctx, n_frames);
  if (!recon || !sums) return fail(ctx, HEVCDL_ERR_INVALID_ARG, "null pointer");
  TRY(ensure_staging(ctx));
  TRY(lazy_alloc(ctx, ctx->dbk.d_sums, sizeof(unsigned long long) * 49 * (size_t)ctx->cfg.max_frames, "deblocking metric sums (cfg.max_frames)"));
  HIPCHK(hipMemcpy(ctx->stage.d_recon, recon, ctx->frame_bytes * n_frames, hipMemcpyHostToDevice));
  TRY(hevcdl_dbk_metric_frames_dev(ctx, ctx->stage.d_recon, n_frames, ctx->dbk.d_sums, nullptr));
  TRY(sync_or_fail(ctx, "deblocking metric kernel"));
  HIPCHK(hipMemcpy(sums, ctx->dbk.d_sums, sizeof(unsigned long long) * 2 * (size_t)n_frames, hipMemcpyDeviceToHost));
  return HEVCDL_OK;
}

extern "C" hevcdl_status hevcdl_dbk_metric_choice(int width, int height, int bit_depth, uint64_t col_sum, uint64_t row_sum, int pps_beta_offset_div2, int pps_tc_offset_div2,
                                                  hevcdl_dbk_choice *out)
{
  if (!out || width <= 0 || height <= 0 || hevcdl_dbk_metric_edges(width) < 1 || hevcdl_dbk_metric_edges(height) < 1) return HEVCDL_ERR_INVALID_ARG;
  if (bit_depth < 8 || bit_depth > 16) return HEVCDL_ERR_UNSUPPORTED;
  const int offset = hevcdl_dbk_metric_offset(width, height, bit_depth, col_sum, row_sum);
  out->override_enabled = 1; out->override_flag = offset != 0; out->disabled = 0;                  // TEncGOP.cpp:3284-3300 (the PPS of a run with the metric never disables the filter: TEncTop.cpp:1010)
  out->beta_offset_div2 = offset ? offset : pps_beta_offset_div2; out->tc_offset_div2 = offset ? offset : pps_tc_offset_div2;
  return HEVCDL_OK;
}

// ---- DeblockingFilterMetric 2: TEncGOP::applyDeblockingFilterParameterSelection, called at TEncGOP.cpp:1735 ----
extern "C" hevcdl_status hevcdl_dbk_trial_frames_dev(hevcdl_ctx *ctx, const void *d_org, const void *d_recon, int n_frames, const void *d_records, void *d_tables, void *stream)
{
  FRAMES_OR_RETURN(ctx, n_frames);
  if (!d_org || !d_recon || !d_records || !d_tables) return fail(ctx, HEVCDL_ERR_INVALID_ARG, "null device pointer");
  hevcdl_dbk_trial_params q;
  memset(&q, 0, sizeof q);
  hevcdl_dbk_params &p = q.d;
  p.qp_map = nullptr; p.cb_qp_offset = p.cr_qp_offset = 0;
  p.in = (const uint8_t *)d_recon; p.records = (const unsigned char *)d_records;
  p.width = ctx->cfg.width; p.height = ctx->cfg.height; p.ctus_x = ctx->ctus_x; p.ctus_per_frame = ctx->ctus; p.n_frames = n_frames;
  p.pel_max = (1 << ctx->cfg.bit_depth) - 1;
  p.lf_across_tiles = ctx->cfg.lf_across_tiles != 0; p.tile_cols = ctx->cfg.tile_columns; p.tile_rows = ctx->cfg.tile_rows;
  memcpy(p.col_bd, ctx->col_bd, sizeof p.col_bd); memcpy(p.row_bd, ctx->row_bd, sizeof p.row_bd);
  q.org = (const uint8_t *)d_org; q.table = d_tables; q.shift = 2 * (ctx->cfg.bit_depth - 8);
  for (int b = -3; b <= 3; b++) for (int t = -3; t <= 3; t++) { // the distinct (tc, beta) pairs of luma and the distinct chroma tc values (a function of t alone)
    int tc, beta, tc_c;
    dbk_triple(ctx, ctx->cfg.qp, b, t, &tc, &beta, &tc_c);
    const int e = 7 * (b + 3) + (t + 3);
    int j = 0; while (j < q.n_luma && (q.tc[j] != tc || q.beta[j] != beta)) j++;
    if (j == q.n_luma) { q.tc[j] = tc; q.beta[j] = beta; q.n_luma++; }
    q.luma_of[e] = j;
    if (b == -3) { int k = 0; while (k < q.n_chroma && q.tc_c[k] != tc_c) k++; if (k == q.n_chroma) q.tc_c[q.n_chroma++] = tc_c; q.chroma_of[t + 3] = k; }
  }
  HIPCHK(hipMemsetAsync(d_tables, 0, sizeof(unsigned long long) * 49 * (size_t)n_frames, (hipStream_t)stream));
  hevcdl_launch_dbk_trial(&q, stream);
  return launch_status(ctx);
}

extern "C" hevcdl_status hevcdl_dbk_trial_frames(hevcdl_ctx *ctx, const void *org, const void *recon, int n_frames, const hevcdl_ctu_record *records, uint64_t *tables)
{
  FRAMES_OR_RETURN(ctx, n_frames);
  if (!org || !recon || !records || !tables) return fail(ctx, HEVCDL_ERR_INVALID_ARG, "null pointer");
  TRY(ensure_staging(ctx));
  TRY(lazy_alloc(ctx, ctx->dbk.d_sums, sizeof(unsigned long long) * 49 * (size_t)ctx->cfg.max_frames, "deblocking trial tables (cfg.max_frames)"));
  HIPCHK(hipMemcpy(ctx->stage.d_yuv, org, ctx->frame_bytes * n_frames, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(ctx->stage.d_recon, recon, ctx->frame_bytes * n_frames, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(ctx->stage.d_records, records, ctx->records_bytes(n_frames), hipMemcpyHostToDevice));
  TRY(hevcdl_dbk_trial_frames_dev(ctx, ctx->stage.d_yuv, ctx->stage.d_recon, n_frames, ctx->stage.d_records, ctx->dbk.d_sums, nullptr));
  TRY(sync_or_fail(ctx, "deblocking trial kernels"));
  HIPCHK(hipMemcpy(tables, ctx->dbk.d_sums, sizeof(unsigned long long) * 49 * (size_t)n_frames, hipMemcpyDeviceToHost));
  return HEVCDL_OK;
}

extern "C" hevcdl_status hevcdl_dbk_walk_table(const uint64_t *table, int pps_beta_offset_div2, int pps_tc_offset_div2, int32_t *state4, hevcdl_dbk_choice *out)
{
  if (!table || !state4 || !out) return HEVCDL_ERR_INVALID_ARG;
  hevcdl_dbk_walk_state st = { state4[0], state4[1], state4[2], state4[3] };
  const hevcdl_dbk_walk_result r = hevcdl_dbk_walk(table, pps_beta_offset_div2, pps_tc_offset_div2, &st);
  state4[0] = st.available; state4[1] = st.disabled; state4[2] = st.beta_offset_div2; state4[3] = st.tc_offset_div2;
  out->override_enabled = 1; out->override_flag = r.override_flag; out->disabled = r.disabled; out->beta_offset_div2 = r.beta_offset_div2; out->tc_offset_div2 = r.tc_offset_div2;
  return HEVCDL_OK;
}

extern "C" hevcdl_status hevcdl_dbk_select_reset(hevcdl_ctx *ctx)
{
  if (!ctx) return HEVCDL_ERR_INVALID_ARG;
  ctx->dbk.walk = hevcdl_dbk_walk_state{ 0, 0, 0, 0 };
  return HEVCDL_OK;
}

extern "C" hevcdl_status hevcdl_get_dbk_choice(hevcdl_ctx *ctx, int first, int count, hevcdl_dbk_choice *out)
{
  if (!ctx) return HEVCDL_ERR_INVALID_ARG;
  if (!out || first < 0 || count < 0 || (long long)first + count > (long long)ctx->dbk.h_choice.size()) return fail(ctx, HEVCDL_ERR_INVALID_ARG, "hevcdl_get_dbk_choice: pictures outside the last picture pipeline call");
  std::copy(ctx->dbk.h_choice.begin() + first, ctx->dbk.h_choice.begin() + first + count, out);
  return HEVCDL_OK;
}

// ---- SAO (row f-2, second half): TEncSampleAdaptiveOffset::SAOProcess, TEncSampleAdaptiveOffset.cpp:244, called at TEncGOP.cpp:1797 ----
extern "C" hevcdl_status hevcdl_sao_frames_dev(hevcdl_ctx *ctx, const void *d_org, const void *d_deblocked, int n_frames, void *d_params, void *d_out, void *stream)
{
  return hevcdl_sao_frames_qp_dev(ctx, d_org, d_deblocked, n_frames, nullptr, d_params, d_out, stream);
}

// the per-picture QP table of a batch (hevcdl_frame_qp) from the pictures' candidate indices -- or, idx NULL, from the list and the modifier of hevcdl_set_frame_qps --, uploaded in front of the launches that read it on their stream (the host
// copy lives in the context until the next call, like the deblocking rows)
static hevcdl_status upload_frame_qp(hevcdl_ctx *ctx, const int32_t *idx, int n_frames, hipStream_t s)
{
  TRY(lazy_alloc(ctx, ctx->qprd.d_frame_qp, sizeof(hevcdl_frame_qp) * (size_t)ctx->cfg.max_frames, "per-picture QP table (cfg.max_frames)"));
  std::vector<hevcdl_frame_qp> &h = ctx->qprd.h_frame_qp;
  h.resize((size_t)n_frames);
  for (int i = 0; i < n_frames; i++) {
    hevcdl_qp_rd_candidate fam;
    if (!idx) hevcdl_frame_qp_family(frame_qp_at(ctx, i), ctx->cfg.bit_depth, ctx->fqp.lambda_modifier, &fam);
    const hevcdl_qp_rd_candidate &c = idx ? ctx->qprd.cand[idx[i]] : fam; h[(size_t)i] = hevcdl_frame_qp{ c.lambda, c.lambda_chroma, c.qp, 0 };
  }      // slice lambdas per component, TEncSlice.cpp:112-140, 656-660
  HIPCHK(hipMemcpyAsync(ctx->qprd.d_frame_qp, h.data(), sizeof(hevcdl_frame_qp) * h.size(), hipMemcpyHostToDevice, s));
  return HEVCDL_OK;
}

extern "C" hevcdl_status hevcdl_sao_frames_qp_dev(hevcdl_ctx *ctx, const void *d_org, const void *d_deblocked, int n_frames, const int32_t *idx, void *d_params, void *d_out, void *stream)
{
  FRAMES_OR_RETURN(ctx, n_frames);
  TRY(check_qp_rd_idx(ctx, idx, n_frames));
  if (!d_org || !d_deblocked || !d_params || !d_out) return fail(ctx, HEVCDL_ERR_INVALID_ARG, "null device pointer");
  const size_t nf = (size_t)ctx->cfg.max_frames;
  TRY(lazy_alloc(ctx, ctx->sao.d_sao_stats, (size_t)ctx->ctus * 3 * 5 * 256 * nf, "SAO statistics (cfg.max_frames)"));
  TRY(lazy_alloc(ctx, ctx->sao.d_sao_recon, ctx->sao_bytes(nf), "SAO reconstruction parameters (cfg.max_frames)"));
  TRY(lazy_alloc(ctx, ctx->sao.d_sao_cand, (size_t)ctx->ctus * (3 * 5 * 16 + 32) * nf, "SAO candidates (cfg.max_frames)"));      // candidates, then the chain's records
  hevcdl_sao_params p;
  p.org = (const uint8_t *)d_org; p.deblocked = (const uint8_t *)d_deblocked; p.out = (uint8_t *)d_out;
  p.stats = ctx->sao.d_sao_stats; p.params = (unsigned char *)d_params; p.recon_params = ctx->sao.d_sao_recon; p.cand = ctx->sao.d_sao_cand; p.crec = ctx->sao.d_sao_cand + (size_t)ctx->ctus * 3 * 5 * 16 * nf;
  p.width = ctx->cfg.width; p.height = ctx->cfg.height; p.ctus_x = ctx->ctus_x; p.ctus_per_frame = ctx->ctus; p.n_frames = n_frames; p.qp = ctx->cfg.qp;
  p.lambda = ctx->cfg.lambda; p.lambda_chroma = ctx->cfg.lambda_chroma;          // slice lambdas per component, TEncSlice.cpp:112-140
  p.tile_cols = ctx->cfg.tile_columns; p.tile_rows = ctx->cfg.tile_rows; p.bit_depth = ctx->cfg.bit_depth; p.lf_across_tiles = ctx->cfg.lf_across_tiles != 0;
  memcpy(p.col_bd, ctx->col_bd, sizeof p.col_bd); memcpy(p.row_bd, ctx->row_bd, sizeof p.row_bd);
  p.frame_qp = nullptr;
  if (idx || ctx->fqp.active()) { TRY(upload_frame_qp(ctx, idx, n_frames, (hipStream_t)stream)); p.frame_qp = ctx->qprd.d_frame_qp; }
  hevcdl_launch_sao(&p, stream);
  return launch_status(ctx);
}

extern "C" hevcdl_status hevcdl_sao_frames(hevcdl_ctx *ctx, const uint8_t *org, const uint8_t *deblocked, int n_frames, hevcdl_sao_blk *params, uint8_t *out)
{
  return hevcdl_sao_frames_qp(ctx, org, deblocked, n_frames, nullptr, params, out);
}

extern "C" hevcdl_status hevcdl_sao_frames_qp(hevcdl_ctx *ctx, const uint8_t *org, const uint8_t *deblocked, int n_frames, const int32_t *idx, hevcdl_sao_blk *params, uint8_t *out)
{
  FRAMES_OR_RETURN(ctx, n_frames);
  if (!org || !deblocked || !params || !out) return fail(ctx, HEVCDL_ERR_INVALID_ARG, "null pointer");
  TRY(ensure_staging(ctx));
  TRY(lazy_alloc(ctx, ctx->sao.d_sao_params, ctx->sao_bytes(ctx->cfg.max_frames), "SAO parameters (cfg.max_frames)"));
  HIPCHK(hipMemcpy(ctx->stage.d_yuv, org, ctx->frame_bytes * n_frames, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(ctx->stage.d_recon, deblocked, ctx->frame_bytes * n_frames, hipMemcpyHostToDevice));
  // the records staging area is free here and large enough for one more picture set (15120 B per CTU >= 6144)
  TRY(hevcdl_sao_frames_qp_dev(ctx, ctx->stage.d_yuv, ctx->stage.d_recon, n_frames, idx, ctx->sao.d_sao_params, ctx->stage.d_records, nullptr));
  TRY(sync_or_fail(ctx, "sao kernels"));
  HIPCHK(hipMemcpy(params, ctx->sao.d_sao_params, ctx->sao_bytes(n_frames), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(out, ctx->stage.d_records, ctx->frame_bytes * n_frames, hipMemcpyDeviceToHost));
  return HEVCDL_OK;
}

// ---- SAO with GIVEN parameters: what a decoder runs behind the deblocking filter (the parameters of a parsed stream, hevcdl_parse_stream) ----
// params: HOST memory, [n_frames][ctus] as the writer takes them (a merged CTU: mode 2 and the direction in component 0).  They are checked and resolved on the host --
// a merge takes the resolved parameters of its candidate, which must exist inside the picture and inside the CTU's tile / row slice of the context; modes 0 / 1, types 0 .. 4, band positions 0 .. 31, offsets within +-31 --
// and staged in the context (one host copy, one device buffer: one such call at a time, like hevcdl_deblock_frames_choice_dev).
extern "C" hevcdl_status hevcdl_sao_apply_frames_dev(hevcdl_ctx *ctx, const void *d_deblocked, int n_frames, const hevcdl_sao_blk *params, void *d_out, void *stream)
{
  FRAMES_OR_RETURN(ctx, n_frames);
  if (!d_deblocked || !params || !d_out) return fail(ctx, HEVCDL_ERR_INVALID_ARG, "null pointer");
  if (d_deblocked == d_out) return fail(ctx, HEVCDL_ERR_INVALID_ARG, "SAO reads the neighbours of every sample: the output must not be the input");
  std::vector<hevcdl_sao_blk> &h = ctx->sao.given;
  h.assign((size_t)n_frames * ctx->ctus, hevcdl_sao_blk{});
  for (int f = 0; f < n_frames; f++) for (int a = 0; a < ctx->ctus; a++) {
    const hevcdl_sao_blk &in = params[(size_t)f * ctx->ctus + a];
    hevcdl_sao_blk &out = h[(size_t)f * ctx->ctus + a];
    if (in.c[0].mode == 2) {
      const int dir = in.c[0].type;
      if (!(dir == 0 ? a % ctx->ctus_x > 0 : (dir == 1 && a >= ctx->ctus_x))) return fail(ctx, HEVCDL_ERR_INVALID_ARG, "an SAO merge without its candidate inside the picture");
      // ... and inside the CTU's unit of the context's grid (tiles; the rows of SliceMode 1 slices): sao() has no merge flag across such a border
      bool border = false;
      if (dir == 0) { for (int t = 1; t < ctx->cfg.tile_columns; t++) border |= ctx->col_bd[t] == a % ctx->ctus_x; }
      else { for (int t = 1; t < ctx->cfg.tile_rows; t++) border |= ctx->row_bd[t] == a / ctx->ctus_x; }
      if (border) return fail(ctx, HEVCDL_ERR_INVALID_ARG, "an SAO merge across a tile or slice border of the context");
      out = h[(size_t)f * ctx->ctus + (dir == 0 ? a - 1 : a - ctx->ctus_x)];
      continue;
    }
    for (int c = 0; c < 3; c++) {
      const hevcdl_sao_offset &o = in.c[c];
      if (o.mode == 0) continue;
      if (o.mode != 1 || o.type < 0 || o.type > 4 || o.aux < 0 || o.aux > 31) return fail(ctx, HEVCDL_ERR_INVALID_ARG, "SAO parameters out of range (mode 0 .. 2, type 0 .. 4, band position 0 .. 31)");
      out.c[c].mode = 1; out.c[c].type = o.type; out.c[c].aux = o.type == 4 ? o.aux : 0;
      for (int k = 0; k < 4; k++) {
        const int i = o.type == 4 ? (o.aux + k) & 31 : (k < 2 ? k : k + 1);
        if (o.offset[i] < -31 || o.offset[i] > 31) return fail(ctx, HEVCDL_ERR_INVALID_ARG, "an SAO offset outside +-31");
        out.c[c].offset[i] = o.offset[i];
      }
    }
  }
  TRY(lazy_alloc(ctx, ctx->sao.d_sao_recon, ctx->sao_bytes((size_t)ctx->cfg.max_frames), "SAO reconstruction parameters (cfg.max_frames)"));
  HIPCHK(hipMemcpyAsync(ctx->sao.d_sao_recon, h.data(), ctx->sao_bytes((size_t)n_frames), hipMemcpyHostToDevice, (hipStream_t)stream));
  hevcdl_sao_params p;
  memset(&p, 0, sizeof p);
  p.deblocked = (const uint8_t *)d_deblocked; p.out = (uint8_t *)d_out; p.recon_params = ctx->sao.d_sao_recon;
  p.width = ctx->cfg.width; p.height = ctx->cfg.height; p.ctus_x = ctx->ctus_x; p.ctus_per_frame = ctx->ctus; p.n_frames = n_frames; p.qp = ctx->cfg.qp;
  p.tile_cols = ctx->cfg.tile_columns; p.tile_rows = ctx->cfg.tile_rows; p.bit_depth = ctx->cfg.bit_depth; p.lf_across_tiles = ctx->cfg.lf_across_tiles != 0;
  memcpy(p.col_bd, ctx->col_bd, sizeof p.col_bd); memcpy(p.row_bd, ctx->row_bd, sizeof p.row_bd);
  hevcdl_launch_sao_apply(&p, stream);
  return launch_status(ctx);
}

extern "C" hevcdl_status hevcdl_sao_apply_frames(hevcdl_ctx *ctx, const void *deblocked, int n_frames, const hevcdl_sao_blk *params, void *out)
{
  FRAMES_OR_RETURN(ctx, n_frames);
  if (!deblocked || !params || !out) return fail(ctx, HEVCDL_ERR_INVALID_ARG, "null pointer");
  TRY(ensure_staging(ctx));
  HIPCHK(hipMemcpy(ctx->stage.d_recon, deblocked, ctx->frame_bytes * n_frames, hipMemcpyHostToDevice));
  // (the records staging area is free here and large enough for one more picture set, as in hevcdl_sao_frames_qp)
  TRY(hevcdl_sao_apply_frames_dev(ctx, ctx->stage.d_recon, n_frames, params, ctx->stage.d_records, nullptr));
  TRY(sync_or_fail(ctx, "sao apply kernels"));
  HIPCHK(hipMemcpy(out, ctx->stage.d_records, ctx->frame_bytes * n_frames, hipMemcpyDeviceToHost));
  return HEVCDL_OK;
}

// ---- the decoder: hevcdl_parse_stream -> hevcdl_recon_kernel -> deblocking -> SAO with the stream's parameters -> digests by the report kernels ----
extern "C" hevcdl_status hevcdl_config_from_stream(const hevcdl_stream_config *sc, const hevcdl_slice_layout *slices_opt, int max_frames, int device, hevcdl_config *out)
{
  if (!sc || sc->struct_size != sizeof *sc || !out || max_frames < 1) return HEVCDL_ERR_INVALID_ARG;
  TRY(hevcdl_config_default_bd(out, sc->width, sc->height, sc->qp, sc->bit_depth));
  out->max_frames = max_frames; out->device = device; out->tools = sc->tools;
  out->tile_columns = sc->tile_columns; out->tile_rows = sc->tile_rows; out->tile_uniform_spacing = sc->tile_uniform_spacing;
  memcpy(out->tile_column_width, sc->tile_column_width, sizeof out->tile_column_width); memcpy(out->tile_row_height, sc->tile_row_height, sizeof out->tile_row_height);
  out->lf_across_tiles = sc->lf_across_tiles; out->lf_beta_offset_div2 = sc->lf_beta_offset_div2; out->lf_tc_offset_div2 = sc->lf_tc_offset_div2;
  if (slices_opt && slices_opt->mode) { out->slice_mode = slices_opt->mode; out->slice_argument = slices_opt->argument; out->lf_across_slices = slices_opt->lf_across_slices; }
  return HEVCDL_OK;      // (wavefront and the segment keys change the stream alone: a decoding context does not need them)
}

static hevcdl_status ensure_report_workspace(hevcdl_ctx *ctx);      // (with the report entry points below)

// ---- slice data decoded on the device (hevcdl_enable_device_parse) ----
extern "C" hevcdl_status hevcdl_enable_device_parse(hevcdl_ctx *ctx, int on)
{
  if (!ctx) return HEVCDL_ERR_INVALID_ARG;
  TRY(check_frames(ctx, 0));
  if (!on) {
    if (!ctx->dp.on) return HEVCDL_OK;
    TRY(sync_or_fail(ctx, "hevcdl_enable_device_parse"));
    ctx->dp = DeviceParse();
    return HEVCDL_OK;
  }
  if (ctx->dp.on) return HEVCDL_OK;
  DeviceParse &g = ctx->dp;
  // a picture's units: its tiles (the context's grid: row slices are a column of them) or one; its sub-streams: those, or its CTU rows.  Bytes: 256 a CTU to begin with
  const size_t per = (size_t)std::max(ctx->cfg.tile_columns * ctx->cfg.tile_rows, 1) + (size_t)ctx->ctus_y, n = per * (size_t)ctx->cfg.max_frames;
  const size_t rbsp = (size_t)256 * ctx->ctus * ctx->cfg.max_frames;
  TRY(alloc_all(ctx, { want(g.d_tables, sizeof(hevcdl_ec::EcTables)), want(g.d_rbsp, rbsp), want(g.d_sao, ctx->sao_bytes((size_t)ctx->cfg.max_frames)), want(g.d_subs, n * sizeof(hevcdl_sd::SdSub)),
                       want(g.d_units, n * sizeof(hevcdl_sd::SdUnit)), want(g.d_results, n * sizeof(hevcdl_sd::SdResult)) }, "device parse buffers (cfg.max_frames)"));
  const hipError_t e = hipMemcpy(g.d_tables, &hevcdl_ec::ec_tables(), sizeof(hevcdl_ec::EcTables), hipMemcpyHostToDevice);
  if (e != hipSuccess) { ctx->dp = DeviceParse(); return hip_fail(ctx, "device parse tables", e); }
  g.rbsp_bytes = rbsp; g.n_subs = g.n_units = n; g.on = true;
  return HEVCDL_OK;
}

// pictures [first, first + cnt) of su: bytes and tables up, the kernel into stage.d_records and dp.d_sao, the error slots back -- an error is HEVCDL_ERR_INVALID_ARG with
// picture, CTU and sentence -- and with want_sao the SAO blocks into dp.h_sao
static hevcdl_status device_parse_batch(hevcdl_ctx *ctx, const hevcdl_parse::StreamUnits &su, int first, int cnt, bool want_sao, signed char *d_qp_map = nullptr)
{
  DeviceParse &g = ctx->dp;
  size_t sub0, n_subs, byte0, n_bytes;
  const hevcdl_status st = hevcdl_parse::batch_tables(su, first, cnt, g.h_units, sub0, n_subs, byte0, n_bytes);
  if (st != HEVCDL_OK) return fail(ctx, st, hevcdl_parse_error());
  TRY(ensure_staging(ctx));
  if (n_bytes > g.rbsp_bytes || n_subs > g.n_subs || g.h_units.size() > g.n_units) { // a batch that needs more: nothing of the last one is in flight (every batch ends with a wait)
    TRY(sync_or_fail(ctx, "device parse buffers"));
    if (n_bytes > g.rbsp_bytes) { g.d_rbsp.reset(); g.rbsp_bytes = 0; TRY(lazy_alloc(ctx, g.d_rbsp, n_bytes, "device parse: the RBSP bytes of a batch")); g.rbsp_bytes = n_bytes; }
    if (n_subs > g.n_subs) { g.d_subs.reset(); g.n_subs = 0; TRY(lazy_alloc(ctx, g.d_subs, n_subs * sizeof(hevcdl_sd::SdSub), "device parse: the sub-stream table of a batch")); g.n_subs = n_subs; }
    if (g.h_units.size() > g.n_units) {
      g.d_units.reset(); g.d_results.reset(); g.n_units = 0;
      TRY(lazy_alloc(ctx, g.d_units, g.h_units.size() * sizeof(hevcdl_sd::SdUnit), "device parse: the unit table of a batch"));
      TRY(lazy_alloc(ctx, g.d_results, g.h_units.size() * sizeof(hevcdl_sd::SdResult), "device parse: the error slots of a batch"));
      g.n_units = g.h_units.size();
    }
  }
  if (n_bytes) HIPCHK(hipMemcpy(g.d_rbsp, su.rbsp.data() + byte0, n_bytes, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(g.d_subs, su.subs.data() + sub0, n_subs * sizeof(hevcdl_sd::SdSub), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(g.d_units, g.h_units.data(), g.h_units.size() * sizeof(hevcdl_sd::SdUnit), hipMemcpyHostToDevice));
  hevcdl_slice_decode_params k;
  k.sd = su.sd; k.blob = g.d_rbsp; k.blob_bytes = n_bytes; k.subs = g.d_subs; k.units = g.d_units; k.n_subs = (int)n_subs; k.n_units = (int)g.h_units.size();
  k.records = ctx->stage.d_records; k.sao = g.d_sao; k.ctus = ctx->ctus; k.n_pics = cnt; k.results = g.d_results; k.tables = g.d_tables; k.qp_map = (int8_t *)d_qp_map;
  if (!hevcdl_launch_slice_decode(&k, nullptr)) return fail(ctx, HEVCDL_ERR_INVALID_ARG, "device parse: the unit tables of a batch do not fit a launch");
  TRY(launch_status(ctx));
  g.h_results.resize(g.h_units.size());
  HIPCHK(hipMemcpy(g.h_results.data(), g.d_results, g.h_units.size() * sizeof(hevcdl_sd::SdResult), hipMemcpyDeviceToHost));
  hevcdl_sd::SdResult res = { 0, -1 };
  const int bad = hevcdl_slice_decode_first_error(g.h_units, g.h_results.data(), &res);
  if (bad >= 0) { hevcdl_parse::set_slice_error(first + bad, res); return fail(ctx, HEVCDL_ERR_INVALID_ARG, hevcdl_parse_error()); }
  if (want_sao) { g.h_sao.resize((size_t)cnt * ctx->ctus); HIPCHK(hipMemcpy(g.h_sao.data(), g.d_sao, ctx->sao_bytes((size_t)cnt), hipMemcpyDeviceToHost)); }
  return HEVCDL_OK;
}
namespace { struct FrameQpGuard { hevcdl_ctx *c; ~FrameQpGuard() { c->fqp.list.clear(); } }; }

extern "C" hevcdl_status hevcdl_decode_stream(hevcdl_ctx *ctx, const uint8_t *stream, size_t bytes, void *pictures_opt, int picture_capacity, int *n_pictures,
                                             hevcdl_parsed_picture *info_opt, int32_t *hash_ok_opt)
{
  if (!ctx) return HEVCDL_ERR_INVALID_ARG;
  if (n_pictures) *n_pictures = 0;
  if (!stream || !n_pictures || picture_capacity < 0) return fail(ctx, HEVCDL_ERR_INVALID_ARG, "null stream or picture count");
  hevcdl_stream_config sc; memset(&sc, 0, sizeof sc); sc.struct_size = sizeof sc;
  hevcdl_slice_layout sl = { 0, 0, 1 }; hevcdl_segment_layout sg = { 0, 0 };
  int n = 0;
  const unsigned accept = (ctx->cuqp.on ? HEVCDL_ACCEPT_CU_QP : 0u) | (ctx->sclist.on ? HEVCDL_ACCEPT_SCALING_LISTS : 0u);      // off: every stream is answered as ever
  hevcdl_qp_info qi = { 0, 0, 0, 0 };
  hevcdl_scaling_info si; si.enabled = 0;
  hevcdl_status st = hevcdl_parse_stream_sl(stream, bytes, accept, &sc, &sl, &sg, nullptr, 0, &n, nullptr, nullptr, 0, &qi, nullptr, &si);
  if (st != HEVCDL_OK) return fail(ctx, st, hevcdl_parse_error());
  const bool use_map = qi.cu_qp_delta_enabled || qi.cb_qp_offset || qi.cr_qp_offset;      // a stream without either takes the constant-QP launches, also when enabled
  const bool use_sl = si.enabled != 0;                                                    // likewise a stream without scaling lists
  const bool want_map = use_map || use_sl;                                                // the scaling-list instantiation always reads the map (a constant one for a stream of one QP)
  *n_pictures = n;
  { // the context must describe the stream: size, depth and the grid the in-loop filters stop at (tiles, row slices) with its flag
    hevcdl_config want, grid; const char *why = "";
    if (hevcdl_config_from_stream(&sc, &sl, ctx->cfg.max_frames, ctx->cfg.device, &want) != HEVCDL_OK || hevcdl_slice_grid(&want, &grid, &why) != HEVCDL_OK)
      return fail(ctx, HEVCDL_ERR_UNSUPPORTED, why[0] ? why : "the stream's configuration cannot be run by a context");
    int cb[21], rb[23];
    const bool same = grid.width == ctx->cfg.width && grid.height == ctx->cfg.height && grid.bit_depth == ctx->cfg.bit_depth && grid.tile_columns == ctx->cfg.tile_columns &&
                      grid.tile_rows == ctx->cfg.tile_rows && (grid.lf_across_tiles != 0) == (ctx->cfg.lf_across_tiles != 0) &&
                      !hevcdl_tile_bounds(ctx->ctus_x, grid.tile_columns, grid.tile_uniform_spacing, grid.tile_column_width, 1, cb) &&
                      !hevcdl_tile_bounds(ctx->ctus_y, grid.tile_rows, grid.tile_uniform_spacing, grid.tile_row_height, 1, rb) &&
                      !memcmp(cb, ctx->col_bd, sizeof(int) * (size_t)(grid.tile_columns + 1)) && !memcmp(rb, ctx->row_bd, sizeof(int) * (size_t)(grid.tile_rows + 1));
    if (!same) return fail(ctx, HEVCDL_ERR_INVALID_ARG, "the context does not describe the stream (size, bit depth, tiles, slices or the loop-filter flags differ): create it from hevcdl_config_from_stream");
  }
  if (ctx->cfg.delta_qp_rd || ctx->cfg.deblocking_metric) return fail(ctx, HEVCDL_ERR_UNSUPPORTED, "a context with delta_qp_rd or deblocking_metric does not decode");
  if (n > picture_capacity) return fail(ctx, HEVCDL_ERR_INVALID_ARG, "the stream holds more pictures than there is room for (*n_pictures says how many)");
  std::vector<hevcdl_parsed_picture> pics; std::vector<hevcdl_ctu_record> recs; std::vector<hevcdl_sao_blk> sao; std::vector<int8_t> qmap;
  hevcdl_parse::StreamUnits su;                      // device parse: the slice data of the stream, cut into units
  const bool dev_parse = ctx->dp.on;
  if (dev_parse) {
    try { st = hevcdl_parse::collect_units(stream, bytes, 1, 1, (size_t)-1, su, accept); } catch (...) { return fail(ctx, HEVCDL_ERR_OOM, "host memory for the stream's slice data"); }
    if (st != HEVCDL_OK) return fail(ctx, st, hevcdl_parse_error());
    if (su.ctus != ctx->ctus) return fail(ctx, HEVCDL_ERR_INVALID_ARG, "the context does not describe the stream");
    pics = su.pictures;
    if (su.pending != HEVCDL_OK) { // the headers refuse a later picture: as the host parser would, an error in the slice data of a picture in front of it comes first
      for (int first = 0; first < (int)pics.size(); first += ctx->cfg.max_frames) TRY(device_parse_batch(ctx, su, first, std::min(ctx->cfg.max_frames, (int)pics.size() - first), false));
      return fail(ctx, su.pending, su.pending_sentence);
    }
  } else {
    try { pics.resize((size_t)n); recs.resize((size_t)n * ctx->ctus); sao.resize((size_t)n * ctx->ctus); if (want_map) qmap.resize((size_t)n * ctx->ctus * 256); } catch (...) { return fail(ctx, HEVCDL_ERR_OOM, "host memory for the stream's records"); }
    st = hevcdl_parse_stream_qp(stream, bytes, accept, &sc, &sl, &sg, pics.data(), n, &n, recs.data(), sao.data(), recs.size(), nullptr, want_map ? qmap.data() : nullptr);
    if (st != HEVCDL_OK) return fail(ctx, st, hevcdl_parse_error());
  }
  TRY(ensure_staging(ctx));
  TRY(lazy_alloc(ctx, ctx->stage.d_picture, ctx->frame_bytes * (size_t)ctx->cfg.max_frames, "output pictures (cfg.max_frames)"));
  TRY(ensure_report_workspace(ctx));
  const size_t work = hevcdl_recon_work_bytes(ctx->cfg.width, ctx->cfg.height, ctx->cfg.max_frames);
  TRY(lazy_alloc(ctx, ctx->dec.d_work, work, "reconstruction row counts (cfg.max_frames)"));
  HIPCHK(hipSetDevice(ctx->cfg.device));
  FrameQpGuard guard{ ctx };
  CuQpActive map_guard{ ctx };
  if (want_map) TRY(ensure_qp_map(ctx));
  if (use_sl) { // the stream's factors: 2 KB, uploaded once, read by every launch of the stream
    TRY(lazy_alloc(ctx, ctx->sclist.d_factor, (size_t)HEVCDL_SCALING_FACTOR_BYTES, "scaling factors"));
    HIPCHK(hipMemcpy(ctx->sclist.d_factor, si.factor, HEVCDL_SCALING_FACTOR_BYTES, hipMemcpyHostToDevice));
  }
  std::vector<int> qps; std::vector<hevcdl_dbk_choice> choices; std::vector<hevcdl_picture_report_t> rep;
  for (int first = 0; first < n; first += ctx->cfg.max_frames) {
    const int cnt = std::min(ctx->cfg.max_frames, n - first);
    qps.resize((size_t)cnt); choices.resize((size_t)cnt); rep.resize((size_t)cnt);
    bool any_sao = false, own_qp = false;
    for (int i = 0; i < cnt; i++) { qps[i] = pics[first + i].qp; choices[i] = pics[first + i].dbk; any_sao |= pics[first + i].sao != 0; own_qp |= qps[i] != ctx->cfg.qp; }
    if (dev_parse) TRY(device_parse_batch(ctx, su, first, cnt, any_sao, want_map ? ctx->cuqp.d_map.p : nullptr));      // the records into stage.d_records, the SAO blocks into dp.h_sao; an error before anything else is launched
    else HIPCHK(hipMemcpyAsync(ctx->stage.d_records, recs.data() + (size_t)first * ctx->ctus, ctx->records_bytes((size_t)cnt), hipMemcpyHostToDevice, nullptr));
    const uint32_t *d_err = nullptr;
    if (want_map && !dev_parse) HIPCHK(hipMemcpyAsync(ctx->cuqp.d_map, qmap.data() + (size_t)first * ctx->ctus * 256, (size_t)cnt * ctx->ctus * 256, hipMemcpyHostToDevice, nullptr));
    if (use_sl) { // scaling lists: the third instantiation of the reconstruction; the deblocking filter reads the map only where the stream has a QP per CU or chroma offsets
      st = hevcdl_recon_enqueue_sl(&sc, &sl, &qi, ctx->cuqp.d_map, ctx->sclist.d_factor, ctx->stage.d_records, cnt, ctx->stage.d_recon, ctx->dec.d_work, work, nullptr, ctx->dec.keep, &d_err);
      if (use_map) { ctx->cuqp.active = ctx->cuqp.d_map; ctx->cuqp.info = qi; }
    } else
    if (use_map) { // the map beside the records: uploaded behind a host parse, written there by the kernel with device parse; the two QP-map instantiations read it
      st = hevcdl_recon_enqueue_qp(&sc, &sl, &qi, ctx->cuqp.d_map, ctx->stage.d_records, cnt, ctx->stage.d_recon, ctx->dec.d_work, work, nullptr, ctx->dec.keep, &d_err);
      ctx->cuqp.active = ctx->cuqp.d_map; ctx->cuqp.info = qi;
    } else
    st = hevcdl_recon_enqueue(&sc, &sl, qps.data(), ctx->stage.d_records, cnt, ctx->stage.d_recon, ctx->dec.d_work, work, nullptr, ctx->dec.keep, &d_err);
    if (st != HEVCDL_OK) return fail(ctx, st, hevcdl_parse_error());
    if (own_qp) TRY(hevcdl_set_frame_qps(ctx, qps.data(), cnt)); else ctx->fqp.list.clear();
    TRY(hevcdl_deblock_frames_choice_dev(ctx, ctx->stage.d_recon, cnt, ctx->stage.d_records, choices.data(), ctx->stage.d_recon, nullptr));
    const void *d_final = ctx->stage.d_recon;
    if (any_sao) { TRY(hevcdl_sao_apply_frames_dev(ctx, ctx->stage.d_recon, cnt, dev_parse ? ctx->dp.h_sao.data() : sao.data() + (size_t)first * ctx->ctus, ctx->stage.d_picture, nullptr)); d_final = ctx->stage.d_picture; }
    for (int i = 0; i < cnt; i++) if (hash_ok_opt) hash_ok_opt[first + i] = -1;
    for (int method = 1; method <= 3; method++) { // the digests of the pictures still in HBM, by the report kernels, against the stream's SEI
      bool any = false;
      for (int i = 0; i < cnt; i++) any |= pics[first + i].hash_method == method;
      if (!any) continue;
      TRY(hevcdl_picture_report_dev(ctx, nullptr, d_final, cnt, method, ctx->rp.d_rp_out, nullptr));
      HIPCHK(hipMemcpy(rep.data(), ctx->rp.d_rp_out, sizeof(hevcdl_picture_report_t) * (size_t)cnt, hipMemcpyDeviceToHost));
      for (int i = 0; i < cnt; i++) {
        const hevcdl_parsed_picture &pc = pics[first + i];
        if (pc.hash_method == method && hash_ok_opt) hash_ok_opt[first + i] = rep[i].plane_bytes == pc.hash_plane_bytes && !memcmp(rep[i].digest, pc.digest, (size_t)(3 * pc.hash_plane_bytes));
      }
    }
    uint32_t err = 0;
    HIPCHK(hipMemcpy(&err, d_err, 4, hipMemcpyDeviceToHost));
    if (err) return fail(ctx, HEVCDL_ERR_HIP, "reconstruction: a CTU row waited for the row above longer than the limit");
    if (pictures_opt) HIPCHK(hipMemcpy((unsigned char *)pictures_opt + (size_t)first * ctx->frame_bytes, d_final, ctx->frame_bytes * (size_t)cnt, hipMemcpyDeviceToHost));
    TRY(sync_or_fail(ctx, "decoder"));
  }
  if (info_opt) memcpy(info_opt, pics.data(), sizeof(hevcdl_parsed_picture) * (size_t)n);
  return HEVCDL_OK;
}

// ---- picture quality (row f-3): SSE and MS-SSIM of TEncGOP::xCalculateAddPSNR / xCalculateMSSSIM (TEncGOP.cpp:2380-2420, 2559-2727) on the device ----
// the normalised 11 x 11 Gaussian window, computed by the host's libm in the reference's loop order (TEncGOP.cpp:2591-2611)
static void quality_weights(double *w)
{
  double sum = 0.0;
  for (int y = 0; y < 11; y++) for (int x = 0; x < 11; x++) { w[y * 11 + x] = exp(-((y - 5) * (y - 5) + (x - 5) * (x - 5)) / (5 - 0.5)); sum += w[y * 11 + x]; }
  for (int y = 0; y < 11; y++) for (int x = 0; x < 11; x++) w[y * 11 + x] /= sum;
}
static void quality_constants(hevcdl_quality_params *p, int bit_depth)
{
  const unsigned max_value = (1u << bit_depth) - 1;                   // :2664-2666
  p->c1 = (0.01 * max_value) * (0.01 * max_value); p->c2 = (0.03 * max_value) * (0.03 * max_value);
}

// packed 4:2:0 pictures of w x h luma samples at the context's bit depth: the context's own pictures, or the window crops of a padded source format
static void quality_sized_params(const hevcdl_ctx *ctx, hevcdl_quality_params *p, int w, int h)
{
  memset(p, 0, sizeof *p);
  p->n_planes = 3; p->plane_w[0] = w; p->plane_h[0] = h; p->plane_w[1] = p->plane_w[2] = w >> 1; p->plane_h[1] = p->plane_h[2] = h >> 1;
  p->plane_off[0] = 0; p->plane_off[1] = (size_t)w * h; p->plane_off[2] = (size_t)w * h + (size_t)(w >> 1) * (h >> 1);
  p->frame_samples = (size_t)w * h * 3 / 2; p->sample_bytes = ctx->cfg.bit_depth > 8 ? 2 : 1;
  quality_constants(p, ctx->cfg.bit_depth);
  hevcdl_quality_layout(p);
}
static void quality_picture_params(const hevcdl_ctx *ctx, hevcdl_quality_params *p) { quality_sized_params(ctx, p, ctx->cfg.width, ctx->cfg.height); }

// The pass's workspace: pyramid levels and tile sums of q_group pictures, the window.  Allocated by hevcdl_enable_quality(ctx, 1) -- so that a lack of memory shows up there,
// where a front end sizes its batch, and not in the middle of an encode -- or by the first hevcdl_picture_quality* call of a context that never enabled the switch.
static hevcdl_status ensure_quality_workspace(hevcdl_ctx *ctx)
{
  if (ctx->q.d_q_weights) return HEVCDL_OK;
  hevcdl_quality_params p; quality_picture_params(ctx, &p);
  double wt[121]; quality_weights(wt);
  const int group = std::min(ctx->cfg.max_frames, 16);                // pictures per pass: bounds the pyramid workspace (33 MB a picture at 2160p)
  Quality &q = ctx->q;
  TRY(alloc_all(ctx, { want(q.d_q_pyr, std::max<size_t>(p.pyr_pic_words, 1) * 4 * group), want(q.d_q_partial, std::max<size_t>(p.part_pic, 1) * sizeof(double) * group), want(q.d_q_weights, sizeof wt) },
                "picture quality workspace"));
  const hipError_t e = hipMemcpy(q.d_q_weights, wt, sizeof wt, hipMemcpyHostToDevice);
  if (e != hipSuccess) { q.d_q_pyr.reset(); q.d_q_partial.reset(); q.d_q_weights.reset(); return hip_fail(ctx, "picture quality workspace", e); }
  q.q_group = group;
  return HEVCDL_OK;
}

// do out_bytes at out reach into in_bytes at in?  (results must not lie inside the pictures they are computed from; every other overlap is the caller's business)
static bool overlaps(const void *out, size_t out_bytes, const void *in, size_t in_bytes)
{
  const uintptr_t o = (uintptr_t)out, a = (uintptr_t)in;
  return in && o < a + in_bytes && a < o + out_bytes;
}

// the quality launches for packed pictures of w x h luma samples (at most the context's size: the workspace is the context's)
static hevcdl_status quality_sized_dev(hevcdl_ctx *ctx, const void *d_org, const void *d_pic, int n_frames, void *d_out, hipStream_t s, int w, int h)
{
  TRY(ensure_quality_workspace(ctx));
  hevcdl_quality_params p; quality_sized_params(ctx, &p, w, h);
  if (w != ctx->cfg.width || h != ctx->cfg.height) { // a window: its levels and tile sums must fit the slots laid out for the whole picture
    hevcdl_quality_params full; quality_picture_params(ctx, &full);
    if (p.pyr_pic_words > full.pyr_pic_words || p.part_pic > full.part_pic) return fail(ctx, HEVCDL_ERR_INVALID_ARG, "picture quality: the window needs more workspace than the picture");
  }
  const size_t frame_bytes = p.frame_samples * p.sample_bytes;
  p.pyr = ctx->q.d_q_pyr; p.partial = ctx->q.d_q_partial; p.weights = ctx->q.d_q_weights; p.out = d_out;
  HIPCHK(hipMemsetAsync(d_out, 0, sizeof(hevcdl_quality) * (size_t)n_frames, s));
  for (int first = 0; first < n_frames; first += ctx->q.q_group) {        // a picture's result does not depend on the pass it falls into: every picture has its own workspace slot
    p.n_pics = std::min(ctx->q.q_group, n_frames - first); p.out_first = first;
    p.org = (const unsigned char *)d_org + frame_bytes * (size_t)first; p.pic = (const unsigned char *)d_pic + frame_bytes * (size_t)first;
    hevcdl_launch_quality(&p, s);
  }
  return launch_status(ctx);
}

extern "C" hevcdl_status hevcdl_picture_quality_dev(hevcdl_ctx *ctx, const void *d_org, const void *d_pic, int n_frames, void *d_out, void *stream)
{
  FRAMES_OR_RETURN(ctx, n_frames);
  if (!d_org || !d_pic || !d_out) return fail(ctx, HEVCDL_ERR_INVALID_ARG, "null device pointer");
  const size_t out_b = sizeof(hevcdl_quality) * (size_t)n_frames, span = ctx->frame_bytes * (size_t)n_frames;      // (d_org == d_pic is a picture compared with itself)
  if (overlaps(d_out, out_b, d_org, span) || overlaps(d_out, out_b, d_pic, span)) return fail(ctx, HEVCDL_ERR_INVALID_ARG, "picture quality: the output overlaps an input");
  return quality_sized_dev(ctx, d_org, d_pic, n_frames, d_out, (hipStream_t)stream, ctx->cfg.width, ctx->cfg.height);
}

extern "C" hevcdl_status hevcdl_picture_quality(hevcdl_ctx *ctx, const void *org, const void *pic, int n_frames, hevcdl_quality *out)
{
  FRAMES_OR_RETURN(ctx, n_frames);
  if (!org || !pic || !out) return fail(ctx, HEVCDL_ERR_INVALID_ARG, "null pointer");
  TRY(ensure_staging(ctx));
  TRY(lazy_alloc(ctx, ctx->q.d_q_out, sizeof(hevcdl_quality) * (size_t)ctx->cfg.max_frames, "picture quality results"));
  HIPCHK(hipMemcpy(ctx->stage.d_yuv, org, ctx->frame_bytes * n_frames, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(ctx->stage.d_recon, pic, ctx->frame_bytes * n_frames, hipMemcpyHostToDevice));
  TRY(hevcdl_picture_quality_dev(ctx, ctx->stage.d_yuv, ctx->stage.d_recon, n_frames, ctx->q.d_q_out, nullptr));
  TRY(sync_or_fail(ctx, "quality kernels"));
  HIPCHK(hipMemcpy(out, ctx->q.d_q_out, sizeof(hevcdl_quality) * (size_t)n_frames, hipMemcpyDeviceToHost));
  return HEVCDL_OK;
}

// One plane of any size (host buffers, no context): what the picture entry points do per plane, for callers whose planes are not a context's 4:2:0 picture.
extern "C" hevcdl_status hevcdl_plane_quality(int device, const void *org, const void *pic, int width, int height, int bit_depth, uint64_t *sse, double *msssim)
{
  if (!org || !pic || !sse || !msssim || width < 1 || height < 1 || width > 16384 || height > 16384) return HEVCDL_ERR_INVALID_ARG;
  if (bit_depth < 8 || bit_depth > 16) return HEVCDL_ERR_UNSUPPORTED;
  TRY(select_device(device));
  hevcdl_quality_params p;
  memset(&p, 0, sizeof p);
  p.n_planes = 1; p.plane_w[0] = width; p.plane_h[0] = height; p.frame_samples = (size_t)width * height; p.sample_bytes = bit_depth > 8 ? 2 : 1; p.n_pics = 1;
  quality_constants(&p, bit_depth);
  hevcdl_quality_layout(&p);
  double wt[121]; quality_weights(wt);
  const size_t bytes = p.frame_samples * p.sample_bytes;
  DevBuf<unsigned char> d_org, d_pic, d_pyr, d_part, d_wt, d_out;
  TRY(alloc_all(nullptr, { want(d_org, bytes), want(d_pic, bytes), want(d_pyr, std::max<size_t>(p.pyr_pic_words, 1) * 4), want(d_part, std::max<size_t>(p.part_pic, 1) * sizeof(double)),
                           want(d_wt, sizeof wt), want(d_out, sizeof(hevcdl_quality)) }, ""));
  hevcdl_quality q; memset(&q, 0, sizeof q);
  hipError_t e = hipMemcpy(d_org, org, bytes, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d_pic, pic, bytes, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d_wt, wt, sizeof wt, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemset(d_out, 0, sizeof q);
  if (e == hipSuccess) {
    p.org = d_org; p.pic = d_pic; p.pyr = d_pyr; p.partial = d_part; p.weights = d_wt; p.out = d_out;
    hevcdl_launch_quality(&p, nullptr);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(&q, d_out, sizeof q, hipMemcpyDeviceToHost);
  }
  if (e != hipSuccess) return hip_fail(nullptr, "", e);
  *sse = q.sse[0]; *msssim = q.msssim[0];
  return HEVCDL_OK;
}

extern "C" hevcdl_status hevcdl_enable_quality(hevcdl_ctx *ctx, int on)
{
  if (!ctx) return HEVCDL_ERR_INVALID_ARG;
  if (on) { // the whole of what the switch costs is reserved here: a refused allocation is this call's HEVCDL_ERR_OOM, not a later encode's
    TRY(check_frames(ctx, 0));
    TRY(ensure_quality_workspace(ctx));
    TRY(lazy_alloc(ctx, ctx->q.d_q_out, sizeof(hevcdl_quality) * (size_t)ctx->cfg.max_frames, "picture quality results"));
    ctx->q.quality_on = true;
    return HEVCDL_OK;
  }
  ctx->q.quality_on = false; ctx->q.h_quality.clear();
  TRY(sync_or_fail(ctx, "hevcdl_enable_quality"));
  ctx->q = Quality();      // off: the workspace goes back (a later hevcdl_picture_quality* call allocates its own again)
  return HEVCDL_OK;
}

// what the hevcdl_get_* of a switch check in this order: the pointers and signs, the switch (turned on by `enabler`), the range against the `have` pictures of the last batch
static hevcdl_status check_batch_range(hevcdl_ctx *ctx, const char *who, bool pointers, bool on, const char *enabler, int first, int count, long long have)
{
  char msg[160];
  if (!pointers || first < 0 || count < 0) snprintf(msg, sizeof msg, "%s: bad range", who);
  else if (!on) snprintf(msg, sizeof msg, "%s: %s was not called", who, enabler);
  else if ((long long)first + count > have) snprintf(msg, sizeof msg, "%s: pictures outside the last batch", who);
  else return HEVCDL_OK;
  return fail(ctx, HEVCDL_ERR_INVALID_ARG, msg);
}

extern "C" hevcdl_status hevcdl_get_quality(hevcdl_ctx *ctx, int first, int count, hevcdl_quality *out)
{
  if (!ctx) return HEVCDL_ERR_INVALID_ARG;
  TRY(check_batch_range(ctx, "hevcdl_get_quality", out != nullptr, ctx->q.quality_on, "hevcdl_enable_quality", first, count, (long long)ctx->q.h_quality.size()));
  if (count) memcpy(out, ctx->q.h_quality.data() + first, sizeof(hevcdl_quality) * (size_t)count);
  return HEVCDL_OK;
}

// ---- picture report: SSE of the output picture and the digests of SEIDecodedPictureHash on the device (report_kernel.hip; the SSE kernel is quality_kernel.hip's) ----
static void report_plane_params(hevcdl_report_params *p, int n_planes, const int *pw, const int *ph, int sample_bytes)
{
  memset(p, 0, sizeof *p);
  size_t off = 0, max_n = 1;
  for (int c = 0; c < n_planes; c++) {
    p->plane_w[c] = pw[c]; p->plane_h[c] = ph[c]; p->plane_off[c] = off;
    const size_t n = (size_t)pw[c] * ph[c] * sample_bytes;
    off += n; max_n = std::max(max_n, n);
  }
  p->frame_bytes = off; p->n_planes = n_planes; p->sample_bytes = sample_bytes;
  p->chunk_bytes = HEVCDL_REPORT_CHUNK_BYTES; p->chunk_stride = (int)hevcdl_ph::report_chunks(max_n, HEVCDL_REPORT_CHUNK_BYTES);
}
static void report_picture_params(const hevcdl_ctx *ctx, hevcdl_report_params *p)
{
  const int w = ctx->cfg.width, h = ctx->cfg.height, pw[3] = { w, w >> 1, w >> 1 }, ph[3] = { h, h >> 1, h >> 1 };
  report_plane_params(p, 3, pw, ph, ctx->cfg.bit_depth > 8 ? 2 : 1);
}

static hevcdl_status check_method(hevcdl_ctx *ctx, int method, const char *who)
{
  if (method >= 0 && method <= 3) return HEVCDL_OK;
  char msg[160]; snprintf(msg, sizeof msg, "%s: method must be 0 (none), 1 (MD5), 2 (CRC) or 3 (checksum)", who);
  return fail(ctx, HEVCDL_ERR_INVALID_ARG, msg);
}

static hevcdl_status ensure_report_workspace(hevcdl_ctx *ctx)
{
  if (ctx->rp.d_rp_partials) return HEVCDL_OK;
  hevcdl_report_params p; report_picture_params(ctx, &p);
  const size_t nf = (size_t)ctx->cfg.max_frames;
  return alloc_all(ctx, { want(ctx->rp.d_rp_out, sizeof(hevcdl_picture_report_t) * nf), want(ctx->rp.d_rp_sse, sizeof(hevcdl_quality) * nf),
                          want(ctx->rp.d_rp_partials, sizeof(uint32_t) * 3 * (size_t)p.chunk_stride * nf) }, "picture report workspace");
}

// sse_org / sse_pic: the pictures the SSE is taken over, packed at sse_w x sse_h luma samples -- the originals and d_pic themselves, or the window crops of a padded
// source format (the digests always cover the whole coded picture d_pic)
static hevcdl_status report_dev(hevcdl_ctx *ctx, const void *d_org_opt, const void *d_pic, int n_frames, int method, void *d_out, void *stream,
                                const void *sse_org, const void *sse_pic, int sse_w, int sse_h)
{
  TRY(check_frames(ctx, n_frames));
  TRY(check_method(ctx, method, "picture report"));
  if (n_frames == 0) return HEVCDL_OK;
  if (!d_pic || !d_out || ((uintptr_t)d_out & 7)) return fail(ctx, HEVCDL_ERR_INVALID_ARG, "picture report: null or misaligned device pointer");
  const size_t out_b = sizeof(hevcdl_picture_report_t) * (size_t)n_frames, span = ctx->frame_bytes * (size_t)n_frames;
  if (overlaps(d_out, out_b, d_org_opt, span) || overlaps(d_out, out_b, d_pic, span)) return fail(ctx, HEVCDL_ERR_INVALID_ARG, "picture report: the output overlaps an input");
  hipStream_t s = (hipStream_t)stream;
  TRY(ensure_report_workspace(ctx));
  if (ctx->profile) for (Event &e : ctx->rp_ev) if (!e) HIPCHK(hipEventCreate(&e.p));
  HIPCHK(hipMemsetAsync(d_out, 0, sizeof(hevcdl_picture_report_t) * (size_t)n_frames, s));
  if (ctx->profile) HIPCHK(hipEventRecord(ctx->rp_ev[0], s));
  if (d_org_opt) { // the exact SSE: quality_kernel.hip's kernel alone, into hevcdl_quality-shaped words the finish kernel copies from
    hevcdl_quality_params q; quality_sized_params(ctx, &q, sse_w, sse_h);
    q.org = sse_org; q.pic = sse_pic; q.out = ctx->rp.d_rp_sse; q.n_pics = n_frames; q.out_first = 0;
    HIPCHK(hipMemsetAsync(ctx->rp.d_rp_sse, 0, sizeof(hevcdl_quality) * (size_t)n_frames, s));
    hevcdl_launch_quality_sse(&q, s);
  }
  hevcdl_report_params p; report_picture_params(ctx, &p);
  p.pic = d_pic; p.out = d_out; p.partials = ctx->rp.d_rp_partials; p.sse = d_org_opt ? ctx->rp.d_rp_sse.p : nullptr; p.n_pics = n_frames; p.out_first = 0; p.method = method;
  void *ev[3] = { ctx->rp_ev[1].p, ctx->rp_ev[2].p, ctx->rp_ev[3].p };
  hevcdl_launch_report(&p, s, ctx->profile ? ev : nullptr);
  HIPCHK(hipGetLastError());
  if (ctx->profile) { // timing is a diagnostic: the call then waits for its launches
    HIPCHK(hipEventSynchronize(ctx->rp_ev[3]));
    for (int i = 0; i < 3; i++) { float ms = 0.f; HIPCHK(hipEventElapsedTime(&ms, ctx->rp_ev[i], ctx->rp_ev[i + 1])); ctx->rp_ms[i] = ms; }
  }
  return HEVCDL_OK;
}

extern "C" hevcdl_status hevcdl_picture_report_dev(hevcdl_ctx *ctx, const void *d_org_opt, const void *d_pic, int n_frames, int method, void *d_out, void *stream)
{
  if (!ctx) return HEVCDL_ERR_INVALID_ARG;
  return report_dev(ctx, d_org_opt, d_pic, n_frames, method, d_out, stream, d_org_opt, d_pic, ctx->cfg.width, ctx->cfg.height);
}

extern "C" hevcdl_status hevcdl_picture_report(hevcdl_ctx *ctx, const void *org_opt, const void *pic, int n_frames, int method, hevcdl_picture_report_t *out)
{
  TRY(check_frames(ctx, n_frames));
  TRY(check_method(ctx, method, "picture report"));
  if (n_frames == 0) return HEVCDL_OK;
  if (!pic || !out) return fail(ctx, HEVCDL_ERR_INVALID_ARG, "null pointer");
  TRY(ensure_staging(ctx));
  TRY(ensure_report_workspace(ctx));
  if (org_opt) HIPCHK(hipMemcpy(ctx->stage.d_yuv, org_opt, ctx->frame_bytes * n_frames, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(ctx->stage.d_recon, pic, ctx->frame_bytes * n_frames, hipMemcpyHostToDevice));
  TRY(hevcdl_picture_report_dev(ctx, org_opt ? ctx->stage.d_yuv.p : nullptr, ctx->stage.d_recon, n_frames, method, ctx->rp.d_rp_out, nullptr));
  TRY(sync_or_fail(ctx, "report kernels"));
  HIPCHK(hipMemcpy(out, ctx->rp.d_rp_out, sizeof(hevcdl_picture_report_t) * (size_t)n_frames, hipMemcpyDeviceToHost));
  return HEVCDL_OK;
}

// One plane of any size (host buffers, no context) through the same kernels: for callers (the tests) whose planes are not a context's 4:2:0 picture.
extern "C" hevcdl_status hevcdl_plane_hash(int device, const void *plane, int width, int height, int bit_depth, int method, uint8_t *digest16)
{
  if (!plane || !digest16 || width < 1 || height < 1 || width > (1 << 20) || height > (1 << 20) || (long long)width * height > (1ll << 28) || method < 1 || method > 3) return HEVCDL_ERR_INVALID_ARG;
  if (bit_depth < 8 || bit_depth > 16) return HEVCDL_ERR_UNSUPPORTED;
  TRY(select_device(device));
  hevcdl_report_params p; report_plane_params(&p, 1, &width, &height, bit_depth > 8 ? 2 : 1);
  p.n_pics = 1; p.method = method;
  DevBuf<unsigned char> d_pic, d_out; DevBuf<uint32_t> d_part;
  TRY(alloc_all(nullptr, { want(d_pic, p.frame_bytes), want(d_part, sizeof(uint32_t) * 3 * (size_t)p.chunk_stride), want(d_out, sizeof(hevcdl_picture_report_t)) }, ""));
  hevcdl_picture_report_t r; memset(&r, 0, sizeof r);
  hipError_t e = hipMemcpy(d_pic, plane, p.frame_bytes, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemset(d_out, 0, sizeof r);
  if (e == hipSuccess) {
    p.pic = d_pic; p.partials = d_part; p.out = d_out;
    hevcdl_launch_report(&p, nullptr, nullptr);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(&r, d_out, sizeof r, hipMemcpyDeviceToHost);
  }
  if (e != hipSuccess) return hip_fail(nullptr, "", e);
  memset(digest16, 0, 16); memcpy(digest16, r.digest, (size_t)r.plane_bytes);
  return HEVCDL_OK;
}

extern "C" hevcdl_status hevcdl_enable_picture_report(hevcdl_ctx *ctx, int on, int method)
{
  if (!ctx) return HEVCDL_ERR_INVALID_ARG;
  if (on) { // the whole of what the switch costs is reserved here
    TRY(check_method(ctx, method, "hevcdl_enable_picture_report"));
    TRY(check_frames(ctx, 0));
    TRY(ensure_report_workspace(ctx));
    ctx->rp.report_on = true; ctx->rp.report_method = method;
    return HEVCDL_OK;
  }
  ctx->rp.report_on = false; ctx->rp.report_method = 0; ctx->rp.h_report.clear();
  TRY(sync_or_fail(ctx, "hevcdl_enable_picture_report"));
  ctx->rp = Report();      // off: the workspace goes back (a later hevcdl_picture_report* call allocates its own again)
  return HEVCDL_OK;
}

extern "C" hevcdl_status hevcdl_get_picture_report(hevcdl_ctx *ctx, int first, int count, hevcdl_picture_report_t *out)
{
  if (!ctx) return HEVCDL_ERR_INVALID_ARG;
  TRY(check_batch_range(ctx, "hevcdl_get_picture_report", out != nullptr, ctx->rp.report_on, "hevcdl_enable_picture_report", first, count, (long long)ctx->rp.h_report.size()));
  if (count) memcpy(out, ctx->rp.h_report.data() + first, sizeof(hevcdl_picture_report_t) * (size_t)count);
  return HEVCDL_OK;
}

extern "C" hevcdl_status hevcdl_get_report_info(hevcdl_ctx *ctx, double *kernel_ms)
{
  if (!ctx || !kernel_ms) return HEVCDL_ERR_INVALID_ARG;
  for (int i = 0; i < 3; i++) kernel_ms[i] = ctx->rp_ms[i];
  return HEVCDL_OK;
}

// ---- source and output formats (source_kernel.hip; the arithmetic and the host mirrors: source_core.h, hevcdl_bitstream.cpp) ---------------------------------------
static void source_release(hevcdl_ctx *ctx)
{
  ctx->src = Source();
}

extern "C" hevcdl_status hevcdl_set_source_format(hevcdl_ctx *ctx, const hevcdl_source_format *fmt)
{
  TRY(check_frames(ctx, 0));
  if (fmt && (fmt->struct_size != sizeof *fmt || !hevcdl_src::format_fits(fmt->source_width, fmt->source_height, fmt->input_bit_depth, fmt->output_bit_depth, ctx->cfg.width, ctx->cfg.height)))
    return fail(ctx, HEVCDL_ERR_INVALID_ARG, "source format: even source size of at least 2 x 2 and at most the context's, even padding, bit depths 8 .. 16");
  if (fmt && !hevcdl_source_format_fits(fmt, ctx->cfg.width, ctx->cfg.height))
    return fail(ctx, HEVCDL_ERR_INVALID_ARG, "source format: chroma format 400 / 420 / 422 / 444, colour space 0 / 1 (not with 400), window offsets even, with something left of the picture and without padding");
  TRY(sync_or_fail(ctx, "hevcdl_set_source_format"));
  source_release(ctx);
  if (!fmt) return HEVCDL_OK;
  ctx->src.src_fmt = *fmt;
  const bool windowed = fmt->source_width != ctx->cfg.width || fmt->source_height != ctx->cfg.height;
  const size_t nf = (size_t)ctx->cfg.max_frames, win_b = hevcdl_src::picture_samples(fmt->source_width, fmt->source_height) * (ctx->cfg.bit_depth > 8 ? 2 : 1);
  Source &g = ctx->src;
  const char *what = "source format buffers (cfg.max_frames)";
  hevcdl_status st = alloc_all(ctx, { want(g.d_src, std::max(hevcdl_source_frame_bytes(fmt), hevcdl_output_frame_bytes(fmt)) * nf) }, what);      // the whole of what the format costs is reserved here
  if (!st && windowed) st = alloc_all(ctx, { want(g.d_win_org, win_b * nf), want(g.d_win_pic, win_b * nf), want(g.d_win_sse, sizeof(hevcdl_quality) * nf) }, what);
  if (st) { source_release(ctx); return st; }
  ctx->src.source_on = true; ctx->src.source_windowed = windowed;
  return HEVCDL_OK;
}

static hevcdl_status source_check(hevcdl_ctx *ctx, int n_frames, const void *a, const void *b, int a_bytes, int b_bytes)
{
  TRY(check_frames(ctx, n_frames));
  if (!ctx->src.source_on) return fail(ctx, HEVCDL_ERR_INVALID_ARG, "hevcdl_set_source_format was not called");
  if (n_frames && (!a || !b || ((uintptr_t)a & (a_bytes - 1)) || ((uintptr_t)b & (b_bytes - 1)))) return fail(ctx, HEVCDL_ERR_INVALID_ARG, "source format: null or misaligned device pointer");
  return HEVCDL_OK;
}

extern "C" hevcdl_status hevcdl_load_source_dev(hevcdl_ctx *ctx, const void *d_src, int n_frames, void *d_coded, void *stream)
{
  if (!ctx) return HEVCDL_ERR_INVALID_ARG;
  hevcdl_source_params p; memset(&p, 0, sizeof p);
  p.src_bytes = ctx->src.src_fmt.input_bit_depth > 8 ? 2 : 1; p.dst_bytes = ctx->cfg.bit_depth > 8 ? 2 : 1;
  TRY(source_check(ctx, n_frames, d_src, d_coded, p.src_bytes, p.dst_bytes));
  if (n_frames == 0) return HEVCDL_OK;
  p.src = d_src; p.dst = d_coded; p.src_w = ctx->src.src_fmt.source_width; p.src_h = ctx->src.src_fmt.source_height; p.dst_w = ctx->cfg.width; p.dst_h = ctx->cfg.height;
  p.from_depth = ctx->src.src_fmt.input_bit_depth; p.to_depth = ctx->cfg.bit_depth; p.n_pics = n_frames;
  const hevcdl_source_format &f = ctx->src.src_fmt;
  if (hevcdl_src::chroma_format_id(f.chroma_format) != hevcdl_src::FMT_420 || f.colour_space) { // the file's layout: the kernels of their own (a 4:2:0 file in the coded order runs what it ran)
    hevcdl_source_fmt_params q; memset(&q, 0, sizeof q);
    q.b = p; q.chroma_format = hevcdl_src::chroma_format_id(f.chroma_format); q.swap = f.colour_space;
    hevcdl_launch_source_load_fmt(&q, stream);
  } else
  hevcdl_launch_source_load(&p, stream);
  return launch_status(ctx);
}

// coded pictures -> pictures of the window's size at to_depth.  output: the output frames (the explicit window, the planes back in the file's order); otherwise the crop
// the quality kernels measure a padded picture by (the coded picture minus the padding, coded plane order)
static hevcdl_status store_window_dev(hevcdl_ctx *ctx, const void *d_pictures, int n_frames, void *d_out, void *stream, int to_depth, bool output)
{
  hevcdl_source_params p; memset(&p, 0, sizeof p);
  p.src_bytes = ctx->cfg.bit_depth > 8 ? 2 : 1; p.dst_bytes = to_depth > 8 ? 2 : 1;
  TRY(source_check(ctx, n_frames, d_pictures, d_out, p.src_bytes, p.dst_bytes));
  if (n_frames == 0) return HEVCDL_OK;
  p.src = d_pictures; p.dst = d_out; p.src_w = ctx->cfg.width; p.src_h = ctx->cfg.height; p.dst_w = ctx->src.src_fmt.source_width; p.dst_h = ctx->src.src_fmt.source_height;
  p.from_depth = ctx->cfg.bit_depth; p.to_depth = to_depth; p.n_pics = n_frames;
  const hevcdl_source_format &f = ctx->src.src_fmt;
  const int swap = f.colour_space && !f.output_internal_colour_space;
  if (output && (swap || (f.conf_win_left | f.conf_win_right | f.conf_win_top | f.conf_win_bottom))) {
    hevcdl_source_fmt_params q; memset(&q, 0, sizeof q);
    q.b = p; hevcdl_source_window_size(&f, &q.b.dst_w, &q.b.dst_h);
    q.chroma_format = hevcdl_src::FMT_420; q.swap = swap; q.win_x = f.conf_win_left; q.win_y = f.conf_win_top;
    hevcdl_launch_source_store_fmt(&q, stream);
  } else
  hevcdl_launch_source_store(&p, stream);
  return launch_status(ctx);
}
extern "C" hevcdl_status hevcdl_store_output_dev(hevcdl_ctx *ctx, const void *d_pictures, int n_frames, void *d_out, void *stream)
{
  if (!ctx) return HEVCDL_ERR_INVALID_ARG;
  return store_window_dev(ctx, d_pictures, n_frames, d_out, stream, ctx->src.src_fmt.output_bit_depth, true);
}
// the window at the internal depth, contiguous: what the quality kernels measure a padded picture by (the store kernel with OUT = PEL, no scaling)
static hevcdl_status crop_window_dev(hevcdl_ctx *ctx, const void *d_pictures, int n_frames, void *d_out, void *stream) { return store_window_dev(ctx, d_pictures, n_frames, d_out, stream, ctx->cfg.bit_depth, false); }

extern "C" hevcdl_status hevcdl_load_source(hevcdl_ctx *ctx, const void *src, int n_frames, void *coded_out)
{
  TRY(source_check(ctx, n_frames, src, coded_out, 1, 1));
  if (n_frames == 0) return HEVCDL_OK;
  TRY(ensure_staging(ctx));
  HIPCHK(hipMemcpy(ctx->src.d_src, src, hevcdl_source_frame_bytes(&ctx->src.src_fmt) * n_frames, hipMemcpyHostToDevice));
  TRY(hevcdl_load_source_dev(ctx, ctx->src.d_src, n_frames, ctx->stage.d_yuv, nullptr));
  TRY(sync_or_fail(ctx, "source load kernel"));
  HIPCHK(hipMemcpy(coded_out, ctx->stage.d_yuv, ctx->frame_bytes * n_frames, hipMemcpyDeviceToHost));
  return HEVCDL_OK;
}

extern "C" hevcdl_status hevcdl_store_output(hevcdl_ctx *ctx, const void *pictures, int n_frames, void *out)
{
  TRY(source_check(ctx, n_frames, pictures, out, 1, 1));
  if (n_frames == 0) return HEVCDL_OK;
  TRY(ensure_staging(ctx));
  HIPCHK(hipMemcpy(ctx->stage.d_recon, pictures, ctx->frame_bytes * n_frames, hipMemcpyHostToDevice));
  TRY(hevcdl_store_output_dev(ctx, ctx->stage.d_recon, n_frames, ctx->src.d_src, nullptr));
  TRY(sync_or_fail(ctx, "source store kernel"));
  HIPCHK(hipMemcpy(out, ctx->src.d_src, hevcdl_output_frame_bytes(&ctx->src.src_fmt) * n_frames, hipMemcpyDeviceToHost));
  return HEVCDL_OK;
}

// output-format frames of pictures of the last picture pipeline call, cropped and scaled where the pictures are: a run that needs its pictures only for the reconstruction
// file fetches the window at the output depth instead of the coded pictures (the upload buffer is free again once the load kernel has run: it is the staging)
extern "C" hevcdl_status hevcdl_get_output_frames(hevcdl_ctx *ctx, int first, int count, void *out)
{
  if (!ctx) return HEVCDL_ERR_INVALID_ARG;
  if (!ctx->src.source_on) return fail(ctx, HEVCDL_ERR_INVALID_ARG, "hevcdl_get_output_frames: hevcdl_set_source_format was not called");
  if (!out || first < 0 || count < 0 || !ctx->src.d_last_final || (long long)first + count > ctx->src.last_frames) return fail(ctx, HEVCDL_ERR_INVALID_ARG, "hevcdl_get_output_frames: pictures outside the last batch");
  if (count == 0) return HEVCDL_OK;
  TRY(hevcdl_store_output_dev(ctx, ctx->src.d_last_final + ctx->frame_bytes * (size_t)first, count, ctx->src.d_src, nullptr));
  HIPCHK(hipStreamSynchronize(nullptr));
  HIPCHK(hipMemcpy(out, ctx->src.d_src, hevcdl_output_frame_bytes(&ctx->src.src_fmt) * (size_t)count, hipMemcpyDeviceToHost));
  return HEVCDL_OK;
}

// ---- whole picture pipeline for host buffers: the stages of TEncGOP::compressGOP between reading a picture and writing its NAL units, with
// the picture staying in HBM in between (one upload of the originals, one download of records / final picture / SAO parameters) ----------
// device side of hevcdl_encode_pictures*: upload, labels, decisions, in-loop filters; the results stay in HBM (*d_final: the output pictures)
static hevcdl_status entropy_pipeline(hevcdl_ctx *ctx, int n_frames, int want_sao);
static hevcdl_status encode_pictures_device(hevcdl_ctx *ctx, const void *yuv, int n_frames, const uint8_t *labels_opt, int deblock, int want_sao, uint8_t **d_final)
{
  ctx->dbk.h_choice.clear();
  if (ctx->cfg.deblocking_metric != 0 && !deblock) return fail(ctx, HEVCDL_ERR_INVALID_ARG, "If DeblockingFilterMetric is non-zero then both LoopFilterDisable and LoopFilterOffsetInPPS must be 0");
  TRY(ensure_staging(ctx));
  if (want_sao) TRY(lazy_alloc(ctx, ctx->sao.d_sao_params, ctx->sao_bytes(ctx->cfg.max_frames), "SAO parameters (cfg.max_frames)"));
  if (want_sao) TRY(lazy_alloc(ctx, ctx->stage.d_picture, ctx->frame_bytes * (size_t)ctx->cfg.max_frames, "output pictures (cfg.max_frames)"));
  ctx->src.d_last_final = nullptr; ctx->src.last_frames = 0;
  const bool windowed = ctx->src.source_on && ctx->src.source_windowed;
  const int ww = windowed ? ctx->src.src_fmt.source_width : ctx->cfg.width, wh = windowed ? ctx->src.src_fmt.source_height : ctx->cfg.height;      // what SSE and MS-SSIM are taken over
  if (ctx->src.source_on) { // hevcdl_set_source_format: the source's own bytes go up; the load kernel pads and converts them in front of everything else
    HIPCHK(hipMemcpy(ctx->src.d_src, yuv, hevcdl_source_frame_bytes(&ctx->src.src_fmt) * n_frames, hipMemcpyHostToDevice));
    TRY(hevcdl_load_source_dev(ctx, ctx->src.d_src, n_frames, ctx->stage.d_yuv, nullptr));
    if (windowed) { TRY(crop_window_dev(ctx, ctx->stage.d_yuv, n_frames, ctx->src.d_win_org, nullptr)); }
  } else
  HIPCHK(hipMemcpy(ctx->stage.d_yuv, yuv, ctx->frame_bytes * n_frames, hipMemcpyHostToDevice));
  TRY(stage_labels(ctx, labels_opt, n_frames));
  TRY(hevcdl_compress_frames_dev(ctx, ctx->stage.d_yuv, n_frames, ctx->stage.d_labels, ctx->stage.d_records, ctx->stage.d_recon, ctx->stage.d_stats, nullptr));
  const int32_t *pic_idx = nullptr;      // DeltaQpRD: the candidate every picture ended with -- a few words a picture to the host, then every later stage runs with the picture's own QP
  ctx->qprd.h_idx.clear();
  if (ctx->qprd.n) {
    std::vector<hevcdl_qp_rd_row> &rows = ctx->qprd.h_rows;
    rows.resize((size_t)n_frames);
    HIPCHK(hipMemcpy(rows.data(), ctx->qprd.d_rows, sizeof(hevcdl_qp_rd_row) * (size_t)n_frames, hipMemcpyDeviceToHost));      // (behind the launches of the null stream)
    for (const hevcdl_qp_rd_row &r : rows) ctx->qprd.h_idx.push_back(r.best_idx);
    TRY(check_qp_rd_idx(ctx, ctx->qprd.h_idx.data(), n_frames));
    pic_idx = ctx->qprd.h_idx.data();
  }
  if (windowed) { // the statistics' SSE (the reconstruction before the in-loop filters) over the window: the decision kernel summed over the padding too
    TRY(crop_window_dev(ctx, ctx->stage.d_recon, n_frames, ctx->src.d_win_pic, nullptr));
    hevcdl_quality_params q; quality_sized_params(ctx, &q, ww, wh);
    q.org = ctx->src.d_win_org; q.pic = ctx->src.d_win_pic; q.out = ctx->src.d_win_sse; q.n_pics = n_frames; q.out_first = 0;
    HIPCHK(hipMemsetAsync(ctx->src.d_win_sse, 0, sizeof(hevcdl_quality) * (size_t)n_frames, nullptr));
    hevcdl_launch_quality_sse(&q, nullptr);
    hipLaunchKernelGGL(hevcdl_stats_sse_kernel, dim3((3 * n_frames + 255) / 256), dim3(256), 0, nullptr, (const hevcdl_quality *)ctx->src.d_win_sse.p, (hevcdl_frame_stats *)ctx->stage.d_stats.p, n_frames);
    HIPCHK(hipGetLastError());
  }
  *d_final = ctx->stage.d_recon;
  { // what every picture's slice header says and its filter runs with: the cfg's values, or (DeblockingFilterMetric 1) what the picture's blockiness asks for -- the
    // metric launch, two words a picture to the host, the reference's integer lines there, a row of parameters a picture back
    std::vector<hevcdl_dbk_choice> &ch = ctx->dbk.h_choice;
    const int enabled = ctx->cfg.deblocking_metric != 0 || ctx->cfg.lf_offset_in_pps == 0;      // TEncTop.cpp:1007-1016
    const hevcdl_dbk_choice plain = { enabled, enabled, deblock ? 0 : 1, deblock ? ctx->cfg.lf_beta_offset_div2 : 0, deblock ? ctx->cfg.lf_tc_offset_div2 : 0 };
    ch.assign((size_t)n_frames, plain);
    if (ctx->cfg.deblocking_metric == 1) {
      TRY(lazy_alloc(ctx, ctx->dbk.d_sums, sizeof(unsigned long long) * 49 * (size_t)ctx->cfg.max_frames, "deblocking metric sums (cfg.max_frames)"));
      TRY(hevcdl_dbk_metric_frames_dev(ctx, ctx->stage.d_recon, n_frames, ctx->dbk.d_sums, nullptr));
      ctx->dbk.h_sums.resize((size_t)2 * n_frames);
      HIPCHK(hipMemcpy(ctx->dbk.h_sums.data(), ctx->dbk.d_sums, sizeof(unsigned long long) * 2 * (size_t)n_frames, hipMemcpyDeviceToHost));      // (behind the launches of the null stream)
      for (int i = 0; i < n_frames; i++)
        hevcdl_dbk_metric_choice(ctx->cfg.width, ctx->cfg.height, ctx->cfg.bit_depth, ctx->dbk.h_sums[2 * i], ctx->dbk.h_sums[2 * i + 1], ctx->cfg.lf_beta_offset_div2, ctx->cfg.lf_tc_offset_div2, &ch[(size_t)i]);
      TRY(hevcdl_deblock_frames_choice_dev(ctx, ctx->stage.d_recon, n_frames, ctx->stage.d_records, ch.data(), ctx->stage.d_recon, nullptr));      // in place
    } else if (ctx->cfg.deblocking_metric == 2) { // one trial launch fills a 7 x 7 table a picture; the walk takes the pictures in order, each from the state the one before left
      TRY(lazy_alloc(ctx, ctx->dbk.d_sums, sizeof(unsigned long long) * 49 * (size_t)ctx->cfg.max_frames, "deblocking trial tables (cfg.max_frames)"));
      TRY(hevcdl_dbk_trial_frames_dev(ctx, ctx->stage.d_yuv, ctx->stage.d_recon, n_frames, ctx->stage.d_records, ctx->dbk.d_sums, nullptr));
      ctx->dbk.h_sums.resize((size_t)49 * n_frames);
      HIPCHK(hipMemcpy(ctx->dbk.h_sums.data(), ctx->dbk.d_sums, sizeof(unsigned long long) * 49 * (size_t)n_frames, hipMemcpyDeviceToHost));
      for (int i = 0; i < n_frames; i++) {
        const hevcdl_dbk_walk_result r = hevcdl_dbk_walk((const uint64_t *)&ctx->dbk.h_sums[(size_t)49 * i], ctx->cfg.lf_beta_offset_div2, ctx->cfg.lf_tc_offset_div2, &ctx->dbk.walk);
        ch[(size_t)i] = hevcdl_dbk_choice{ 1, r.override_flag, r.disabled, r.beta_offset_div2, r.tc_offset_div2 };
      }
      TRY(hevcdl_deblock_frames_choice_dev(ctx, ctx->stage.d_recon, n_frames, ctx->stage.d_records, ch.data(), ctx->stage.d_recon, nullptr));      // in place
    } else
    if (deblock) { TRY(hevcdl_deblock_frames_qp_dev(ctx, ctx->stage.d_recon, n_frames, ctx->stage.d_records, nullptr, pic_idx, ctx->stage.d_recon, nullptr)); }      // in place (pic_idx NULL: hevcdl_deblock_frames_dev)
  }
  if (want_sao) { TRY(hevcdl_sao_frames_qp_dev(ctx, ctx->stage.d_yuv, ctx->stage.d_recon, n_frames, pic_idx, ctx->sao.d_sao_params, ctx->stage.d_picture, nullptr)); *d_final = ctx->stage.d_picture; }
  ctx->q.h_quality.clear();
  ctx->rp.h_report.clear();
  if (windowed && (ctx->q.quality_on || ctx->rp.report_on)) { TRY(crop_window_dev(ctx, *d_final, n_frames, ctx->src.d_win_pic, nullptr)); }      // the output pictures' window (TEncGOP.cpp:2302-2303, 2375-2376, 2413-2414)
  if (ctx->q.quality_on) { // the output pictures against the originals, both still in HBM
    TRY(lazy_alloc(ctx, ctx->q.d_q_out, sizeof(hevcdl_quality) * (size_t)ctx->cfg.max_frames, "picture quality results"));
    TRY(windowed ? quality_sized_dev(ctx, ctx->src.d_win_org, ctx->src.d_win_pic, n_frames, ctx->q.d_q_out, nullptr, ww, wh)
                 : hevcdl_picture_quality_dev(ctx, ctx->stage.d_yuv, *d_final, n_frames, ctx->q.d_q_out, nullptr));
  }
  if (ctx->rp.report_on) { // hevcdl_enable_picture_report: SSE and digests of the output pictures, where they are (the digests over the whole coded picture, as the hash SEI)
    TRY(windowed ? report_dev(ctx, ctx->stage.d_yuv, *d_final, n_frames, ctx->rp.report_method, ctx->rp.d_rp_out, nullptr, ctx->src.d_win_org, ctx->src.d_win_pic, ww, wh)
                 : hevcdl_picture_report_dev(ctx, ctx->stage.d_yuv, *d_final, n_frames, ctx->rp.report_method, ctx->rp.d_rp_out, nullptr));
  }
  TRY(sync_or_fail(ctx, "picture pipeline"));
  // YCbCrtoYCrCb without SNRInternalColourSpace: the reference measures against the file's planes, so its U column is the coded picture's third plane (TEncGOP.cpp xCalculateAddPSNR)
  const bool file_order = ctx->src.source_on && ctx->src.src_fmt.colour_space && !ctx->src.src_fmt.snr_internal_colour_space;
  if (ctx->rp.report_on) {
    ctx->rp.h_report.resize(n_frames);
    HIPCHK(hipMemcpy(ctx->rp.h_report.data(), ctx->rp.d_rp_out, sizeof(hevcdl_picture_report_t) * (size_t)n_frames, hipMemcpyDeviceToHost));
    if (file_order) for (hevcdl_picture_report_t &r : ctx->rp.h_report) std::swap(r.sse[1], r.sse[2]);      // (the digests stay the coded picture's)
  }
  if (ctx->q.quality_on) {
    ctx->q.h_quality.resize(n_frames);
    HIPCHK(hipMemcpy(ctx->q.h_quality.data(), ctx->q.d_q_out, sizeof(hevcdl_quality) * (size_t)n_frames, hipMemcpyDeviceToHost));
    if (file_order) for (hevcdl_quality &r : ctx->q.h_quality) { std::swap(r.sse[1], r.sse[2]); std::swap(r.msssim[1], r.msssim[2]); }
  }
  if (ctx->ec.entropy_on) { TRY(entropy_pipeline(ctx, n_frames, want_sao)); }      // hevcdl_enable_device_entropy: the slice data too, from the records still in HBM
  ctx->src.d_last_final = *d_final; ctx->src.last_frames = n_frames;
  return HEVCDL_OK;
}

extern "C" hevcdl_status hevcdl_encode_pictures(hevcdl_ctx *ctx, const void *yuv, int n_frames, const uint8_t *labels_opt, int deblock, hevcdl_ctu_record *records,
                                                void *picture_out, hevcdl_sao_blk *sao_opt, hevcdl_frame_stats *stats_opt)
{
  FRAMES_OR_RETURN(ctx, n_frames);
  if (!yuv || !records || !picture_out) return fail(ctx, HEVCDL_ERR_INVALID_ARG, "null pointer");
  uint8_t *d_final = nullptr;
  TRY(encode_pictures_device(ctx, yuv, n_frames, labels_opt, deblock, sao_opt != nullptr, &d_final));
  HIPCHK(hipMemcpy(records, ctx->stage.d_records, ctx->records_bytes(n_frames), hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(picture_out, d_final, ctx->frame_bytes * n_frames, hipMemcpyDeviceToHost));
  if (sao_opt) HIPCHK(hipMemcpy(sao_opt, ctx->sao.d_sao_params, ctx->sao_bytes(n_frames), hipMemcpyDeviceToHost));
  if (stats_opt) HIPCHK(hipMemcpy(stats_opt, ctx->stage.d_stats, sizeof(hevcdl_frame_stats) * n_frames, hipMemcpyDeviceToHost));
  return HEVCDL_OK;
}

// the two page-locked chunk buffers of hevcdl_encode_pictures_chunked / _stream, grown to `need` bytes each
static hevcdl_status ensure_chunk_buffers(hevcdl_ctx *ctx, size_t need)
{
  Staging &g = ctx->stage;
  if (g.h_chunk_bytes >= need) return HEVCDL_OK;
  for (HostBuf &h : g.h_chunk) h.reset();
  g.h_chunk_bytes = 0;
  for (HostBuf &h : g.h_chunk) HIPCHK(hipHostMalloc((void **)&h.p, need, hipHostMallocDefault));
  g.h_chunk_bytes = need;
  return HEVCDL_OK;
}

extern "C" hevcdl_status hevcdl_encode_pictures_chunked(hevcdl_ctx *ctx, const void *yuv, int n_frames, const uint8_t *labels_opt, int deblock, int want_sao,
                                                        int chunk_frames, hevcdl_chunk_fn fn, void *user)
{
  FRAMES_OR_RETURN(ctx, n_frames);
  if (!yuv || !fn) return fail(ctx, HEVCDL_ERR_INVALID_ARG, "null pointer");
  const int chunk = std::min(n_frames, chunk_frames > 0 ? chunk_frames : 64);
  const size_t rec_b = ctx->records_bytes(1), sao_b = ctx->sao_bytes(1), pic_b = ctx->frame_bytes, stat_b = sizeof(hevcdl_frame_stats);
  auto up64 = [](size_t v) { return (v + 63) & ~(size_t)63; };      // every section of a chunk buffer starts on a 64-byte boundary (the callback gets pointers to structs with 64-bit members)
  const size_t o_pic = up64(rec_b * chunk), o_sao = up64(o_pic + pic_b * chunk), o_stat = up64(o_sao + sao_b * chunk), need = o_stat + stat_b * chunk;      // layout of a chunk buffer
  TRY(ensure_chunk_buffers(ctx, need));
  if (!ctx->stage.copy_stream) { HIPCHK(hipStreamCreateWithFlags(&ctx->stage.copy_stream.p, hipStreamNonBlocking)); for (Event &e : ctx->stage.copy_ev) HIPCHK(hipEventCreateWithFlags(&e.p, hipEventDisableTiming)); }
  uint8_t *d_final = nullptr;
  TRY(encode_pictures_device(ctx, yuv, n_frames, labels_opt, deblock, want_sao, &d_final));
  auto fetch = [&](int ci) -> hipError_t { // chunk ci -> buffer ci & 1, asynchronously
    const int first = ci * chunk, cnt = std::min(chunk, n_frames - first);
    unsigned char *h = ctx->stage.h_chunk[ci & 1];
    hipError_t e = hipMemcpyAsync(h, ctx->stage.d_records + rec_b * first, rec_b * cnt, hipMemcpyDeviceToHost, ctx->stage.copy_stream);
    if (e == hipSuccess) e = hipMemcpyAsync(h + o_pic, d_final + pic_b * first, pic_b * cnt, hipMemcpyDeviceToHost, ctx->stage.copy_stream);
    if (e == hipSuccess && want_sao) e = hipMemcpyAsync(h + o_sao, ctx->sao.d_sao_params + sao_b * first, sao_b * cnt, hipMemcpyDeviceToHost, ctx->stage.copy_stream);
    if (e == hipSuccess) e = hipMemcpyAsync(h + o_stat, ctx->stage.d_stats + stat_b * first, stat_b * cnt, hipMemcpyDeviceToHost, ctx->stage.copy_stream);
    if (e == hipSuccess) e = hipEventRecord(ctx->stage.copy_ev[ci & 1], ctx->stage.copy_stream);
    return e;
  };
  const int n_chunks = (n_frames + chunk - 1) / chunk;
  HIPCHK(fetch(0));
  for (int ci = 0; ci < n_chunks; ci++) {
    { hipError_t e_ = hipEventSynchronize(ctx->stage.copy_ev[ci & 1]);
      if (e_ == hipSuccess && ci + 1 < n_chunks) e_ = fetch(ci + 1);                   // into the other buffer, behind the caller's work on this one
      if (e_ != hipSuccess) { (void)hipStreamSynchronize(ctx->stage.copy_stream); return fail(ctx, HEVCDL_ERR_HIP, "chunk copy", e_); } }     // no copy into the library's buffers is left in flight
    const int first = ci * chunk, cnt = std::min(chunk, n_frames - first);
    unsigned char *h = ctx->stage.h_chunk[ci & 1];
    if (fn(user, first, cnt, (const hevcdl_ctu_record *)h, h + o_pic, want_sao ? (const hevcdl_sao_blk *)(h + o_sao) : nullptr, (const hevcdl_frame_stats *)(h + o_stat)) != 0) {
      hipStreamSynchronize(ctx->stage.copy_stream);
      return fail(ctx, HEVCDL_ERR_INVALID_ARG, "the chunk callback asked to stop");
    }
  }
  return HEVCDL_OK;
}

// ---- slice data on the device (entropy_kernel.hip) ---------------------------------------------------------------------------------------------------------
// what the kernels need to know of a stream configuration
struct EntropyPlan {
  hevcdl_entropy_params k;             // geometry, QP, tools filled; pointers not
  std::vector<uint32_t> off, cap; size_t frame_stride; int units;
};
static hevcdl_status entropy_plan(const hevcdl_stream_config *cfg, const hevcdl_slice_layout *layout, const hevcdl_segment_layout *segments, int capacity_per_ctu, EntropyPlan &pl)
{
  int n = 0; size_t bytes = 0;
  TRY(hevcdl_slice_data_layout_segments(cfg, layout, segments, capacity_per_ctu, &n, &bytes, nullptr, nullptr));
  pl.off.resize((size_t)n); pl.cap.resize((size_t)n);
  TRY(hevcdl_slice_data_layout_segments(cfg, layout, segments, capacity_per_ctu, &n, &bytes, pl.off.data(), pl.cap.data()));
  pl.units = n; pl.frame_stride = bytes;
  hevcdl_entropy_params &k = pl.k; memset(&k, 0, sizeof k);
  k.width = cfg->width; k.height = cfg->height; k.ctus_x = (cfg->width + 63) >> 6; k.ctus_y = (cfg->height + 63) >> 6; k.qp = cfg->qp; k.tools = (int)cfg->tools;
  k.max_sao_offset = (1 << ((cfg->bit_depth < 10 ? cfg->bit_depth : 10) - 5)) - 1; k.wpp = cfg->wavefront != 0; k.units = n; k.frame_stride = bytes;
  int rows = 0;
  return (hevcdl_status)hevcdl_substream_grid(cfg, layout, segments, &k.tile_cols, &rows, k.col_bd, k.row_bd, &k.slice_units, &k.segment_units);    // the writer's own grid: the cfg's tiles, or a column of row slices
}

extern "C" hevcdl_status hevcdl_code_slice_data(int device, const hevcdl_stream_config *cfg, const hevcdl_ctu_record *records, const hevcdl_sao_blk *sao_opt, int n_frames,
                                                int capacity_per_ctu, uint8_t *out, size_t out_capacity, uint32_t *sizes, uint32_t *overflow)
{
  return hevcdl_code_slice_data_slices(device, cfg, nullptr, records, sao_opt, n_frames, capacity_per_ctu, out, out_capacity, sizes, overflow);
}

extern "C" hevcdl_status hevcdl_code_slice_data_slices(int device, const hevcdl_stream_config *cfg, const hevcdl_slice_layout *layout, const hevcdl_ctu_record *records,
                                                       const hevcdl_sao_blk *sao_opt, int n_frames, int capacity_per_ctu, uint8_t *out, size_t out_capacity, uint32_t *sizes, uint32_t *overflow)
{
  return hevcdl_code_slice_data_segments(device, cfg, layout, nullptr, records, sao_opt, n_frames, capacity_per_ctu, out, out_capacity, sizes, overflow);
}

extern "C" hevcdl_status hevcdl_code_slice_data_segments(int device, const hevcdl_stream_config *cfg, const hevcdl_slice_layout *layout, const hevcdl_segment_layout *segments,
                                                         const hevcdl_ctu_record *records, const hevcdl_sao_blk *sao_opt, int n_frames, int capacity_per_ctu, uint8_t *out, size_t out_capacity,
                                                         uint32_t *sizes, uint32_t *overflow)
{
  if (!cfg || !records || !out || !sizes || !overflow || n_frames < 0) return HEVCDL_ERR_INVALID_ARG;
  EntropyPlan pl;
  TRY(entropy_plan(cfg, layout, segments, capacity_per_ctu, pl));
  if ((cfg->sao_enabled != 0) != (sao_opt != nullptr)) return HEVCDL_ERR_INVALID_ARG;
  if (out_capacity / (pl.frame_stride ? pl.frame_stride : 1) < (size_t)n_frames) return HEVCDL_ERR_INVALID_ARG;
  if (n_frames == 0) return HEVCDL_OK;
  TRY(select_device(device));
  const size_t ctus = (size_t)pl.k.ctus_x * pl.k.ctus_y, n_sub = (size_t)n_frames * pl.units;
  const size_t rec_b = ctus * sizeof(hevcdl_ctu_record) * n_frames, sao_b = sao_opt ? ctus * sizeof(hevcdl_sao_blk) * n_frames : 4, out_b = pl.frame_stride * n_frames, unit_b = 4 * (size_t)pl.units;
  const size_t sync_b = (size_t)n_frames * pl.k.ctus_y * hevcdl_ec::EC_SYNC_BYTES;
  DevBuf<unsigned char> d_rec, d_sao, d_tables, d_out, d_sync; DevBuf<uint32_t> d_off, d_cap, d_sizes;      // d_sizes: the lengths, then the overflow flags
  TRY(alloc_all(nullptr, { want(d_rec, rec_b), want(d_sao, sao_b), want(d_tables, sizeof(hevcdl_ec::EcTables)), want(d_out, out_b), want(d_off, unit_b), want(d_cap, unit_b),
                           want(d_sizes, 8 * n_sub), want(d_sync, sync_b) }, ""));
  hipError_t e = hipMemcpy(d_rec, records, rec_b, hipMemcpyHostToDevice);
  if (e == hipSuccess && sao_opt) e = hipMemcpy(d_sao, sao_opt, sao_b, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d_tables, &hevcdl_ec::ec_tables(), sizeof(hevcdl_ec::EcTables), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d_out, out, out_b, hipMemcpyHostToDevice);      // what the kernels do not write comes back as the caller left it
  if (e == hipSuccess) e = hipMemcpy(d_off, pl.off.data(), unit_b, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d_cap, pl.cap.data(), unit_b, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemset(d_sizes, 0, 8 * n_sub);
  if (e == hipSuccess) e = hipMemset(d_sync, 0, sync_b);
  if (e == hipSuccess) {
    hevcdl_entropy_params k = pl.k;
    k.records = d_rec; k.sao = sao_opt ? d_sao.p : nullptr; k.tables = d_tables; k.out = d_out; k.unit_off = d_off; k.unit_cap = d_cap;
    k.sizes = d_sizes; k.overflow = d_sizes + n_sub; k.sync = d_sync; k.n_frames = n_frames;
    hevcdl_launch_entropy(&k, nullptr, nullptr);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(out, d_out, out_b, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(sizes, d_sizes, 4 * n_sub, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(overflow, d_sizes + n_sub, 4 * n_sub, hipMemcpyDeviceToHost);
  }
  if (e != hipSuccess) return hip_fail(nullptr, "", e);
  return HEVCDL_OK;
}

// the stream configuration a context's pictures are written with, as far as the slice data depends on it
static void entropy_stream_config(const hevcdl_ctx *ctx, int want_sao, hevcdl_stream_config *sc)
{
  const hevcdl_config &c = ctx->cfg;
  hevcdl_stream_config_default(sc, c.width, c.height, c.qp);
  sc->sao_enabled = want_sao != 0; sc->bit_depth = c.bit_depth; sc->tools = c.tools; sc->wavefront = c.wavefront;
  if (ctx->slices.mode == 1) return;      // the context's grid is the slices': the stream has no tiles, the writer derives the sub-streams from ctx->slices
  sc->tile_columns = c.tile_columns; sc->tile_rows = c.tile_rows; sc->tile_uniform_spacing = c.tile_uniform_spacing;
  memcpy(sc->tile_column_width, c.tile_column_width, sizeof sc->tile_column_width); memcpy(sc->tile_row_height, c.tile_row_height, sizeof sc->tile_row_height);
  sc->lf_across_tiles = ctx->stream_lf_across_tiles;
}

extern "C" hevcdl_status hevcdl_get_slice_layout(const hevcdl_ctx *ctx, hevcdl_slice_layout *out)
{
  if (!ctx || !out) return HEVCDL_ERR_INVALID_ARG;
  *out = ctx->slices;
  return HEVCDL_OK;
}

extern "C" hevcdl_status hevcdl_get_segment_layout(const hevcdl_ctx *ctx, hevcdl_segment_layout *out)
{
  if (!ctx || !out) return HEVCDL_ERR_INVALID_ARG;
  *out = ctx->segments;
  return HEVCDL_OK;
}

static void entropy_release(hevcdl_ctx *ctx)
{
  ctx->ec = Entropy();
}

extern "C" hevcdl_status hevcdl_enable_device_entropy(hevcdl_ctx *ctx, int on)
{
  if (!ctx) return HEVCDL_ERR_INVALID_ARG;
  TRY(check_frames(ctx, 0));
  if (!on) {
    if (!ctx->ec.entropy_on) return HEVCDL_OK;
    TRY(sync_or_fail(ctx, "hevcdl_enable_device_entropy"));
    entropy_release(ctx);
    return HEVCDL_OK;
  }
  if (ctx->ec.entropy_on) return HEVCDL_OK;
  hevcdl_stream_config sc; entropy_stream_config(ctx, 0, &sc);
  EntropyPlan pl;
  const hevcdl_status st = entropy_plan(&sc, &ctx->slices, &ctx->segments, ctx->ec_capacity_per_ctu, pl); if (st) return fail(ctx, st, "device entropy: stream configuration");
  // the workspace holds the regions of at most ENTROPY_WS_BYTES worth of pictures (84 MB a picture at 2160p: 2040 CTUs x 40 KB); larger batches go through it in passes
  const size_t ENTROPY_WS_BYTES = (size_t)512 << 20;
  const int pass = (int)std::max<size_t>(1, std::min<size_t>((size_t)ctx->cfg.max_frames, ENTROPY_WS_BYTES / pl.frame_stride));
  const size_t n_sub = (size_t)pass * pl.units;
  Entropy &g = ctx->ec;
  const size_t unit_b = 4 * (size_t)pl.units, sync_b = (size_t)pass * ctx->ctus_y * hevcdl_ec::EC_SYNC_BYTES;
  TRY(alloc_all(ctx, { want(g.d_ec_tables, sizeof(hevcdl_ec::EcTables)), want(g.d_ec_ws, pl.frame_stride * pass), want(g.d_ec_packed, pl.frame_stride * pass), want(g.d_ec_sync, sync_b),
                       want(g.d_ec_off, unit_b), want(g.d_ec_cap, unit_b), want(g.d_ec_sizes, 4 * n_sub), want(g.d_ec_ovf, 4 * n_sub), want(g.d_ec_dst, 8 * n_sub) }, "device entropy workspace"));
  hipError_t e = hipMemcpy(g.d_ec_tables, &hevcdl_ec::ec_tables(), sizeof(hevcdl_ec::EcTables), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(g.d_ec_off, pl.off.data(), unit_b, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(g.d_ec_cap, pl.cap.data(), unit_b, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemset(g.d_ec_sync, 0, sync_b);
  if (e != hipSuccess) { entropy_release(ctx); return hip_fail(ctx, "device entropy workspace", e); }
  ctx->ec.ec_off = pl.off; ctx->ec.ec_cap = pl.cap; ctx->ec.ec_units = pl.units; ctx->ec.ec_pass_frames = pass; ctx->ec.ec_frame_stride = pl.frame_stride; ctx->ec.entropy_on = true;
  return HEVCDL_OK;
}

// The slice data of the n_frames pictures whose records (and SAO parameters) the picture pipeline has just left in HBM -> ctx->ec.h_slice*.  Passes of ec_pass_frames
// pictures: the two kernels, the lengths to the host, an exclusive scan, the pack kernel, one copy of the used bytes.
static hevcdl_status entropy_pipeline(hevcdl_ctx *ctx, int n_frames, int want_sao)
{
  hevcdl_stream_config sc; entropy_stream_config(ctx, want_sao, &sc);
  EntropyPlan pl;
  hevcdl_status st = entropy_plan(&sc, &ctx->slices, &ctx->segments, ctx->ec_capacity_per_ctu, pl); if (st) return fail(ctx, st, "device entropy: stream configuration");
  const int units = ctx->ec.ec_units;
  ctx->ec_ms[0] = ctx->ec_ms[1] = ctx->ec_ms[2] = 0;
  Event ev[5];      // with the profile switch: start, between the two launches, end of the coding, around the pack launch
  if (ctx->profile) for (Event &e : ev) HIPCHK(hipEventCreate(&e.p));
  const size_t rec_b = ctx->records_bytes(1), sao_b = ctx->sao_bytes(1);
  ctx->ec.h_slice.clear(); ctx->ec.h_slice_sizes.assign((size_t)n_frames * units, 0); ctx->ec.h_slice_at.assign((size_t)n_frames + 1, 0); ctx->ec.ec_fallbacks = 0;
  std::vector<uint32_t> ovf; std::vector<unsigned long long> dst; std::vector<int> fallback;
  const bool searched = ctx->qprd.n != 0 && (int)ctx->qprd.h_idx.size() == n_frames;      // DeltaQpRD: the contexts of every picture start from its own QP
  const bool per_picture_qp = searched || !ctx->fqp.list.empty();                          // ... as with a list of hevcdl_set_frame_qps
  if (per_picture_qp) TRY(upload_frame_qp(ctx, searched ? ctx->qprd.h_idx.data() : nullptr, n_frames, nullptr));
  for (int first = 0; first < n_frames; first += ctx->ec.ec_pass_frames) {
    const int cnt = std::min(ctx->ec.ec_pass_frames, n_frames - first); const size_t n_sub = (size_t)cnt * units;
    hevcdl_entropy_params k = pl.k;
    k.records = ctx->stage.d_records + rec_b * first; k.sao = want_sao ? ctx->sao.d_sao_params + sao_b * first : (unsigned char *)nullptr; k.tables = ctx->ec.d_ec_tables; k.out = ctx->ec.d_ec_ws;
    k.unit_off = ctx->ec.d_ec_off; k.unit_cap = ctx->ec.d_ec_cap; k.sizes = ctx->ec.d_ec_sizes; k.overflow = ctx->ec.d_ec_ovf; k.sync = ctx->ec.d_ec_sync; k.n_frames = cnt;
    if (per_picture_qp) k.frame_qp = ctx->qprd.d_frame_qp.p + first;
    if (ev[0]) HIPCHK(hipEventRecord(ev[0], nullptr));
    hevcdl_launch_entropy(&k, nullptr, ev[1]);
    if (ev[2]) HIPCHK(hipEventRecord(ev[2], nullptr));
    HIPCHK(hipGetLastError());
    uint32_t *sz = ctx->ec.h_slice_sizes.data() + (size_t)first * units;
    ovf.resize(n_sub); dst.resize(n_sub);
    HIPCHK(hipMemcpy(sz, ctx->ec.d_ec_sizes, 4 * n_sub, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(ovf.data(), ctx->ec.d_ec_ovf, 4 * n_sub, hipMemcpyDeviceToHost));
    unsigned long long at = 0; bool pass_fallback = false;
    for (int f = 0; f < cnt; f++) {
      bool bad = false;
      for (int u = 0; u < units; u++) bad = bad || ovf[(size_t)f * units + u] != 0 || sz[(size_t)f * units + u] > ctx->ec.ec_cap[(size_t)u];
      if (bad) { pass_fallback = true; fallback.push_back(first + f); for (int u = 0; u < units; u++) sz[(size_t)f * units + u] = 0; }
      ctx->ec.h_slice_at[(size_t)first + f] = ctx->ec.h_slice.size() + (size_t)at;
      for (int u = 0; u < units; u++) { dst[(size_t)f * units + u] = at; at += sz[(size_t)f * units + u]; }
    }
    HIPCHK(hipMemcpy(ctx->ec.d_ec_dst, dst.data(), 8 * n_sub, hipMemcpyHostToDevice));
    hevcdl_entropy_pack_params pk; memset(&pk, 0, sizeof pk);
    pk.src = ctx->ec.d_ec_ws; pk.dst = ctx->ec.d_ec_packed; pk.unit_off = ctx->ec.d_ec_off; pk.unit_cap = ctx->ec.d_ec_cap; pk.sizes = ctx->ec.d_ec_sizes; pk.dst_off = ctx->ec.d_ec_dst;
    pk.frame_stride = ctx->ec.ec_frame_stride; pk.dst_cap = ctx->ec.ec_frame_stride * (size_t)cnt; pk.n_frames = cnt; pk.units = units;
    if (pass_fallback) HIPCHK(hipMemcpy(ctx->ec.d_ec_sizes, sz, 4 * n_sub, hipMemcpyHostToDevice));      // the lengths the offsets were made from (0 for a picture the host codes)
    if (ev[3]) HIPCHK(hipEventRecord(ev[3], nullptr));
    hevcdl_launch_entropy_pack(&pk, nullptr);
    if (ev[4]) HIPCHK(hipEventRecord(ev[4], nullptr));
    HIPCHK(hipGetLastError());
    const size_t old = ctx->ec.h_slice.size();
    ctx->ec.h_slice.resize(old + (size_t)at);
    if (at) HIPCHK(hipMemcpy(ctx->ec.h_slice.data() + old, ctx->ec.d_ec_packed, (size_t)at, hipMemcpyDeviceToHost));
    if (ev[0]) {
      HIPCHK(hipEventSynchronize(ev[4]));
      float ms = 0;
      HIPCHK(hipEventElapsedTime(&ms, ev[0], ev[1])); ctx->ec_ms[0] += ms;
      HIPCHK(hipEventElapsedTime(&ms, ev[1], ev[2])); ctx->ec_ms[1] += ms;
      HIPCHK(hipEventElapsedTime(&ms, ev[3], ev[4])); ctx->ec_ms[2] += ms;
    }
  }
  ctx->ec.h_slice_at[(size_t)n_frames] = ctx->ec.h_slice.size();
  if (!fallback.empty()) { // a sub-stream did not fit its region: the host codes those pictures (their records only; a first call sizes, a second writes), and the batch is put together again in picture order
    std::vector<uint8_t> all; std::vector<size_t> at((size_t)n_frames + 1, 0);
    std::vector<hevcdl_ctu_record> rec((size_t)ctx->ctus); std::vector<hevcdl_sao_blk> sao(want_sao ? (size_t)ctx->ctus : 0);
    size_t fb = 0;
    for (int f = 0; f < n_frames; f++) {
      at[(size_t)f] = all.size();
      if (fb < fallback.size() && fallback[fb] == f) {
        fb++;
        HIPCHK(hipMemcpy(rec.data(), ctx->stage.d_records + rec_b * f, rec_b, hipMemcpyDeviceToHost));
        if (want_sao) HIPCHK(hipMemcpy(sao.data(), ctx->sao.d_sao_params + sao_b * f, sao_b, hipMemcpyDeviceToHost));
        size_t total = 0; uint32_t *sz = ctx->ec.h_slice_sizes.data() + (size_t)f * units;
        if (per_picture_qp) sc.qp = searched ? ctx->qprd.cand[ctx->qprd.h_idx[(size_t)f]].qp : frame_qp_at(ctx, f);
        hevcdl_host_writer_slice_data(&sc, &ctx->slices, &ctx->segments, rec.data(), want_sao ? sao.data() : nullptr, nullptr, 0, sz, &total);
        all.resize(at[(size_t)f] + total);
        if (hevcdl_host_writer_slice_data(&sc, &ctx->slices, &ctx->segments, rec.data(), want_sao ? sao.data() : nullptr, all.data() + at[(size_t)f], total, sz, &total) != 0) return fail(ctx, HEVCDL_ERR_INVALID_ARG, "device entropy: host fallback");
      } else all.insert(all.end(), ctx->ec.h_slice.begin() + (ptrdiff_t)ctx->ec.h_slice_at[(size_t)f], ctx->ec.h_slice.begin() + (ptrdiff_t)ctx->ec.h_slice_at[(size_t)f + 1]);
    }
    at[(size_t)n_frames] = all.size();
    ctx->ec.h_slice.swap(all); ctx->ec.h_slice_at.swap(at); ctx->ec.ec_fallbacks = (int)fallback.size();
  }
  return HEVCDL_OK;
}

extern "C" hevcdl_status hevcdl_set_entropy_capacity(hevcdl_ctx *ctx, int capacity_per_ctu)
{
  if (!ctx) return HEVCDL_ERR_INVALID_ARG;
  if (ctx->ec.entropy_on) return fail(ctx, HEVCDL_ERR_INVALID_ARG, "hevcdl_set_entropy_capacity: the switch is on");
  if (capacity_per_ctu > 0 && (capacity_per_ctu & 3)) return fail(ctx, HEVCDL_ERR_INVALID_ARG, "hevcdl_set_entropy_capacity: not a multiple of 4");
  ctx->ec_capacity_per_ctu = capacity_per_ctu > 0 ? capacity_per_ctu : 0;
  return HEVCDL_OK;
}

extern "C" hevcdl_status hevcdl_get_entropy_info(hevcdl_ctx *ctx, int *fallbacks_opt, double *kernel_ms_opt)
{
  if (!ctx) return HEVCDL_ERR_INVALID_ARG;
  if (!ctx->ec.entropy_on) return fail(ctx, HEVCDL_ERR_INVALID_ARG, "hevcdl_get_entropy_info: hevcdl_enable_device_entropy was not called");
  if (fallbacks_opt) *fallbacks_opt = ctx->ec.ec_fallbacks;
  if (kernel_ms_opt) for (int i = 0; i < 3; i++) kernel_ms_opt[i] = ctx->ec_ms[i];
  return HEVCDL_OK;
}

extern "C" hevcdl_status hevcdl_get_slice_data(hevcdl_ctx *ctx, int first, int count, const uint8_t **data, const uint32_t **sizes, int *n_substreams_per_picture)
{
  if (!ctx) return HEVCDL_ERR_INVALID_ARG;
  TRY(check_batch_range(ctx, "hevcdl_get_slice_data", data && sizes && n_substreams_per_picture, ctx->ec.entropy_on, "hevcdl_enable_device_entropy", first, count,
                        (long long)ctx->ec.h_slice_at.size() - 1));      // (h_slice_at holds the start of every picture and the end)
  *data = ctx->ec.h_slice.data() + ctx->ec.h_slice_at[(size_t)first]; *sizes = ctx->ec.h_slice_sizes.data() + (size_t)first * ctx->ec.ec_units; *n_substreams_per_picture = ctx->ec.ec_units;
  return HEVCDL_OK;
}

extern "C" hevcdl_status hevcdl_encode_pictures_stream(hevcdl_ctx *ctx, const void *yuv, int n_frames, const uint8_t *labels_opt, int deblock, int want_sao,
                                                       int want_pictures, int want_records, int chunk_frames, hevcdl_stream_fn fn, void *user)
{
  TRY(check_frames(ctx, n_frames));
  if (!ctx->ec.entropy_on) return fail(ctx, HEVCDL_ERR_INVALID_ARG, "hevcdl_encode_pictures_stream: hevcdl_enable_device_entropy was not called");
  if (n_frames == 0) return HEVCDL_OK;
  if (!yuv || !fn) return fail(ctx, HEVCDL_ERR_INVALID_ARG, "null pointer");
  const int chunk = std::min(n_frames, chunk_frames > 0 ? chunk_frames : 64);
  const size_t rec_b = want_records ? ctx->records_bytes(1) : 0, pic_b = want_pictures ? ctx->frame_bytes : 0, stat_b = sizeof(hevcdl_frame_stats);
  auto up64 = [](size_t v) { return (v + 63) & ~(size_t)63; };
  const size_t o_pic = up64(rec_b * chunk), o_stat = up64(o_pic + pic_b * chunk), need = o_stat + stat_b * chunk;
  TRY(ensure_chunk_buffers(ctx, need));
  uint8_t *d_final = nullptr;
  TRY(encode_pictures_device(ctx, yuv, n_frames, labels_opt, deblock, want_sao, &d_final));      // runs the entropy kernels too (the switch is on)
  unsigned char *h = ctx->stage.h_chunk[0];
  for (int first = 0; first < n_frames; first += chunk) { // records and pictures leave HBM only when asked for; the statistics are 40 bytes a picture
    const int cnt = std::min(chunk, n_frames - first);
    if (want_records) HIPCHK(hipMemcpy(h, ctx->stage.d_records + rec_b * first, rec_b * cnt, hipMemcpyDeviceToHost));
    if (want_pictures) HIPCHK(hipMemcpy(h + o_pic, d_final + pic_b * first, pic_b * cnt, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(h + o_stat, ctx->stage.d_stats + stat_b * first, stat_b * cnt, hipMemcpyDeviceToHost));
    if (fn(user, first, cnt, ctx->ec.h_slice.data() + ctx->ec.h_slice_at[(size_t)first], ctx->ec.h_slice_sizes.data() + (size_t)first * ctx->ec.ec_units, ctx->ec.ec_units,
           (const hevcdl_frame_stats *)(h + o_stat), want_pictures ? h + o_pic : nullptr, want_records ? (const hevcdl_ctu_record *)h : nullptr) != 0)
      return fail(ctx, HEVCDL_ERR_INVALID_ARG, "the stream callback asked to stop");
  }
  return HEVCDL_OK;
}

// ---- per-CTU session: the semantic drop-in for TEncCu::compressCtu + encodeCtu (TEncSlice.cpp:879,893) ----------------
extern "C" hevcdl_status hevcdl_begin_frames(hevcdl_ctx *ctx, const uint8_t *yuv, int n_frames, const uint8_t *labels_opt, uint8_t *labels_out_opt)
{
  TRY(check_frames(ctx, n_frames));
  if (ctx->slices.mode != 0) return fail(ctx, HEVCDL_ERR_INVALID_ARG, "begin_frames: the per-CTU session does not code slices; use hevcdl_compress_frames");
  if (ctx->qprd.n) return fail(ctx, HEVCDL_ERR_UNSUPPORTED, "begin_frames: the per-CTU session does not search the slice QP (DeltaQpRD codes every picture 2N+1 times); use hevcdl_compress_frames");
  if (ctx->fqp.active()) return fail(ctx, HEVCDL_ERR_UNSUPPORTED, HEVCDL_FRAME_QP_REFUSE_SESSION);
  if (n_frames == 0 || !yuv) return fail(ctx, HEVCDL_ERR_INVALID_ARG, "begin_frames: no frames");
  TRY(ensure_staging(ctx));
  TRY(lazy_alloc(ctx, ctx->ses.d_cabac, sizeof(hevcdl_cabac_state) * (size_t)ctx->cfg.max_frames, "coder states of the per-CTU session (cfg.max_frames)"));
  HIPCHK(hipMemcpy(ctx->stage.d_yuv, yuv, ctx->frame_bytes * n_frames, hipMemcpyHostToDevice));
  TRY(stage_labels(ctx, labels_opt, n_frames));
  HIPCHK(hipMemset(ctx->stage.d_recon, 0, ctx->frame_bytes * n_frames));
  HIPCHK(hipMemset(ctx->stage.d_records, 0, ctx->records_bytes(n_frames)));
  if (ctx->rd.d_wpp) HIPCHK(hipMemset(ctx->rd.d_wpp, 0, (size_t)256 * ctx->ctus_y * n_frames));      // WaveFrontSynchro: the rows' synchronisation contexts of this session
  HIPCHK(hipDeviceSynchronize());
  if (labels_out_opt) HIPCHK(hipMemcpy(labels_out_opt, ctx->stage.d_labels, ctx->labels_bytes(n_frames), hipMemcpyDeviceToHost));
  ctx->ses.next_ctu.assign(n_frames, 0); ctx->ses.session_frames = n_frames;
  return HEVCDL_OK;
}

extern "C" hevcdl_status hevcdl_compress_ctu(hevcdl_ctx *ctx, int frame, int ctu_addr, const hevcdl_cabac_state *state_in_opt,
                                             hevcdl_ctu_record *record, hevcdl_cabac_state *state_out_opt)
{
  if (!ctx) return HEVCDL_ERR_INVALID_ARG;
  if (ctx->cfg.tile_columns * ctx->cfg.tile_rows != 1) return fail(ctx, HEVCDL_ERR_UNSUPPORTED, "compress_ctu: the per-CTU session walks the untiled raster scan; with tiles use hevcdl_compress_frames");
  if (frame < 0 || frame >= ctx->ses.session_frames) return fail(ctx, HEVCDL_ERR_INVALID_ARG, "compress_ctu: frame outside the session (hevcdl_begin_frames)");
  if (ctu_addr < 0 || ctu_addr >= ctx->ctus || !record) return fail(ctx, HEVCDL_ERR_INVALID_ARG, "compress_ctu: bad CTU address / null record");
  // the CTUs of a slice are a chain: neighbours' reconstruction and records must exist
  if (ctu_addr > ctx->ses.next_ctu[frame]) return fail(ctx, HEVCDL_ERR_INVALID_ARG, "compress_ctu: CTUs must be submitted in coding order");
  if (ctu_addr < ctx->ses.next_ctu[frame] && !state_in_opt) return fail(ctx, HEVCDL_ERR_INVALID_ARG, "compress_ctu: re-coding an earlier CTU needs its entry state");
  HIPCHK(hipSetDevice(ctx->cfg.device));
  unsigned char *cab = ctx->ses.d_cabac + sizeof(hevcdl_cabac_state) * (size_t)frame;
  if (state_in_opt) HIPCHK(hipMemcpy(cab, state_in_opt, sizeof(hevcdl_cabac_state), hipMemcpyHostToDevice));
  const void *cab_in = (state_in_opt || ctu_addr > 0) ? cab : nullptr;      // NULL: slice-start contexts from the QP
  hevcdl_status st = launch_rd(ctx, ctx->stage.d_yuv + ctx->frame_bytes * frame, 1, ctx->stage.d_labels + ctx->labels_bytes(frame),
                               ctx->stage.d_records + ctx->records_bytes(frame), ctx->stage.d_recon + ctx->frame_bytes * frame, nullptr, nullptr,
                               ctu_addr, ctu_addr + 1, cab_in, cab, 0, -1, frame);
  if (st) return st;
  TRY(sync_or_fail(ctx, "rd kernel"));
  HIPCHK(hipMemcpy(record, ctx->stage.d_records + ctx->records_bytes(frame) + sizeof(hevcdl_ctu_record) * (size_t)ctu_addr, sizeof(hevcdl_ctu_record), hipMemcpyDeviceToHost));
  if (state_out_opt) HIPCHK(hipMemcpy(state_out_opt, cab, sizeof(hevcdl_cabac_state), hipMemcpyDeviceToHost));
  if (ctu_addr == ctx->ses.next_ctu[frame]) ctx->ses.next_ctu[frame] = ctu_addr + 1;
  return HEVCDL_OK;
}

extern "C" hevcdl_status hevcdl_get_recon(hevcdl_ctx *ctx, int frame, uint8_t *recon)
{
  if (!ctx) return HEVCDL_ERR_INVALID_ARG;
  if (frame < 0 || frame >= ctx->ses.session_frames || !recon) return fail(ctx, HEVCDL_ERR_INVALID_ARG, "get_recon: frame outside the session / null pointer");
  HIPCHK(hipSetDevice(ctx->cfg.device));
  HIPCHK(hipMemcpy(recon, ctx->stage.d_recon + ctx->frame_bytes * frame, ctx->frame_bytes, hipMemcpyDeviceToHost));
  return HEVCDL_OK;
}

// ---- DeltaQpRD: the public side (the search itself: qp_rd_search above) ------------------------------------------------------------------------------------------------
extern "C" hevcdl_status hevcdl_qp_rd_candidates(const hevcdl_config *cfg, hevcdl_qp_rd_candidate *out, int capacity, int *count, double *frame_lambda)
{
  if (!cfg || !out || !count || !frame_lambda || cfg->delta_qp_rd < 0 || cfg->delta_qp_rd > HEVCDL_QP_RD_MAX_N || capacity < 2 * cfg->delta_qp_rd + 1 || cfg->qp < 0 || cfg->qp > 51) return HEVCDL_ERR_INVALID_ARG;
  if ((cfg->bit_depth != 8 && cfg->bit_depth != 10) || (cfg->bit_depth > 8 && cfg->qp - cfg->delta_qp_rd < 0)) return HEVCDL_ERR_UNSUPPORTED;
  const int n = hevcdl_qp_rd_table(cfg->qp, cfg->delta_qp_rd, cfg->bit_depth, out, frame_lambda);
  if (n < 1) return HEVCDL_ERR_INVALID_ARG;
  *count = n;
  return HEVCDL_OK;
}

extern "C" int hevcdl_qp_rd_pick_index(const uint64_t *bits, const uint64_t *dist, int n, double frame_lambda)
{
  return !bits || !dist || n < 1 ? -1 : hevcdl_qp_rd_pick(bits, dist, n, frame_lambda);
}

extern "C" hevcdl_status hevcdl_get_qp_rd(hevcdl_ctx *ctx, int first, int count, hevcdl_qp_rd_row *rows, int32_t *qps_opt)
{
  if (!ctx) return HEVCDL_ERR_INVALID_ARG;
  TRY(check_batch_range(ctx, "hevcdl_get_qp_rd", rows != nullptr, ctx->qprd.n != 0, "hevcdl_create with cfg.delta_qp_rd", first, count, (long long)ctx->qprd.last_frames));
  if (count == 0) return HEVCDL_OK;
  if ((int)ctx->qprd.h_rows.size() == ctx->qprd.last_frames) memcpy(rows, ctx->qprd.h_rows.data() + first, sizeof(hevcdl_qp_rd_row) * (size_t)count);      // a picture pipeline fetched them
  else {
    TRY(sync_or_fail(ctx, "hevcdl_get_qp_rd"));
    HIPCHK(hipMemcpy(rows, ctx->qprd.d_rows.p + first, sizeof(hevcdl_qp_rd_row) * (size_t)count, hipMemcpyDeviceToHost));
  }
  for (int i = 0; i < count; i++) {
    if (rows[i].best_idx < 0 || rows[i].best_idx >= ctx->qprd.count) return fail(ctx, HEVCDL_ERR_HIP, "hevcdl_get_qp_rd: a row's index lies outside the candidate table");
    if (qps_opt) qps_opt[i] = ctx->qprd.cand[rows[i].best_idx].qp;
  }
  return HEVCDL_OK;
}

static double sum_event_pairs(std::vector<Event> &v, unsigned *pairs_opt);
extern "C" hevcdl_status hevcdl_get_qp_rd_info(hevcdl_ctx *ctx, size_t *trial_bytes, uint64_t *kernel_launches, double *kernel_ms_opt)
{
  if (!ctx || !trial_bytes || !kernel_launches) return HEVCDL_ERR_INVALID_ARG;
  *trial_bytes = ctx->qprd.d_rows ? ctx->qprd.trial_bytes : 0; *kernel_launches = ctx->qprd.launches;
  if (kernel_ms_opt) { // HIP-event times of the sum and the keep launches of the last search, each summed over its candidates; zeros without hevcdl_profile_enable
    TRY(sync_or_fail(ctx, "hevcdl_get_qp_rd_info"));
    kernel_ms_opt[0] = sum_event_pairs(ctx->qprd.ev_sum, nullptr); kernel_ms_opt[1] = sum_event_pairs(ctx->qprd.ev_keep, nullptr);
  }
  return HEVCDL_OK;
}

// the two kernels alone (host buffers, no context): the destinations travel with their guard margins, so that a write outside a payload shows in what comes back
extern "C" hevcdl_status hevcdl_qp_rd_step(int device, int ctus_per_frame, size_t frame_bytes, int n_frames, int idx, double frame_lambda, const hevcdl_ctu_record *trial_records,
                                           const void *trial_recon, const hevcdl_frame_stats *trial_stats, hevcdl_qp_rd_row *rows, void *records, void *recon, void *stats, size_t guard_bytes)
{
  if (ctus_per_frame < 1 || n_frames < 1 || n_frames > 65535 || idx < 0 || idx >= HEVCDL_QP_RD_MAX_CANDIDATES || (frame_bytes & 15) || (guard_bytes & 15) || !trial_records || !rows) return HEVCDL_ERR_INVALID_ARG;
  if (idx > 0 && (!trial_recon || !trial_stats || !records || !recon || !stats)) return HEVCDL_ERR_INVALID_ARG;
  TRY(select_device(device));
  const size_t nf = (size_t)n_frames, rec_b = sizeof(hevcdl_ctu_record) * (size_t)ctus_per_frame * nf, pic_b = frame_bytes * nf, stat_b = sizeof(hevcdl_frame_stats) * nf, row_b = sizeof(hevcdl_qp_rd_row) * nf;
  const size_t g = guard_bytes;
  DevBuf<unsigned char> t_rec, t_pic, t_stat, d_rec, d_pic, d_stat; DevBuf<hevcdl_qp_rd_row> d_rows;
  TRY(alloc_all(nullptr, { want(t_rec, rec_b), want(t_pic, pic_b + 16), want(t_stat, stat_b), want(d_rec, rec_b + 2 * g), want(d_pic, pic_b + 2 * g + 16), want(d_stat, stat_b + 2 * g), want(d_rows, row_b) }, ""));
  hipError_t e = hipMemcpy(t_rec, trial_records, rec_b, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d_rows, rows, row_b, hipMemcpyHostToDevice);
  if (e == hipSuccess && idx > 0) {
    if (pic_b) e = hipMemcpy(t_pic, trial_recon, pic_b, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(t_stat, trial_stats, stat_b, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_rec, records, rec_b + 2 * g, hipMemcpyHostToDevice);
    if (e == hipSuccess && pic_b + 2 * g) e = hipMemcpy(d_pic, recon, pic_b + 2 * g, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_stat, stats, stat_b + 2 * g, hipMemcpyHostToDevice);
  }
  if (e == hipSuccess) {
    hevcdl_qp_rd_sum_params sp; memset(&sp, 0, sizeof sp);
    sp.records = t_rec; sp.rows = d_rows; sp.ctus_per_frame = ctus_per_frame; sp.n_frames = n_frames; sp.idx = idx; sp.frame_lambda = frame_lambda;
    hevcdl_launch_qp_rd_sum(&sp, nullptr);
    if (idx > 0) {
      hevcdl_qp_rd_keep_params kp; memset(&kp, 0, sizeof kp);
      kp.src_records = t_rec; kp.src_recon = t_pic; kp.src_stats = t_stat; kp.dst_records = d_rec + g; kp.dst_recon = d_pic + g; kp.dst_stats = d_stat + g;
      kp.rows = d_rows; kp.rec16 = sizeof(hevcdl_ctu_record) * (size_t)ctus_per_frame / 16; kp.pic16 = kp.rec16 + frame_bytes / 16; kp.n_frames = n_frames;
      hevcdl_launch_qp_rd_keep(&kp, nullptr);
    }
    e = hipGetLastError();
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(rows, d_rows, row_b, hipMemcpyDeviceToHost);
    if (e == hipSuccess && idx > 0) {
      e = hipMemcpy(records, d_rec, rec_b + 2 * g, hipMemcpyDeviceToHost);
      if (e == hipSuccess && pic_b + 2 * g) e = hipMemcpy(recon, d_pic, pic_b + 2 * g, hipMemcpyDeviceToHost);
      if (e == hipSuccess) e = hipMemcpy(stats, d_stat, stat_b + 2 * g, hipMemcpyDeviceToHost);
    }
  }
  if (e != hipSuccess) return hip_fail(nullptr, "", e);
  return HEVCDL_OK;
}

// ---- a QP per picture: the public side (the grouped decisions: frame_qp_decide above) ----------------------------------------------------------------------------------
extern "C" hevcdl_status hevcdl_frame_qp_check(const hevcdl_config *cfg, const int *qp, int n, double lambda_modifier, const char **why)
{
  static const char *none = "";
  if (!cfg || n < 0) { if (why) *why = none; return HEVCDL_ERR_INVALID_ARG; }
  const char *w = none;
  const hevcdl_status st = hevcdl_frame_qp_keys(cfg, qp, n, lambda_modifier, &w);
  if (why) *why = w;
  return st;
}

extern "C" hevcdl_status hevcdl_set_frame_qps(hevcdl_ctx *ctx, const int *qp, int n)
{
  if (!ctx) return HEVCDL_ERR_INVALID_ARG;
  if (n < 0) return fail(ctx, HEVCDL_ERR_INVALID_ARG, "hevcdl_set_frame_qps: n < 0");
  if (!qp || n == 0) { ctx->fqp.list.clear(); return HEVCDL_OK; }
  const char *why = "";
  const hevcdl_status st = hevcdl_frame_qp_keys(&ctx->cfg, qp, n, ctx->fqp.lambda_modifier, &why);
  if (st != HEVCDL_OK) return fail(ctx, st, why);
  ctx->fqp.list.assign(qp, qp + n);
  return HEVCDL_OK;
}

extern "C" hevcdl_status hevcdl_set_lambda_modifier(hevcdl_ctx *ctx, double lambda_modifier)
{
  if (!ctx) return HEVCDL_ERR_INVALID_ARG;
  const char *why = "";
  const hevcdl_status st = hevcdl_frame_qp_keys(&ctx->cfg, ctx->fqp.list.data(), (int)ctx->fqp.list.size(), lambda_modifier, &why);
  if (st != HEVCDL_OK) return fail(ctx, st, why);
  ctx->fqp.lambda_modifier = lambda_modifier;
  return HEVCDL_OK;
}

extern "C" hevcdl_status hevcdl_get_frame_qps(hevcdl_ctx *ctx, int first, int count, int32_t *qp)
{
  if (!ctx) return HEVCDL_ERR_INVALID_ARG;
  TRY(check_batch_range(ctx, "hevcdl_get_frame_qps", qp != nullptr, true, "", first, count, (long long)ctx->fqp.used.size()));
  for (int i = 0; i < count; i++) qp[i] = ctx->fqp.used[(size_t)first + i];
  return HEVCDL_OK;
}

extern "C" hevcdl_status hevcdl_frame_qp_list(int base_qp, const int *dqp, int n, int intra_qp_offset, int bit_depth, int *out)
{
  if (n < 0 || (n && !out) || (bit_depth != 8 && bit_depth != 10) || base_qp < 0 || base_qp > 51) return HEVCDL_ERR_INVALID_ARG;
  for (int i = 0; i < n; i++) {
    out[i] = hevcdl_frame_qp_of(base_qp, dqp ? dqp[i] : 0, intra_qp_offset, bit_depth);
    if (out[i] < 0) return HEVCDL_ERR_INVALID_ARG;
  }
  return HEVCDL_OK;
}

extern "C" hevcdl_status hevcdl_frame_qp_offsets(int n, int qpif, int frame_skip, int temporal_subsample_ratio, const char *dqp_file, int *dqp, int *file_values)
{
  if (n < 0 || (n && !dqp) || frame_skip < 0 || temporal_subsample_ratio < 1) return HEVCDL_ERR_INVALID_ARG;
  if (file_values) *file_values = 0;
  hevcdl_dqp_increment(dqp, n, qpif >= 0, (unsigned)(qpif >= 0 ? qpif : 0), (unsigned)frame_skip, (unsigned)temporal_subsample_ratio);
  if (dqp_file && dqp_file[0]) {
    const int got = hevcdl_dqp_read_file(dqp_file, dqp, n);
    if (got < 0) return HEVCDL_ERR_INVALID_ARG;
    if (file_values) *file_values = got;
  }
  return HEVCDL_OK;
}

extern "C" hevcdl_status hevcdl_frame_qp_families(int qp, int bit_depth, double lambda_modifier, hevcdl_qp_rd_candidate *out)
{
  if (!out || qp < 0 || qp > 51 || (bit_depth != 8 && bit_depth != 10) || !(lambda_modifier > 0.0) || !(lambda_modifier < 1.0e30)) return HEVCDL_ERR_INVALID_ARG;
  hevcdl_frame_qp_family(qp, bit_depth, lambda_modifier, out);
  return HEVCDL_OK;
}

extern "C" int hevcdl_frame_qp_grouping(const int *qp, int n, int *perm, int *run_qp, int *run_first, int *run_count, int *contiguous)
{
  if (n < 0 || (n && (!qp || !perm)) || !run_qp || !run_first || !run_count) return -1;
  std::vector<hevcdl_qp_run> runs(52);
  const int n_runs = hevcdl_frame_qp_group(qp, n, perm, runs.data(), nullptr);
  if (n_runs < 0) return -1;
  for (int r = 0; r < n_runs; r++) { run_qp[r] = runs[(size_t)r].qp; run_first[r] = runs[(size_t)r].first; run_count[r] = runs[(size_t)r].count; }
  if (contiguous) *contiguous = n == 0 || hevcdl_frame_qp_contiguous_runs(qp, n, runs.data()) > 0;
  return n_runs;
}

extern "C" hevcdl_status hevcdl_get_frame_qp_info(hevcdl_ctx *ctx, size_t *set_bytes, int *rd_launches, int *permute_launches, double *kernel_ms_opt)
{
  if (!ctx || !set_bytes || !rd_launches || !permute_launches) return HEVCDL_ERR_INVALID_ARG;
  *set_bytes = ctx->fqp.d_perm ? ctx->fqp.set_bytes : 0; *rd_launches = ctx->fqp.rd_launches; *permute_launches = ctx->fqp.permute_launches;
  if (kernel_ms_opt) { // the gather pair first, then the scatter pair; zeros without hevcdl_profile_enable or when nothing was copied
    TRY(sync_or_fail(ctx, "hevcdl_get_frame_qp_info"));
    std::vector<Event> &v = ctx->fqp.ev_permute;
    for (int i = 0; i < 2; i++) { float t = 0; kernel_ms_opt[i] = (v.size() == 4 && hipEventElapsedTime(&t, v[(size_t)2 * i], v[(size_t)2 * i + 1]) == hipSuccess) ? t : 0.0; }
    v.clear();
  }
  return HEVCDL_OK;
}

// the kernel alone (host buffers, no context): the destinations travel with their guard margins, so that a write outside a payload shows in what comes back
extern "C" hevcdl_status hevcdl_frame_permute_step(int device, int n_ranges, const size_t *bytes, int n_frames, const int *perm, int scatter, const void *const *src, void *const *dst, size_t guard_bytes)
{
  if (n_ranges < 1 || n_ranges > 4 || n_frames < 1 || n_frames > 65535 || !bytes || !perm || !src || !dst) return HEVCDL_ERR_INVALID_ARG;
  { std::vector<char> seen((size_t)n_frames, 0);
    for (int i = 0; i < n_frames; i++) { if (perm[i] < 0 || perm[i] >= n_frames || seen[(size_t)perm[i]]) return HEVCDL_ERR_INVALID_ARG; seen[(size_t)perm[i]] = 1; } }
  for (int k = 0; k < n_ranges; k++) if (!bytes[k] || !src[k] || !dst[k]) return HEVCDL_ERR_INVALID_ARG;
  TRY(select_device(device));
  const size_t nf = (size_t)n_frames, g = guard_bytes;
  DevBuf<unsigned char> d_src[4], d_dst[4]; DevBuf<int> d_perm;
  hipError_t e = hipMalloc(&d_perm.p, sizeof(int) * nf);
  for (int k = 0; k < n_ranges && e == hipSuccess; k++) {
    e = hipMalloc(&d_src[k].p, bytes[k] * nf);
    if (e == hipSuccess) e = hipMalloc(&d_dst[k].p, bytes[k] * nf + 2 * g);
    if (e == hipSuccess) e = hipMemcpy(d_src[k], src[k], bytes[k] * nf, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_dst[k], dst[k], bytes[k] * nf + 2 * g, hipMemcpyHostToDevice);
  }
  if (e == hipSuccess) e = hipMemcpy(d_perm, perm, sizeof(int) * nf, hipMemcpyHostToDevice);
  if (e == hipSuccess) {
    hevcdl_frame_permute_params p; memset(&p, 0, sizeof p);
    p.perm = d_perm; p.n_frames = n_frames; p.n_ranges = n_ranges; p.scatter = scatter != 0;
    for (int k = 0; k < n_ranges; k++) { p.r[k].src = d_src[k]; p.r[k].dst = d_dst[k] + g; p.r[k].bytes = bytes[k]; }
    hevcdl_launch_frame_permute(&p, nullptr);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipDeviceSynchronize();
    for (int k = 0; k < n_ranges && e == hipSuccess; k++) e = hipMemcpy(dst[k], d_dst[k], bytes[k] * nf + 2 * g, hipMemcpyDeviceToHost);
  }
  if (e != hipSuccess) return hip_fail(nullptr, "", e);
  return HEVCDL_OK;
}

extern "C" hevcdl_status hevcdl_profile_enable(hevcdl_ctx *ctx, int enable)
{
  if (!ctx) return HEVCDL_ERR_INVALID_ARG;
  ctx->profile = enable != 0;
  return HEVCDL_OK;
}

// ms between the events of the start/stop pairs in v (and how many pairs were timed); the events are released
static double sum_event_pairs(std::vector<Event> &v, unsigned *pairs_opt)
{
  double ms = 0; unsigned n = 0;
  for (size_t i = 0; i + 1 < v.size(); i += 2) { float t = 0; if (hipEventElapsedTime(&t, v[i], v[i + 1]) == hipSuccess) { ms += t; n++; } }
  v.clear();
  if (pairs_opt) *pairs_opt = n;
  return ms;
}

extern "C" hevcdl_status hevcdl_profile_get(hevcdl_ctx *ctx, hevcdl_profile *out)
{
  if (!ctx || !out) return HEVCDL_ERR_INVALID_ARG;
  HIPCHK(hipSetDevice(ctx->cfg.device));
  HIPCHK(hipDeviceSynchronize());
  memset(out, 0, sizeof *out);
  out->cnn_ms = sum_event_pairs(ctx->ev_cnn, &out->cnn_launches);
  out->rd_ms = sum_event_pairs(ctx->ev_rd, &out->rd_launches);
  out->cnn_conv_ms = sum_event_pairs(ctx->ev_conv, nullptr);
  return HEVCDL_OK;
}
