// entropy_kernel.hip -- the slice data of an I picture coded on the device (gfx950): entropy_coder.h instantiated for one wave per sub-stream.
//
// hevcdl_entropy_kernel: a wave takes one sub-stream (frame x tile, frame x CTU row, or frame) and runs the shared coder over its CTUs.  Control flow is wave-uniform: every
// lane computes the same coder (the wave index is made uniform, so the compiler keeps the state in scalar registers where it can); the ~160 context bytes, the 16 levels
// of the coefficient group in work and 256 bytes of output staging live in the wave's own LDS; staged bytes leave as one dword store per lane.  Samples are never touched:
// the inputs are the CTU records, the SAO parameters, the tile bound tables, QP, tools and the bit depth (SAO offset range).
//
// WaveFrontSynchro without any wave waiting on another -- two ordinary launches on one stream:
//   phase 1  one wave per frame walks row 0, 1, ... and codes only the first two CTUs of each row, contexts only (the contexts do not depend on the arithmetic), and stores
//            the contexts behind each row's second CTU (TEncSlice.cpp:1127-1130): 68 of 2040 CTUs at 2160p;
//   phase 2  one wave per (frame, row) starts from the stored contexts of the row above (row 0, and pictures one CTU wide: slice-start contexts) and codes the row.
// No kernel here holds a spin loop, a flag another wave sets, a cooperative launch or a grid-wide barrier.
//
// Safety: plain C++; every read of a record goes through the masked / range-checked indices of entropy_coder.h, every loop there has a bound that
// does not depend on record contents, every store below is checked against the sub-stream's capacity: a wave writes its own region, its length and overflow words and
// (phase 1) its frame's context slots, nothing else.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "hevcdl.h"
#include "hevcdl_dev.h"
#define HEVCDL_EC_STAGED 1
#define EC_FN __device__ inline
#include "entropy_coder.h"

using namespace hevcdl_ec;

namespace {
constexpr int EC_WAVES = 4;                  // waves (= sub-streams) per workgroup
struct WaveLds { uint8_t ctx[EC_SYNC_BYTES]; uint8_t stage[EC_STAGE_BYTES]; uint16_t absb[16]; };
}

// The bytes of the stage that belong to [base, end), base = the stage-aligned position below end: lane l stores dword l.  Every lane wrote every staged byte itself (the
// coder is wave-uniform), so no lane reads what another one wrote.  The region starts on a dword boundary and its capacity is a multiple of 4, so a whole dword at a
// position below `end` <= capacity lies inside the region; the check is made all the same.
__device__ void hevcdl_ec::ec_flush_stage(EcCoder &s, uint32_t end)
{
  if (end == 0 || end > s.cap) return;
  const uint32_t base = (end - 1) & ~(uint32_t)(EC_STAGE_BYTES - 1), nbytes = end - base, lane = threadIdx.x & 63u;
  if (lane * 4 < nbytes) {
    uint32_t w = ((const uint32_t *)s.stage)[lane];
    const uint32_t have = nbytes - lane * 4;
    if (have < 4) w &= (1u << (8 * have)) - 1u;                       // the last dword of a sub-stream: bytes behind its end are written as zeros
    const uint32_t at = base + lane * 4;
    if (at + 4 <= s.cap) *(uint32_t *)(s.out + at) = w;
  }
}

extern "C" __global__ __launch_bounds__(EC_WAVES * 64) void hevcdl_entropy_kernel(hevcdl_entropy_params p)
{
  __shared__ __attribute__((aligned(16))) WaveLds lds[EC_WAVES];
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = (int)(threadIdx.x & 63u);
  const int units = p.phase == 1 ? 1 : p.units;
  const long long n = (long long)p.n_frames * units, u = (long long)blockIdx.x * EC_WAVES + wave;
  if (u >= n) return;
  const int f = (int)(u / units), k = (int)(u - (long long)f * units);
  WaveLds &l = lds[wave];
  const EcTables *t = (const EcTables *)p.tables;
  EcPic pic;
  pic.W = p.width; pic.H = p.height; pic.ctus_x = p.ctus_x; pic.ctus_y = p.ctus_y; pic.ctus = p.ctus_x * p.ctus_y;
  pic.recs = (const hevcdl_ctu_record *)p.records + (size_t)f * pic.ctus;
  pic.sao = p.sao ? (const hevcdl_sao_blk *)p.sao + (size_t)f * pic.ctus : nullptr;
  pic.tools = (uint32_t)p.tools; pic.max_sao_offset = p.max_sao_offset; pic.tx0 = 0; pic.ty0 = 0;
  const int slice_qp = p.frame_qp ? p.frame_qp[f].qp : p.qp;      // the picture's own slice QP (DeltaQpRD), or the launch's
  EcCoder s;
  s.t = t; s.ctx = l.ctx; s.absb = l.absb; s.stage = l.stage; s.out = nullptr; s.cap = 0; s.dry = 0;
  ec_start(s);
  for (int i = 0; i < EC_SYNC_BYTES; i++) l.ctx[i] = 0;
  uint32_t *sync = (uint32_t *)(p.sync + (size_t)f * p.ctus_y * EC_SYNC_BYTES);      // only dereferenced with wavefront (phase 1 / 2), where the buffer exists

  if (p.phase == 1) { // contexts only, first two CTUs of every row; the slot of row r = the contexts behind CTU 1 of row r
    if (p.ctus_x < 2 || !p.sync) return;
    s.dry = 1;
    ec_init_contexts(l.ctx, t, slice_qp);
    for (int row = 0; row < p.ctus_y; row++) {
      ec_code_ctu(s, pic, 0, row);
      ec_code_ctu(s, pic, 1, row);
      if (lane < EC_SYNC_BYTES / 4) sync[row * (EC_SYNC_BYTES / 4) + lane] = ((const uint32_t *)l.ctx)[lane];
    }
    return;
  }

  if (k >= p.units) return;
  int cx0, cx1, cy0, cy1;
  ec_unit_rect(p.wpp, p.tile_cols, p.col_bd, p.row_bd, p.ctus_x, k, cx0, cx1, cy0, cy1);
  if (cx0 < 0 || cy0 < 0 || cx1 > p.ctus_x || cy1 > p.ctus_y) return;
  if (!p.wpp) { pic.tx0 = cx0 * 64; pic.ty0 = cy0 * 64; }
  pic.slice_end_ctu = ec_slice_end_ctu(ec_ends_segment(p.wpp ? 0 : p.slice_units, p.segment_units, k, p.units), p.ctus_x, cx1, cy1);
  if (p.wpp && k > 0 && p.ctus_x > 1 && p.sync) { // every lane copies the whole set: nothing a lane reads from LDS later was written by another lane
    const uint32_t *src = sync + (k - 1) * (EC_SYNC_BYTES / 4);
    for (int i = 0; i < EC_SYNC_BYTES / 4; i++) ((uint32_t *)l.ctx)[i] = src[i];
  } else ec_init_contexts(l.ctx, t, slice_qp);
  s.out = p.out + (size_t)f * p.frame_stride + p.unit_off[k];
  s.cap = p.unit_cap[k] & ~3u;
  ec_code_substream(s, pic, cx0, cx1, cy0, cy1);
  const uint32_t stored = s.pos < s.cap ? s.pos : s.cap;
  if (stored & (EC_STAGE_BYTES - 1)) ec_flush_stage(s, stored);
  if (lane == 0) { p.sizes[u] = s.pos; p.overflow[u] = s.overflow; }
}

// The used bytes of the sub-streams of a batch, one behind the other: workgroup i copies sub-stream i to dst + dst_off[i] (the host's exclusive scan over the downloaded
// lengths).  A length is clipped to the region's capacity and to the destination.
extern "C" __global__ __launch_bounds__(256) void hevcdl_entropy_pack_kernel(hevcdl_entropy_pack_params p)
{
  const long long i = blockIdx.x;
  if (i >= (long long)p.n_frames * p.units) return;
  const int f = (int)(i / p.units), k = (int)(i - (long long)f * p.units);
  uint32_t len = p.sizes[i];
  if (len > p.unit_cap[k]) len = p.unit_cap[k];
  const unsigned long long at = p.dst_off[i];
  if (at > p.dst_cap || len > p.dst_cap - at) return;
  const unsigned char *src = p.src + (size_t)f * p.frame_stride + p.unit_off[k];
  for (uint32_t b = threadIdx.x; b < len; b += blockDim.x) p.dst[at + b] = src[b];
}

extern "C" void hevcdl_launch_entropy(const hevcdl_entropy_params *p, void *stream, void *mid_event_opt)
{
  if (mid_event_opt && (p->n_frames <= 0 || p->units <= 0 || !(p->wpp && p->ctus_x > 1))) (void)hipEventRecord((hipEvent_t)mid_event_opt, (hipStream_t)stream);
  if (p->n_frames <= 0 || p->units <= 0) return;
  hevcdl_entropy_params q = *p;
  hipStream_t s = (hipStream_t)stream;
  if (q.wpp && q.ctus_x > 1) {
    q.phase = 1;
    hipLaunchKernelGGL(hevcdl_entropy_kernel, dim3((unsigned)((q.n_frames + EC_WAVES - 1) / EC_WAVES)), dim3(EC_WAVES * 64), 0, s, q);
    if (mid_event_opt) (void)hipEventRecord((hipEvent_t)mid_event_opt, s);
  }
  q.phase = q.wpp ? 2 : 0;
  const long long n = (long long)q.n_frames * q.units;
  hipLaunchKernelGGL(hevcdl_entropy_kernel, dim3((unsigned)((n + EC_WAVES - 1) / EC_WAVES)), dim3(EC_WAVES * 64), 0, s, q);
}

extern "C" void hevcdl_launch_entropy_pack(const hevcdl_entropy_pack_params *p, void *stream)
{
  const long long n = (long long)p->n_frames * p->units;
  if (n <= 0) return;
  hipLaunchKernelGGL(hevcdl_entropy_pack_kernel, dim3((unsigned)n), dim3(256), 0, (hipStream_t)stream, *p);
}
