// dbk_select_kernel.hip -- per-picture deblocking parameters for gfx950 (MI355X): the measurement of DeblockingFilterMetric 1 and, at the end of the file, the filter
// trials of DeblockingFilterMetric 2 (hevcdl_dbk_trial_kernel).
//
// Replaces the two loops of TEncGOP::applyDeblockingFilterMetric (HM_dl/source/Lib/TLibEncoder/TEncGOP.cpp:3216-3268) over the luma reconstruction BEFORE deblocking:
// on every vertical edge at a multiple of 32 (the largest transform block) and every row, and on every horizontal edge and every column, a line p2 p1 p0 | q0 q1 q2
// across the edge adds |p0 - q0| when its a = (|p2 - 2 p1 + p0| + |q0 - 2 q1 + q2|) << 1 lies strictly between thr1 and thr2.  The sums are integers, so their order is
// free: lanes keep 32-bit partial sums (a lane sees a few thousand lines of at most 1023 each), a workgroup folds them and adds one 64-bit word per direction to the
// picture's pair.  The host turns the pair into the picture's offset (csrc/dbk_select.h).
//
// The kernel touches 6 of every 32 columns (vertical edges: two aligned groups of four samples of a row, one lane per row) and 6 of every 32 rows (horizontal edges: six rows
// of four adjacent columns a lane, adjacent lanes on adjacent dwords): about three eighths of the luma plane's cache lines, once.  Only the edges that count are visited.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include "hevcdl_dev.h"
#include "deblock_core.h"

namespace {

__device__ __forceinline__ int iabs(int v) { return v < 0 ? -v : v; }
// one line across an edge (TEncGOP.cpp:3221-3231): what it adds to the edge's sum
__device__ __forceinline__ uint32_t metric_line(int p2, int p1, int p0, int q0, int q1, int q2, int thr1, int thr2)
{
  const int a = (iabs(p2 - 2 * p1 + p0) + iabs(q0 - 2 * q1 + q2)) << 1;
  return (thr1 < a && a < thr2) ? (uint32_t)iabs(p0 - q0) : 0u;
}

enum { DBK_TRIAL_TW = 256, DBK_TRIAL_TH = 32 };      // the rectangle of hevcdl_deblock_fused_kernel

} // namespace

// grid: (workgroups of a picture, 1, pictures).  Items of a picture: first the lines of the vertical edges, edges_x * height of them, one (edge, row) each, rows of an
// edge on adjacent lanes; then the horizontal edges in groups of four columns, edges_y * (width / 4), one (edge, column group) each.  width is a multiple of 8.
template <typename PEL>
__global__ __launch_bounds__(256) void hevcdl_dbk_metric_kernel(hevcdl_dbk_metric_params p)
{
  const int frame = blockIdx.z, W = p.width, H = p.height;
  const size_t ysz = (size_t)W * H, fsz = ysz + (ysz >> 1);
  const PEL GLB *src = (const PEL GLB *)p.recon + (size_t)frame * fsz;
  const int n_v = p.edges_x * H, groups = W >> 2, n_h = p.edges_y * groups;
  uint32_t col = 0, row = 0;
  for (int it = blockIdx.x * 256 + threadIdx.x; it < n_v + n_h; it += gridDim.x * 256) {
    if (it < n_v) {
      const int c = 32 * (it / H + 1), r = it % H;            // c + 3 < W: c <= 32 (edges_x) = 32 ((W >> 5) - 1) <= W - 32
      int l[4], q[4];
      load4<PEL>(src + (size_t)r * W + c - 4, l); load4<PEL>(src + (size_t)r * W + c, q);
      col += metric_line(l[1], l[2], l[3], q[0], q[1], q[2], p.thr1, p.thr2);
    } else {
      const int j = it - n_v, r = 32 * (j / groups + 1), c = 4 * (j % groups);      // rows r - 3 .. r + 2, r + 2 < H as above
      int m[6][4];
#pragma unroll
      for (int k = 0; k < 6; k++) load4<PEL>(src + (size_t)(r - 3 + k) * W + c, m[k]);
#pragma unroll
      for (int i = 0; i < 4; i++) row += metric_line(m[0][i], m[1][i], m[2][i], m[3][i], m[4][i], m[5][i], p.thr1, p.thr2);
    }
  }
  // fold: lanes of a wave by shuffles (a wave's sum fits 32 bits: see above), the four waves through LDS into a 64-bit word
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) { col += __shfl_down(col, d, 64); row += __shfl_down(row, d, 64); }
  __shared__ uint32_t part[4][2];
  if ((threadIdx.x & 63) == 0) { part[threadIdx.x >> 6][0] = col; part[threadIdx.x >> 6][1] = row; }
  __syncthreads();
  if (threadIdx.x < 2) {
    const unsigned long long s = (unsigned long long)part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] + part[3][threadIdx.x];
    if (s) atomicAdd((unsigned long long *)p.sums + 2 * (size_t)frame + threadIdx.x, s);
  }
}

// p.sums must be zero before the launch (the caller clears it on the same stream)
extern "C" void hevcdl_launch_dbk_metric(const hevcdl_dbk_metric_params *pp, void *stream)
{
  const hevcdl_dbk_metric_params p = *pp;
  const long long items = (long long)p.edges_x * p.height + (long long)p.edges_y * (p.width >> 2);
  const unsigned blocks = (unsigned)std::min<long long>(std::max<long long>((items + 255) / 256, 1), 1024);
  const dim3 grid(blocks, 1, (unsigned)p.n_frames);
  if (p.sample_bytes == 1) hipLaunchKernelGGL(hevcdl_dbk_metric_kernel<uint8_t>, grid, dim3(256), 0, (hipStream_t)stream, p);
  else hipLaunchKernelGGL(hevcdl_dbk_metric_kernel<uint16_t>, grid, dim3(256), 0, (hipStream_t)stream, p);
}

// ---- DeblockingFilterMetric 2: the distortion of every trial of TEncGOP::applyDeblockingFilterParameterSelection (TEncGOP.cpp:3347-3377) in one launch --------------------
// The reference restores the reconstruction, filters the whole picture with (slice_beta_offset_div2, slice_tc_offset_div2) = (b, t) and sums the squared error against the
// original over all three components, (d * d) >> 2 (bd - 8) PER SAMPLE (xFindDistortionFrame, :2172-2200), for up to 49 pairs b, t in -3 .. 3.  Here a workgroup takes the
// rectangle of hevcdl_deblock_fused_kernel (deblock_kernel.hip: TW x TH shifted by 4, vertical edges in registers, horizontal edges from LDS), loads it ONCE from the
// reconstruction -- and the samples it owns once from the original --, and loops over the trials inside: filter a copy of the registers, through LDS, filter, square against
// the original, fold.  No trial picture is ever written: a trial costs ALU and LDS, not HBM.  The samples a thread squares are exactly those the fused kernel's stage 2
// stores, so every sample of the picture is counted once.  Luma depends on (tc, beta) only and chroma on the chroma tc only (a function of t): the host passes the DISTINCT
// luma pairs and chroma values with a map from the 49 entries (at low QP many offsets clip to the same table entries), and a wave adds its sum to every entry mapped.
template <int CHROMA, typename PEL>
__global__ __launch_bounds__(256) void hevcdl_dbk_trial_kernel(hevcdl_dbk_trial_params q)
{
  const hevcdl_dbk_params &p = q.d;
  constexpr int TW = DBK_TRIAL_TW, TH = DBK_TRIAL_TH, DW = TW * (int)sizeof(PEL) / 4, QD = (int)sizeof(PEL);
  constexpr int EXN = TW / 8, XGN = TW / 4;
  static_assert(EXN * (TH / 4) == 256 && XGN * (TH / 8) == 256, "one thread per block in both stages");
  __shared__ uint32_t tile[TH][DW + 1];
  const int frame = blockIdx.z, tid = threadIdx.x;
  const int W = p.width >> CHROMA, H = p.height >> CHROMA;
  const int tiles_x = (W + 4 + TW - 1) / TW, n_tiles = tiles_x * ((H + 4 + TH - 1) / TH), per_xcd = (n_tiles + 7) / 8;      // the XCD remap of the fused kernel
  const int lin = (int)blockIdx.x, vt = (lin & 7) * per_xcd + (lin >> 3);
  if (vt >= n_tiles) return;
  const int X0 = (vt % tiles_x) * TW, Y0 = (vt / tiles_x) * TH;
  const size_t ysz = (size_t)p.width * p.height, fsz = ysz + (ysz >> 1);
  const unsigned char GLB *recs = (const unsigned char GLB *)p.records + (size_t)frame * p.ctus_per_frame * REC_SIZE;
  const int ex = tid % EXN, sy = tid / EXN;
  const int x = X0 + 8 * ex, y = Y0 - 4 + 4 * sy;
  const bool rows_ok = y >= 0 && y < H, has_l = x > 0 && x <= W, has_r = x < W, s1 = rows_ok && (has_l || has_r);
  const int xg = tid % XGN, eb = tid / XGN;
  const int xh = X0 - 4 + 4 * xg, yh = Y0 + 8 * eb;
  const bool cols_ok = xh >= 0 && xh < W, has_u = yh > 0 && yh <= H, has_d = yh < H, s2 = cols_ok && (has_u || has_d);
  bool v0 = false, v1 = false, h0 = false, h1 = false;
  if (s1 && has_l && has_r) {
    if (CHROMA) { v0 = edge_flag(p, recs, p.ctus_x, 2 * x, 2 * y, 0); v1 = edge_flag(p, recs, p.ctus_x, 2 * x, 2 * y + 4, 0); }
    else v0 = edge_flag(p, recs, p.ctus_x, x, y, 0);
  }
  if (cols_ok && has_u && has_d) {
    if (CHROMA) { h0 = edge_flag(p, recs, p.ctus_x, 2 * xh, 2 * yh, 1); h1 = edge_flag(p, recs, p.ctus_x, 2 * xh + 4, 2 * yh, 1); }
    else h0 = edge_flag(p, recs, p.ctus_x, xh, yh, 1);
  }
  unsigned long long GLB *table = (unsigned long long GLB *)q.table + (size_t)frame * 49;
  const int n_trials = CHROMA ? q.n_chroma : q.n_luma;
#pragma unroll 1
  for (int c = 0; c < (CHROMA ? 2 : 1); c++) {
    const size_t plane = (size_t)frame * fsz + (CHROMA ? ysz + (size_t)c * (ysz >> 2) : 0);
    const PEL GLB *src = (const PEL GLB *)p.in + plane, *org = (const PEL GLB *)q.org + plane;
    int m0[4][8];                                             // the rectangle's share of this thread, loaded once: row i: p3 p2 p1 p0 | q0 q1 q2 q3
    int o[8][4];                                              // the original under the 4 x 8 block this thread owns in stage 2
#pragma unroll
    for (int i = 0; i < 4; i++) {
      int l[4] = { 0, 0, 0, 0 }, r[4] = { 0, 0, 0, 0 };
      if (s1) { const size_t at = (size_t)(y + i) * W + x; if (has_l) load4<PEL>(src + at - 4, l); if (has_r) load4<PEL>(src + at, r); }
#pragma unroll
      for (int k = 0; k < 4; k++) { m0[i][k] = l[k]; m0[i][4 + k] = r[k]; }
    }
#pragma unroll
    for (int k = 0; k < 8; k++) {
      o[k][0] = o[k][1] = o[k][2] = o[k][3] = 0;
      if (s2 && (k < 4 ? has_u : has_d)) load4<PEL>(org + (size_t)(yh - 4 + k) * W + xh, o[k]);
    }
#pragma unroll 1
    for (int j = 0; j < n_trials; j++) {
      const int tc = CHROMA ? q.tc_c[j] : q.tc[j], beta = q.beta[CHROMA ? 0 : j];
      if (s1) {
        int m[4][8];
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
          for (int k = 0; k < 8; k++) m[i][k] = m0[i][k];
        if (!CHROMA) { if (v0) filter_luma_pk(m, tc, beta, p.pel_max); }
        else {
#pragma unroll
          for (int i = 0; i < 4; i++) if (i < 2 ? v0 : v1) filter_chroma(m[i][2], m[i][3], m[i][4], m[i][5], tc, p.pel_max);
        }
#pragma unroll
        for (int i = 0; i < 4; i++) {
          uint32_t *row = &tile[4 * sy + i][2 * QD * ex];
          if constexpr (sizeof(PEL) == 1) {
            row[0] = (uint32_t)m[i][0] | ((uint32_t)m[i][1] << 8) | ((uint32_t)m[i][2] << 16) | ((uint32_t)m[i][3] << 24);
            row[1] = (uint32_t)m[i][4] | ((uint32_t)m[i][5] << 8) | ((uint32_t)m[i][6] << 16) | ((uint32_t)m[i][7] << 24);
          } else {
#pragma unroll
            for (int k = 0; k < 4; k++) row[k] = (uint32_t)m[i][2 * k] | ((uint32_t)m[i][2 * k + 1] << 16);
          }
        }
      }
      __syncthreads();
      uint32_t sse = 0;
      if (s2) {
        int m[4][8];                                          // column i: p3 p2 p1 p0 | q0 q1 q2 q3 downwards
#pragma unroll
        for (int k = 0; k < 8; k++) {
          const uint32_t *row = &tile[8 * eb + k][QD * xg];
          if constexpr (sizeof(PEL) == 1) { const uint32_t w = row[0]; m[0][k] = w & 255; m[1][k] = (w >> 8) & 255; m[2][k] = (w >> 16) & 255; m[3][k] = w >> 24; }
          else { const uint32_t w0 = row[0], w1 = row[1]; m[0][k] = w0 & 0xffff; m[1][k] = w0 >> 16; m[2][k] = w1 & 0xffff; m[3][k] = w1 >> 16; }
        }
        if (!CHROMA) { if (h0) filter_luma_pk(m, tc, beta, p.pel_max); }
        else {
#pragma unroll
          for (int i = 0; i < 4; i++) if (i < 2 ? h0 : h1) filter_chroma(m[i][2], m[i][3], m[i][4], m[i][5], tc, p.pel_max);
        }
#pragma unroll
        for (int k = 0; k < 8; k++) if (k < 4 ? has_u : has_d) {
#pragma unroll
          for (int i = 0; i < 4; i++) { const int d = m[i][k] - o[k][i]; sse += (uint32_t)(d * d) >> q.shift; }      // per sample, as the reference shifts
        }
      }
      __syncthreads();                                        // the next trial overwrites the tile
#pragma unroll
      for (int d = 32; d > 0; d >>= 1) sse += __shfl_down(sse, d, 64);      // a thread adds at most 32 x 255^2 (or 32 x (1023^2 >> 4)): a wave's sum fits 32 bits
      if ((tid & 63) == 0 && sse) {
        if (!CHROMA) { for (int e = 0; e < 49; e++) if (q.luma_of[e] == j) atomicAdd((unsigned long long *)&table[e], (unsigned long long)sse); }
        else for (int t = 0; t < 7; t++) if (q.chroma_of[t] == j) for (int b = 0; b < 7; b++) atomicAdd((unsigned long long *)&table[7 * b + t], (unsigned long long)sse);
      }
    }
  }
}

// q.table ([frame][49] uint64, entry 7 (b + 3) + (t + 3)) must be zero before the launch (the caller clears it on the same stream)
extern "C" void hevcdl_launch_dbk_trial(const hevcdl_dbk_trial_params *qq, void *stream)
{
  const hevcdl_dbk_trial_params q = *qq;
  hipStream_t s = (hipStream_t)stream;
  const int W = q.d.width, H = q.d.height;
  auto grid = [&](int w, int h) { const int n = ((w + 4 + DBK_TRIAL_TW - 1) / DBK_TRIAL_TW) * ((h + 4 + DBK_TRIAL_TH - 1) / DBK_TRIAL_TH); return dim3((unsigned)(((n + 7) / 8) * 8), 1, q.d.n_frames); };
  if (q.d.pel_max == 255) {
    hipLaunchKernelGGL((hevcdl_dbk_trial_kernel<0, uint8_t>), grid(W, H), dim3(256), 0, s, q);
    hipLaunchKernelGGL((hevcdl_dbk_trial_kernel<1, uint8_t>), grid(W >> 1, H >> 1), dim3(256), 0, s, q);
  } else {
    hipLaunchKernelGGL((hevcdl_dbk_trial_kernel<0, uint16_t>), grid(W, H), dim3(256), 0, s, q);
    hipLaunchKernelGGL((hevcdl_dbk_trial_kernel<1, uint16_t>), grid(W >> 1, H >> 1), dim3(256), 0, s, q);
  }
}
