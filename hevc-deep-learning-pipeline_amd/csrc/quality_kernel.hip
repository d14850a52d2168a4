// quality_kernel.hip -- picture quality metrics for gfx950 (MI355X): the exact SSE and the MS-SSIM of the reference's PrintMSSSIM key.
//
// Replaces TEncGOP::xCalculateMSSSIM (HM_dl/source/Lib/TLibEncoder/TEncGOP.cpp:2559-2727, called per plane at :2401-2420) and the SSD loop of
// xCalculateAddPSNR (:2380-2390) for planes that are already in HBM.  The arithmetic of the reference, restated:
//   scales     1 .. 5 by the plane's size: a width or height below 22 / 44 / 88 / 176 gives 1 / 2 / 3 / 4 scales, otherwise 5       (:2567-2587)
//   pyramid    level s has (width >> s) x (height >> s) values; value (y, x) is the mean of FLAT entries 2y * 2Ws + 2x (+ 1) and
//              (2y + 1) * 2Ws + 2x (+ 1) of level s - 1, Ws = width >> s: the row pitch the reference reads level s - 1 with is 2 Ws, which is
//              one less than that level's own pitch when its width is odd (:2643-2661).  Every value is an integer / 4^s, so the levels are
//              held here as 32-bit numerators (at most 1023 * 256) and scaled by the exact power of two when they are read.
//   window     11 x 11, exp(-(dy^2 + dx^2) / 4.5) normalised by the sum of all 121, computed on the host in the reference's loop order (:2591-2611)
//   block      five sums over the window, y then x, each term (a * b) * w added to the running sum in f64 without contraction; then the three
//              variances, (2 s_or + c2) / (s_oo + s_rr + c2), and on the coarsest scale only times (2 m_o m_r + c1) / (m_o^2 + m_r^2 + c1), with
//              c1 = (0.01 max)^2, c2 = (0.03 max)^2, max = (1 << bitDepth) - 1                                                        (:2663-2715)
//   mean       sum of the blocks of a scale / (blocksPerRow * blocksPerColumn); the product over the scales of pow(mean, exponent)     (:2717-2724)
// Every block value is bit-identical to the reference's (same operations in the same order: this file is compiled with -ffp-contract=off and
// says so again below).  The reference adds the blocks of a scale serially in raster order; here a lane adds its four blocks, a workgroup
// reduces its 256 lanes by a fixed tree, and one workgroup per (picture, plane, scale) adds the workgroups' partial sums in a fixed order: no
// floating-point atomics, the same bits on every run, for every batch size and every position in the batch.
//
// Kernels:
//   hevcdl_quality_sse_kernel       exact integer SSE per (picture, plane); 64-bit integer atomics (exact, order-free)
//   hevcdl_quality_pyramid_kernel   level s from level s - 1 (level 1 straight from the samples)
//   hevcdl_quality_ssim_kernel      one workgroup per 64 x 16 tile of blocks of a (picture, plane, scale): the 74 x 26 samples under it go into
//                                   LDS once as f64; lane (lx, ly) computes the four blocks (x = lx, y = 4 ly .. 4 ly + 3), walking the 14 sample
//                                   rows under them once: a row's 11 samples and their three products (exact, so computing them once per row and
//                                   not once per block changes no bit) are used by up to four blocks.  Neighbouring lanes read neighbouring
//                                   f64s (no bank conflict); the weights are read with a uniform index (scalar loads).
//   hevcdl_quality_finish_kernel    partial sums -> mean per scale -> pow and product -> hevcdl_quality
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "hevcdl.h"
#include "hevcdl_dev.h"

#pragma clang fp contract(off)

namespace {

#define GLB __attribute__((address_space(1)))
#define LDS __attribute__((address_space(3)))

enum { WIN = 11, TILE_W = 64, TILE_H = 16, RUN = 4, LW = TILE_W + WIN - 1, LH = TILE_H + WIN - 1 };

// sample / numerator i of a level as f64 (level 0: the picture's samples; above: 32-bit numerators times 4^-s)
template <typename PEL> __device__ __forceinline__ double level_value(const void GLB *base, int level0, size_t i, double inv)
{
  return level0 ? (double)((const PEL GLB *)base)[i] : (double)((const uint32_t GLB *)base)[i] * inv;
}

template <typename PEL> __global__ __launch_bounds__(256) void hevcdl_quality_sse_kernel(hevcdl_quality_params p)
{
  const int plane = blockIdx.y, pic = blockIdx.z;
  const size_t n = (size_t)p.plane_w[plane] * p.plane_h[plane];
  const PEL GLB *o = (const PEL GLB *)p.org + (size_t)pic * p.frame_samples + p.plane_off[plane];
  const PEL GLB *r = (const PEL GLB *)p.pic + (size_t)pic * p.frame_samples + p.plane_off[plane];
  unsigned long long acc = 0;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    const long long d = (long long)o[i] - (long long)r[i];
    acc += (unsigned long long)(d * d);
  }
  __shared__ unsigned long long part[256];
  part[threadIdx.x] = acc;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) { if ((int)threadIdx.x < s) part[threadIdx.x] += part[threadIdx.x + s]; __syncthreads(); }
  if (threadIdx.x == 0 && part[0]) atomicAdd((unsigned long long *)p.out + ((size_t)(p.out_first + pic) * 6 + plane), part[0]);      // hevcdl_quality.sse[plane] (zeroed by the caller)
}

// level s (numerators) of both pictures from level s - 1; grid (elements / 256, 2 * planes, pictures)
template <typename PEL> __global__ __launch_bounds__(256) void hevcdl_quality_pyramid_kernel(hevcdl_quality_params p, int s)
{
  const int plane = blockIdx.y >> 1, which = blockIdx.y & 1, pic = blockIdx.z;
  if (s >= p.scales[plane]) return;
  const int ws = p.plane_w[plane] >> s, hs = p.plane_h[plane] >> s;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= ws * hs) return;
  const int y = i / ws, x = i - y * ws;
  const size_t a = (size_t)(2 * y) * (2 * ws) + 2 * x, b = (size_t)(2 * y + 1) * (2 * ws) + 2 * x;      // flat, with the pitch the reference reads with (:2651-2654)
  uint32_t GLB *dst = (uint32_t GLB *)p.pyr + (size_t)pic * p.pyr_pic_words + p.pyr_off[plane][s] + (which ? p.pyr_half : 0);
  uint32_t v;
  if (s == 1) {
    const PEL GLB *src = (const PEL GLB *)(which ? p.pic : p.org) + (size_t)pic * p.frame_samples + p.plane_off[plane];
    v = (uint32_t)src[a] + src[a + 1] + src[b] + src[b + 1];
  } else {
    const uint32_t GLB *src = (const uint32_t GLB *)p.pyr + (size_t)pic * p.pyr_pic_words + p.pyr_off[plane][s - 1] + (which ? p.pyr_half : 0);
    v = src[a] + src[a + 1] + src[b] + src[b + 1];
  }
  dst[i] = v;
}

// grid (tiles_x * tiles_y of the largest plane of the launch, plane, picture); `s` = scale of the launch
template <typename PEL> __global__ __launch_bounds__(256) void hevcdl_quality_ssim_kernel(hevcdl_quality_params p, int s)
{
  const int plane = blockIdx.y, pic = blockIdx.z;
  if (s >= p.scales[plane]) return;
  const int ws = p.plane_w[plane] >> s, hs = p.plane_h[plane] >> s;
  const int bw = ws - WIN + 1, bh = hs - WIN + 1;                      // blocksPerRow, blocksPerColumn (:2674-2675)
  if (bw <= 0 || bh <= 0) return;                                      // the reference's loops are empty
  const int tiles_x = (bw + TILE_W - 1) / TILE_W, tiles_y = (bh + TILE_H - 1) / TILE_H;
  if ((int)blockIdx.x >= tiles_x * tiles_y) return;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x, x0 = tx * TILE_W, y0 = ty * TILE_H;
  const int tid = threadIdx.x;
  __shared__ double so[LH][LW], sr[LH][LW];
  __shared__ double red[256];
  {
    const double inv = 1.0 / (double)(1 << (2 * s));
    const void GLB *bo, *br;
    if (s == 0) {
      bo = (const void GLB *)((const PEL GLB *)p.org + (size_t)pic * p.frame_samples + p.plane_off[plane]);
      br = (const void GLB *)((const PEL GLB *)p.pic + (size_t)pic * p.frame_samples + p.plane_off[plane]);
    } else {
      const uint32_t GLB *b = (const uint32_t GLB *)p.pyr + (size_t)pic * p.pyr_pic_words + p.pyr_off[plane][s];
      bo = (const void GLB *)b; br = (const void GLB *)(b + p.pyr_half);
    }
    for (int i = tid; i < LH * LW; i += 256) {
      const int yy = i / LW, xx = i - yy * LW, gy = y0 + yy, gx = x0 + xx;
      const bool in = gy < hs && gx < ws;                                // outside: only under blocks that are not counted
      const size_t gi = in ? (size_t)gy * ws + gx : 0;
      const double vo = level_value<PEL>(bo, s == 0, gi, inv), vr = level_value<PEL>(br, s == 0, gi, inv);
      ((double LDS *)&so[0][0])[i] = in ? vo : 0.0;
      ((double LDS *)&sr[0][0])[i] = in ? vr : 0.0;
    }
  }
  __syncthreads();
  const int lx = tid & (TILE_W - 1), ly = tid >> 6;                      // blocks (x0 + lx, y0 + RUN * ly + j), j = 0 .. RUN - 1
  const double GLB *w = (const double GLB *)p.weights;
  double m_o[RUN], m_r[RUN], m_oo[RUN], m_rr[RUN], m_or[RUN];
#pragma unroll
  for (int j = 0; j < RUN; j++) m_o[j] = m_r[j] = m_oo[j] = m_rr[j] = m_or[j] = 0.0;
  const double LDS *po = (const double LDS *)&so[RUN * ly][lx], *pr = (const double LDS *)&sr[RUN * ly][lx];
#pragma unroll 1
  for (int yy = 0; yy < WIN + RUN - 1; yy++) {                           // sample rows under the lane's blocks, top to bottom
    double o[WIN], r[WIN], oo[WIN], rr[WIN], orr[WIN];
#pragma unroll
    for (int x = 0; x < WIN; x++) { o[x] = po[yy * LW + x]; r[x] = pr[yy * LW + x]; oo[x] = o[x] * o[x]; rr[x] = r[x] * r[x]; orr[x] = o[x] * r[x]; }
#pragma unroll
    for (int j = 0; j < RUN; j++) {
      const int wy = yy - j;                                             // the window row of block j this sample row is (uniform over the wave)
      if (wy >= 0 && wy < WIN) {
        const double GLB *wr = w + wy * WIN;
#pragma unroll
        for (int x = 0; x < WIN; x++) {                                  // :2699-2703, in that order
          const double g = wr[x];
          m_o[j] += o[x] * g; m_r[j] += r[x] * g; m_oo[j] += oo[x] * g; m_rr[j] += rr[x] * g; m_or[j] += orr[x] * g;
        }
      }
    }
  }
  const double c1 = p.c1, c2 = p.c2;
  const bool last = s == p.scales[plane] - 1;
  double sum = 0.0;
#pragma unroll
  for (int j = 0; j < RUN; j++) {
    const double var_o = m_oo[j] - (m_o[j] * m_o[j]), var_r = m_rr[j] - (m_r[j] * m_r[j]), cov = m_or[j] - (m_o[j] * m_r[j]);      // :2707-2709
    double v = ((2.0 * cov + c2) / (var_o + var_r + c2));                                                                      // :2711
    if (last) v *= (2.0 * m_o[j] * m_r[j] + c1) / (m_o[j] * m_o[j] + m_r[j] * m_r[j] + c1);                                   // :2714
    if (x0 + lx < bw && y0 + RUN * ly + j < bh) sum += v;
  }
  red[tid] = sum;
  __syncthreads();
  for (int st = 128; st > 0; st >>= 1) { if (tid < st) red[tid] += red[tid + st]; __syncthreads(); }
  if (tid == 0) ((double GLB *)p.partial)[(size_t)pic * p.part_pic + p.part_off[plane][s] + blockIdx.x] = red[0];
}

// grid (pictures); 15 x 16 lanes: lanes 16 k .. 16 k + 15 add the partial sums of (plane, scale) k = 5 plane + scale
__global__ __launch_bounds__(256) void hevcdl_quality_finish_kernel(hevcdl_quality_params p)
{
  const int pic = blockIdx.x, tid = threadIdx.x, k = tid >> 4, l = tid & 15;
  __shared__ double red[256];
  __shared__ double mean[15];
  double acc = 0.0;
  int plane = 0, s = 0, n = 0, bw = 0, bh = 0;
  if (k < 15) {
    plane = k / 5; s = k - 5 * plane;
    if (s < p.scales[plane]) {
      bw = (p.plane_w[plane] >> s) - WIN + 1; bh = (p.plane_h[plane] >> s) - WIN + 1;
      if (bw > 0 && bh > 0) n = ((bw + TILE_W - 1) / TILE_W) * ((bh + TILE_H - 1) / TILE_H);
      const double GLB *src = (const double GLB *)p.partial + (size_t)pic * p.part_pic + p.part_off[plane][s];
      for (int i = l; i < n; i += 16) acc += src[i];
    }
  }
  red[tid] = acc;
  __syncthreads();
  for (int st = 8; st > 0; st >>= 1) { if (l < st) red[tid] += red[tid + st]; __syncthreads(); }
  if (k < 15 && l == 0) mean[k] = red[tid] / (double)(bw * bh);          // meanSSIM /= totalBlocks (:2721): 0 / totalBlocks where the loops were empty
  __syncthreads();
  if (tid < p.n_planes) {
    // exponentWeights (:2614-2618)
    const double ex[5][5] = { { 1.0, 0, 0, 0, 0 }, { 0.1356, 0.8644, 0, 0, 0 }, { 0.0711, 0.4530, 0.4760, 0, 0 }, { 0.0517, 0.3295, 0.3462, 0.2726, 0 },
                              { 0.0448, 0.2856, 0.3001, 0.2363, 0.1333 } };
    const int ns = p.scales[tid];
    double v = 1.0;
    for (int sc = 0; sc < ns; sc++) v *= pow(mean[5 * tid + sc], ex[ns - 1][sc]);      // :2723
    ((double GLB *)p.out)[(size_t)(p.out_first + pic) * 6 + 3 + tid] = v;      // hevcdl_quality.msssim[plane]
  }
}

// workgroups of the SSE kernel per (picture, plane): 4096 samples each, at most 1024
int sse_blocks_of(const hevcdl_quality_params &p)
{
  int max_n = 0;
  for (int c = 0; c < p.n_planes; c++) max_n = max_n > p.plane_w[c] * p.plane_h[c] ? max_n : p.plane_w[c] * p.plane_h[c];
  const int b = (max_n + 256 * 16 - 1) / (256 * 16);
  return b > 1024 ? 1024 : b;
}

template <typename PEL> void launch(const hevcdl_quality_params &p, hipStream_t st)
{
  int max_n = 0, max_scales = 0, n_planes = p.n_planes;
  for (int c = 0; c < n_planes; c++) { max_n = max_n > p.plane_w[c] * p.plane_h[c] ? max_n : p.plane_w[c] * p.plane_h[c]; max_scales = max_scales > p.scales[c] ? max_scales : p.scales[c]; }
  hipLaunchKernelGGL(hevcdl_quality_sse_kernel<PEL>, dim3(sse_blocks_of(p), n_planes, p.n_pics), dim3(256), 0, st, p);
  for (int s = 1; s < max_scales; s++)
    hipLaunchKernelGGL(hevcdl_quality_pyramid_kernel<PEL>, dim3(((max_n >> (2 * s)) + 255) / 256 + 1, 2 * n_planes, p.n_pics), dim3(256), 0, st, p, s);
  for (int s = 0; s < max_scales; s++) {
    int tiles = 0;
    for (int c = 0; c < n_planes; c++) {
      const int bw = (p.plane_w[c] >> s) - WIN + 1, bh = (p.plane_h[c] >> s) - WIN + 1;
      if (s < p.scales[c] && bw > 0 && bh > 0) { const int t = ((bw + TILE_W - 1) / TILE_W) * ((bh + TILE_H - 1) / TILE_H); tiles = tiles > t ? tiles : t; }
    }
    if (tiles) hipLaunchKernelGGL(hevcdl_quality_ssim_kernel<PEL>, dim3(tiles, n_planes, p.n_pics), dim3(256), 0, st, p, s);
  }
  hipLaunchKernelGGL(hevcdl_quality_finish_kernel, dim3(p.n_pics), dim3(256), 0, st, p);
}

}  // namespace

// number of scales of a plane (:2567-2587)
extern "C" int hevcdl_quality_scales(int w, int h)
{
  return (w < 22 || h < 22) ? 1 : (w < 44 || h < 44) ? 2 : (w < 88 || h < 88) ? 3 : (w < 176 || h < 176) ? 4 : 5;
}

// Fills the layout fields of p (scales, offsets into the pyramid and partial-sum workspaces) from plane_w / plane_h / n_planes.
extern "C" void hevcdl_quality_layout(hevcdl_quality_params *p)
{
  size_t words = 0; int parts = 0;
  for (int c = 0; c < 3; c++) {
    p->scales[c] = c < p->n_planes ? hevcdl_quality_scales(p->plane_w[c], p->plane_h[c]) : 0;
    for (int s = 0; s < 5; s++) {
      p->pyr_off[c][s] = words; p->part_off[c][s] = parts;
      if (s >= p->scales[c]) continue;
      const int ws = p->plane_w[c] >> s, hs = p->plane_h[c] >> s, bw = ws - WIN + 1, bh = hs - WIN + 1;
      if (s > 0) words += (size_t)ws * hs;
      if (bw > 0 && bh > 0) parts += ((bw + TILE_W - 1) / TILE_W) * ((bh + TILE_H - 1) / TILE_H);
    }
  }
  p->pyr_half = words; p->pyr_pic_words = 2 * words; p->part_pic = parts;
}

extern "C" void hevcdl_launch_quality(const hevcdl_quality_params *pp, void *stream)
{
  if (pp->sample_bytes == 1) launch<uint8_t>(*pp, (hipStream_t)stream);
  else launch<uint16_t>(*pp, (hipStream_t)stream);
}

// The SSE kernel alone (the picture report, report_kernel.hip): the same launch as the first one of hevcdl_launch_quality; nothing of the pyramid workspace is read.
extern "C" void hevcdl_launch_quality_sse(const hevcdl_quality_params *pp, void *stream)
{
  if (pp->sample_bytes == 1) hipLaunchKernelGGL(hevcdl_quality_sse_kernel<uint8_t>, dim3(sse_blocks_of(*pp), pp->n_planes, pp->n_pics), dim3(256), 0, (hipStream_t)stream, *pp);
  else hipLaunchKernelGGL(hevcdl_quality_sse_kernel<uint16_t>, dim3(sse_blocks_of(*pp), pp->n_planes, pp->n_pics), dim3(256), 0, (hipStream_t)stream, *pp);
}
