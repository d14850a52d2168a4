// qp_rd_kernel.hip -- device side of the cfg key DeltaQpRD (TEncSlice::precompressSlice, TEncSlice.cpp:572-661): behind every candidate's decision launch the picture
// sums of the candidate (m_uiPicTotalBits / m_uiPicDist, :959-961) and the comparison with the best so far; behind every candidate but the first the copy of a new best's
// outputs from the trial set over the call's own.  The comparison itself is csrc/qp_rd.h, the source the host runs too.
//
// Both are plain launches in stream order behind the decision launch whose records they read: nothing here waits for another wave, no flag is polled, no atomics.  Every
// loop bound is a launch parameter.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "hevcdl.h"
#include "hevcdl_dev.h"
#include "qp_rd.h"

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));      // one dwordx4 load or store

// One workgroup of 256 lanes per picture.  Lane l reads bits and dist (two adjacent words) of CTUs l, l + 256, ...; the 256 partial sums go through a fixed binary tree in
// LDS.  The sums are 64-bit integers: exact, and the same whatever the order.  Lane 0 then runs the comparison in f64 and writes the picture's row.
extern "C" __global__ __launch_bounds__(256) void hevcdl_qp_rd_sum_kernel(hevcdl_qp_rd_sum_params p)
{
  __shared__ unsigned long long s_bits[256], s_dist[256];
  const int pic = (int)blockIdx.x, lane = (int)threadIdx.x;
  if (pic >= p.n_frames) return;
  const unsigned char *recs = p.records + (size_t)pic * p.ctus_per_frame * sizeof(hevcdl_ctu_record);
  unsigned long long bits = 0, dist = 0;
  for (int it = 0; it < p.ctu_iters; it++) {
    const int a = it * 256 + lane;
    if (a < p.ctus_per_frame) {
      const uint2 w = *(const uint2 *)(recs + (size_t)a * sizeof(hevcdl_ctu_record) + offsetof(hevcdl_ctu_record, bits));      // bits, dist: 8-byte aligned in a 15120-byte record
      bits += w.x; dist += w.y;
    }
  }
  s_bits[lane] = bits; s_dist[lane] = dist;
  __syncthreads();
  for (int half = 128; half > 0; half >>= 1) {
    if (lane < half) { s_bits[lane] += s_bits[lane + half]; s_dist[lane] += s_dist[lane + half]; }
    __syncthreads();
  }
  if (lane == 0) {
    hevcdl_qp_rd_row *row = p.rows + pic;
    double best = p.idx == 0 ? HEVCDL_QP_RD_MAX_DOUBLE : row->best_cost;      // dPicRdCostBest = MAX_DOUBLE, TEncSlice.cpp:604
    const int better = hevcdl_qp_rd_better(s_bits[0], s_dist[0], p.frame_lambda, &best);
    row->bits[p.idx] = s_bits[0]; row->dist[p.idx] = s_dist[0];
    row->best_cost = best;
    if (better || p.idx == 0) row->best_idx = p.idx;
    row->take = better && p.idx > 0;      // candidate 0 was written into the call's own buffers: nothing to copy
  }
}

// Grid (chunk, picture).  A picture's records and reconstruction are one run of pic16 16-byte units (the first rec16 of them the records); workgroup (c, f) copies units
// [c * chunk16, (c + 1) * chunk16) of picture f when the picture's row says so, four units a lane in flight (dwordx4 loads, then dwordx4 stores).  The flag is read through
// readfirstlane: a wave-uniform value, so a picture that is not taken costs its workgroups one scalar load.  Workgroup (0, f) also copies the 40 bytes of statistics.
extern "C" __global__ __launch_bounds__(256) void hevcdl_qp_rd_keep_kernel(hevcdl_qp_rd_keep_params p)
{
  const int pic = (int)blockIdx.y, lane = (int)threadIdx.x;
  if (pic >= p.n_frames) return;
  const int take = __builtin_amdgcn_readfirstlane(p.rows[pic].take);
  if (!take) return;
  const unsigned long long rec16 = p.rec16, pic16 = p.pic16, img16 = pic16 - rec16;
  const u32x4 *__restrict__ src_r = (const u32x4 *)p.src_records + (size_t)pic * rec16, *__restrict__ src_i = (const u32x4 *)p.src_recon + (size_t)pic * img16;
  u32x4 *__restrict__ dst_r = (u32x4 *)p.dst_records + (size_t)pic * rec16, *__restrict__ dst_i = (u32x4 *)p.dst_recon + (size_t)pic * img16;
  const unsigned long long begin = (unsigned long long)blockIdx.x * p.chunk16;
  for (int it = 0; it < p.chunk_iters; it++) {
    const unsigned long long u0 = begin + (unsigned long long)it * 1024 + lane;
    u32x4 v[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const unsigned long long u = u0 + 256ull * k;
      if (u < pic16) v[k] = u < rec16 ? src_r[u] : src_i[u - rec16];
    }
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const unsigned long long u = u0 + 256ull * k;
      if (u < pic16) { if (u < rec16) dst_r[u] = v[k]; else dst_i[u - rec16] = v[k]; }
    }
  }
  if (blockIdx.x == 0 && p.dst_stats && lane < (int)(sizeof(hevcdl_frame_stats) / 8))
    ((unsigned long long *)p.dst_stats)[(size_t)pic * (sizeof(hevcdl_frame_stats) / 8) + lane] = ((const unsigned long long *)p.src_stats)[(size_t)pic * (sizeof(hevcdl_frame_stats) / 8) + lane];
}

extern "C" void hevcdl_launch_qp_rd_sum(const hevcdl_qp_rd_sum_params *pp, void *stream)
{
  if (pp->n_frames <= 0 || pp->ctus_per_frame <= 0) return;
  hevcdl_qp_rd_sum_params p = *pp;
  p.ctu_iters = (p.ctus_per_frame + 255) / 256;
  hipLaunchKernelGGL(hevcdl_qp_rd_sum_kernel, dim3((unsigned)p.n_frames), dim3(256), 0, (hipStream_t)stream, p);
}

extern "C" void hevcdl_launch_qp_rd_keep(const hevcdl_qp_rd_keep_params *pp, void *stream)
{
  if (pp->n_frames <= 0 || pp->pic16 == 0) return;
  hevcdl_qp_rd_keep_params p = *pp;
  // 128 KB a workgroup (8 rounds of 256 lanes x 4 units), fewer rounds for a small picture: a 2160p picture (43 MB) is 336 workgroups
  const unsigned long long rounds = (p.pic16 + 1023) / 1024;
  p.chunk_iters = (int)(rounds < 8 ? rounds : 8);
  p.chunk16 = 1024ull * p.chunk_iters;
  const unsigned long long chunks = (p.pic16 + p.chunk16 - 1) / p.chunk16;
  for (int first = 0; first < pp->n_frames; first += 65535) {      // (gridDim.y holds 65535 pictures)
    hevcdl_qp_rd_keep_params q = p;
    q.n_frames = pp->n_frames - first < 65535 ? pp->n_frames - first : 65535;
    q.rows = p.rows + first;
    q.src_records = p.src_records + (size_t)first * p.rec16 * 16; q.dst_records = p.dst_records + (size_t)first * p.rec16 * 16;
    q.src_recon = p.src_recon + (size_t)first * (p.pic16 - p.rec16) * 16; q.dst_recon = p.dst_recon + (size_t)first * (p.pic16 - p.rec16) * 16;
    if (p.dst_stats) { q.src_stats = p.src_stats + (size_t)first * sizeof(hevcdl_frame_stats); q.dst_stats = p.dst_stats + (size_t)first * sizeof(hevcdl_frame_stats); }
    hipLaunchKernelGGL(hevcdl_qp_rd_keep_kernel, dim3((unsigned)chunks, (unsigned)q.n_frames), dim3(256), 0, (hipStream_t)stream, q);
  }
}
