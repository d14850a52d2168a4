// deblock_core.h -- device helpers of the deblocking kernels (deblock_kernel.hip: the filter; dbk_select_kernel.hip: the filter trials of DeblockingFilterMetric 2):
// sample access, the TU-edge lookup and the luma / chroma filters of TComLoopFilter.cpp:557-954 in packed 16-bit arithmetic.  Included by those two files only.
#ifndef HEVCDL_DEBLOCK_CORE_H
#define HEVCDL_DEBLOCK_CORE_H
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "hevcdl_dev.h"

namespace {

#define GLB __attribute__((address_space(1)))
enum { REC_SIZE = 15120, REC_TRIDX = 4 * 256 };

__device__ __forceinline__ int clip3i(int lo, int hi, int v) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ int clipbd(int v, int mx) { return v < 0 ? 0 : (v > mx ? mx : v); }      // ClipBD

// four neighbouring samples of a row as one access: a dword of 8-bit samples, two dwords of 16-bit samples (10-bit pictures)
template <typename PEL> __device__ __forceinline__ void load4(const PEL GLB *p, int (&v)[4])
{
  if constexpr (sizeof(PEL) == 1) { const uint32_t w = *(const uint32_t GLB *)p; v[0] = w & 255; v[1] = (w >> 8) & 255; v[2] = (w >> 16) & 255; v[3] = w >> 24; }
  else { const unsigned long long w = *(const unsigned long long GLB *)p; v[0] = (int)(w & 0xffff); v[1] = (int)((w >> 16) & 0xffff); v[2] = (int)((w >> 32) & 0xffff); v[3] = (int)(w >> 48); }
}
template <typename PEL> __device__ __forceinline__ void store4(PEL GLB *p, int a, int b, int c, int d)
{
  if constexpr (sizeof(PEL) == 1) *(uint32_t GLB *)p = (uint32_t)a | ((uint32_t)b << 8) | ((uint32_t)c << 16) | ((uint32_t)d << 24);
  else *(unsigned long long GLB *)p = (unsigned long long)(uint32_t)a | ((unsigned long long)(uint32_t)b << 16) | ((unsigned long long)(uint32_t)c << 32) | ((unsigned long long)(uint32_t)d << 48);
}

// TU edge at the left (dir 0) / top (dir 1) border of the 4x4 partition at luma (x, y) of this frame?
__device__ __forceinline__ bool edge_flag(const hevcdl_dbk_params &p, const unsigned char GLB *recs, int ctus_x, int x, int y, int dir)
{
  if (!p.lf_across_tiles) { // xSetLoopfilterParam TComLoopFilter.cpp:362-400: the neighbouring CU of another tile does not exist for the filter
    const int pos = (dir ? y : x) >> 6, n = dir ? p.tile_rows : p.tile_cols;
    if ((((dir ? y : x)) & 63) == 0) for (int t = 1; t < n; t++) if ((dir ? p.row_bd[t] : p.col_bd[t]) == pos) return false;
  }
  const unsigned char GLB *r = recs + (size_t)((y >> 6) * ctus_x + (x >> 6)) * REC_SIZE;
  const int x4 = (x & 63) >> 2, y4 = (y & 63) >> 2;
  int z = 0;
#pragma unroll
  for (int b = 0; b < 4; b++) z |= (((x4 >> b) & 1) << (2 * b)) | (((y4 >> b) & 1) << (2 * b + 1));
  const int tu = 64 >> (r[z] + r[REC_TRIDX + z]);
  const int pos = dir ? y : x;
  return pos > 0 && (pos & (tu - 1)) == 0;
}

// ---- a QP per edge (the QPMAP instantiations of hevcdl_deblock_fused_kernel) ----
// Table 8-12 (tC, beta; the host's copy: dbk_select.h) in the code object: on the device once, with the module.  Every index is clamped where it is used.
__device__ const unsigned char DBK_TC_DEV[54] = { 0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,1,1,1,1,1,1,1,1,1,2,2,2,2,3,3,3,3,4,4,4,5,5,6,6,7,8,9,10,11,13,14,16,18,20,22,24 };
__device__ const unsigned char DBK_BETA_DEV[52] = { 0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,6,7,8,9,10,11,12,13,14,15,16,17,18,20,22,24,26,28,30,32,34,36,38,40,42,44,46,48,50,52,54,56,58,60,62,64 };
__device__ __forceinline__ int dbk_tc_of(int idx) { return DBK_TC_DEV[clip3i(0, 53, idx)]; }
__device__ __forceinline__ int dbk_beta_of(int idx) { return DBK_BETA_DEV[clip3i(0, 51, idx)]; }
// QpY of the 4x4 partition at luma (x, y) of this frame's map (x, y inside the picture), clamped to what a stream can carry
__device__ __forceinline__ int map_qp(const signed char GLB *map, int ctus_x, int x, int y)
{
  const int x4 = (x & 63) >> 2, y4 = (y & 63) >> 2;
  int z = 0;
#pragma unroll
  for (int b = 0; b < 4; b++) z |= (((x4 >> b) & 1) << (2 * b)) | (((y4 >> b) & 1) << (2 * b + 1));
  return clip3i(-48, 51, map[(size_t)((y >> 6) * ctus_x + (x >> 6)) * 256 + z]);
}
// (QpQ + QpP + 1) >> 1 of the edge at the left (dir 0) / top (dir 1) border of the partition at luma (x, y); x > 0 resp. y > 0 (an edge that edge_flag found)
__device__ __forceinline__ int edge_qpl(const signed char GLB *map, int ctus_x, int x, int y, int dir)
{
  return (map_qp(map, ctus_x, x, y) + map_qp(map, ctus_x, dir ? x : x - 1, dir ? y - 1 : y) + 1) >> 1;
}
// QpC of a chroma edge: Table 8-10 (ChromaArrayType 1) of qPL + cQpPicOffset
__device__ const unsigned char DBK_QPC_DEV[14] = { 29, 30, 31, 32, 33, 33, 34, 34, 35, 35, 36, 36, 37, 37 };      // qPi 30 .. 42
__device__ __forceinline__ int chroma_qp_of(int qpi) { return qpi < 30 ? qpi : (qpi >= 43 ? qpi - 6 : (int)DBK_QPC_DEV[qpi - 30]); }

// Luma decision + filter of one 4-line segment (xEdgeFilterLuma / xPelFilterLuma, TComLoopFilter.cpp:557-700, 830-920), two lines at a time in
// packed 16-bit arithmetic (v_pk_*_i16): every intermediate fits 16 bits at 8 and at 10 bits (largest: 9 * 1023 + 3 * 1023 + 8).  Lines are
// paired (0, 3) and (1, 2): the decisions are taken from lines 0 and 3, so one packed evaluation gives both; the per-line condition of the
// normal filter becomes a half-word mask.  Positions of a line: p3 p2 p1 p0 | q0 q1 q2 q3.
typedef short s2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ s2 pk(int lo, int hi) { return __builtin_bit_cast(s2, ((uint32_t)lo & 0xffffu) | ((uint32_t)hi << 16)); }
__device__ __forceinline__ s2 pk1(int v) { return pk(v, v); }
__device__ __forceinline__ s2 pk_abs(s2 v) { const s2 n = -v; return __builtin_elementwise_max(v, n); }
__device__ __forceinline__ s2 pk_clip(s2 lo, s2 hi, s2 v) { return __builtin_elementwise_min(__builtin_elementwise_max(v, lo), hi); }
__device__ __forceinline__ s2 pk_sel(s2 mask, s2 a, s2 b) { return (a & mask) | (b & ~mask); }
__device__ __forceinline__ void filter_luma_pairs(s2 (&a)[8], s2 (&b)[8], int tc, int beta, int mx)
{ // a: lines (0, 3); b: lines (1, 2); positions p3 p2 p1 p0 | q0 q1 q2 q3
  const s2 two = pk1(2);
  const s2 dpv = pk_abs(a[1] - two * a[2] + a[3]), dqv = pk_abs(a[4] - two * a[5] + a[6]);
  const int dp0 = dpv.x, dp3 = dpv.y, dq0 = dqv.x, dq3 = dqv.y;
  const int d0 = dp0 + dq0, d3 = dp3 + dq3, d = d0 + d3;
  if (d >= beta) return;
  const int side = (beta + (beta >> 1)) >> 3, thr_cut = tc * 10;
  const bool fp = (dp0 + dp3) < side, fq = (dq0 + dq3) < side;
  const s2 flat = pk_abs(a[0] - a[3]) + pk_abs(a[7] - a[4]), gap = pk_abs(a[3] - a[4]);
  const bool sw = flat.x < (beta >> 3) && flat.y < (beta >> 3) && 2 * d0 < (beta >> 2) && 2 * d3 < (beta >> 2) && gap.x < ((tc * 5 + 1) >> 1) && gap.y < ((tc * 5 + 1) >> 1);
  const s2 zero = pk1(0), vmx = pk1(mx), vtc = pk1(tc), vtc2 = pk1(tc >> 1), v2tc = pk1(2 * tc);
  auto run = [&](s2 (&v)[8]) {
    const s2 m0 = v[0], m1 = v[1], m2 = v[2], m3 = v[3], m4 = v[4], m5 = v[5], m6 = v[6], m7 = v[7];
    if (sw) {
      v[3] = pk_clip(m3 - v2tc, m3 + v2tc, (m1 + two * m2 + two * m3 + two * m4 + m5 + pk1(4)) >> 3);
      v[4] = pk_clip(m4 - v2tc, m4 + v2tc, (m2 + two * m3 + two * m4 + two * m5 + m6 + pk1(4)) >> 3);
      v[2] = pk_clip(m2 - v2tc, m2 + v2tc, (m1 + m2 + m3 + m4 + two) >> 2);
      v[5] = pk_clip(m5 - v2tc, m5 + v2tc, (m3 + m4 + m5 + m6 + two) >> 2);
      v[1] = pk_clip(m1 - v2tc, m1 + v2tc, (two * m0 + pk1(3) * m1 + m2 + m3 + m4 + pk1(4)) >> 3);
      v[6] = pk_clip(m6 - v2tc, m6 + v2tc, (m3 + m4 + m5 + pk1(3) * m6 + two * m7 + pk1(4)) >> 3);
    } else {
      const s2 delta0 = (pk1(9) * (m4 - m3) - pk1(3) * (m5 - m2) + pk1(8)) >> 4;
      const s2 on = pk_abs(delta0) < pk1(thr_cut);          // half-word mask: this line is filtered
      const s2 delta = pk_clip(-vtc, vtc, delta0);
      v[3] = pk_sel(on, pk_clip(zero, vmx, m3 + delta), m3);
      v[4] = pk_sel(on, pk_clip(zero, vmx, m4 - delta), m4);
      if (fp) v[2] = pk_sel(on, pk_clip(zero, vmx, m2 + pk_clip(-vtc2, vtc2, ((((m1 + m3 + pk1(1)) >> 1) - m2 + delta) >> 1))), m2);
      if (fq) v[5] = pk_sel(on, pk_clip(zero, vmx, m5 + pk_clip(-vtc2, vtc2, ((((m6 + m4 + pk1(1)) >> 1) - m5 - delta) >> 1))), m5);
    }
  };
  run(a); run(b);
}
__device__ __forceinline__ void filter_luma_pk(int (&m)[4][8], int tc, int beta, int mx)
{
  s2 a[8], b[8];
#pragma unroll
  for (int k = 0; k < 8; k++) { a[k] = pk(m[0][k], m[3][k]); b[k] = pk(m[1][k], m[2][k]); }
  filter_luma_pairs(a, b, tc, beta, mx);
#pragma unroll
  for (int k = 1; k < 7; k++) { m[0][k] = a[k].x; m[3][k] = a[k].y; m[1][k] = b[k].x; m[2][k] = b[k].y; }
}
// 8-bit samples: line pairs straight out of / into the dwords of four samples with v_perm_b32 (selector bytes 0-3: second operand, 4-7: first, 0x0c: zero)
__device__ __forceinline__ s2 perm_s2(uint32_t hi, uint32_t lo, uint32_t sel) { return __builtin_bit_cast(s2, __builtin_amdgcn_perm(hi, lo, sel)); }
__device__ __forceinline__ uint32_t u32(s2 v) { return __builtin_bit_cast(uint32_t, v); }
// rows[i] = the four samples k0 .. k0 + 3 of line i  ->  v[k0 + k] = (line la, line lb) at position k0 + k
__device__ __forceinline__ void rows_to_pairs(uint32_t ra, uint32_t rb, s2 (&v)[8], int k0)
{
#pragma unroll
  for (int k = 0; k < 4; k++) v[k0 + k] = perm_s2(rb, ra, 0x0c000c00u | ((uint32_t)(4 + k) << 16) | (uint32_t)k);
}
__device__ __forceinline__ void pairs_to_rows(const s2 (&v)[8], int k0, uint32_t &ra, uint32_t &rb)
{
  const uint32_t u = __builtin_amdgcn_perm(u32(v[k0 + 1]), u32(v[k0]), 0x06020400u), w = __builtin_amdgcn_perm(u32(v[k0 + 3]), u32(v[k0 + 2]), 0x06020400u);
  ra = __builtin_amdgcn_perm(w, u, 0x05040100u); rb = __builtin_amdgcn_perm(w, u, 0x07060302u);
}
// chroma on two lines at a time: p1 p0 | q0 q1 -> p0, q0
__device__ __forceinline__ void filter_chroma_pairs(s2 p1, s2 &p0, s2 &q0, s2 q1, int tc, int mx)
{
  const s2 delta = pk_clip(pk1(-tc), pk1(tc), (((q0 - p0) << 2) + p1 - q1 + pk1(4)) >> 3);
  p0 = pk_clip(pk1(0), pk1(mx), p0 + delta); q0 = pk_clip(pk1(0), pk1(mx), q0 - delta);
}
// chroma (Bs 2): p1 p0 | q0 q1 -> p0, q0
__device__ __forceinline__ void filter_chroma(int m2, int &m3, int &m4, int m5, int tc, int mx)
{
  const int delta = clip3i(-tc, tc, ((((m4 - m3) << 2) + m2 - m5 + 4) >> 3));
  m3 = clipbd(m3 + delta, mx); m4 = clipbd(m4 - delta, mx);
}


} // namespace
#endif
