// deblock_kernel.hip -- HEVC deblocking filter for gfx950 (MI355X), row f-2 of SURVEY.md section 8 (first half; SAO: sao_kernel.hip).
//
// Replaces, for the configuration of the hot path (all-intra => boundary strength 2 on every TU/CU edge, one slice,
// constant QP, beta/tc offsets 0, no PCM / lossless, 8- or 10-bit 4:2:0; with tiles the filter crosses tile borders):
//   TComLoopFilter::loopFilterPic        HM_dl/source/Lib/TLibCommon/TComLoopFilter.cpp:130-156
//   xDeblockCU / xSetEdgefilterTU / PU   :170-360   (left/top edge of every TU, on the 8x8 grid, not at the picture border)
//   xEdgeFilterLuma / xEdgeFilterChroma  :557-826
//   xPelFilterLuma / xPelFilterChroma / xUseStrongFiltering / xCalcDP / xCalcDQ   :830-954
// Input: the reconstruction hevcdl_compress_frames leaves + the CTU records (depth, trIdx give the TU grid).
//
// This stage is genuinely HBM bound (a few ALU ops per sample).  The reference filters all vertical edges of the picture, then all
// horizontal edges; here both happen in one kernel over LDS tiles placed so that no tile needs a halo (hevcdl_deblock_fused_kernel):
// one read and one write of the picture in all.  A thread owns an exclusive 8x4 (vertical edges) / 4x8 (horizontal edges) block of samples
// centred on one 4-sample edge segment -- the unit of the filter decision -- with dword accesses, adjacent lanes on adjacent dwords.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "hevcdl_dev.h"
#include "deblock_core.h"


// Both passes in one kernel, every sample read once and written once.  A workgroup owns the TW x TH (256 x 32) samples whose top-left corner
// sits 4 samples left of and above a point of the TW x TH grid: [X0 - 4, X0 + TW - 4) x [Y0 - 4, Y0 + TH - 4).  An edge of the 8x8 grid reads 4 samples
// and changes at most 3 on either side, so every vertical edge X0 + 8i and every horizontal edge Y0 + 8j lies with everything it reads and
// writes inside that rectangle -- and the horizontal edges read nothing but vertically filtered samples of the same rectangle: no halo, no
// second trip through HBM.  Stage 1: thread = (edge column, 4-row segment), 8 x 4 samples from HBM (two dword loads per row, adjacent
// lanes adjacent), vertical edge filtered in registers, block to LDS.  Stage 2: thread = (4-sample column group, edge row), 4 x 8 samples from
// LDS, horizontal edge filtered, block to HBM (a dword store per row, adjacent lanes adjacent).  CHROMA == 1: the same on both chroma planes
// in chroma coordinates (edge grid 8 chroma = 16 luma samples; a 4-sample chroma segment spans two luma partitions = two edge flags; the
// filter reads 2 and changes 1 sample per side).  in == out is allowed (a workgroup reads and writes its own rectangle only).
#ifndef DBK_TW
#define DBK_TW 256
#define DBK_TH 32
#endif
#ifndef DBK_WAVES
#define DBK_WAVES 8
#endif
// QPMAP == 1 (p.qp_map non-null): tc and beta are looked up per edge segment from the QpY of the two partitions it separates, the chroma tc per plane (hevcdl_dev.h).  The
// flags' QPs are fetched where the flags are; everything else is the code of QPMAP == 0, which compiles to what it was.
template <int CHROMA, typename PEL, int QPMAP = 0>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(DBK_WAVES, DBK_WAVES))) void hevcdl_deblock_fused_kernel(hevcdl_dbk_params p)
{
  constexpr int TW = DBK_TW, TH = DBK_TH, DW = TW * (int)sizeof(PEL) / 4, QD = (int)sizeof(PEL);      // dwords per tile row; dwords per 4 samples
  constexpr int EXN = TW / 8, XGN = TW / 4;                 // edge columns / 4-sample column groups per tile
  static_assert(EXN * (TH / 4) == 256 && XGN * (TH / 8) == 256, "one thread per block in both stages");
  __shared__ uint32_t tile[TH][DW + 1];
  const int frame = blockIdx.z, tid = threadIdx.x;
  const int W = p.width >> CHROMA, H = p.height >> CHROMA;
  // Neighbouring tiles of a row share the cache lines at their common border (the rectangles start 4 samples left of the grid).  Workgroups
  // are dealt to the 8 XCDs round-robin in launch order, each XCD with its own L2: the launch index is therefore remapped so that every XCD
  // gets a contiguous run of tiles -- the two halves of a shared line meet in one L2 and leave it as a whole line.
  const int tiles_x = (W + 4 + TW - 1) / TW, n_tiles = tiles_x * ((H + 4 + TH - 1) / TH), per_xcd = (n_tiles + 7) / 8;
  const int lin = (int)blockIdx.x, vt = (lin & 7) * per_xcd + (lin >> 3);
  if (vt >= n_tiles) return;
  const int X0 = (vt % tiles_x) * TW, Y0 = (vt / tiles_x) * TH;
  const size_t ysz = (size_t)p.width * p.height, fsz = ysz + (ysz >> 1);
  const unsigned char GLB *recs = (const unsigned char GLB *)p.records + (size_t)frame * p.ctus_per_frame * REC_SIZE;
  // the picture's own parameters, read once per workgroup (a scalar load: the address is uniform).  A disabled picture runs with (0, 0, 0): beta 0 stops every luma edge
  // at its first test and a chroma delta clipped to 0 changes nothing, so the picture passes through as it is
  int tc = p.tc, beta = p.beta, tc_c = p.tc_c;
  [[maybe_unused]] int tc_off = 0, beta_off = 0; [[maybe_unused]] bool pic_off = false;
  [[maybe_unused]] const signed char GLB *qmap = nullptr;
  [[maybe_unused]] const int bd_scale = (p.pel_max + 1) >> 8;
  [[maybe_unused]] int qv0 = 0, qv1 = 0, qh0 = 0, qh1 = 0;      // qPL of the edges behind v0, v1, h0, h1
  if constexpr (QPMAP) {
    const int GLB *fp = (const int GLB *)p.frame_params + 4 * frame;
    tc_off = fp[0]; beta_off = fp[1]; pic_off = fp[3] != 0;
    qmap = (const signed char GLB *)p.qp_map + (size_t)frame * p.ctus_per_frame * 256;
  } else
  if (p.frame_params) { const int GLB *fp = (const int GLB *)p.frame_params + 4 * frame; const bool off = fp[3] != 0; tc = off ? 0 : fp[0]; beta = off ? 0 : fp[1]; tc_c = off ? 0 : fp[2]; }
  // stage 1 role: edge column x, rows y .. y + 3
  const int ex = tid % EXN, sy = tid / EXN;
  const int x = X0 + 8 * ex, y = Y0 - 4 + 4 * sy;
  const bool rows_ok = y >= 0 && y < H, has_l = x > 0 && x <= W, has_r = x < W;
  // stage 2 role: columns xh .. xh + 3, edge row yh, rows yh - 4 .. yh + 3
  const int xg = tid % XGN, eb = tid / XGN;
  const int xh = X0 - 4 + 4 * xg, yh = Y0 + 8 * eb;
  const bool cols_ok = xh >= 0 && xh < W, has_u = yh > 0 && yh <= H, has_d = yh < H;
  bool v0 = false, v1 = false, h0 = false, h1 = false;
#pragma unroll 1
  for (int c = 0; c < (CHROMA ? 2 : 1); c++) {
    const size_t plane = (size_t)frame * fsz + (CHROMA ? ysz + (size_t)c * (ysz >> 2) : 0);
    const PEL GLB *src = (const PEL GLB *)p.in + plane; PEL GLB *dst = (PEL GLB *)p.out + plane;
    if (c) __syncthreads();                                 // stage 2 of the first chroma plane has read the tile
    constexpr bool RAW = sizeof(PEL) == 1;                    // 8-bit samples: blocks stay dwords; only blocks with an edge are opened up, into packed line pairs
    if constexpr (RAW) {
      if (rows_ok && (has_l || has_r)) {
        uint32_t l[4] = { 0, 0, 0, 0 }, r[4] = { 0, 0, 0, 0 };
#pragma unroll
        for (int i = 0; i < 4; i++) {
          const size_t o = (size_t)(y + i) * W + x;
          if (has_l) l[i] = *(const uint32_t GLB *)(src + o - 4);
          if (has_r) r[i] = *(const uint32_t GLB *)(src + o);
        }
        if constexpr (!CHROMA) {
          if (has_l && has_r) v0 = edge_flag(p, recs, p.ctus_x, x, y, 0);
          if constexpr (QPMAP) { v0 = v0 && !pic_off; if (v0) { const int q = edge_qpl(qmap, p.ctus_x, x, y, 0); tc = dbk_tc_of(q + 2 + tc_off) * bd_scale; beta = dbk_beta_of(q + beta_off) * bd_scale; } }
          if (v0) {
            s2 a[8], b[8];
            rows_to_pairs(l[0], l[3], a, 0); rows_to_pairs(r[0], r[3], a, 4); rows_to_pairs(l[1], l[2], b, 0); rows_to_pairs(r[1], r[2], b, 4);
            filter_luma_pairs(a, b, tc, beta, p.pel_max);
            pairs_to_rows(a, 0, l[0], l[3]); pairs_to_rows(a, 4, r[0], r[3]); pairs_to_rows(b, 0, l[1], l[2]); pairs_to_rows(b, 4, r[1], r[2]);
          }
        } else {
          if (c == 0 && has_l && has_r) { v0 = edge_flag(p, recs, p.ctus_x, 2 * x, 2 * y, 0); v1 = edge_flag(p, recs, p.ctus_x, 2 * x, 2 * y + 4, 0); }
          if constexpr (QPMAP) if (c == 0) { v0 = v0 && !pic_off; v1 = v1 && !pic_off; if (v0) qv0 = edge_qpl(qmap, p.ctus_x, 2 * x, 2 * y, 0); if (v1) qv1 = edge_qpl(qmap, p.ctus_x, 2 * x, 2 * y + 4, 0); }
#pragma unroll
          for (int h = 0; h < 2; h++) if (h ? v1 : v0) { // rows (0, 1) under the first flag, (2, 3) under the second: p1 p0 = bytes 2, 3 of the left dwords, q0 q1 = bytes 0, 1 of the right ones
            uint32_t &la = l[2 * h], &lb = l[2 * h + 1], &ra = r[2 * h], &rb = r[2 * h + 1];
            const s2 p1 = perm_s2(lb, la, 0x0c060c02u), q1 = perm_s2(rb, ra, 0x0c050c01u);
            s2 p0 = perm_s2(lb, la, 0x0c070c03u), q0 = perm_s2(rb, ra, 0x0c040c00u);
            if constexpr (QPMAP) tc_c = dbk_tc_of(chroma_qp_of((h ? qv1 : qv0) + (c ? p.cr_qp_offset : p.cb_qp_offset)) + 2 + tc_off) * bd_scale;
            filter_chroma_pairs(p1, p0, q0, q1, tc_c, p.pel_max);
            la = __builtin_amdgcn_perm(u32(p0), la, 0x04020100u); lb = __builtin_amdgcn_perm(u32(p0), lb, 0x06020100u);
            ra = __builtin_amdgcn_perm(u32(q0), ra, 0x03020104u); rb = __builtin_amdgcn_perm(u32(q0), rb, 0x03020106u);
          }
        }
#pragma unroll
        for (int i = 0; i < 4; i++) { uint32_t *row = &tile[4 * sy + i][2 * ex]; row[0] = l[i]; row[1] = r[i]; }
      }
    } else
    if (rows_ok && (has_l || has_r)) {
      int m[4][8];                                            // row i: p3 p2 p1 p0 | q0 q1 q2 q3
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const size_t o = (size_t)(y + i) * W + x;
        int l[4] = { 0, 0, 0, 0 }, r[4] = { 0, 0, 0, 0 };
        if (has_l) load4<PEL>(src + o - 4, l);
        if (has_r) load4<PEL>(src + o, r);
#pragma unroll
        for (int k = 0; k < 4; k++) { m[i][k] = l[k]; m[i][4 + k] = r[k]; }
      }
      if (c == 0) { // the TU grid is looked up behind the sample loads: both are in flight together
        if (has_l && has_r) {
          if (CHROMA) { v0 = edge_flag(p, recs, p.ctus_x, 2 * x, 2 * y, 0); v1 = edge_flag(p, recs, p.ctus_x, 2 * x, 2 * y + 4, 0); }
          else v0 = edge_flag(p, recs, p.ctus_x, x, y, 0);
        }
        if constexpr (QPMAP) {
          v0 = v0 && !pic_off; v1 = v1 && !pic_off;
          if (v0) qv0 = CHROMA ? edge_qpl(qmap, p.ctus_x, 2 * x, 2 * y, 0) : edge_qpl(qmap, p.ctus_x, x, y, 0);
          if (v1) qv1 = edge_qpl(qmap, p.ctus_x, 2 * x, 2 * y + 4, 0);
        }
      }
      if (!CHROMA) {
        if constexpr (QPMAP) { tc = dbk_tc_of(qv0 + 2 + tc_off) * bd_scale; beta = dbk_beta_of(qv0 + beta_off) * bd_scale; }
        if (v0) filter_luma_pk(m, tc, beta, p.pel_max);
      } else {
#pragma unroll
        for (int i = 0; i < 4; i++) if (i < 2 ? v0 : v1) {
          if constexpr (QPMAP) tc_c = dbk_tc_of(chroma_qp_of((i < 2 ? qv0 : qv1) + (c ? p.cr_qp_offset : p.cb_qp_offset)) + 2 + tc_off) * bd_scale;
          filter_chroma(m[i][2], m[i][3], m[i][4], m[i][5], tc_c, p.pel_max);
        }
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
    if (c == 0 && cols_ok && has_u && has_d) { // (issued before the barrier: back by the time stage 2 needs it)
      if (CHROMA) { h0 = edge_flag(p, recs, p.ctus_x, 2 * xh, 2 * yh, 1); h1 = edge_flag(p, recs, p.ctus_x, 2 * xh + 4, 2 * yh, 1); }
      else h0 = edge_flag(p, recs, p.ctus_x, xh, yh, 1);
      if constexpr (QPMAP) {
        h0 = h0 && !pic_off; h1 = h1 && !pic_off;
        if (h0) qh0 = CHROMA ? edge_qpl(qmap, p.ctus_x, 2 * xh, 2 * yh, 1) : edge_qpl(qmap, p.ctus_x, xh, yh, 1);
        if (h1) qh1 = edge_qpl(qmap, p.ctus_x, 2 * xh + 4, 2 * yh, 1);
      }
    }
    __syncthreads();
    if constexpr (RAW) {
      if (cols_ok && (has_u || has_d)) {
        uint32_t w[8];                                        // row k of the band: the four lines (columns) at position k
#pragma unroll
        for (int k = 0; k < 8; k++) w[k] = tile[8 * eb + k][xg];
        if constexpr (!CHROMA) {
          if (h0) {
            if constexpr (QPMAP) { tc = dbk_tc_of(qh0 + 2 + tc_off) * bd_scale; beta = dbk_beta_of(qh0 + beta_off) * bd_scale; }
            s2 a[8], b[8];
#pragma unroll
            for (int k = 0; k < 8; k++) { a[k] = perm_s2(w[k], w[k], 0x0c030c00u); b[k] = perm_s2(w[k], w[k], 0x0c020c01u); }
            filter_luma_pairs(a, b, tc, beta, p.pel_max);
#pragma unroll
            for (int k = 1; k < 7; k++) w[k] = __builtin_amdgcn_perm(u32(b[k]), u32(a[k]), 0x02060400u);
          }
        } else if (h0 || h1) { // columns (0, 1) under the first flag, (2, 3) under the second; p1 p0 | q0 q1 = rows 2 .. 5 of the band
          s2 a[4], b[4];
#pragma unroll
          for (int k = 0; k < 4; k++) { a[k] = perm_s2(w[2 + k], w[2 + k], 0x0c010c00u); b[k] = perm_s2(w[2 + k], w[2 + k], 0x0c030c02u); }
          [[maybe_unused]] const int coff = c ? p.cr_qp_offset : p.cb_qp_offset;
          if constexpr (QPMAP) tc_c = dbk_tc_of(chroma_qp_of(qh0 + coff) + 2 + tc_off) * bd_scale;
          if (h0) filter_chroma_pairs(a[0], a[1], a[2], a[3], tc_c, p.pel_max);
          if constexpr (QPMAP) tc_c = dbk_tc_of(chroma_qp_of(qh1 + coff) + 2 + tc_off) * bd_scale;
          if (h1) filter_chroma_pairs(b[0], b[1], b[2], b[3], tc_c, p.pel_max);
          w[3] = __builtin_amdgcn_perm(u32(b[1]), u32(a[1]), 0x06040200u); w[4] = __builtin_amdgcn_perm(u32(b[2]), u32(a[2]), 0x06040200u);
        }
#pragma unroll
        for (int k = 0; k < 8; k++) if (k < 4 ? has_u : has_d) *(uint32_t GLB *)(dst + (size_t)(yh - 4 + k) * W + xh) = w[k];
      }
    } else
    if (cols_ok && (has_u || has_d)) {
      int m[4][8];                                            // column i: p3 p2 p1 p0 | q0 q1 q2 q3 downwards
#pragma unroll
      for (int k = 0; k < 8; k++) {
        const uint32_t *row = &tile[8 * eb + k][QD * xg];
        if constexpr (sizeof(PEL) == 1) { const uint32_t w = row[0]; m[0][k] = w & 255; m[1][k] = (w >> 8) & 255; m[2][k] = (w >> 16) & 255; m[3][k] = w >> 24; }
        else { const uint32_t w0 = row[0], w1 = row[1]; m[0][k] = w0 & 0xffff; m[1][k] = w0 >> 16; m[2][k] = w1 & 0xffff; m[3][k] = w1 >> 16; }
      }
      if (!CHROMA) {
        if constexpr (QPMAP) { tc = dbk_tc_of(qh0 + 2 + tc_off) * bd_scale; beta = dbk_beta_of(qh0 + beta_off) * bd_scale; }
        if (h0) filter_luma_pk(m, tc, beta, p.pel_max);
      } else {
#pragma unroll
        for (int i = 0; i < 4; i++) if (i < 2 ? h0 : h1) {
          if constexpr (QPMAP) tc_c = dbk_tc_of(chroma_qp_of((i < 2 ? qh0 : qh1) + (c ? p.cr_qp_offset : p.cb_qp_offset)) + 2 + tc_off) * bd_scale;
          filter_chroma(m[i][2], m[i][3], m[i][4], m[i][5], tc_c, p.pel_max);
        }
      }
#pragma unroll
      for (int k = 0; k < 8; k++) if (k < 4 ? has_u : has_d) store4<PEL>(dst + (size_t)(yh - 4 + k) * W + xh, m[0][k], m[1][k], m[2][k], m[3][k]);
    }
  }
}

static unsigned long long g_dbk_qp_launches = 0;      // launches of the QPMAP instantiations (a luma and a chroma kernel count as one)
extern "C" unsigned long long hevcdl_deblock_qp_launches(void) { return g_dbk_qp_launches; }

extern "C" void hevcdl_launch_deblock(const hevcdl_dbk_params *pp, void *stream)
{
  const hevcdl_dbk_params p = *pp;
  hipStream_t s = (hipStream_t)stream;
  const int W = p.width, H = p.height, cw = W >> 1, chh = H >> 1;
  auto grid = [&](int w, int h) { const int n = ((w + 4 + DBK_TW - 1) / DBK_TW) * ((h + 4 + DBK_TH - 1) / DBK_TH); return dim3((unsigned)(((n + 7) / 8) * 8), 1, p.n_frames); };
  const dim3 g0 = grid(W, H), g1 = grid(cw, chh);
  if (p.qp_map) { // a QP per edge: needs the per-picture rows (offsets, disabled)
    if (!p.frame_params) return;
    g_dbk_qp_launches++;
    if (p.pel_max == 255) {
      hipLaunchKernelGGL((hevcdl_deblock_fused_kernel<0, uint8_t, 1>), g0, dim3(256), 0, s, p);
      hipLaunchKernelGGL((hevcdl_deblock_fused_kernel<1, uint8_t, 1>), g1, dim3(256), 0, s, p);
    } else {
      hipLaunchKernelGGL((hevcdl_deblock_fused_kernel<0, uint16_t, 1>), g0, dim3(256), 0, s, p);
      hipLaunchKernelGGL((hevcdl_deblock_fused_kernel<1, uint16_t, 1>), g1, dim3(256), 0, s, p);
    }
    return;
  }
  if (p.pel_max == 255) {
    hipLaunchKernelGGL((hevcdl_deblock_fused_kernel<0, uint8_t>), g0, dim3(256), 0, s, p);
    hipLaunchKernelGGL((hevcdl_deblock_fused_kernel<1, uint8_t>), g1, dim3(256), 0, s, p);
  } else { // 16-bit sample planes (10-bit pictures)
    hipLaunchKernelGGL((hevcdl_deblock_fused_kernel<0, uint16_t>), g0, dim3(256), 0, s, p);
    hipLaunchKernelGGL((hevcdl_deblock_fused_kernel<1, uint16_t>), g1, dim3(256), 0, s, p);
  }
}
