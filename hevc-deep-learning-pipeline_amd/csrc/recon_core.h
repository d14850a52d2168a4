// recon_core.h -- the unfiltered reconstruction of an intra picture from CTU records, as ONE source for the device (recon_kernel.hip: a wave per CTU row, lanes over
// samples) and for the host (the same functions with one "lane": hevcdl_reconstruct_frames_host, the CPU net of the kernel's arithmetic and index logic).
// Restated from ITU-T H.265: 6.4.1 (availability, for the neighbours a reference line touches), 8.4.4.2.2 (reference samples and their substitution), 8.4.4.2.3 ([1 2 1] and
// strong smoothing), 8.4.4.2.4-6 (planar, DC, angular with the DC and edge filters), 8.6.2 / 8.6.3 (chroma QP, dequantisation: flat, or with the scaling factors of 7.4.5), 8.6.4 (transform skip, DST, DCT),
// 8.6.7 (clipping).  Integer arithmetic throughout: nothing carries a tolerance.  rd_kernel.hip is not included and not touched.
//
// Construction rules, as for the entropy coder: no recursion (the two quadtrees are walked in z-order over the 256 partitions of a CTU), no allocation, every loop
// bounded by a constant or by a block size that was clamped to 4 .. 32, every index into a record masked (z & 255) and every sample position checked against the
// picture before it is read or written; records that passed hevcdl_validate_records never reach a clamp.
#ifndef HEVCDL_RECON_CORE_H
#define HEVCDL_RECON_CORE_H
#include <stdint.h>
#include "hevcdl.h"

#ifdef __HIPCC__
#define RC_FN __host__ __device__ inline
#else
#define RC_FN inline
#endif
#if defined(__HIP_DEVICE_COMPILE__)
#define RC_SYNC() __syncthreads()      // the workgroup IS one wave: the barrier orders the lanes' LDS and global accesses of two phases
#define RC_GLB
#else
#define RC_SYNC() ((void)0)
#define RC_GLB
#endif

namespace hevcdl_rc {

struct RcPic {
  int W, H, ctus_x, ctus_y, bit_depth, qp, strong;      // strong: strong_intra_smoothing_enabled_flag
  const uint32_t *unit;          // [ctus] tile and slice of every CTU as one number: a neighbour in another unit is not available (6.4.1)
  const hevcdl_ctu_record *recs; // [ctus]
  void *out;                     // planar 4:2:0, uint8 or (bit_depth > 8) uint16 samples
};
// The same picture with a QP per CU (hevcdl_parse_stream_qp): the second instantiation of rc_ctu / rc_block.  8.6.1: a transform unit is dequantised with its CU's QpY;
// chroma with qPi = Clip3(-QpBdOffset, 57, QpY + pps_cb_qp_offset) (Cr: pps_cr_qp_offset) through Table 8-10.  RcPic and everything instantiated with it stay as they are.
struct RcPicQp : RcPic {
  const int8_t *qp_map;          // [ctus][256] QpY of every 4x4 partition in z-order
  int cb_off, cr_off;            // pps_cb_qp_offset, pps_cr_qp_offset
};
// The same picture with scaling lists on top of the QP map (hevcdl_parse_stream_sl): the third instantiation.  factor: the 2032 bytes of hevcdl_scaling_info -- ScalingFactor
// of 7.4.5 in raster order, Y 4 8 16 32, Cb 4 8 16, Cr 4 8 16.  It always has the map: a stream of one QP has a constant one.
struct RcPicSl : RcPicQp {
  const uint8_t *factor;
};
// the working set of one wave (LDS on the device)
struct RcWork {
  int16_t ref[132], fref[132];   // 4 n + 1 reference samples from the lowest left one up to the corner and along the top; filtered
  int16_t ext[100];              // the angular modes' extended reference, index -32 .. 65 at +33
  int16_t pred[1024];
  int32_t tmp[1024];
  int16_t res[1024];
  int32_t dc;
};

RC_FN int rc_z_of(int x4, int y4)
{
  int z = 0;
  for (int b = 0; b < 4; b++) z |= (((x4 >> b) & 1) << (2 * b)) | (((y4 >> b) & 1) << (2 * b + 1));
  return z;
}
RC_FN int rc_clip(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

template <typename PEL> RC_FN PEL *rc_plane(const RcPic &p, int comp, int &stride)
{
  stride = comp ? p.W >> 1 : p.W;
  const size_t ysz = (size_t)p.W * p.H;
  return (PEL *)p.out + (comp == 0 ? 0 : (comp == 1 ? ysz : ysz + (ysz >> 2)));
}

// 6.4.1 for the 4x4 luma block at (xn, yn) seen from the block at (xc, yc), both in luma samples
RC_FN bool rc_available(const RcPic &p, int xc, int yc, int xn, int yn)
{
  if (xn < 0 || yn < 0 || xn >= p.W || yn >= p.H) return false;
  const int cxn = xn >> 6, cyn = yn >> 6, cxc = xc >> 6, cyc = yc >> 6;
  if (cxn == cxc && cyn == cyc) return rc_z_of((xn >> 2) & 15, (yn >> 2) & 15) < rc_z_of((xc >> 2) & 15, (yc >> 2) & 15);
  if (cyn > cyc || (cyn == cyc && cxn > cxc)) return false;                                    // a CTU that follows in decoding order
  const int an = cyn * p.ctus_x + cxn, ac = cyc * p.ctus_x + cxc;
  if (an < 0 || an >= p.ctus_x * p.ctus_y || ac < 0 || ac >= p.ctus_x * p.ctus_y) return false;
  return p.unit[an] == p.unit[ac];
}

// the intraPredAngle of modes 2 .. 34 and the inverse angles of modes 11 .. 25 (Tables 8-4, 8-5)
RC_FN int rc_angle(int mode)
{
  const int8_t a[33] = { 32, 26, 21, 17, 13, 9, 5, 2, 0, -2, -5, -9, -13, -17, -21, -26, -32, -26, -21, -17, -13, -9, -5, -2, 0, 2, 5, 9, 13, 17, 21, 26, 32 };
  return a[rc_clip(mode, 2, 34) - 2];
}
RC_FN int rc_inv_angle(int mode)
{
  const int16_t a[15] = { -4096, -1638, -910, -630, -482, -390, -315, -256, -315, -390, -482, -630, -910, -1638, -4096 };
  return a[rc_clip(mode, 11, 25) - 11];
}
// the transform matrix of 8.6.4.2: coefficient (k, n) of the 32-point DCT from the 32 distinct magnitudes; an N-point transform uses the rows k * 32 / N
RC_FN int rc_dct(int k, int n)
{
  const int8_t t[33] = { 64, 90, 90, 90, 89, 88, 87, 85, 83, 82, 80, 78, 75, 73, 70, 67, 64, 61, 57, 54, 50, 46, 43, 38, 36, 31, 25, 22, 18, 13, 9, 4, 0 };
  int m = (k * (2 * n + 1)) & 127;
  if (m > 64) m = 128 - m;
  return m > 32 ? -t[64 - m] : t[m];
}
RC_FN int rc_dst(int k, int n)
{
  const int8_t t[16] = { 29, 55, 74, 84, 74, 74, 0, -74, 84, -29, -74, 55, 55, -84, 74, -29 };
  return t[((k & 3) << 2) | (n & 3)];
}
RC_FN int rc_chroma_qp(int qp)
{ // Table 8-10, ChromaArrayType 1, pps / slice offsets 0
  const int8_t t[14] = { 29, 30, 31, 32, 33, 33, 34, 34, 35, 35, 36, 36, 37, 37 };
  return qp < 30 ? qp : (qp >= 43 ? qp - 6 : t[qp - 30]);
}

// QpY of the CU that partition z of CTU a lies in; the QP a block of component comp is dequantised with (QpBdOffset added)
RC_FN int rc_cu_qpy(const RcPic &, int, int) { return 0; }
RC_FN int rc_cu_qpy(const RcPicQp &p, int a, int z) { return rc_clip(p.qp_map[(size_t)a * 256 + (z & 255)], -6 * (p.bit_depth - 8), 51); }      // clamped before it indexes levelScale
RC_FN int rc_block_qp(const RcPic &p, int comp, int)
{
  const int bd = p.bit_depth;
  return comp ? rc_chroma_qp(p.qp) + 6 * (bd - 8) : p.qp + 6 * (bd - 8);
}
RC_FN int rc_block_qp(const RcPicQp &p, int comp, int qpy)
{
  const int off = 6 * (p.bit_depth - 8);
  if (!comp) return qpy + off;
  return rc_chroma_qp(rc_clip(qpy + (comp == 1 ? p.cb_off : p.cr_off), -off, 57)) + off;
}

// m[x][y] of 8.6.4.2 for the coefficients of a block: the flat 16 folded into `flat` = 16 * levelScale << (qP / 6) as it ever was, or the block's plane of factors
RC_FN const uint8_t *rc_factors(const RcPic &, int, int) { return nullptr; }
RC_FN const uint8_t *rc_factors(const RcPicSl &p, int comp, int log2n)
{
  const int at[4] = { 0, 16, 80, 336 };
  return p.factor + (comp ? 1360 + (comp - 1) * 336 : 0) + at[comp && log2n > 4 ? 2 : log2n - 2];      // (a chroma block of 32 does not exist in 4:2:0)
}
RC_FN int64_t rc_coef_scale(const RcPic &, const uint8_t *, int, int64_t flat) { return flat; }
RC_FN int64_t rc_coef_scale(const RcPicSl &, const uint8_t *m, int i, int64_t flat) { return (flat >> 4) * (int64_t)m[i]; }

// One transform block: prediction from the reconstructed neighbours in the picture, residual from the levels, sum, clip, store.  (x, y): the block's position in samples
// of its component; lx, ly: the same in luma samples; n = 1 << log2n.
template <typename PEL, typename PIC>
RC_FN void rc_block(const PIC &p, RcWork &w, int lane, int nl, int comp, int lx, int ly, int log2n, int mode, int cbf, int tskip, const int16_t *lvl, int qpy)
{
  log2n = rc_clip(log2n, 2, 5); mode = rc_clip(mode, 0, 34);
  const int n = 1 << log2n, nn = n * n, sh = comp ? 1 : 0, x = lx >> sh, y = ly >> sh, bd = p.bit_depth, pmax = (1 << bd) - 1;
  int stride; PEL *pl = rc_plane<PEL>(p, comp, stride);
  const int pw = p.W >> sh, ph = p.H >> sh;
  if (x < 0 || y < 0 || x + n > pw || y + n > ph) return;                                       // (a block of a valid record lies inside the picture)
  // ---- 8.4.4.2.2: the 4 n + 1 neighbours; entry i: i < 2 n the left column from the bottom up, 2 n the corner, above it the top row.  A unit of availability is a 4x4
  // luma block: 4 samples of a luma line, 2 of a chroma line (the sample's own position says which)
  const int len = 4 * n + 1;
  for (int i = lane; i < len; i += nl) {
    int sx, sy;
    if (i < 2 * n) { sx = x - 1; sy = y + 2 * n - 1 - i; } else if (i == 2 * n) { sx = x - 1; sy = y - 1; } else { sx = x + i - 2 * n - 1; sy = y - 1; }
    int v = -1;
    if (sx >= 0 && sy >= 0 && sx < pw && sy < ph && rc_available(p, lx, ly, (sx << sh) & ~3, (sy << sh) & ~3)) v = (int)pl[(size_t)sy * stride + sx];
    w.ref[i] = (int16_t)v;
  }
  RC_SYNC();
  if (lane == 0) { // the substitution is a chain from the first entry on
    int first = -1;
    for (int i = 0; i < len; i++) if (w.ref[i] >= 0) { first = i; break; }
    if (first < 0) { for (int i = 0; i < len; i++) w.ref[i] = (int16_t)(1 << (bd - 1)); }
    else {
      for (int i = 0; i < first; i++) w.ref[i] = w.ref[first];
      for (int i = first + 1; i < len; i++) if (w.ref[i] < 0) w.ref[i] = w.ref[i - 1];
    }
  }
  RC_SYNC();
  // ---- 8.4.4.2.3: filtering of the neighbours (luma only in 4:2:0)
  const int16_t *r = w.ref;
  {
    int filter = 0;
    if (!comp && mode != 1 && n > 4) {
      const int dv = mode > 26 ? mode - 26 : 26 - mode, dh = mode > 10 ? mode - 10 : 10 - mode, d = dv < dh ? dv : dh;
      filter = d > (n == 8 ? 7 : (n == 16 ? 1 : 0));
    }
    if (filter) {
      const int c = w.ref[2 * n], a = w.ref[0], b = w.ref[4 * n], thr = 1 << (bd - 5);
      const int da = a + c - 2 * w.ref[n], db = c + b - 2 * w.ref[3 * n];
      const bool strong = p.strong && n == 32 && (da < 0 ? -da : da) < thr && (db < 0 ? -db : db) < thr;
      for (int i = lane; i < len; i += nl) {
        int v;
        if (i == 0 || i == len - 1) v = w.ref[i];
        else if (strong) v = i == 2 * n ? c : (i < 2 * n ? ((64 - (2 * n - i)) * c + (2 * n - i) * a + 32) >> 6 : ((64 - (i - 2 * n)) * c + (i - 2 * n) * b + 32) >> 6);
        else v = (w.ref[i - 1] + 2 * w.ref[i] + w.ref[i + 1] + 2) >> 2;
        w.fref[i] = (int16_t)v;
      }
      RC_SYNC();
      r = w.fref;
    }
  }
  // left(j) = p[-1][j], top(i) = p[i][-1], j, i from -1
#define RC_LEFT(j) ((int)r[2 * n - 1 - (j)])
#define RC_TOP(i) ((int)r[2 * n + 1 + (i)])
  const bool edge = !comp && n < 32;
  if (mode == 0) {
    for (int i = lane; i < nn; i += nl) {
      const int py = i >> log2n, px = i & (n - 1);
      w.pred[i] = (int16_t)(((n - 1 - px) * RC_LEFT(py) + (px + 1) * RC_TOP(n) + (n - 1 - py) * RC_TOP(px) + (py + 1) * RC_LEFT(n) + n) >> (log2n + 1));
    }
  } else if (mode == 1) {
    if (lane == 0) { int s = n; for (int i = 0; i < n; i++) s += RC_LEFT(i) + RC_TOP(i); w.dc = s >> (log2n + 1); }
    RC_SYNC();
    const int dc = w.dc;
    for (int i = lane; i < nn; i += nl) {
      const int py = i >> log2n, px = i & (n - 1);
      int v = dc;
      if (edge) {
        if (px == 0 && py == 0) v = (RC_LEFT(0) + 2 * dc + RC_TOP(0) + 2) >> 2;
        else if (py == 0) v = (RC_TOP(px) + 3 * dc + 2) >> 2;
        else if (px == 0) v = (RC_LEFT(py) + 3 * dc + 2) >> 2;
      }
      w.pred[i] = (int16_t)v;
    }
  } else {
    const int ang = rc_angle(mode), vert = mode >= 18;
    // ref[k], k = -n .. 2 n, at ext[k + 33]: the main side from the corner on, a negative angle's projection of the other side below it
    const int last = (n * ang) >> 5;
    for (int k = lane - 33; k <= 2 * n; k += nl) {
      if (k < -n) continue;
      int v;
      if (k >= 0) v = vert ? RC_TOP(k - 1) : RC_LEFT(k - 1);
      else if (ang < 0 && k >= last) { const int o = -1 + ((k * rc_inv_angle(mode) + 128) >> 8); v = vert ? RC_LEFT(rc_clip(o, -1, 2 * n - 1)) : RC_TOP(rc_clip(o, -1, 2 * n - 1)); }
      else v = 0;
      w.ext[k + 33] = (int16_t)v;
    }
    RC_SYNC();
    for (int i = lane; i < nn; i += nl) {
      const int py = i >> log2n, px = i & (n - 1), a = vert ? px : py, b = vert ? py : px;      // a: along the main side, b: away from it
      const int idx = ((b + 1) * ang) >> 5, f = ((b + 1) * ang) & 31;
      int v = f ? ((32 - f) * w.ext[a + idx + 1 + 33] + f * w.ext[a + idx + 2 + 33] + 16) >> 5 : w.ext[a + idx + 1 + 33];
      if (ang == 0 && edge && a == 0) v = rc_clip(v + (((vert ? RC_LEFT(b) : RC_TOP(b)) - RC_LEFT(-1)) >> 1), 0, pmax);
      w.pred[i] = (int16_t)v;
    }
  }
#undef RC_LEFT
#undef RC_TOP
  RC_SYNC();
  // ---- 8.6: the residual
  if (cbf) {
    const int qp = rc_block_qp(p, comp, qpy);
    const int ls[6] = { 40, 45, 51, 57, 64, 72 };
    const int64_t scale = (int64_t)(16 * ls[qp % 6]) << (qp / 6);
    const int bds = bd + log2n - 5, sh2 = 20 - bd;
    const uint8_t *m = rc_factors(p, comp, log2n);                                               // (consecutive lanes read consecutive bytes of a 2 KB table)
    for (int i = lane; i < nn; i += nl) {
      const int64_t d = ((int64_t)lvl[i] * rc_coef_scale(p, m, i, scale) + ((int64_t)1 << (bds - 1))) >> bds;
      w.tmp[i] = (int32_t)(d < -32768 ? -32768 : (d > 32767 ? 32767 : d));
    }
    RC_SYNC();
    if (tskip && n == 4) {
      for (int i = lane; i < nn; i += nl) w.res[i] = (int16_t)((w.tmp[i] * 128 + (1 << (sh2 - 1))) >> sh2);      // (x 128, not << 7: a negative value is not shifted left)
    } else {
      const int dst = !comp && n == 4, step = 32 >> log2n;
      // first stage down the columns: e[y][x] = sum_k M[k][y] d[k][x], clipped to 16 bits behind a shift of 7; kept in res
      for (int i = lane; i < nn; i += nl) {
        const int py = i >> log2n, px = i & (n - 1);
        int64_t s = 0;
        for (int k = 0; k < n; k++) s += (int64_t)(dst ? rc_dst(k, py) : rc_dct(k * step, py)) * w.tmp[(k << log2n) + px];
        s = (s + 64) >> 7;
        w.res[i] = (int16_t)(s < -32768 ? -32768 : (s > 32767 ? 32767 : s));
      }
      RC_SYNC();
      // second stage along the rows
      for (int i = lane; i < nn; i += nl) {
        const int py = i >> log2n, px = i & (n - 1);
        int64_t s = 0;
        for (int k = 0; k < n; k++) s += (int64_t)(dst ? rc_dst(k, px) : rc_dct(k * step, px)) * w.res[(py << log2n) + k];
        w.tmp[i] = (int32_t)((s + ((int64_t)1 << (sh2 - 1))) >> sh2);
      }
      RC_SYNC();
      for (int i = lane; i < nn; i += nl) w.res[i] = (int16_t)rc_clip(w.tmp[i], -32768, 32767);
    }
    RC_SYNC();
  }
  for (int i = lane; i < nn; i += nl) {
    const int py = i >> log2n, px = i & (n - 1);
    pl[(size_t)(y + py) * stride + x + px] = (PEL)rc_clip(w.pred[i] + (cbf ? w.res[i] : 0), 0, pmax);
  }
  RC_SYNC();
}

// One CTU: its transform units in z-order -- the coding order -- each luma block followed by its chroma blocks (the 4x4 chroma blocks of four 4x4 luma blocks behind the
// fourth).
template <typename PEL, typename PIC>
RC_FN void rc_ctu(const PIC &p, RcWork &w, int lane, int nl, int cx, int cy)
{
  const int a = cy * p.ctus_x + cx;
  if (cx < 0 || cy < 0 || cx >= p.ctus_x || cy >= p.ctus_y) return;
  const hevcdl_ctu_record &r = p.recs[a];
  const int x0 = cx * 64, y0 = cy * 64;
  for (int z = 0; z < 256;) {
    int zx = 0, zy = 0;
    for (int b = 0; b < 4; b++) { zx |= ((z >> (2 * b)) & 1) << b; zy |= ((z >> (2 * b + 1)) & 1) << b; }
    const int x = x0 + 4 * zx, y = y0 + 4 * zy;
    if (x >= p.W || y >= p.H) { z++; continue; }
    const int depth = r.depth[z] & 3, trd = r.tr_idx[z] & 7, log2n = rc_clip(6 - depth - trd, 2, 5), np = 1 << (2 * (log2n - 2));
    if (z & (np - 1)) { z++; continue; }                                                         // (not the first partition of its unit: garbage records only)
    const int luma = r.luma_dir[z], cd = r.chroma_dir[z], qpy = rc_cu_qpy(p, a, z);
    rc_block<PEL>(p, w, lane, nl, 0, x, y, log2n, luma, (r.cbf[0][z] >> trd) & 1, r.tskip[0][z], r.coeff_y + 16 * z, qpy);
    int zc = -1, l2c = 0;
    if (log2n > 2) { zc = z; l2c = log2n - 1; } else if ((z & 3) == 3) { zc = z & ~3; l2c = 2; }
    if (zc >= 0) {
      const int cu_np = 256 >> (2 * depth), zcu = z & ~(cu_np - 1);
      const int mode_c = cd == 36 ? r.luma_dir[r.part_size[zcu] == 3 ? zc : zcu] : cd;         // DM: the luma mode of the chroma block's place (an 8x8 NxN CU: its first)
      int zx2 = 0, zy2 = 0;
      for (int b = 0; b < 4; b++) { zx2 |= ((zc >> (2 * b)) & 1) << b; zy2 |= ((zc >> (2 * b + 1)) & 1) << b; }
      for (int c = 1; c < 3; c++)
        rc_block<PEL>(p, w, lane, nl, c, x0 + 4 * zx2, y0 + 4 * zy2, l2c, mode_c, (r.cbf[c][zc] >> trd) & 1, r.tskip[c][zc], (c == 1 ? r.coeff_cb : r.coeff_cr) + 4 * zc, qpy);
    }
    z += np;
  }
}

} // namespace hevcdl_rc
#endif
