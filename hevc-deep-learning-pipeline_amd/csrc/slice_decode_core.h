// slice_decode_core.h -- the arithmetic DECODER and the slice-data syntax of an I slice as ONE source for the host and the device: the mirror image of entropy_coder.h.
//
// A restatement of what struct Engine and struct Picture of hevcdl_parse.cpp do (ITU-T H.265 9.3.4.3 and 7.3.8: sao, coding_quadtree, coding_unit with the candidate
// modes of 8.4.2, transform_tree, residual_coding with transform skip and sign data hiding, end_of_slice_segment_flag / end_of_subset_one_bit and the alignment of every
// sub-stream), stated so that a GPU wave can run it.  Two instantiations: hevcdl_slice_decode_kernel (slice_decode_kernel.hip) and hevcdl_parse_stream_core
// (hevcdl_parse.cpp).  hevcdl_parse_stream is the second implementation this one is held against: same records, same SAO blocks, byte for byte.  Only the slice data
// is decoded twice: the code in front of it (NAL units, parameter sets, slice headers, layouts) is one walk over the stream, walk_stream, that both run.
//
// What it decodes is a UNIT (SdUnit): the longest run of CTUs one decoder must walk serially -- a tile, a row slice, or a whole picture (WaveFrontSynchro rows included:
// they are walked one after the other).  A unit is a rectangle of CTUs walked in raster order, fed by sub-streams (SdSub) out of one blob of RBSP bytes.  Neighbours
// outside the unit are unavailable (6.4.1: another tile, another slice), so a unit reads nothing another unit writes.
//
// Construction rules (a stream is untrusted input; they are what makes a GPU fault an implausible outcome of a damaged one):
//   * no recursion: the coding quadtree and the transform tree are walked iteratively in z-order.  Arriving at partition z, the node that starts there has the smallest
//     depth d with z % (256 >> 2d) == 0 -- its ancestors were split, or z would have been passed over -- and the flags are read downwards from d;
//   * no dynamic allocation, no std:: containers, no function pointers;
//   * every loop has a bound that does not depend on stream contents: 32 prefix bins, 32 escape bins, the SAO maximum, the block's scan, 64 coefficient groups, 16
//     positions, 4 + 5 tree levels, 256 partitions, the CTUs of the unit;
//   * every value that addresses memory is checked where it is read (last position, prediction modes, levels, the unit's rectangle against the picture, a sub-stream
//     against the blob); partition indices are masked to the record;
//   * the bit reader knows the end of its sub-stream: past it, it yields zeros and sets a sticky flag; a decoder that has gone bad leaves its CTU loop without another
//     store and reports (SdResult: a code of SdError and the CTU).
#ifndef HEVCDL_SLICE_DECODE_CORE_H
#define HEVCDL_SLICE_DECODE_CORE_H
#include <stdint.h>
#include "hevcdl.h"
#include "entropy_tables.h"
#include "entropy_coder.h"

#ifndef SD_FN
#ifdef __HIPCC__
#define SD_FN __host__ __device__ inline
#else
#define SD_FN inline
#endif
#endif

namespace hevcdl_sd {
using namespace hevcdl_ec;

enum SdError {
  SD_OK = 0,
  SD_E_UNIT,               // the unit table
  SD_E_SUBSTREAM_START,
  SD_E_TB_SIZE, SD_E_TB_LEAVES, SD_E_LAST_POS, SD_E_LAST_SCAN, SD_E_LEVEL, SD_E_LUMA_MODE,
  SD_E_DATA_ENDS,
  SD_E_TRAILING_BITS, SD_E_NO_END, SD_E_EARLY_END, SD_E_SUBSET_BIT, SD_E_ALIGNMENT,
  SD_E_QP_DELTA,
  SD_E_COUNT
};
// the sentence of a code (host side: the kernel reports the code)
inline const char *sd_error_sentence(int code)
{
  static const char *const s[SD_E_COUNT] = {
    "",
    "the unit table does not fit the picture or the slice data",
    "a sub-stream too short for the arithmetic decoder, or one that starts with an offset of 510 / 511",
    "a transform block outside 4 .. 32",
    "a transform block that leaves its CTU",
    "last significant position outside the block",
    "last significant position outside the scan",
    "a level outside 16 bits",
    "a luma prediction mode above 34",
    "the slice data ends inside the CTU",
    "rbsp_slice_segment_trailing_bits() behind the CTU are damaged, or bytes follow them",
    "no end_of_slice_segment_flag behind the last CTU of its slice segment",
    "end_of_slice_segment_flag inside its slice segment",
    "end_of_subset_one_bit behind the CTU is 0",
    "byte_alignment() behind the CTU is damaged, or its entry point is wrong",
    "CuQpDeltaVal outside its range",
  };
  return (unsigned)code < (unsigned)SD_E_COUNT ? s[code] : "an unknown error code";
}

// what every unit of a launch shares: the stream's parameter sets as far as slice data reads them
struct SdStream {
  int32_t W, H, ctus_x, ctus_y;
  int32_t wpp, tskip, sign_hiding, max_sao;      // entropy_coding_sync_enabled_flag, transform_skip_enabled_flag, sign_data_hiding_enabled_flag, (1 << (min(bitDepth, 10) - 5)) - 1
  int32_t row_slices;                            // SliceMode 1: the one layout in which the CTU behind a slice is neither a new tile nor a new wavefront row (sd_decode_unit)
  int32_t cu_qp, log2_qg, qp_bd_offset;          // cu_qp_delta_enabled_flag (0 unless the caller accepts it), Log2MinCuQpDeltaSize = 6 - diff_cu_qp_delta_depth, QpBdOffset = 6 * (bitDepth - 8)
};
// The two contexts of cu_qp_delta_abs stand BEHIND the coder's NUM_CTX, which keep their numbers: the encoder's coder never sees them.  Initialisation value 154 for both
// (ITU-T H.265 Table 9-4 names Table 9-24 for cu_qp_delta_abs: ctxIdx 0 .. 1 of initType 0 are 154, 154): slope 0, offset 64 -- state 0, MPS 1 at every slice QP.
enum { SD_CTX_DQP = NUM_CTX, SD_NUM_CTX = NUM_CTX + 2, SD_DQP_INIT = 154 };
struct SdSub { uint32_t off, size, ends_segment, pad; };      // off: from the first byte of its picture in the blob
struct SdUnit {
  int32_t pic, first_ts, n_ctus, slice_addr, qp, sub0, n_subs, sao_on;      // slice_addr: SliceAddrRs of its CTUs (one slice a unit: availability inside the unit does not ask for it)
  int32_t cx0, cx1, cy0, cy1;                    // its CTUs: a rectangle, walked in raster order; (cx1 - cx0) * (cy1 - cy0) == n_ctus
  uint32_t rbsp0, rbsp_bytes;                    // its picture's bytes in the blob
};
struct SdResult { int32_t code, ctu; };          // ctu: raster address in its picture, -1 where the error is not one of a CTU

struct SdState {
  const EcTables *t; const SdStream *s;
  uint8_t *ctx, *sync;                           // EC_SYNC_BYTES each
  uint16_t *cg_pos; int16_t *cg_val;             // 16 + 16: the coefficient group in work
  uint8_t *dry_depth, *dry_dir;                  // 2 x 256 each: the CTUs walked behind the end of a row slice (sd_decode_unit), current and previous
  int8_t *qp_cur;                                // 256: QpY of the partitions of the CTU in work (qPY_A / qPY_B come from inside the CTB only, 8.6.1); used with qp_map or s->cu_qp
  int8_t *qp_map;                                // [ctus][256] of the unit's picture, or null: QpY of every 4x4 partition of a coded CU in z-order, 0 outside the picture
  int slice_qp, last_qp, qg_pred, is_coded, delta_val;      // SliceQpY; QpY of the last CU in decoding order (qPY_PREV of the next group); qPY_PRED, IsCuQpDeltaCoded, CuQpDeltaVal of the group
  hevcdl_ctu_record *recs; hevcdl_sao_blk *sao;  // of the unit's picture.  NOT const, NOT restrict: depth and luma_dir are read back behind the unit's own stores
  int cx0, cx1, cy0, cy1, cur_cx, cur_cy, dry;
  // bit reader and arithmetic decoder
  const uint8_t *d; uint32_t size, pos; uint64_t win; int nwin; uint32_t last;
  uint32_t range, offset; int bad, err;
};

// ---- stores: one lane each on the host; across the lanes of a wave on the device (slice_decode_kernel.hip) -------------------------------------------------
#ifdef HEVCDL_SD_LANES
__device__ void sd_fill8(uint8_t *p, int n, int v);
__device__ void sd_or8(uint8_t *p, int n, int v);
__device__ void sd_clear32(void *p, int dwords);
__device__ void sd_put8(uint8_t *p, int v);
__device__ void sd_put32(int32_t *p, int v);
__device__ void sd_put_levels(int16_t *coef, const uint16_t *pos, const int16_t *val, int n);
#else
SD_FN void sd_fill8(uint8_t *p, int n, int v) { for (int i = 0; i < n; i++) p[i] = (uint8_t)v; }
SD_FN void sd_or8(uint8_t *p, int n, int v) { for (int i = 0; i < n; i++) p[i] |= (uint8_t)v; }
SD_FN void sd_clear32(void *p, int dwords) { uint32_t *q = (uint32_t *)p; for (int i = 0; i < dwords; i++) q[i] = 0; }
SD_FN void sd_put8(uint8_t *p, int v) { *p = (uint8_t)v; }
SD_FN void sd_put32(int32_t *p, int v) { *p = v; }
SD_FN void sd_put_levels(int16_t *coef, const uint16_t *pos, const int16_t *val, int n) { for (int i = 0; i < n; i++) coef[pos[i]] = val[i]; }
#endif

// ---- the bounded bit reader -------------------------------------------------------------------------------------------------------------------------------
SD_FN uint32_t sd_byte(const SdState &s, uint32_t i) { return i < s.size ? s.d[i] : 0u; }
SD_FN uint32_t sd_bits(SdState &s, int n)
{ // n <= 32.  The window is refilled a dword at a time; bytes behind the end are zeros, and CONSUMING a bit behind the end sets the sticky flag
  if (n <= 0) return 0;
  if (n > 32) n = 32;
  if (s.nwin < n) {
    const uint32_t w = (sd_byte(s, s.pos) << 24) | (sd_byte(s, s.pos + 1) << 16) | (sd_byte(s, s.pos + 2) << 8) | sd_byte(s, s.pos + 3);
    s.win = (s.win << 32) | w; s.nwin += 32; s.pos += 4;
  }
  s.nwin -= n;
  const uint32_t v = (uint32_t)(s.win >> s.nwin) & (n == 32 ? 0xffffffffu : ((1u << n) - 1u));
  if ((uint64_t)s.pos * 8 - (uint64_t)s.nwin > (uint64_t)s.size * 8) s.bad = 1;
  s.last = v & 1u;
  return v;
}
SD_FN uint64_t sd_consumed(const SdState &s) { return (uint64_t)s.pos * 8 - (uint64_t)s.nwin; }

// ---- 9.3.4.3 ---------------------------------------------------------------------------------------------------------------------------------------------
SD_FN void sd_start(SdState &s, const uint8_t *data, uint32_t n)
{
  s.d = data; s.size = n; s.pos = 0; s.win = 0; s.nwin = 0; s.last = 0; s.bad = 0; s.range = 510;
  s.offset = sd_bits(s, 9);
  if (s.offset >= 510) s.bad = 1;
}
SD_FN int sd_bin(SdState &s, int c)
{
  if ((unsigned)c >= (unsigned)SD_NUM_CTX) { s.bad = 1; return 0; }
  const uint32_t cv = s.ctx[c] & 127u, st = cv >> 1; int v = (int)(cv & 1);
  const uint32_t lps = s.t->lps[st][(s.range >> 6) & 3];
  s.range -= lps;
  if (s.offset >= s.range) { v = !v; s.offset -= s.range; s.range = lps; s.ctx[c] = s.t->next_lps[cv]; }
  else s.ctx[c] = s.t->next_mps[cv];
  if (s.range < 256) {
    int sh = s.range ? __builtin_clz(s.range) - 23 : 8;
    if (sh > 8) sh = 8;
    s.range <<= sh; s.offset = (s.offset << sh) | sd_bits(s, sh);
  }
  return v;
}
SD_FN uint32_t sd_eps(SdState &s, int n)
{
  if (n <= 0) return 0;
  if (n > 32) n = 32;
  const uint32_t b = sd_bits(s, n); uint32_t v = 0;
  for (int i = n - 1; i >= 0; i--) {
    s.offset = (s.offset << 1) | ((b >> i) & 1u); v <<= 1;
    if (s.offset >= s.range) { s.offset -= s.range; v |= 1u; }
  }
  return v;
}
SD_FN int sd_ep(SdState &s) { return (int)sd_eps(s, 1); }
SD_FN int sd_terminate(SdState &s)
{
  s.range -= 2;
  if (s.offset >= s.range) return 1;
  if (s.range < 256) { s.range <<= 1; s.offset = (s.offset << 1) | sd_bits(s, 1); }
  return 0;
}
// behind a terminating bin of 1: the last bit read is the 1 of byte_alignment() / rbsp_slice_segment_trailing_bits(), zeros up to the byte boundary, nothing after
SD_FN bool sd_finish(SdState &s)
{
  const uint64_t c = sd_consumed(s);
  if (s.bad || c == 0 || c > (uint64_t)s.size * 8 || !s.last) return false;
  if (sd_bits(s, (int)((8 - (c & 7)) & 7)) != 0) return false;
  return sd_consumed(s) == (uint64_t)s.size * 8 && !s.bad;
}

// the coder's contexts and, behind them, the two of cu_qp_delta_abs
SD_FN void sd_init_contexts(SdState &s, int qp)
{
  ec_init_contexts(s.ctx, s.t, qp);
  const int v = SD_DQP_INIT, slope = (v >> 4) * 5 - 45, offset = ((v & 15) << 3) - 16;
  int st = ((slope * qp) >> 4) + offset; st = st < 1 ? 1 : (st > 126 ? 126 : st);
  const int mps = st >= 64;
  for (int i = SD_CTX_DQP; i < SD_NUM_CTX; i++) s.ctx[i] = (uint8_t)(((mps ? st - 64 : 63 - st) << 1) + mps);
}

// ---- 8.6.1: the luma QP of a quantisation group and of a CU -----------------------------------------------------------------------------------------------
// a quantisation group starts at the coding-quadtree node (x, y): IsCuQpDeltaCoded and CuQpDeltaVal are reset, qPY_PRED is taken from the left and the upper partition
// where they lie in the same CTB, else from qPY_PREV -- the QpY of the last CU decoded, SliceQpY behind the start of a slice, a tile or a wavefront row
SD_FN void sd_start_qg(SdState &s, int x, int y)
{
  s.is_coded = 0; s.delta_val = 0;
  const int xl = ((x - 1) >> 2) & 15, yl = (y >> 2) & 15, xu = (x >> 2) & 15, yu = ((y - 1) >> 2) & 15;
  const int a = (x & 63) ? s.qp_cur[s.t->r2z[(yl << 4) | xl]] : s.last_qp, b = (y & 63) ? s.qp_cur[s.t->r2z[(yu << 4) | xu]] : s.last_qp;
  s.qg_pred = (a + b + 1) >> 1;
}
// cu_qp_delta_abs (prefix: truncated unary, cMax 5, context 0 for the first bin and 1 for the others; suffix: EG0 in bypass bins) and cu_qp_delta_sign_flag, 7.3.8.14 / 9.3.3.10
SD_FN void sd_cu_qp_delta(SdState &s)
{
  int v = 0;
  for (int k = 0; k < 5; k++) { if (!sd_bin(s, SD_CTX_DQP + (k ? 1 : 0))) break; v++; }
  if (v == 5) {
    int k = 0;
    for (int i = 0; i < 32; i++) { if (!sd_ep(s)) break; if (k < 8) v += 1 << k; k++; }
    if (k >= 8) { s.err = SD_E_QP_DELTA; return; }                      // (>= 260: far outside any range; the suffix bits are not read)
    v += (int)sd_eps(s, k);
  }
  if (v && sd_ep(s)) v = -v;
  const int half = s.s->qp_bd_offset >> 1;
  if (v < -(26 + half) || v > 25 + half) { s.err = SD_E_QP_DELTA; return; }
  s.is_coded = 1; s.delta_val = v;
}
// QpY of the CU whose syntax has just been read: every partition of it in the CTU's map and, where there is one, in the picture's
SD_FN void sd_finish_cu_qp(SdState &s, int rs, int z, int nparts)
{
  int qp = s.slice_qp;
  if (s.s->cu_qp) {
    const int off = s.s->qp_bd_offset < 0 ? 0 : (s.s->qp_bd_offset > 48 ? 48 : s.s->qp_bd_offset);
    qp = ((s.qg_pred + s.delta_val + 52 + 2 * off) % (52 + off)) - off;
    s.last_qp = qp;
  }
  sd_fill8((uint8_t *)s.qp_cur + (z & 255), nparts, qp);
  if (s.qp_map && !s.dry) sd_fill8((uint8_t *)s.qp_map + (size_t)rs * 256 + (z & 255), nparts, qp);
}

// ---- the unit's records ----------------------------------------------------------------------------------------------------------------------------------
SD_FN int sd_z_of(const SdState &s, int x, int y) { return s.t->r2z[(((y >> 2) & 15) << 4) | ((x >> 2) & 15)]; }
// 6.4.1 for a left, an upper or an upper-right neighbour: inside the picture and in a CTU of the unit that is decoded already (a unit is one slice of one tile)
SD_FN bool sd_available(const SdState &s, int xn, int yn)
{
  if (xn < 0 || yn < 0 || xn >= s.s->W || yn >= s.s->H) return false;
  const int nx = xn >> 6, ny = yn >> 6;
  if (nx == s.cur_cx && ny == s.cur_cy) return true;
  if (nx < s.cx0 || nx >= s.cx1 || ny < s.cy0) return false;
  return ny < s.cur_cy || (ny == s.cur_cy && nx < s.cur_cx);
}
// which of the two dry CTUs a position lies in: 0 the current one, 1 the one before it, -1 neither (a CTU of the unit itself: its records), -2 an older dry CTU, which is
// not kept: the upper neighbour from the second row behind the slice on, in a picture more than one CTU wide.  Its depth reads 0 -- the one place where this walk may name
// another CTU than the parser, after a damaged slice has yielded more than a whole row of CTUs from the bits behind its end
SD_FN int sd_dry_slot(const SdState &s, int xn, int yn)
{
  if (!s.dry) return -1;
  const int nx = xn >> 6, ny = yn >> 6;
  if (nx == s.cur_cx && ny == s.cur_cy) return 0;
  if (ny >= s.cy1) return (s.cur_cy - ny) * s.s->ctus_x + s.cur_cx - nx == 1 ? 1 : -2;      // the CTU before it in raster order: its left neighbour, in a picture one CTU wide the upper one
  return -1;
}
SD_FN int sd_depth_at(const SdState &s, int xn, int yn)
{
  const int z = sd_z_of(s, xn, yn), slot = sd_dry_slot(s, xn, yn);
  if (slot >= 0) return s.dry_depth[slot * 256 + z];
  if (s.dry && (yn >> 6) >= s.cy1) return 0;
  return s.recs[(yn >> 6) * s.s->ctus_x + (xn >> 6)].depth[z];
}
SD_FN int sd_dir_at(const SdState &s, int xn, int yn)
{
  const int z = sd_z_of(s, xn, yn), slot = sd_dry_slot(s, xn, yn);
  if (slot >= 0) return s.dry_dir[slot * 256 + z];
  if (s.dry && (yn >> 6) >= s.cy1) return DC;
  return s.recs[(yn >> 6) * s.s->ctus_x + (xn >> 6)].luma_dir[z];
}

// ---- sao() 7.3.8.3: the inverse of ec_code_sao_blk; the block was cleared with its picture ------------------------------------------------------------------
SD_FN void sd_sao(SdState &s, int rs)
{
  const int rx = s.cur_cx, ry = s.cur_cy;
  int left = 0, up = 0;
  if (rx > 0 && sd_available(s, (rx - 1) << 6, ry << 6)) left = sd_bin(s, CTX_SAO_MERGE);
  if (ry > 0 && !left && sd_available(s, rx << 6, (ry - 1) << 6)) up = sd_bin(s, CTX_SAO_MERGE);
  hevcdl_sao_blk *b = s.dry ? nullptr : s.sao + rs;
  if (left || up) { if (b) { sd_put32(&b->c[0].mode, 2); sd_put32(&b->c[0].type, left ? 0 : 1); } return; }
  int type_idx = 0, eo = 0;
  const int max_sao = s.s->max_sao < 31 ? s.s->max_sao : 31;
  for (int c = 0; c < 3; c++) {
    if (c < 2) { type_idx = 0; if (sd_bin(s, CTX_SAO_TYPE)) type_idx = sd_ep(s) ? 2 : 1; }
    if (!type_idx) continue;
    int a[4];
    for (int i = 0; i < 4; i++) { a[i] = 0; for (int k = 0; k < 31 && a[i] < max_sao; k++) { if (!sd_ep(s)) break; a[i]++; } }
    if (type_idx == 1) {
      int neg[4];
      for (int i = 0; i < 4; i++) neg[i] = a[i] ? sd_ep(s) : 0;
      const int band = (int)sd_eps(s, 5);
      if (b) {
        sd_put32(&b->c[c].mode, 1); sd_put32(&b->c[c].type, 4); sd_put32(&b->c[c].aux, band);
        for (int i = 0; i < 4; i++) sd_put32(&b->c[c].offset[(band + i) & 31], neg[i] ? -a[i] : a[i]);
      }
    } else {
      if (c < 2) eo = (int)sd_eps(s, 2);
      if (b) {
        sd_put32(&b->c[c].mode, 1); sd_put32(&b->c[c].type, eo);
        sd_put32(&b->c[c].offset[0], a[0]); sd_put32(&b->c[c].offset[1], a[1]); sd_put32(&b->c[c].offset[3], -a[2]); sd_put32(&b->c[c].offset[4], -a[3]);
      }
    }
  }
}

// ---- residual_coding() 7.3.8.11: the inverse of ec_code_coeff ---------------------------------------------------------------------------------------------
SD_FN void sd_residual(SdState &s, hevcdl_ctu_record *r, int comp, int z, int log2n, int dir_mode)
{
  const EcTables *t = s.t;
  const int ch = comp ? 1 : 0;
  EcCParam cp; ec_get_cparam(t, cp, comp, log2n, dir_mode);
  if (cp.log2 != log2n) { s.err = SD_E_TB_SIZE; return; }
  const int n = cp.n, nn = n * n;
  const int base = (z & 255) * (comp ? 4 : 16);
  if (base + nn > (comp ? 1024 : 4096)) { s.err = SD_E_TB_LEAVES; return; }
  int16_t *coef = r ? (comp == 0 ? r->coeff_y : (comp == 1 ? r->coeff_cb : r->coeff_cr)) + base : nullptr;
  if (n == 4 && s.s->tskip) { const int f = sd_bin(s, CTX_TSKIP + ch); if (r) sd_put8(&r->tskip[comp][z & 255], f); }
  int px, py;
  { // last_sig_coeff_{x,y}_prefix / _suffix
    const int gmax = t->group_idx[n - 1], cw = log2n - 2;
    const int off = ch ? 0 : (cw * 3 + ((cw + 1) >> 2)), shift = ch ? cw : ((cw + 3) >> 2);
    const int bx = CTX_LAST_X + (ch ? 15 : 0) + off, by = CTX_LAST_Y + (ch ? 15 : 0) + off;
    int gx = 0, gy = 0;
    for (int k = 0; k < 32 && gx < gmax; k++) { if (!sd_bin(s, bx + (gx >> shift))) break; gx++; }
    for (int k = 0; k < 32 && gy < gmax; k++) { if (!sd_bin(s, by + (gy >> shift))) break; gy++; }
    px = gx > 3 ? t->min_in_group[gx] + (int)sd_eps(s, (gx - 2) >> 1) : gx;
    py = gy > 3 ? t->min_in_group[gy] + (int)sd_eps(s, (gy - 2) >> 1) : gy;
    if (px >= n || py >= n) { s.err = SD_E_LAST_POS; return; }
    if (cp.scan_type == SCAN_VER) { const int tmp = px; px = py; py = tmp; }
  }
  const int pos_last = py * n + px;
  int scan_last = -1;
  for (int q = 0; q < nn; q++) if ((cp.scan[q] & (nn - 1)) == pos_last) { scan_last = q; break; }
  if (scan_last < 0) { s.err = SD_E_LAST_SCAN; return; }
  const int cg_off = CTX_SIG_CG + (ch ? 2 : 0), sig_off = CTX_SIG + (ch ? 28 : 0);
  const int last_set = scan_last >> 4;
  uint64_t cgf = 0;
  int c1 = 1, sp = scan_last;
  for (int subset = last_set; subset >= 0 && !s.bad; subset--) {
    int num_nz = 0, go_rice = 0;
    const int sub_pos = subset << 4;
    int last_nz = -1, first_nz = 16;
    if (sp == scan_last) { s.cg_pos[0] = (uint16_t)pos_last; num_nz = 1; last_nz = first_nz = sp; sp--; }
    const int cgblk = cp.scan_cg[subset] & 63, gy = cgblk >> (log2n - 2), gx = cgblk & (cp.wg - 1);
    const int right = (gx < cp.wg - 1) ? (int)((cgf >> (gy * cp.wg + gx + 1)) & 1) : 0, lower = (gy < cp.wg - 1) ? (int)((cgf >> ((gy + 1) * cp.wg + gx)) & 1) : 0;
    if (subset == last_set || subset == 0) cgf |= 1ull << cgblk;
    else if (sd_bin(s, cg_off + ((right + lower) != 0))) cgf |= 1ull << cgblk;
    if ((cgf >> cgblk) & 1) {
      const int pat = cp.wg <= 1 ? 0 : right + (lower << 1);
      for (int q = 0; q < 16 && sp >= sub_pos; q++, sp--) {
        const int raster = cp.scan[sp] & (nn - 1);
        int sig = 1;                                                   // the group's only possible level: inferred
        if (sp > sub_pos || subset == 0 || num_nz) sig = sd_bin(s, sig_off + ec_sig_ctx_inc(t, cp, pat, raster));
        if (sig && num_nz < 16) { s.cg_pos[num_nz++] = (uint16_t)raster; if (last_nz == -1) last_nz = sp; first_nz = sp; }
      }
    } else sp = sub_pos - 1;
    if (num_nz == 0) continue;
    const int sign_hidden = s.s->sign_hiding && (last_nz - first_nz >= 4);
    const int cset = (ch ? 4 : 0) + ((!ch && subset > 0) ? 2 : 0) + (c1 == 0 ? 1 : 0);
    c1 = 1;
    const int n_c1 = num_nz < 8 ? num_nz : 8; int first_c2 = -1;
    uint32_t greater1 = 0;                                             // bit i: coeff_abs_level_greater1_flag of level i
    for (int i = 0; i < n_c1; i++) {
      const int sym = sd_bin(s, CTX_ONE + 4 * cset + c1);
      greater1 |= (uint32_t)sym << i;
      if (sym) { c1 = 0; if (first_c2 == -1) first_c2 = i; }
      else if (c1 < 3 && c1 > 0) c1++;
    }
    int greater2 = 0;
    if (c1 == 0 && first_c2 != -1) greater2 = sd_bin(s, CTX_ABS + cset);
    const int n_signs = num_nz - sign_hidden;
    const uint32_t signs = sd_eps(s, n_signs);
    int first_coeff2 = 1; uint32_t sum = 0;
    for (int i = 0; i < num_nz; i++) {
      int a = 1 + (int)((greater1 >> i) & 1u) + (i == first_c2 ? greater2 : 0);
      const int bse = (i < 8) ? (2 + first_coeff2) : 1;
      if (a == bse) { // coeff_abs_level_remaining: the inverse of xWriteCoefRemainExGolomb
        int q = 0;
        for (int k = 0; k < 32; k++) { if (!sd_ep(s)) break; q++; }
        int rem;
        if (q < 3) rem = (q << go_rice) + (int)sd_eps(s, go_rice);
        else {
          const int len = q - 3 + go_rice;
          if (len > 17) { s.err = SD_E_LEVEL; return; }
          rem = (int)sd_eps(s, len) + (3 << go_rice) + ((1 << len) - (1 << go_rice));
        }
        a += rem;
        if (a > (3 << go_rice)) go_rice = go_rice + 1 < 4 ? go_rice + 1 : 4;
      }
      if (a >= 2) first_coeff2 = 0;
      sum += (uint32_t)a;
      const int neg = i < n_signs ? (int)((signs >> (n_signs - 1 - i)) & 1) : (int)(sum & 1);      // the hidden sign is the last one's: the parity of the group's sum
      const int v = neg ? -a : a;
      if (v < -32768 || v > 32767) { s.err = SD_E_LEVEL; return; }
      s.cg_val[i] = (int16_t)v;
    }
    if (coef) sd_put_levels(coef, s.cg_pos, s.cg_val, num_nz);
  }
}

struct SdCu { int x, y, log2, z, nparts, nxn, mode_c; hevcdl_ctu_record *r; };

// transform_tree() 7.3.8.8 and transform_unit() 7.3.8.10 of one CU, its 4x4 partitions in z-order.  Standing on zrel, the walk goes down from the shallowest level trd
// whose node starts there; the chroma flags of the node's ancestors are in cb[] / cr[], indexed by depth (cb[trd]: what a node of depth trd inherits)
SD_FN void sd_transform_tree(SdState &s, const SdCu &cu)
{
  hevcdl_ctu_record *r = cu.r;
  const int max_depth = 2 + cu.nxn;
  int cb[6] = { 0, 0, 0, 0, 0, 0 }, cr[6] = { 0, 0, 0, 0, 0, 0 };
  int zrel = 0;
  for (int it = 0; it < 256 && zrel < cu.nparts && !s.bad && !s.err; it++) {
    int trd = 0;
    for (int k = 0; k < 4 && (zrel & ((cu.nparts >> (2 * trd)) - 1)) != 0 && cu.log2 - trd > 2; k++) trd++;
    for (int lvl = 0; lvl < 5 && trd < 5; lvl++, trd++) {
      const int log2 = cu.log2 - trd, np = cu.nparts >> (2 * trd), z = cu.z + zrel;
      int split;
      if (log2 <= 5 && log2 > 2 && trd < max_depth && !(cu.nxn && trd == 0)) split = sd_bin(s, CTX_SUBDIV + 5 - log2);
      else split = (log2 > 5 || (cu.nxn && trd == 0)) ? 1 : 0;
      int cbf_c[3] = { 0, cb[trd], cr[trd] };
      if (log2 > 2) for (int c = 1; c < 3; c++) {
        cbf_c[c] = (trd == 0 || cbf_c[c]) ? sd_bin(s, CTX_QT_CBF + 5 + trd) : 0;
        if (cbf_c[c] && r) sd_or8(&r->cbf[c][z & 255], np, (1 << trd) | ((log2 == 3 && split) ? (2 << trd) : 0));
      }
      if (split) { cb[trd + 1] = cbf_c[1]; cr[trd + 1] = cbf_c[2]; continue; }      // the first child starts at the same partition
      const int cbf_y = sd_bin(s, CTX_QT_CBF + (trd == 0 ? 1 : 0));
      // transform_unit(): cbfChroma of a 4x4 luma block is its parent's -- cbf_c[] was inherited and not read again
      if (s.s->cu_qp && !s.is_coded && (cbf_y || cbf_c[1] || cbf_c[2])) { sd_cu_qp_delta(s); if (s.err) return; }
      if (r) sd_fill8(&r->tr_idx[z & 255], np, trd);
      const int luma_mode = s.dry ? s.dry_dir[z & 255] : r->luma_dir[z & 255];
      if (cbf_y) {
        if (r) for (int d = 0; d <= trd; d++) {
          const int nd = cu.nparts >> (2 * d), org = cu.z + (zrel & ~(nd - 1));
          sd_or8(&r->cbf[0][org & 255], nd, 1 << d);
        }
        sd_residual(s, r, 0, z, log2, luma_mode);
      }
      if (log2 > 2) { for (int c = 1; c < 3; c++) if (cbf_c[c] && !s.err) sd_residual(s, r, c, z, log2 - 1, cu.mode_c); }
      else if ((zrel & 3) == 3) for (int c = 1; c < 3; c++) if (cbf_c[c] && !s.err) sd_residual(s, r, c, cu.z + (zrel & ~3), 2, cu.mode_c);
      zrel += np;
      break;
    }
  }
}

// coding_unit() 7.3.8.5 with 8.4.2 / 8.4.3
SD_FN void sd_coding_unit(SdState &s, hevcdl_ctu_record *r, int x0, int y0, int log2, int depth)
{
  SdCu cu; cu.x = x0; cu.y = y0; cu.log2 = log2; cu.z = sd_z_of(s, x0, y0); cu.nparts = 1 << (2 * (log2 - 2)); cu.r = r;
  cu.nxn = log2 == 3 ? !sd_bin(s, CTX_PART_SIZE) : 0;
  if (r) { sd_fill8(&r->depth[cu.z], cu.nparts, depth); sd_fill8(&r->part_size[cu.z], cu.nparts, cu.nxn ? SIZE_NxN : SIZE_2Nx2N); }
  else sd_fill8(&s.dry_depth[cu.z], cu.nparts, depth);
  const int npu = cu.nxn ? 4 : 1, pb = cu.nxn ? 4 : (1 << log2), ppu = cu.nparts / npu;
  int prev[4], coded[4];
  for (int j = 0; j < npu; j++) prev[j] = sd_bin(s, CTX_INTRA_PRED);
  for (int j = 0; j < npu; j++) coded[j] = prev[j] ? (sd_ep(s) ? 1 + sd_ep(s) : 0) : (int)sd_eps(s, 5);
  int luma0 = 0;
  for (int j = 0; j < npu; j++) {
    const int xp = x0 + (j & 1) * pb, yp = y0 + (j >> 1) * pb;
    int left = DC, above = DC;
    if (sd_available(s, xp - 1, yp)) left = sd_dir_at(s, xp - 1, yp);
    if ((yp & 63) != 0 && sd_available(s, xp, yp - 1)) above = sd_dir_at(s, xp, yp - 1);
    int c0, c1, c2;
    if (left == above) {
      if (left > 1) { c0 = left; c1 = ((left + 29) % 32) + 2; c2 = ((left - 1) % 32) + 2; }
      else { c0 = PLANAR; c1 = DC; c2 = VER; }
    } else {
      c0 = left; c1 = above;
      c2 = (left && above) ? PLANAR : ((left + above) < 2 ? VER : DC);
    }
    int mode;
    if (prev[j]) mode = coded[j] == 0 ? c0 : (coded[j] == 1 ? c1 : c2);
    else {
      int tmp;
      if (c0 > c1) { tmp = c0; c0 = c1; c1 = tmp; } if (c0 > c2) { tmp = c0; c0 = c2; c2 = tmp; } if (c1 > c2) { tmp = c1; c1 = c2; c2 = tmp; }      // the candidates in ascending order
      mode = coded[j];
      if (mode >= c0) mode++;
      if (mode >= c1) mode++;
      if (mode >= c2) mode++;
    }
    if (mode < 0 || mode > 34) { s.err = SD_E_LUMA_MODE; return; }
    if (j == 0) luma0 = mode;
    sd_fill8(r ? &r->luma_dir[cu.z + j * ppu] : &s.dry_dir[cu.z + j * ppu], ppu, mode);
  }
  int icpm = 4;
  if (sd_bin(s, CTX_CHROMA_PRED)) icpm = (int)sd_eps(s, 2);
  int rec_c = DM_CHROMA; cu.mode_c = luma0;
  if (icpm != 4) {
    const int m = icpm == 0 ? PLANAR : (icpm == 1 ? VER : (icpm == 2 ? HOR : DC));
    cu.mode_c = m == luma0 ? 34 : m;
    rec_c = cu.mode_c;
  }
  if (r) sd_fill8(&r->chroma_dir[cu.z], cu.nparts, rec_c);
  sd_transform_tree(s, cu);
  if ((s.s->cu_qp || s.qp_map) && !s.err) sd_finish_cu_qp(s, s.cur_cy * s.s->ctus_x + s.cur_cx, cu.z, cu.nparts);
}

// coding_quadtree() 7.3.8.4 of the CTU at (cur_cx, cur_cy): its 8x8 blocks in z-order; a block covered by a coded CU, or outside the picture, is passed over
SD_FN void sd_coding_quadtree(SdState &s, hevcdl_ctu_record *r)
{
  const int x0 = s.cur_cx << 6, y0 = s.cur_cy << 6, W = s.s->W, H = s.s->H;
  int next_z = 0;
  for (int z = 0; z < 256 && !s.bad && !s.err; z += 4) {
    if (z < next_z) continue;
    int zx = 0, zy = 0;
    for (int b = 0; b < 4; b++) { zx |= ((z >> (2 * b)) & 1) << b; zy |= ((z >> (2 * b + 1)) & 1) << b; }
    const int x = x0 + zx * 4, y = y0 + zy * 4;
    if (x >= W || y >= H) continue;
    int depth = 0;
    for (int k = 0; k < 3 && (z & ((256 >> (2 * depth)) - 1)) != 0; k++) depth++;
    for (int lvl = 0; lvl < 4 && depth < 4; lvl++, depth++) {
      const int size = 64 >> depth, log2 = 6 - depth;
      if (s.s->cu_qp && log2 >= s.s->log2_qg) sd_start_qg(s, x, y);
      int split;
      if (x + size <= W && y + size <= H && log2 > 3) {
        int inc = 0;
        if (sd_available(s, x - 1, y)) inc += sd_depth_at(s, x - 1, y) > depth;
        if (sd_available(s, x, y - 1)) inc += sd_depth_at(s, x, y - 1) > depth;
        split = sd_bin(s, CTX_SPLIT + inc);
      } else split = log2 > 3;
      if (split) continue;
      sd_coding_unit(s, r, x, y, log2, depth);
      next_z = z + (256 >> (2 * depth));
      break;
    }
  }
}

// ---- slice_segment_data() 7.3.8.1 of one unit, with 9.3.1 / 9.3.2: where the contexts of a CTU come from ---------------------------------------------------
// recs / sao: the unit's picture (sao may be null when the unit has none); blob: the RBSP bytes, blob_bytes of them; subs: the launch's table, n_subs_all entries.
// The CTUs of the unit are cleared before they are decoded.
SD_FN SdResult sd_decode_unit(SdState &s, const SdUnit &u, const SdSub *subs, int n_subs_all, const uint8_t *blob, uint64_t blob_bytes)
{
  const SdStream &g = *s.s;
  SdResult res = { SD_OK, -1 };
  const int uw = u.cx1 - u.cx0, uh = u.cy1 - u.cy0;
  if (u.cx0 < 0 || u.cy0 < 0 || uw < 1 || uh < 1 || u.cx1 > g.ctus_x || u.cy1 > g.ctus_y || (long long)uw * uh != u.n_ctus || u.sub0 < 0 || u.n_subs < 1 || u.n_subs > n_subs_all ||
      u.sub0 > n_subs_all - u.n_subs || u.n_subs != (g.wpp ? uh : 1) || (uint64_t)u.rbsp0 + u.rbsp_bytes > blob_bytes || (u.sao_on && !s.sao)) { res.code = SD_E_UNIT; return res; }
  s.cx0 = u.cx0; s.cx1 = u.cx1; s.cy0 = u.cy0; s.cy1 = u.cy1; s.dry = 0; s.err = 0; s.bad = 0;
  if (g.cu_qp && (g.log2_qg < 3 || g.log2_qg > 6 || !s.qp_cur)) { res.code = SD_E_UNIT; return res; }
  s.slice_qp = s.last_qp = s.qg_pred = u.qp; s.is_coded = 0; s.delta_val = 0;
  int have_sync = 0, k = 0;
  bool walk_on = false;
  for (int cy = u.cy0; cy < u.cy1; cy++) for (int cx = u.cx0; cx < u.cx1; cx++) {
    const int rs = cy * g.ctus_x + cx;
    s.cur_cx = cx; s.cur_cy = cy;
    const bool first = cx == u.cx0 && cy == u.cy0, new_row = g.wpp && cx == u.cx0;
    if (first || new_row) {
      if (!first) k++;
      const SdSub &sb = subs[u.sub0 + k];
      if ((uint64_t)sb.off + sb.size > u.rbsp_bytes) { res.code = SD_E_UNIT; return res; }
      sd_start(s, blob + u.rbsp0 + sb.off, sb.size);
      if (s.bad) { res.code = SD_E_SUBSTREAM_START; return res; }
      if (!first && have_sync && sd_available(s, (cx + 1) << 6, (cy - 1) << 6)) { for (int i = 0; i < SD_NUM_CTX; i++) s.ctx[i] = s.sync[i]; }
      else sd_init_contexts(s, u.qp);
      s.last_qp = u.qp;                                                 // qPY_PREV of the first quantisation group of a slice, a tile, a wavefront row: SliceQpY
    }
    hevcdl_ctu_record *r = s.recs + rs;
    sd_clear32(r, (int)(sizeof(hevcdl_ctu_record) / 4));
    if (s.sao) sd_clear32(s.sao + rs, (int)(sizeof(hevcdl_sao_blk) / 4));
    if (s.qp_map) sd_clear32(s.qp_map + (size_t)rs * 256, 64);
    if (u.sao_on) sd_sao(s, rs);
    sd_coding_quadtree(s, r);
    res.ctu = rs;
    if (s.err) { res.code = s.err; return res; }
    const int end = sd_terminate(s);
    if (s.bad) { res.code = SD_E_DATA_ENDS; return res; }
    if (g.wpp && cx == u.cx0 + 1) { for (int i = 0; i < SD_NUM_CTX; i++) s.sync[i] = s.ctx[i]; have_sync = 1; }
    const bool sub_ends = g.wpp ? cx == u.cx1 - 1 : (cx == u.cx1 - 1 && cy == u.cy1 - 1);
    const bool seg_ends = sub_ends && subs[u.sub0 + k].ends_segment;
    if (end) {
      if (!sd_finish(s)) { res.code = SD_E_TRAILING_BITS; return res; }
      if (!seg_ends) { res.code = SD_E_EARLY_END; res.ctu = -1; return res; }      // (the parser: the next segment's address is not the CTU behind this one -- no CTU is named)
      continue;
    }
    if (seg_ends) { // no end where the layout has one: the parser walks on, and so does this -- without a store -- to name the CTU it names
      if (rs == g.ctus_x * g.ctus_y - 1 || !g.row_slices) {
        // behind the picture: nothing to walk.  Tiles, wavefront rows: the CTU behind is a new tile or row, and the bin just read as 0 was its end_of_subset_one_bit's twin
        res.code = rs == g.ctus_x * g.ctus_y - 1 ? SD_E_NO_END : SD_E_SUBSET_BIT;
        if (rs == g.ctus_x * g.ctus_y - 1) res.ctu = -1;
        else if (sd_terminate(s) == 1) { res.code = sd_finish(s) ? SD_E_NO_END : SD_E_ALIGNMENT; if (res.code == SD_E_NO_END) res.ctu = -1; }
        return res;
      }
      walk_on = true;
      break;
    }
    if (sub_ends) {
      if (sd_terminate(s) != 1) { res.code = SD_E_SUBSET_BIT; return res; }
      if (!sd_finish(s)) { res.code = SD_E_ALIGNMENT; return res; }
    }
  }
  if (walk_on) { // SliceMode 1 and the slice did not end with its last CTU.  The parser decodes the CTUs behind it from what the sub-stream has left, with the slice's CTUs as their
    // neighbours, until the data runs out, a syntax error shows or an end flag comes.  The same walk here: depth and luma_dir of the two newest of those CTUs in
    // dry_depth / dry_dir, nothing stored into a record (they are another unit's)
    s.dry = 1;
    const int n = g.ctus_x * g.ctus_y;
    for (int rs = u.cy1 * g.ctus_x; rs < n; rs++) {
      s.cur_cx = rs % g.ctus_x; s.cur_cy = rs / g.ctus_x;
      for (int i = 0; i < 256; i++) { s.dry_depth[256 + i] = s.dry_depth[i]; s.dry_dir[256 + i] = s.dry_dir[i]; s.dry_depth[i] = 0; s.dry_dir[i] = 0; }
      if (u.sao_on) sd_sao(s, rs);
      sd_coding_quadtree(s, nullptr);
      res.ctu = rs;
      if (s.err) { res.code = s.err; return res; }
      const int end = sd_terminate(s);
      if (s.bad) { res.code = SD_E_DATA_ENDS; return res; }
      if (end) { res.code = sd_finish(s) ? SD_E_EARLY_END : SD_E_TRAILING_BITS; if (res.code == SD_E_EARLY_END) res.ctu = -1; return res; }
    }
    res.code = SD_E_NO_END; res.ctu = -1;
  }
  return res;
}

} // namespace hevcdl_sd
#endif
