// entropy_coder.h -- the arithmetic coder and the slice-data syntax of an I slice as ONE source for the host and the device.
//
// Plain inline functions over raw pointers and a small POD state (EcCoder), after the reference's TEncBinCoderCABAC.cpp:70-446, TEncSbac.cpp:613-1720,
// TEncEntropy.cpp:200-398, TEncCu.cpp:1167-1271 and TEncSlice.cpp:985-1170, stated so that a GPU wave can run it.  Two instantiations: hevcdl_entropy_kernel
// (entropy_kernel.hip) and the host's SliceCoder (hevcdl_bitstream.cpp), which is behind hevcdl_write_access_unit, hevcdl_code_slice_data_host and the fallback of the
// device path.  There is no second coder: what this one writes is held to the reference encoder's streams (tests/golden/rd_*.npz), to the test suite's spec-level
// slice-data decoder and to the streams recorded from the former host writer before it went (tests/golden/entropy_host_writer_digests.json).
//
// Construction rules (they are what makes a GPU fault an implausible outcome of garbage input):
//   * no recursion: the CU quadtree and the transform tree are walked iteratively in z-order; the flags of a node (split flag; subdivision flag and chroma cbf flags) are
//     emitted when the walk reaches the node's first partition, which is the pre-order of the recursive writers;
//   * no dynamic allocation, no std:: containers, no function pointers;
//   * every loop has a bound that does not depend on record contents (256 partitions, 4 + 5 tree levels, 64 coefficient groups, 16 positions, 32 escape bits, the
//     sub-stream's capacity);
//   * every index into a record's arrays is masked (z & 255; a transform block is moved to lie inside its coefficient array, a position in it masked to the block) and
//     every CTU address range-checked; neighbours are looked up inside the tile / picture only;
//   * every output byte goes through ec_put_byte, which compares the position with the sub-stream's capacity: past it, a sticky flag is set and the bytes are counted,
//     not stored.
#ifndef HEVCDL_ENTROPY_CODER_H
#define HEVCDL_ENTROPY_CODER_H
#include <stdint.h>
#include "hevcdl.h"
#include "entropy_tables.h"

#ifndef EC_FN
#ifdef __HIPCC__
#define EC_FN __host__ __device__ inline
#else
#define EC_FN inline
#endif
#endif

namespace hevcdl_ec {

enum { EC_REGION_SLACK = 64,              // capacity of a sub-stream = its CTUs x capacity per CTU + this
       EC_REGION_GAP = 64,                // bytes between two sub-stream regions of a slice-data buffer that no coder writes
       // Worst case of one CTU, derived, not measured: a context-coded bin costs at most 6 bits (the longest renormalisation of an LPS), a bypass bin 1.
       // 6144 coefficients x (sig 6 + greater1 6 + sign 1 + 32 escape bits) = 276 480; 384 coefficient groups x (group flag 6 + greater2 6) = 4 608; 384 4x4 blocks x
       // (transform_skip 6 + last position 36 + cbf 6) = 18 432; transform tree 768 + 4 092; 64 8x8 CUs x 58 + 21 split flags x 6 = 3 838; SAO 425; end flag 7:
       // 308 650 bits = 38 582 bytes.  (hevcdl_access_unit_bound per CTU, 12 288, is NOT a bound: a CTU of +-32767 levels codes to 22.8 KB.)
       EC_DEFAULT_CAPACITY_PER_CTU = 40960,
       EC_SYNC_BYTES = 192,               // a stored context set (WaveFrontSynchro): NUM_CTX bytes, padded to whole dwords
       EC_STAGE_BYTES = 256 };            // device: output staging per wave (64 lanes x one dword)

struct EcCoder {
  const EcTables *t;
  uint8_t *ctx;                  // NUM_CTX context bytes ((state << 1) | mps), EC_SYNC_BYTES of storage
  uint16_t *absb;                // 16 absolute levels of the coefficient group being coded
  uint8_t *out;                  // the sub-stream's region; the device coder stages through `stage` and stores whole dwords
  uint8_t *stage;
  uint32_t cap, pos, overflow;   // capacity of the region, bytes produced so far (counted past the capacity too), sticky overflow flag
  uint32_t low, range; int bits_left, buffered; uint32_t buffered_byte;
  uint32_t held; int nheld;      // bit tail (the coder's flush and byte_alignment() write single bits)
  int dry;                       // 1: only the contexts are advanced (WaveFrontSynchro phase 1); nothing is produced
};

// what a sub-stream's coder reads: the picture's records and SAO parameters, the tile (or picture) it lies in
struct EcPic {
  const hevcdl_ctu_record *recs; const hevcdl_sao_blk *sao;      // [ctus]; sao may be null
  int W, H, ctus_x, ctus_y, ctus;
  int tx0, ty0;                  // top-left luma sample of the tile being written: nothing left of / above it is a neighbour
  uint32_t tools; int max_sao_offset;
  int slice_end_ctu = -1;        // raster address of the last CTU of the sub-stream when a slice, or a dependent slice segment, ends with it; -1: none but the picture's last CTU ends one (no slices, or a
                                 // sub-stream inside a slice).  The one member with a default: code that fills an EcPic field by field and knows no slices needs no change
};
struct EcCu { int x, y, log2, depth, zbase, nparts, part; const hevcdl_ctu_record *r; };
struct EcTu { int log2, trd, zrel; };
struct EcCParam { int log2, n, ch, scan_type, wg, first_sig_ctx; const uint16_t *scan; const uint8_t *scan_cg; };

#ifdef HEVCDL_EC_STAGED
__device__ void ec_flush_stage(EcCoder &s, uint32_t end);      // entropy_kernel.hip: the staged bytes [end - 1 rounded down to the stage, end) leave as dwords
#endif

// ---- output ------------------------------------------------------------------------------------------------------------
EC_FN void ec_put_byte(EcCoder &s, uint32_t b)
{
  if (s.pos < s.cap) {
#ifdef HEVCDL_EC_STAGED
    s.stage[s.pos & (EC_STAGE_BYTES - 1)] = (uint8_t)b;
    if ((s.pos & (EC_STAGE_BYTES - 1)) == EC_STAGE_BYTES - 1) ec_flush_stage(s, s.pos + 1);
#else
    s.out[s.pos] = (uint8_t)b;
#endif
  } else s.overflow = 1;
  s.pos++;
}
// `count` bytes of one value (the coder's buffered 0xff runs): stored while they fit, counted afterwards -- the loop is bounded by the capacity
EC_FN void ec_put_run(EcCoder &s, uint32_t b, int count)
{
  for (; count > 0 && s.pos < s.cap; count--) ec_put_byte(s, b);
  if (count > 0) { s.overflow = 1; s.pos += (uint32_t)count; }
}
EC_FN void ec_put_bits(EcCoder &s, uint32_t v, int n)
{ // TComOutputBitstream::write, n <= 24
  for (int i = (n < 24 ? n : 24) - 1; i >= 0; i--) { s.held = (s.held << 1) | ((v >> i) & 1u); if (++s.nheld == 8) { ec_put_byte(s, s.held); s.held = 0; s.nheld = 0; } }
}

// ---- arithmetic coder (TEncBinCABAC) -------------------------------------------------------------------------------------
EC_FN void ec_init_contexts(uint8_t *ctx, const EcTables *t, int qp)
{ // ContextModel::init ContextModel.cpp:56-66
  for (int i = 0; i < NUM_CTX; i++) {
    const int v = t->ctx_init[i], slope = (v >> 4) * 5 - 45, offset = ((v & 15) << 3) - 16;
    int st = ((slope * qp) >> 4) + offset; st = st < 1 ? 1 : (st > 126 ? 126 : st);
    const int mps = st >= 64;
    ctx[i] = (uint8_t)(((mps ? st - 64 : 63 - st) << 1) + mps);
  }
}
EC_FN void ec_start(EcCoder &s)
{
  s.low = 0; s.range = 510; s.bits_left = 23; s.buffered = 0; s.buffered_byte = 0xff; s.held = 0; s.nheld = 0; s.pos = 0; s.overflow = 0;
}
EC_FN void ec_write_out(EcCoder &s)
{
  const uint32_t lead = s.low >> (24 - s.bits_left);
  s.bits_left += 8; s.low &= 0xffffffffu >> s.bits_left;
  if (lead == 0xff) s.buffered++;
  else if (s.buffered > 0) {
    const uint32_t carry = lead >> 8;
    ec_put_byte(s, (s.buffered_byte + carry) & 0xff);
    s.buffered_byte = lead & 0xff;
    ec_put_run(s, (0xff + carry) & 0xff, s.buffered - 1);
    s.buffered = 1;
  } else { s.buffered = 1; s.buffered_byte = lead; }
}
EC_FN void ec_test_write(EcCoder &s) { if (s.bits_left < 12) ec_write_out(s); }
EC_FN void ec_bin(EcCoder &s, int c, int v)
{
  if ((unsigned)c >= (unsigned)NUM_CTX) c = 0;
  const uint32_t cv = s.ctx[c] & 127u; const int st = (int)(cv >> 1), mps = (int)(cv & 1);
  if (s.dry) { s.ctx[c] = (v != mps) ? s.t->next_lps[cv] : s.t->next_mps[cv]; return; }
  const uint32_t lps = s.t->lps[st][(s.range >> 6) & 3];
  s.range -= lps;
  if (v != mps) {
    const int nb = s.t->renorm[(lps >> 3) & 31];
    s.low = (s.low + s.range) << nb; s.range = lps << nb; s.ctx[c] = s.t->next_lps[cv]; s.bits_left -= nb; ec_test_write(s);
  } else {
    s.ctx[c] = s.t->next_mps[cv];
    if (s.range < 256) { s.low <<= 1; s.range <<= 1; s.bits_left--; ec_test_write(s); }
  }
}
EC_FN void ec_ep(EcCoder &s, int v) { if (s.dry) return; s.low <<= 1; if (v) s.low += s.range; s.bits_left--; ec_test_write(s); }
EC_FN void ec_eps(EcCoder &s, uint32_t v, int n)
{
  if (s.dry) return;
  if (n > 32) n = 32;
  if (n < 32) v &= (1u << n) - 1u;            // a caller's value never has more bits; garbage records must not change what the shifts below mean
  for (int k = 0; k < 4 && n > 8; k++) { n -= 8; const uint32_t pat = v >> n; s.low <<= 8; s.low += s.range * pat; v -= pat << n; s.bits_left -= 8; ec_test_write(s); }
  s.low <<= n; s.low += s.range * v; s.bits_left -= n; ec_test_write(s);
}
EC_FN void ec_terminate(EcCoder &s, int v)
{
  if (s.dry) return;
  s.range -= 2;
  if (v) { s.low += s.range; s.low <<= 7; s.range = 2 << 7; s.bits_left -= 7; }
  else if (s.range >= 256) return;
  else { s.low <<= 1; s.range <<= 1; s.bits_left--; }
  ec_test_write(s);
}
EC_FN void ec_finish(EcCoder &s)
{ // TEncBinCABAC::finish, then byte_alignment() (a 1 bit and zeros up to the byte boundary)
  if (s.dry) return;
  if (s.low >> (32 - s.bits_left)) {
    ec_put_byte(s, (s.buffered_byte + 1) & 0xff);
    ec_put_run(s, 0x00, s.buffered - 1);
    s.low -= 1u << (32 - s.bits_left);
  } else {
    if (s.buffered > 0) ec_put_byte(s, s.buffered_byte & 0xff);
    ec_put_run(s, 0xff, s.buffered - 1);
  }
  s.buffered = 0;
  ec_put_bits(s, s.low >> 8, 24 - s.bits_left);
  ec_put_bits(s, 1, 1);
  if (s.nheld) ec_put_bits(s, 0, 8 - s.nheld);
}

// ---- the picture's records ---------------------------------------------------------------------------------------------
EC_FN const hevcdl_ctu_record &ec_rec_at(const EcCoder &s, const EcPic &p, int x4, int y4, int &z)
{
  z = s.t->r2z[((y4 & 15) << 4) | (x4 & 15)];
  int a = (y4 >> 4) * p.ctus_x + (x4 >> 4);
  if ((unsigned)a >= (unsigned)p.ctus) a = 0;
  return p.recs[a];
}
EC_FN int ec_luma_mode_at(const EcCoder &s, const EcPic &p, int x4, int y4) { int z; const hevcdl_ctu_record &r = ec_rec_at(s, p, x4, y4, z); return r.luma_dir[z]; }
EC_FN int ec_depth_at(const EcCoder &s, const EcPic &p, int x4, int y4) { int z; const hevcdl_ctu_record &r = ec_rec_at(s, p, x4, y4, z); return r.depth[z]; }
EC_FN int ec_abs(int v) { return v < 0 ? -v : v; }

// ---- residual_coding(): TEncSbac::codeCoeffNxN TEncSbac.cpp:1115-1541 -----------------------------------------------------
EC_FN void ec_get_cparam(const EcTables *t, EcCParam &cp, int c, int log2n, int dir_mode)
{ // TComDataCU.cpp:3150-3209 (scan choice), TComChromaFormat.cpp:96-160
  cp.log2 = log2n < 2 ? 2 : (log2n > 5 ? 5 : log2n); cp.n = 1 << cp.log2; cp.ch = c ? 1 : 0; cp.wg = cp.n >> 2;
  cp.scan_type = SCAN_DIAG;
  if (cp.n <= (c ? 4 : 8)) { if (ec_abs(dir_mode - VER) <= 4) cp.scan_type = SCAN_HOR; else if (ec_abs(dir_mode - HOR) <= 4) cp.scan_type = SCAN_VER; }
  if (cp.n == 4) cp.first_sig_ctx = 0;
  else if (cp.n == 8) cp.first_sig_ctx = 9 + ((cp.scan_type != SCAN_DIAG) ? (cp.ch ? 0 : 6) : 0);
  else cp.first_sig_ctx = cp.ch ? 12 : 21;
  cp.scan = t->scan[cp.scan_type][cp.log2 - 2]; cp.scan_cg = t->scan_cg[cp.scan_type][cp.log2 - 2];
}
EC_FN int ec_sig_ctx_inc(const EcTables *t, const EcCParam &cp, int pat, int raster)
{ // TComTrQuant.cpp:2707-2803; raster: the level's position in the block
  const int py = raster >> cp.log2, px = raster - (py << cp.log2);
  if (px + py == 0) return 0;
  int offset;
  if (cp.log2 == 2) offset = t->ctx_ind_map_4x4[(4 * py + px) & 15];
  else {
    int cnt; const int xs = px & 3, ys = py & 3;
    if (pat == 0) cnt = (xs + ys >= 3) ? 0 : ((xs + ys >= 1) ? 1 : 2);
    else if (pat == 1) cnt = (ys >= 2) ? 0 : ((ys >= 1) ? 1 : 2);
    else if (pat == 2) cnt = (xs >= 2) ? 0 : ((xs >= 1) ? 1 : 2);
    else cnt = 2;
    offset = ((((px >> 2) + (py >> 2)) > 0) ? (cp.ch ? 0 : 3) : 0) + cnt;
  }
  return cp.first_sig_ctx + offset;
}
// plane: the record's coefficient array of the component, base: first coefficient of the block, mask: 4095 (luma) / 1023 (chroma), the array's size - 1 -- a block
// of a valid record lies inside the array, a block of a garbage record is moved there
EC_FN void ec_code_coeff(EcCoder &s, uint32_t tools, const int16_t *plane, int base, int mask, int comp, int log2n, int dir_mode, int tskip_flag)
{
  const EcTables *t = s.t;
  const int ch = comp ? 1 : 0;
  EcCParam cp; ec_get_cparam(t, cp, comp, log2n, dir_mode);
  log2n = cp.log2;
  const int n = cp.n, nn = n * n;
  if (base + nn > mask + 1) base = mask + 1 - nn;
  const int16_t *coef = plane + base;            // n x n levels inside the array; base is a multiple of 4 levels, so a group's row of four is one aligned 8-byte word
#define EC_COEF(i) ((int)coef[(i) & (nn - 1)])
  // coefficient groups that hold a level, and how many levels the block holds: one pass over the block's rows, the four levels of a group's row at a time (bit 15 of
  // a 16-bit lane of `lanes` is set where the lane is not zero).  Then the last level in scan order: up the scan until all levels are seen -- no further than the
  // coding loop below comes down again, and a block of content ends early in its scan.
  uint64_t cgf = 0; int scan_last = -1, num_sig = 0;
  for (int y = 0; y < n; y++) for (int gx = 0; gx < cp.wg; gx++) {
    uint64_t four; __builtin_memcpy(&four, coef + y * n + 4 * gx, 8);
    if (!four) continue;
    const uint64_t lanes = (((four & 0x7fff7fff7fff7fffull) + 0x7fff7fff7fff7fffull) | four) & 0x8000800080008000ull;
    cgf |= 1ull << ((y >> 2) * cp.wg + gx); num_sig += __builtin_popcountll(lanes);
  }
  for (int q = 0; q < nn && num_sig > 0; q++) if (EC_COEF(cp.scan[q]) != 0) { scan_last = q; num_sig--; }
  if (scan_last < 0) return;
  const int pos_last = cp.scan[scan_last] & (nn - 1);
  if (n == 4 && (tools & HEVCDL_TOOL_TSKIP)) ec_bin(s, CTX_TSKIP + ch, tskip_flag != 0);      // transform_skip_flag only with transform_skip_enabled_flag (TEncSbac.cpp:1007)
  { // codeLastSignificantXY :1115-1181
    int py = pos_last >> log2n, px = pos_last - (py << log2n);
    if (cp.scan_type == SCAN_VER) { const int tmp = px; px = py; py = tmp; }
    const int gx = t->group_idx[px & 31], gy = t->group_idx[py & 31], gmax = t->group_idx[n - 1], cw = log2n - 2;
    const int off = ch ? 0 : (cw * 3 + ((cw + 1) >> 2)), shift = ch ? cw : ((cw + 3) >> 2);     // TComChromaFormat.h:211-226
    const int bx = CTX_LAST_X + (ch ? 15 : 0) + off, by = CTX_LAST_Y + (ch ? 15 : 0) + off;
    int k;
    for (k = 0; k < gx; k++) ec_bin(s, bx + (k >> shift), 1);
    if (gx < gmax) ec_bin(s, bx + (k >> shift), 0);
    for (k = 0; k < gy; k++) ec_bin(s, by + (k >> shift), 1);
    if (gy < gmax) ec_bin(s, by + (k >> shift), 0);
    if (gx > 3) { const int cnt = (gx - 2) >> 1, v = px - t->min_in_group[gx]; for (int i = cnt - 1; i >= 0; i--) ec_ep(s, (v >> i) & 1); }
    if (gy > 3) { const int cnt = (gy - 2) >> 1, v = py - t->min_in_group[gy]; for (int i = cnt - 1; i >= 0; i--) ec_ep(s, (v >> i) & 1); }
  }
  const int cg_off = CTX_SIG_CG + (ch ? 2 : 0), sig_off = CTX_SIG + (ch ? 28 : 0);
  const int last_set = scan_last >> 4;
  int c1 = 1, sp = scan_last;
  for (int subset = last_set; subset >= 0; subset--) {
    int num_nz = 0, go_rice = 0; const int sub_pos = subset << 4;
    int last_nz = -1, first_nz = 16; uint32_t signs = 0;
    if (sp == scan_last) { const int v = EC_COEF(pos_last); s.absb[0] = (uint16_t)ec_abs(v); num_nz = 1; last_nz = sp; first_nz = sp; signs = v < 0; sp--; }
    const int cgblk = cp.scan_cg[subset] & 63, gy = cgblk >> (log2n - 2), gx = cgblk & (cp.wg - 1);
    const int right = (gx < cp.wg - 1) ? (int)((cgf >> (gy * cp.wg + gx + 1)) & 1) : 0, lower = (gy < cp.wg - 1) ? (int)((cgf >> ((gy + 1) * cp.wg + gx)) & 1) : 0;
    if (subset == last_set || subset == 0) cgf |= 1ull << cgblk;
    else ec_bin(s, cg_off + ((right + lower) != 0), (int)((cgf >> cgblk) & 1));
    if ((cgf >> cgblk) & 1) {
      const int pat = cp.wg <= 1 ? 0 : right + (lower << 1);
      for (int q = 0; q < 16 && sp >= sub_pos; q++, sp--) {
        const int raster = cp.scan[sp] & (nn - 1), v = EC_COEF(raster), sig = v != 0;
        if (sp > sub_pos || subset == 0 || num_nz) ec_bin(s, sig_off + ec_sig_ctx_inc(t, cp, pat, raster), sig);
        if (sig) { s.absb[num_nz & 15] = (uint16_t)ec_abs(v); num_nz++; signs = 2 * signs + (v < 0); if (last_nz == -1) last_nz = sp; first_nz = sp; }
      }
    } else sp = sub_pos - 1;
    if (num_nz > 16) num_nz = 16;
    if (num_nz > 0) {
      const int sign_hidden = (tools & HEVCDL_TOOL_SIGN_HIDE) && (last_nz - first_nz >= 4);
      const int cset = (ch ? 4 : 0) + ((!ch && subset > 0) ? 2 : 0) + (c1 == 0 ? 1 : 0);      // TComChromaFormat.h:243-251
      c1 = 1;
      const int n_c1 = num_nz < 8 ? num_nz : 8; int first_c2 = -1, escape = 0;
      for (int i = 0; i < n_c1; i++) {
        const int sym = s.absb[i] > 1;
        ec_bin(s, CTX_ONE + 4 * cset + c1, sym);
        if (sym) { c1 = 0; if (first_c2 == -1) first_c2 = i; else escape = 1; }
        else if (c1 < 3 && c1 > 0) c1++;
      }
      if (c1 == 0 && first_c2 != -1) { const int sym = s.absb[first_c2] > 2; ec_bin(s, CTX_ABS + cset, sym); if (sym) escape = 1; }
      escape = escape || (num_nz > 8);
      if (sign_hidden) ec_eps(s, signs >> 1, num_nz - 1); else ec_eps(s, signs, num_nz);
      int first_coeff2 = 1;
      if (escape) for (int i = 0; i < num_nz; i++) {
        const int a = s.absb[i], bse = (i < 8) ? (2 + first_coeff2) : 1;
        if (a >= bse) { // xWriteCoefRemainExGolomb :337-394
          int code = a - bse;
          if (code < (3 << go_rice)) { const int len = code >> go_rice; ec_eps(s, (1u << (len + 1)) - 2, len + 1); ec_eps(s, (uint32_t)(code & ((1 << go_rice) - 1)), go_rice); }
          else {
            int len = go_rice; code -= 3 << go_rice;
            for (int k = 0; k < 16 && code >= (1 << len); k++) code -= 1 << (len++);
            ec_eps(s, (1u << (3 + len + 1 - go_rice)) - 2, 3 + len + 1 - go_rice); ec_eps(s, (uint32_t)code, len);
          }
          if (a > (3 << go_rice)) go_rice = go_rice + 1 < 4 ? go_rice + 1 : 4;
        }
        if (a >= 2) first_coeff2 = 0;
      }
    }
  }
#undef EC_COEF
}

// ---- prediction modes ----------------------------------------------------------------------------------------------------
EC_FN void ec_code_luma_dirs(EcCoder &s, const EcPic &p, const EcCu &cu, int npu)
{ // codeIntraDirLumaAng TEncSbac.cpp:643-696, getIntraDirPredictor TComDataCU.cpp:1362-1445
  int preds[4][3], idx[4], dir[4];
  const int pu_size = (cu.part == SIZE_NxN) ? (1 << (cu.log2 - 1)) : (1 << cu.log2);
  for (int j = 0; j < npu; j++) {
    const int px = cu.x + (j & 1) * pu_size, py = cu.y + (j >> 1) * pu_size;
    dir[j] = cu.r->luma_dir[(cu.zbase + j * (cu.nparts >> 2) * (cu.part == SIZE_NxN)) & 255];
    int left = DC, above = DC;
    if (px > p.tx0) left = ec_luma_mode_at(s, p, (px >> 2) - 1, py >> 2);
    if ((py & 63) != 0) above = ec_luma_mode_at(s, p, px >> 2, (py >> 2) - 1);
    if (left == above) {
      if (left > 1) { preds[j][0] = left; preds[j][1] = ((left + 29) % 32) + 2; preds[j][2] = ((left - 1) % 32) + 2; }
      else { preds[j][0] = PLANAR; preds[j][1] = DC; preds[j][2] = VER; }
    } else {
      preds[j][0] = left; preds[j][1] = above;
      preds[j][2] = (left && above) ? PLANAR : ((left + above) < 2 ? VER : DC);
    }
    idx[j] = -1;
    for (int i = 0; i < 3; i++) if (dir[j] == preds[j][i]) idx[j] = i;
    ec_bin(s, CTX_INTRA_PRED, idx[j] != -1);
  }
  for (int j = 0; j < npu; j++) {
    if (idx[j] != -1) { ec_ep(s, idx[j] ? 1 : 0); if (idx[j]) ec_ep(s, idx[j] - 1); }
    else {
      int q0 = preds[j][0], q1 = preds[j][1], q2 = preds[j][2], tmp;
      if (q0 > q1) { tmp = q0; q0 = q1; q1 = tmp; }
      if (q0 > q2) { tmp = q0; q0 = q2; q2 = tmp; }
      if (q1 > q2) { tmp = q1; q1 = q2; q2 = tmp; }
      int d = dir[j];
      d = d > q2 ? d - 1 : d; d = d > q1 ? d - 1 : d; d = d > q0 ? d - 1 : d;
      ec_eps(s, (uint32_t)d, 5);
    }
  }
}
EC_FN void ec_code_chroma_dir(EcCoder &s, const EcCu &cu)
{ // codeIntraDirChroma TEncSbac.cpp:698-726, getAllowedChromaDir TComDataCU.cpp:1334-1353
  const int d = cu.r->chroma_dir[cu.zbase & 255];
  if (d == DM_CHROMA) { ec_bin(s, CTX_CHROMA_PRED, 0); return; }
  ec_bin(s, CTX_CHROMA_PRED, 1);
  const int luma = cu.r->luma_dir[cu.zbase & 255];
  int l0 = PLANAR, l1 = VER, l2 = HOR, l3 = DC, k = 0;
  if (l0 == luma) l0 = 34; else if (l1 == luma) l1 = 34; else if (l2 == luma) l2 = 34; else if (l3 == luma) l3 = 34;
  if (d == l0) k = 0; else if (d == l1) k = 1; else if (d == l2) k = 2; else if (d == l3) k = 3;
  ec_eps(s, (uint32_t)k, 2);
}

// ---- transform tree: TEncEntropy::xEncodeTransform TEncEntropy.cpp:200-398 ---------------------------------------------------
EC_FN int ec_min_tu_log2(const EcCu &cu)
{ // getQuadtreeTULog2MinSizeInCU TComDataCU.cpp:1478-1503 (TU log2 2..5, intra TU depth 3)
  const int split = cu.part == SIZE_NxN; int r;
  if (cu.log2 < 2 + 3 - 1 + split) r = 2; else { r = cu.log2 - (3 - 1 + split); if (r > 5) r = 5; }
  return r;
}
EC_FN void ec_code_qt_cbf(EcCoder &s, const EcCu &cu, const EcTu &tu, int comp, int lowest)
{ // codeQtCbf TEncSbac.cpp:920-995
  const int ctx = comp ? tu.trd : (tu.trd == 0 ? 1 : 0);
  const int w = comp ? (tu.log2 > 2 ? 1 << (tu.log2 - 1) : 4) : (1 << tu.log2);
  const int d = tu.trd + ((!lowest && !(w >= 8)) ? 1 : 0);
  const int z = cu.zbase + (comp ? (tu.log2 > 2 ? tu.zrel : (tu.zrel & ~3)) : tu.zrel);
  ec_bin(s, CTX_QT_CBF + (comp ? 5 : 0) + ctx, (cu.r->cbf[comp][z & 255] >> (d & 7)) & 1);
}
// the transform units of one CU in z-order.  A node's flags (split_transform_flag, the chroma cbf flags of its level) are written when the walk stands on the node's
// first 4x4 partition: for every level from the shallowest one whose node starts here down to the leaf -- the recursive writer's pre-order.
EC_FN void ec_code_transform_tree(EcCoder &s, const EcPic &p, const EcCu &cu)
{
  const int min_log2 = ec_min_tu_log2(cu);
  int zrel = 0;
  for (int it = 0; it < 256 && zrel < cu.nparts; it++) {
    int trd = 0;                                                       // shallowest level whose node starts at zrel
    for (int k = 0; k < 4 && (zrel & ((cu.nparts >> (2 * trd)) - 1)) != 0 && cu.log2 - trd > 2; k++) trd++;
    int covered = 1;
    for (int lvl = 0; lvl < 5; lvl++, trd++) {
      EcTu tu; tu.log2 = cu.log2 - trd; tu.trd = trd; tu.zrel = zrel;
      const int np = cu.nparts >> (2 * trd), z = (cu.zbase + zrel) & 255;
      // a valid record splits a 64x64 block and never a 4x4 one; garbage must not either (the flag itself is not coded in both cases)
      const int subdiv = tu.log2 > 5 ? 1 : (tu.log2 <= 2 ? 0 : cu.r->tr_idx[z] > trd);
      if (cu.part == SIZE_NxN && trd == 0) { }
      else if (tu.log2 > 5) { }
      else if (tu.log2 == 2) { }
      else if (tu.log2 == min_log2) { }
      else ec_bin(s, CTX_SUBDIV + 5 - tu.log2, subdiv);
      const int first = trd == 0;
      for (int comp = 1; comp < 3; comp++)
        if (first || tu.log2 > 2)
          if (first || ((cu.r->cbf[comp][z] >> ((trd - 1) & 7)) & 1)) ec_code_qt_cbf(s, cu, tu, comp, !subdiv);
      if (subdiv) continue;                                            // the first child starts at the same partition
      ec_code_qt_cbf(s, cu, tu, 0, 1);
      for (int comp = 0; comp < 3; comp++) {
        if (comp && !(tu.log2 > 2 || (zrel & 3) == 3)) continue;
        if (!((cu.r->cbf[comp][z] >> (trd & 7)) & 1)) continue;
        const int zc = comp ? (tu.log2 > 2 ? zrel : (zrel & ~3)) : zrel, zabs = (cu.zbase + zc) & 255;
        const int l2 = comp ? (tu.log2 > 2 ? tu.log2 - 1 : 2) : tu.log2;
        int mode;
        if (!comp) mode = cu.r->luma_dir[zabs];
        else { const int m = cu.r->chroma_dir[zabs]; mode = m == DM_CHROMA ? cu.r->luma_dir[(cu.zbase + (zc & ~3)) & 255] : m; }
        if (comp == 0) ec_code_coeff(s, p.tools, cu.r->coeff_y, zabs * 16, 4095, 0, l2, mode, cu.r->tskip[0][zabs]);
        else ec_code_coeff(s, p.tools, comp == 1 ? cu.r->coeff_cb : cu.r->coeff_cr, zabs * 4, 1023, comp, l2, mode, cu.r->tskip[comp][zabs]);
      }
      zrel += np > 0 ? np : 1;
      covered = 0;
      break;
    }
    if (covered) zrel++;                                               // not reached: a level-4 node (4x4) is always a leaf
  }
}

// ---- sao(): TEncSbac::codeSAOBlkParam / codeSAOOffsetParam TEncSbac.cpp:1543-1720 ----------------------------------------------
EC_FN void ec_code_sao_offset(EcCoder &s, int comp, const hevcdl_sao_offset &p, int max_off)
{
  const int first = comp != 2;
  if (first) {   // anything but "new" is written as off: a merge reaches this only where its candidate does not exist (ec_code_sao_blk), and sao() cannot say that
    if (p.mode != 1) ec_bin(s, CTX_SAO_TYPE, 0);
    else { ec_bin(s, CTX_SAO_TYPE, 1); ec_ep(s, p.type == 4 ? 0 : 1); }
  }
  if (p.mode != 1) return;
  int off[4], k = 0;
  const int ncls = p.type == 4 ? 4 : 5;
  for (int i = 0; i < ncls; i++) { if (p.type != 4 && i == 2) continue; off[k++] = p.offset[p.type == 4 ? ((p.aux & 31) + i) & 31 : i]; }
  for (int i = 0; i < 4; i++) { // codeSaoMaxUvlc, maximum (1 << (min(bitDepth, 10) - 5)) - 1: 7 at 8 bits, 31 at 10
    int a = off[i] < 0 ? (off[i] < -max_off ? max_off : -off[i]) : (off[i] > max_off ? max_off : off[i]);      // a coded offset never exceeds the maximum: the loop below is bounded by it
    if (a == 0) ec_ep(s, 0);
    else { ec_ep(s, 1); for (int j = 0; j < a - 1; j++) ec_ep(s, 1); if (a < max_off) ec_ep(s, 0); }
  }
  if (p.type == 4) { for (int i = 0; i < 4; i++) if (off[i]) ec_ep(s, off[i] < 0); ec_eps(s, (uint32_t)p.aux, 5); }
  else if (first) ec_eps(s, (uint32_t)p.type, 2);
}
EC_FN void ec_code_sao_blk(EcCoder &s, const hevcdl_sao_blk &b, int left_avail, int above_avail, int max_off)
{
  int is_left = 0, is_above = 0;
  if (left_avail) { is_left = b.c[0].mode == 2 && b.c[0].type == 0; ec_bin(s, CTX_SAO_MERGE, is_left); }
  if (above_avail && !is_left) { is_above = b.c[0].mode == 2 && b.c[0].type == 1; ec_bin(s, CTX_SAO_MERGE, is_above); }
  if (!is_left && !is_above) for (int comp = 0; comp < 3; comp++) ec_code_sao_offset(s, comp, b.c[comp], max_off);
}

// ---- coding quadtree of one CTU: xEncodeCU TEncCu.cpp:1167-1271 (I slice: no skip / pred-mode flags) -----------------------------
// The 8x8 blocks of the CTU in z-order; a block already covered by a coded CU, or outside the picture, is passed over.  Standing on an uncovered block, the walk goes
// down from the shallowest level whose node starts here: split_cu_flag where the node lies inside the picture, the CU itself where it is not split.
EC_FN void ec_code_cu_tree(EcCoder &s, const EcPic &p, int cx, int cy)
{
  int a = cy * p.ctus_x + cx;
  if ((unsigned)a >= (unsigned)p.ctus) return;
  const hevcdl_ctu_record &r = p.recs[a];
  const int x0 = cx * 64, y0 = cy * 64;
  int next_z = 0;
  for (int z = 0; z < 256; z += 4) {
    if (z < next_z) continue;
    int zx = 0, zy = 0;                                                // position of the 8x8 block (z-scan: bits of x and y interleaved)
    for (int b = 0; b < 4; b++) { zx |= ((z >> (2 * b)) & 1) << b; zy |= ((z >> (2 * b + 1)) & 1) << b; }
    const int x = x0 + zx * 4, y = y0 + zy * 4;
    if (x >= p.W || y >= p.H) continue;
    int depth = 0;
    for (int k = 0; k < 3 && (z & ((256 >> (2 * depth)) - 1)) != 0; k++) depth++;
    for (int lvl = 0; lvl < 4 && depth < 4; lvl++, depth++) {
      const int size = 64 >> depth;
      int boundary = 0;
      if (x + size <= p.W && y + size <= p.H) {
        if (depth < 3) {
          int sctx = 0;
          if (x > p.tx0) sctx += ec_depth_at(s, p, (x >> 2) - 1, y >> 2) > depth;
          if (y > p.ty0) sctx += ec_depth_at(s, p, x >> 2, (y >> 2) - 1) > depth;
          ec_bin(s, CTX_SPLIT + sctx, r.depth[z] > depth);
        }
      } else boundary = 1;
      if (depth < 3 && (depth < r.depth[z] || boundary)) continue;
      EcCu cu; cu.x = x; cu.y = y; cu.log2 = 6 - depth; cu.depth = depth; cu.zbase = z; cu.nparts = 256 >> (2 * depth); cu.part = r.part_size[z]; cu.r = &r;
      if (depth == 3) ec_bin(s, CTX_PART_SIZE, cu.part == SIZE_2Nx2N);
      ec_code_luma_dirs(s, p, cu, cu.part == SIZE_NxN ? 4 : 1);
      ec_code_chroma_dir(s, cu);
      ec_code_transform_tree(s, p, cu);
      next_z = z + cu.nparts;
      break;
    }
  }
}

// The CTUs of sub-stream k of a picture: tile k in raster order of the tile grid (1 x 1: the picture), or CTU row k with WaveFrontSynchro.  col_bd / row_bd: tile
// boundaries in CTUs (hevcdl_tile_bounds).  k is clamped to the grid.
EC_FN void ec_unit_rect(int wpp, int tcols, const int *col_bd, const int *row_bd, int ctus_x, int k, int &cx0, int &cx1, int &cy0, int &cy1)
{
  if (wpp) { cx0 = 0; cx1 = ctus_x; cy0 = k; cy1 = k + 1; return; }
  if (tcols < 1) tcols = 1;
  if (tcols > 20) tcols = 20;
  int tr = k / tcols, tc = k - tr * tcols;
  if (tr < 0) tr = 0;
  if (tr > 21) tr = 21;
  if (tc < 0) tc = 0;
  cx0 = col_bd[tc]; cx1 = col_bd[tc + 1]; cy0 = row_bd[tr]; cy1 = row_bd[tr + 1];
}

// Does sub-stream k of `units` end a slice?  slice_units: sub-streams (tiles) per slice -- 0: one slice a picture; SliceMode 1 (a grid of one column, a slice per row
// of it): 1; SliceMode 3: SliceArgument, the last slice taking what is left (TEncSlice::calculateBoundingCtuTsAddrForSlice, FIXED_NUMBER_OF_TILES).
EC_FN int ec_ends_slice(int slice_units, int k, int units) { return k == units - 1 || (slice_units > 0 && (k + 1) % slice_units == 0); }
// Does it end a slice SEGMENT (SliceSegmentMode 1 over WaveFrontSynchro rows, 3 over tiles)?  segment_units: sub-streams (CTU rows, tiles) per segment, counted from the
// start of the slice -- a segment never runs past the end of its slice (TEncSlice.cpp:1285-1288) -- 0: no dependent segments, and the answer is ec_ends_slice's.  The end of
// a segment is coded as the end of a slice: end_of_slice_segment_flag 1 alone.
EC_FN int ec_ends_segment(int slice_units, int segment_units, int k, int units)
{
  if (ec_ends_slice(slice_units, k, units)) return 1;
  if (segment_units <= 0) return 0;
  const int in_slice = slice_units > 0 ? k % slice_units : k;
  return (in_slice + 1) % segment_units == 0;
}
// ... and p.slice_end_ctu of that sub-stream, the CTUs [cx0, cx1) x [cy0, cy1)
EC_FN int ec_slice_end_ctu(int ends_slice, int ctus_x, int cx1, int cy1) { return ends_slice ? (cy1 - 1) * ctus_x + cx1 - 1 : -1; }

// one CTU of a sub-stream: its SAO parameters, its coding quadtree, end_of_slice_segment_flag 0 unless it is the last of its slice (TEncSlice.cpp:1075-1136)
EC_FN void ec_code_ctu(EcCoder &s, const EcPic &p, int cx, int cy)
{
  const int a = cy * p.ctus_x + cx;
  if ((unsigned)a >= (unsigned)p.ctus) return;
  if (p.sao) ec_code_sao_blk(s, p.sao[a], cx * 64 > p.tx0, cy * 64 > p.ty0, p.max_sao_offset);      // merge candidates stay inside the tile (TComPic::getSAOMergeAvailability)
  ec_code_cu_tree(s, p, cx, cy);
  if (a != p.ctus - 1 && a != p.slice_end_ctu) ec_terminate(s, 0);
}
// the CTUs [cx0, cx1) x [cy0, cy1) in raster order, then the sub-stream's end: terminating 1 bin, coder flush, byte_alignment().  The contexts are the caller's
// (slice-start contexts, or the stored ones of a WaveFrontSynchro row).
EC_FN void ec_code_substream(EcCoder &s, const EcPic &p, int cx0, int cx1, int cy0, int cy1)
{
  ec_start(s);
  for (int cy = cy0; cy < cy1; cy++) for (int cx = cx0; cx < cx1; cx++) ec_code_ctu(s, p, cx, cy);
  ec_terminate(s, 1);
  ec_finish(s);
}

} // namespace hevcdl_ec
#endif
