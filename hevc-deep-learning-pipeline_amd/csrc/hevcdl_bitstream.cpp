// hevcdl_bitstream.cpp -- HEVC bitstream writer for the pictures this library decides.
// Host C++ (no GPU): the byte-producing half of the entropy coder is strictly serial per slice and tiny next to the
// decision kernel (a 2160p frame is ~80 KB of output).  SAO parameters (hevcdl_sao_frames) are optional: without them
// the stream signals SAO off.  This file writes everything around the slice data; the slice data itself (arithmetic coder, SAO, CU, TU and residual syntax) is
// entropy_coder.h, the source the device kernel compiles too, instantiated here once (SliceCoder).
//
// Mirrors, for the reference's all-intra configuration (one slice per picture, IntraPeriod 1, parameter sets with every
// picture, deblocking on with zero offsets, sign data hiding, transform skip):
//   access unit / NAL order, start codes     TEncGOP.cpp:1751-1756, AnnexBwrite.h:55-80, NALwrite.cpp:47-120
//   VPS / SPS / PPS / slice segment header   TEncCavlc.cpp:677-753, 500-675, 189-341, 755-1109 (+ codePTL :1111-1229)
//   slice data: sub-streams, CTU loop        TEncSlice.cpp:985-1170 (the syntax below it: entropy_coder.h)
// Pinned byte for byte by tests/golden/rd_*.npz:bitstream_nosao (the reference run with --SAO=0) and :bitstream (default run).
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>
#include "hevcdl.h"
#include "hevcdl_dev.h"
#include "entropy_tables.h"
#define EC_FN static inline      // the coder's functions are this file's own: no calls through the library's symbol table, inlined as the compiler would its own
#include "entropy_coder.h"
#include "picture_hash_core.h"
#include "source_core.h"

namespace {

// the coder's types, functions and tables (entropy_coder.h, entropy_tables.h)
using namespace hevcdl_ec;

// ---- bit writer (TComOutputBitstream) --------------------------------------------------------------------------------
struct BitOut {
  std::vector<uint8_t> b; uint32_t held = 0; int nheld = 0;
  void write(uint32_t v, int n) { for (int i = n - 1; i >= 0; i--) { held = (held << 1) | ((v >> i) & 1u); if (++nheld == 8) { b.push_back((uint8_t)held); held = 0; nheld = 0; } } }
  void flag(int v) { write(v ? 1u : 0u, 1); }
  void ue(uint32_t v) { uint32_t t = v + 1; int len = 0; while ((t >> len) > 1) len++; write(0, len); write(t, len + 1); }
  void se(int v) { ue(v <= 0 ? (uint32_t)(-2 * v) : (uint32_t)(2 * v - 1)); }
  void align_zero() { if (nheld) write(0, 8 - nheld); }
  void trailing() { write(1, 1); align_zero(); }          // rbsp_trailing_bits / byte_alignment()
};

// NAL unit: 2-byte header, emulation prevention (NALwrite.cpp:47-120), Annex B start code (AnnexBwrite.h:55-80)
void put_nal(std::vector<uint8_t> &out, int type, const std::vector<uint8_t> &rbsp, bool long_start_code)
{
  if (long_start_code) out.push_back(0);
  out.push_back(0); out.push_back(0); out.push_back(1);
  out.push_back((uint8_t)(type << 1)); out.push_back(1);          // nuh_layer_id 0, nuh_temporal_id_plus1 1
  int zeros = 0;
  for (uint8_t v : rbsp) {
    if (zeros >= 2 && v <= 3) { out.push_back(3); zeros = 0; }
    out.push_back(v);
    zeros = v == 0 ? zeros + 1 : 0;
  }
  if (!rbsp.empty() && rbsp.back() == 0) out.push_back(3);          // NALwrite.cpp:112-118 (cabac_zero_words guard)
}

// MD5 (RFC 1321) of a byte string: the decoded picture hash of the reference (libmd5 + TComPicYuvMD5.cpp:88-130) is the plain
// MD5 of each colour plane, rows packed, samples as 1 byte (8-bit) or 2 bytes little endian.
struct Md5 {
  uint32_t h[4] = { 0x67452301u, 0xefcdab89u, 0x98badcfeu, 0x10325476u }; uint64_t len = 0; uint8_t buf[64]; int fill = 0;
  static uint32_t rol(uint32_t v, int s) { return (v << s) | (v >> (32 - s)); }
  static const uint32_t *sines()
  { // K[i] = floor(2^32 * |sin(i + 1)|), RFC 1321 section 3.4, computed once
    struct Table { uint32_t k[64]; Table() { for (int i = 0; i < 64; i++) k[i] = (uint32_t)(int64_t)floor(fabs(sin((double)(i + 1))) * 4294967296.0); } };
    static const Table t;                                               // initialised once, thread-safe
    return t.k;
  }
  const uint32_t *K = sines();
  void block(const uint8_t *p)
  {
    uint32_t m[16], a = h[0], b = h[1], c = h[2], d = h[3];
    memcpy(m, p, 64);                                                   // little-endian hosts only, like the rest of the byte packing here
#define MD5_STEP(F, a, b, c, d, g, i, s) a = b + rol(a + F(b, c, d) + K[i] + m[g], s)
#define MD5_F(x, y, z) (z ^ (x & (y ^ z)))
#define MD5_G(x, y, z) (y ^ (z & (x ^ y)))
#define MD5_H(x, y, z) (x ^ y ^ z)
#define MD5_I(x, y, z) (y ^ (x | ~z))
#define MD5_ROUND(F, g0, gs, i0, s0, s1, s2, s3) \
    for (int q = 0; q < 4; q++) { const int i = i0 + 4 * q; \
      MD5_STEP(F, a, b, c, d, (g0 + gs * (i - i0)) & 15, i, s0); MD5_STEP(F, d, a, b, c, (g0 + gs * (i + 1 - i0)) & 15, i + 1, s1); \
      MD5_STEP(F, c, d, a, b, (g0 + gs * (i + 2 - i0)) & 15, i + 2, s2); MD5_STEP(F, b, c, d, a, (g0 + gs * (i + 3 - i0)) & 15, i + 3, s3); }
    MD5_ROUND(MD5_F, 0, 1, 0, 7, 12, 17, 22)
    MD5_ROUND(MD5_G, 1, 5, 16, 5, 9, 14, 20)
    MD5_ROUND(MD5_H, 5, 3, 32, 4, 11, 16, 23)
    MD5_ROUND(MD5_I, 0, 7, 48, 6, 10, 15, 21)
#undef MD5_ROUND
#undef MD5_STEP
#undef MD5_F
#undef MD5_G
#undef MD5_H
#undef MD5_I
    h[0] += a; h[1] += b; h[2] += c; h[3] += d;
  }
  void update(const uint8_t *p, size_t n)
  {
    len += n;
    while (n) {
      if (!fill && n >= 64) { block(p); p += 64; n -= 64; continue; }   // whole blocks straight from the caller's memory
      const size_t take = std::min<size_t>(n, 64 - fill); memcpy(buf + fill, p, take); fill += (int)take; p += take; n -= take; if (fill == 64) { block(buf); fill = 0; }
    }
  }
  void final(uint8_t out[16])
  {
    const uint64_t bits = len * 8; const uint8_t pad = 0x80, zero = 0;
    update(&pad, 1); while (fill != 56) update(&zero, 1);
    uint8_t l[8]; for (int i = 0; i < 8; i++) l[i] = (uint8_t)(bits >> (8 * i));
    update(l, 8);
    for (int i = 0; i < 4; i++) for (int j = 0; j < 4; j++) out[4 * i + j] = (uint8_t)(h[i] >> (8 * j));
  }
};

void profile_tier_level(BitOut &w, int level_idc, int bit_depth)
{ // codePTL / codeProfileTier: Profile main => idc 1, compatibility flags 1 and 2; main10 at 10 bits => idc 2, flag 2 only (TAppEncTop.cpp:120-135)
  w.write(0, 2); w.flag(0); w.write(bit_depth > 8 ? 2 : 1, 5);
  w.write(bit_depth > 8 ? 0x20000000u : 0x60000000u, 32);
  w.flag(0); w.flag(0); w.flag(0); w.flag(0);                       // progressive / interlaced / non-packed / frame-only
  w.write(0, 16); w.write(0, 16); w.write(0, 11); w.flag(0);        // reserved_zero_43bits, inbld_flag
  w.write((uint32_t)level_idc, 8);
}

} // namespace

extern "C" hevcdl_status hevcdl_stream_config_default(hevcdl_stream_config *cfg, int width, int height, int qp)
{
  if (!cfg || width <= 0 || height <= 0 || (width & 7) || (height & 7) || qp < 0 || qp > 51) return HEVCDL_ERR_INVALID_ARG;
  memset(cfg, 0, sizeof *cfg);
  cfg->struct_size = sizeof *cfg; cfg->width = width; cfg->height = height; cfg->qp = qp;
  cfg->level_idc = 186;                    // Level 6.2 (general_level_idc = 30 * level)
  cfg->tile_columns = 1; cfg->tile_rows = 1; cfg->bit_depth = 8; cfg->tile_uniform_spacing = 1; cfg->lf_across_tiles = 1; cfg->wavefront = 0;
  cfg->tools = HEVCDL_TOOLS_REFERENCE; cfg->rewrite_param_sets = 1;
  return HEVCDL_OK;
}

extern "C" hevcdl_status hevcdl_picture_md5(const hevcdl_stream_config *cfg, const void *picture, uint8_t digest[48])
{ // calcMD5 TComPicYuvMD5.cpp:88-130: one digest per colour plane
  if (!cfg || cfg->struct_size != sizeof *cfg || !picture || !digest) return HEVCDL_ERR_INVALID_ARG;
  if (cfg->width <= 0 || cfg->height <= 0 || (cfg->width & 7) || (cfg->height & 7)) return HEVCDL_ERR_INVALID_ARG;
  if (cfg->bit_depth != 8 && cfg->bit_depth != 10) return HEVCDL_ERR_UNSUPPORTED;
  const size_t bps = cfg->bit_depth > 8 ? 2 : 1, ysz = (size_t)cfg->width * cfg->height * bps, csz = ysz / 4;
  const uint8_t *p = (const uint8_t *)picture;
  for (int c = 0; c < 3; c++) { Md5 m; m.update(p + (c == 0 ? 0 : (c == 1 ? ysz : ysz + csz)), c ? csz : ysz); m.final(digest + 16 * c); }
  return HEVCDL_OK;
}

extern "C" hevcdl_status hevcdl_write_digest_sei(const uint8_t digest[48], uint8_t *out, size_t capacity, size_t *out_len)
{ // SEIDecodedPictureHash 1 (MD5): suffix SEI NAL after the slice (TEncGOP.cpp:1938-1960, SEIwrite.cpp xWriteSEIDecodedPictureHash)
  if (!digest || !out || !out_len) return HEVCDL_ERR_INVALID_ARG;
  BitOut w;
  w.write(132, 8); w.write(49, 8); w.write(0, 8);          // payload type decoded_picture_hash, size 1 + 3 * 16, hash_type 0 = MD5
  for (int i = 0; i < 48; i++) w.write(digest[i], 8);
  w.trailing();
  std::vector<uint8_t> nal;
  put_nal(nal, 40, w.b, false);                           // SUFFIX_SEI_NUT
  *out_len = nal.size();
  if (nal.size() > capacity) return HEVCDL_ERR_INVALID_ARG;
  memcpy(out, nal.data(), nal.size());
  return HEVCDL_OK;
}

extern "C" hevcdl_status hevcdl_picture_hash(const hevcdl_stream_config *cfg, const void *picture, int method, uint8_t digest[48], int *plane_bytes)
{ // calcMD5 / calcCRC / calcChecksum TComPicYuvMD5.cpp:88-180: one digest per colour plane
  if (method == 1) { if (plane_bytes) *plane_bytes = 16; return hevcdl_picture_md5(cfg, picture, digest); }
  if (!cfg || cfg->struct_size != sizeof *cfg || !picture || !digest) return HEVCDL_ERR_INVALID_ARG;
  if (cfg->width <= 0 || cfg->height <= 0 || (cfg->width & 7) || (cfg->height & 7)) return HEVCDL_ERR_INVALID_ARG;
  if (cfg->bit_depth != 8 && cfg->bit_depth != 10) return HEVCDL_ERR_UNSUPPORTED;
  if (method != 2 && method != 3) return HEVCDL_ERR_UNSUPPORTED;
  const int wide = cfg->bit_depth > 8;
  const size_t ysz = (size_t)cfg->width * cfg->height;
  for (int c = 0; c < 3; c++) {
    const int pw = c ? cfg->width / 2 : cfg->width, ph = c ? cfg->height / 2 : cfg->height;
    const size_t off = c == 0 ? 0 : (c == 1 ? ysz : ysz + ysz / 4);
    auto sample = [&](int x, int y) -> unsigned { const size_t i = off + (size_t)y * pw + x; return wide ? ((const uint16_t *)picture)[i] : ((const uint8_t *)picture)[i]; };
    if (method == 2) { // CRC-16-CCITT over the bytes of the samples, most significant bit first, low byte first (:89-127)
      unsigned crc = 0xffff;
      auto feed = [&](unsigned byte) { for (int b = 0; b < 8; b++) { const unsigned msb = (crc >> 15) & 1, bit = (byte >> (7 - b)) & 1; crc = (((crc << 1) + bit) & 0xffff) ^ (msb * 0x1021); } };
      for (int y = 0; y < ph; y++) for (int x = 0; x < pw; x++) { const unsigned v = sample(x, y); feed(v & 0xff); if (wide) feed(v >> 8); }
      for (int b = 0; b < 16; b++) { const unsigned msb = (crc >> 15) & 1; crc = ((crc << 1) & 0xffff) ^ (msb * 0x1021); }
      digest[2 * c] = (uint8_t)(crc >> 8); digest[2 * c + 1] = (uint8_t)crc;
    } else {           // checksum: sum of the bytes, each xor-ed with a mask of its position (:141-165)
      uint32_t sum = 0;
      for (int y = 0; y < ph; y++) for (int x = 0; x < pw; x++) {
        const unsigned v = sample(x, y), mask = ((unsigned)x & 0xff) ^ ((unsigned)y & 0xff) ^ ((unsigned)x >> 8) ^ ((unsigned)y >> 8);
        sum += ((v & 0xff) ^ (mask & 0xff));
        if (wide) sum += ((v >> 8) ^ (mask & 0xff));
      }
      for (int k = 0; k < 4; k++) digest[4 * c + k] = (uint8_t)(sum >> (24 - 8 * k));
    }
  }
  if (plane_bytes) *plane_bytes = method == 2 ? 2 : 4;
  return HEVCDL_OK;
}

// TEST AND DIAGNOSTIC: one plane by the chunked forms of csrc/picture_hash_core.h (the source of the device kernels, report_kernel.hip), serially on the CPU
extern "C" int hevcdl_report_chunk_bytes(void) { return HEVCDL_REPORT_CHUNK_BYTES; }
extern "C" hevcdl_status hevcdl_plane_hash_host(const void *plane, int width, int height, int bit_depth, int method, int chunk_bytes, uint8_t *digest16)
{
  if (!plane || !digest16 || width < 1 || height < 1 || width > (1 << 20) || height > (1 << 20) || (long long)width * height > (1ll << 28) || method < 1 || method > 3) return HEVCDL_ERR_INVALID_ARG;
  if (bit_depth < 8 || bit_depth > 16) return HEVCDL_ERR_UNSUPPORTED;
  memset(digest16, 0, 16);
  hevcdl_ph::plane_hash_chunked((const uint8_t *)plane, (uint32_t)width, (uint32_t)height, bit_depth > 8 ? 2 : 1, method, chunk_bytes > 0 ? (uint64_t)chunk_bytes : HEVCDL_REPORT_CHUNK_BYTES, digest16);
  return HEVCDL_OK;
}

extern "C" hevcdl_status hevcdl_write_hash_sei(int method, const uint8_t *digest, uint8_t *out, size_t capacity, size_t *out_len)
{ // SEIwrite.cpp xWriteSEIDecodedPictureHash: hash_type u(8) = method - 1, then per plane 16 bytes (MD5) / u(16) (CRC) / u(32) (checksum)
  if (method == 1) return hevcdl_write_digest_sei(digest, out, capacity, out_len);
  if (!digest || !out || !out_len || (method != 2 && method != 3)) return HEVCDL_ERR_INVALID_ARG;
  const int pb = method == 2 ? 2 : 4;
  BitOut w;
  w.write(132, 8); w.write(1 + 3 * pb, 8); w.write((uint32_t)(method - 1), 8);
  for (int i = 0; i < 3 * pb; i++) w.write(digest[i], 8);
  w.trailing();
  std::vector<uint8_t> nal;
  put_nal(nal, 40, w.b, false);
  *out_len = nal.size();
  if (nal.size() > capacity) return HEVCDL_ERR_INVALID_ARG;
  memcpy(out, nal.data(), nal.size());
  return HEVCDL_OK;
}

extern "C" hevcdl_status hevcdl_write_picture_hash_sei(const hevcdl_stream_config *cfg, const void *picture, uint8_t *out, size_t capacity, size_t *out_len)
{ // the digests of `picture`, then the SEI above
  if (!cfg || cfg->struct_size != sizeof *cfg || !picture || !out || !out_len) return HEVCDL_ERR_INVALID_ARG;
  if (cfg->width <= 0 || cfg->height <= 0 || (cfg->width & 7) || (cfg->height & 7)) return HEVCDL_ERR_INVALID_ARG;
  uint8_t d[48];
  const hevcdl_status st = hevcdl_picture_md5(cfg, picture, d);
  if (st != HEVCDL_OK) return st;
  return hevcdl_write_digest_sei(d, out, capacity, out_len);
}

extern "C" size_t hevcdl_access_unit_bound(int width, int height)
{ // worst case is far below the raw picture size x 2 (the arithmetic coder cannot expand 16-bit levels by more than that)
  return (size_t)width * (size_t)height * 3 + 4096;
}
extern "C" size_t hevcdl_access_unit_bound_slices(int width, int height, const hevcdl_slice_layout *layout)
{ // a slice NAL unit more costs its start code, NAL header and slice header: under 32 bytes without entry points; those are counted in the one-slice bound already
  size_t slices = 0;
  if (layout && layout->mode == 1) slices = 22;
  if (layout && layout->mode == 3) slices = (size_t)((440 + std::max(layout->argument, 1) - 1) / std::max(layout->argument, 1));
  return hevcdl_access_unit_bound(width, height) + 32 * slices;
}
extern "C" size_t hevcdl_access_unit_bound_segments(int width, int height, const hevcdl_slice_layout *layout, const hevcdl_segment_layout *segments)
{ // a dependent segment's NAL unit costs less than a slice's (its header stops behind the address); at most one per CTU row (mode 1) or per tile (mode 3)
  size_t n = 0;
  if (segments && segments->mode == 1) n = (size_t)((std::max(height, 0) + 63) >> 6);
  if (segments && segments->mode == 3) n = 440;
  return hevcdl_access_unit_bound_slices(width, height, layout) + 32 * n;
}

namespace {
// what every form of the access-unit writer derives from the stream configuration before it writes a byte
// tcols x trows, col_bd, row_bd: the grid of sub-streams -- the cfg's tiles, or with SliceMode 1 one column of row slices (`tiled`, what the PPS says, is then 0).
// slice_units: sub-streams per slice (ec_ends_slice), 0 = one slice a picture; lf_slices: pps_loop_filter_across_slices_enabled_flag; seg_units: sub-streams per
// dependent slice segment (ec_ends_segment), 0 = none
struct AuSetup { int dbk_off, dbk_beta, dbk_tc, dbk_control, dbk_override_enabled; hevcdl_dbk_choice slice; int bd, tcols, trows, tiled, wpp, uniform, col_bd[21], row_bd[23], slice_units, lf_slices, seg_units; };
hevcdl_status au_setup(const hevcdl_stream_config *cfg, AuSetup &u, const hevcdl_dbk_choice *choice = nullptr, const hevcdl_slice_layout *layout = nullptr,
                       const hevcdl_segment_layout *segments = nullptr)
{
  if (!cfg || cfg->struct_size != sizeof *cfg) return HEVCDL_ERR_INVALID_ARG;
  if (cfg->width <= 0 || cfg->height <= 0 || (cfg->width & 7) || (cfg->height & 7) || cfg->qp < 0 || cfg->qp > 51) return HEVCDL_ERR_INVALID_ARG;
  if (cfg->lf_beta_offset_div2 < -6 || cfg->lf_beta_offset_div2 > 6 || cfg->lf_tc_offset_div2 < -6 || cfg->lf_tc_offset_div2 > 6) return HEVCDL_ERR_INVALID_ARG;
  if (!hevcdl_src::window_fits(cfg->width, cfg->height, cfg->conf_win_left, cfg->conf_win_right, cfg->conf_win_top, cfg->conf_win_bottom)) return HEVCDL_ERR_INVALID_ARG;      // negative or odd offsets, nothing left of the picture
  // deblocking control as TEncTop.cpp:1007-1035 sets it.  LoopFilterOffsetInPPS 1 without DeblockingFilterMetric (the cfg's values; no choice): no override in the slice
  // header; the PPS carries the disabled flag and the offsets, and the control fields are present when any of them differs from the inferred values.  Either key the other
  // way (the choice says so): override enabled
  u.dbk_override_enabled = choice && choice->override_enabled != 0;
  u.dbk_off = cfg->loop_filter_disable != 0;
  u.dbk_beta = u.dbk_off ? 0 : cfg->lf_beta_offset_div2; u.dbk_tc = u.dbk_off ? 0 : cfg->lf_tc_offset_div2;
  u.dbk_control = u.dbk_override_enabled || u.dbk_off || u.dbk_beta != 0 || u.dbk_tc != 0;
  // the slice's own values: the picture's choice -- the cfg's values repeated behind an override flag of 1 (TEncSlice.cpp:388-404), or what the metric picked
  // (TEncGOP.cpp:3284-3300) -- or, without one, the PPS's
  const hevcdl_dbk_choice pps = { 0, 0, u.dbk_off, u.dbk_beta, u.dbk_tc };
  u.slice = choice ? *choice : pps;
  u.slice.override_flag = u.slice.override_flag != 0; u.slice.disabled = u.slice.disabled != 0;
  if (u.slice.disabled) u.slice.beta_offset_div2 = u.slice.tc_offset_div2 = 0;            // (not coded)
  if (u.slice.beta_offset_div2 < -6 || u.slice.beta_offset_div2 > 6 || u.slice.tc_offset_div2 < -6 || u.slice.tc_offset_div2 > 6) return HEVCDL_ERR_INVALID_ARG;
  if (u.slice.override_flag ? !u.dbk_override_enabled
                            : (u.slice.disabled != pps.disabled || u.slice.beta_offset_div2 != pps.beta_offset_div2 || u.slice.tc_offset_div2 != pps.tc_offset_div2)) return HEVCDL_ERR_INVALID_ARG;
  u.bd = cfg->bit_depth;
  if (u.bd != 8 && u.bd != 10) return HEVCDL_ERR_UNSUPPORTED;
  if (!HEVCDL_TOOLS_SUPPORTED(cfg->tools)) return HEVCDL_ERR_UNSUPPORTED;
  u.tcols = cfg->tile_columns; u.trows = cfg->tile_rows; u.tiled = u.tcols * u.trows > 1;
  if (u.tcols < 1 || u.trows < 1 || u.tcols > 20 || u.trows > 22) return HEVCDL_ERR_INVALID_ARG;
  u.wpp = cfg->wavefront != 0;
  if (u.wpp && u.tiled) return HEVCDL_ERR_UNSUPPORTED;       // the reference refuses the pair outside the high-throughput profile (TAppEncCfg.cpp xCheckParameter)
  u.uniform = cfg->tile_uniform_spacing != 0;
  if (hevcdl_tile_bounds((cfg->width + 63) >> 6, u.tcols, u.uniform, cfg->tile_column_width, u.tiled ? 4 : 1, u.col_bd) ||      // TComPicSym.cpp:380-392
      hevcdl_tile_bounds((cfg->height + 63) >> 6, u.trows, u.uniform, cfg->tile_row_height, 1, u.row_bd)) return HEVCDL_ERR_INVALID_ARG;
  u.slice_units = 0; u.lf_slices = 1;                        // SliceMode 0: LFCrossSliceBoundaryFlag is 1 whatever the cfg says (TAppEncTop.cpp:278-281)
  if (layout && layout->mode != 0) {
    if (layout->mode == 2) return HEVCDL_ERR_UNSUPPORTED;    // slices by bytes
    const int cx = (cfg->width + 63) >> 6, cy = (cfg->height + 63) >> 6;
    u.lf_slices = layout->lf_across_slices != 0;
    if (layout->mode == 1) { // whole CTU rows: one sub-stream per slice, the grid a column of them
      if (u.tiled || u.wpp || layout->argument < 1 || layout->argument % cx != 0) return HEVCDL_ERR_INVALID_ARG;
      const int rows = layout->argument / cx, n = (cy + rows - 1) / rows;
      if (n > 22) return HEVCDL_ERR_INVALID_ARG;
      u.tcols = 1; u.trows = n; u.col_bd[0] = 0; u.col_bd[1] = cx;
      for (int i = 0; i <= n; i++) u.row_bd[i] = std::min(i * rows, cy);
      u.slice_units = 1;
    } else if (layout->mode == 3) {
      if (!u.tiled || layout->argument < 1) return HEVCDL_ERR_INVALID_ARG;
      u.slice_units = layout->argument;
    } else return HEVCDL_ERR_INVALID_ARG;
  }
  u.seg_units = 0;
  if (segments && segments->mode != 0) { // dependent slice segments start where the coder is initialised anyway: at a wavefront row, at a tile
    if (segments->mode == 2) return HEVCDL_ERR_UNSUPPORTED;  // segments by bytes
    const int cx = (cfg->width + 63) >> 6;
    if (segments->mode == 1) {
      if (!u.wpp || u.slice_units != 0 || segments->argument < 1 || segments->argument % cx != 0) return HEVCDL_ERR_INVALID_ARG;
      u.seg_units = segments->argument / cx;                 // CTU rows a segment
    } else if (segments->mode == 3) {
      if (!u.tiled || segments->argument < 1) return HEVCDL_ERR_INVALID_ARG;
      u.seg_units = segments->argument;                      // tiles a segment, counted from the start of the slice
    } else return HEVCDL_ERR_INVALID_ARG;
  }
  return HEVCDL_OK;
}
struct SubStream { const uint8_t *p; size_t n; };
uint32_t count_emulations(const SubStream &b)
{ // TComOutputBitstream::countStartCodeEmulations TComBitStream.cpp:198-228: emulation prevention bytes this byte string will receive
  uint32_t cnt = 0; int zeros = 0;
  for (size_t i = 0; i < b.n; i++) { const uint8_t v = b.p[i]; if (zeros >= 2 && v <= 3) { cnt++; zeros = 0; } zeros = v == 0 ? zeros + 1 : 0; }
  return cnt;
}

// Everything of an access unit around the slice data: parameter sets, slice segment header with the entry points, byte_alignment(), NAL packing.  sub: the
// sub-streams of the picture (one per tile / per CTU row / one), each ending byte aligned.
void au_assemble(const hevcdl_stream_config *cfg, const AuSetup &u, int poc, const std::vector<SubStream> &sub, std::vector<uint8_t> &au)
{
  const int bd = u.bd, tcols = u.tcols, trows = u.trows, tiled = u.tiled, wpp = u.wpp, uniform = u.uniform, dbk_off = u.dbk_off, dbk_beta = u.dbk_beta, dbk_tc = u.dbk_tc, dbk_control = u.dbk_control;
  const int *col_bd = u.col_bd, *row_bd = u.row_bd;
  const bool write_ps = poc == 0 || cfg->rewrite_param_sets != 0;                       // TEncGOP.cpp:1751: the first picture, or every IRAP with ReWriteParamSetsFlag
  if (write_ps) { // VPS  TEncCavlc.cpp:677-753
    BitOut w;
    w.write(0, 4); w.flag(1); w.flag(1); w.write(0, 6); w.write(0, 3); w.flag(1); w.write(0xffff, 16);
    profile_tier_level(w, cfg->level_idc, bd);
    w.flag(1); w.ue(0); w.ue(0); w.ue(0);            // sub_layer_ordering_info_present, max_dec_pic_buffering_minus1, num_reorder, max_latency_plus1
    w.write(0, 6); w.ue(0); w.flag(0); w.flag(0);    // vps_max_layer_id, num_layer_sets_minus1, timing_info_present, extension
    w.trailing();
    put_nal(au, 32, w.b, true);
  }
  if (write_ps) { // SPS  TEncCavlc.cpp:500-675
    BitOut w;
    w.write(0, 4); w.write(0, 3); w.flag(1);
    profile_tier_level(w, cfg->level_idc, bd);
    w.ue(0); w.ue(1); w.ue((uint32_t)cfg->width); w.ue((uint32_t)cfg->height);
    w.flag(1); w.ue((uint32_t)cfg->conf_win_left / 2); w.ue((uint32_t)cfg->conf_win_right / 2); w.ue((uint32_t)cfg->conf_win_top / 2); w.ue((uint32_t)cfg->conf_win_bottom / 2);   // conformance window always present (as the reference writes it): left, right, top, bottom in chroma units (TEncCavlc.cpp:526-535)
    w.ue((uint32_t)bd - 8); w.ue((uint32_t)bd - 8); w.ue(4);     // bit depths - 8, log2_max_pic_order_cnt_lsb_minus4 (8 bits)
    w.flag(1); w.ue(0); w.ue(0); w.ue(0);
    w.ue(0); w.ue(3); w.ue(0); w.ue(3); w.ue(2); w.ue(2);    // CB 8..64, TB 4..32, TU depth inter/intra 3
    w.flag(0); w.flag(1); w.flag(cfg->sao_enabled); w.flag(0); // scaling list, AMP, SAO, PCM
    w.ue(2);                                         // two (empty) short-term RPS of the all-intra GOP table
    w.ue(0); w.ue(0);
    w.flag(0); w.ue(0); w.ue(0);                     // RPS 1: inter_ref_pic_set_prediction_flag 0, no pictures
    w.flag(0); w.flag(1); w.flag((cfg->tools & HEVCDL_TOOL_STRONG_INTRA) != 0); w.flag(0); w.flag(0);     // long-term, temporal MVP, strong intra smoothing, VUI, extension
    w.trailing();
    put_nal(au, 33, w.b, true);
  }
  if (write_ps) { // PPS  TEncCavlc.cpp:189-341
    BitOut w;
    w.ue(0); w.ue(0); w.flag(u.seg_units > 0); w.flag(0); w.write(0, 3); w.flag((cfg->tools & HEVCDL_TOOL_SIGN_HIDE) != 0); w.flag(1); w.ue(3); w.ue(3);   // ids, dependent_slice_segments_enabled_flag, ... sign_data_hiding_enabled_flag, cabac_init_present_flag, ...
    w.se(0); w.flag(0); w.flag((cfg->tools & HEVCDL_TOOL_TSKIP) != 0); w.flag(0);        // init_qp_minus26 0, constrained intra, transform skip, cu_qp_delta
    w.se(0); w.se(0); w.flag(0); w.flag(0); w.flag(0); w.flag(0);      // chroma qp offsets, slice chroma offsets present, weighted (bi)pred, transquant bypass
    w.flag(tiled); w.flag(wpp);                      // tiles_enabled_flag, entropy_coding_sync_enabled_flag (TEncCavlc.cpp:226-227)
    if (tiled) { // :228-246
      w.ue((uint32_t)tcols - 1); w.ue((uint32_t)trows - 1); w.flag(uniform);
      if (!uniform) {
        for (int i = 0; i < tcols - 1; i++) w.ue((uint32_t)(col_bd[i + 1] - col_bd[i]) - 1);    // column_width_minus1
        for (int i = 0; i < trows - 1; i++) w.ue((uint32_t)(row_bd[i + 1] - row_bd[i]) - 1);    // row_height_minus1
      }
      w.flag(cfg->lf_across_tiles != 0);             // loop_filter_across_tiles_enabled_flag
    }
    w.flag(u.lf_slices); w.flag(dbk_control);        // pps_loop_filter_across_slices_enabled_flag, deblocking_filter_control_present  (TEncCavlc.cpp:247-259)
    if (dbk_control) { w.flag(u.dbk_override_enabled); w.flag(dbk_off); if (!dbk_off) { w.se(dbk_beta); w.se(dbk_tc); } }      // deblocking_filter_override_enabled_flag, pps_deblocking_filter_disabled_flag, pps_beta / tc_offset_div2
    w.flag(0); w.flag(0); w.ue(0); w.flag(0); w.flag(0);
    w.trailing();
    put_nal(au, 34, w.b, true);
  }
  // slice segments: header TEncCavlc.cpp:755-1109, data TEncSlice.cpp:985-1170; one NAL unit per slice (TEncGOP.cpp's loop over the slices of a picture), the sub-streams
  // [k0, k1) in each -- and with dependent slice segments one NAL unit per segment, the sub-streams [s0, s1) of its slice: a segment that does not start its slice is
  // dependent, its header stops behind the address and goes on with its own entry points
  const int n_sub = (int)sub.size(), per = u.slice_units > 0 ? u.slice_units : n_sub, ctus_x = (cfg->width + 63) >> 6, ctus = ctus_x * ((cfg->height + 63) >> 6);
  int addr_bits = 0; while (ctus > (1 << addr_bits)) addr_bits++;
  bool first_nal = !write_ps;
  for (int k0 = 0; k0 < n_sub; k0 += per) {
    const int k1 = std::min(k0 + per, n_sub), seg = u.seg_units > 0 ? u.seg_units : k1 - k0;
    for (int s0 = k0; s0 < k1; s0 += seg) {
      const int s1 = std::min(s0 + seg, k1), dependent = s0 > k0;
      BitOut w;
      const int idr = poc == 0;
      int addr = 0;                                    // slice_segment_address: raster address of the segment's first CTU
      if (s0 > 0) { int cx0, cx1, cy0, cy1; ec_unit_rect(wpp, tcols, col_bd, row_bd, ctus_x, s0, cx0, cx1, cy0, cy1); addr = cy0 * ctus_x + cx0; }
      w.flag(addr == 0); w.flag(0); w.ue(0);           // first_slice_segment_in_pic, no_output_of_prior_pics, pps id
      if (u.seg_units > 0 && addr > 0) w.flag(dependent);      // dependent_slice_segment_flag: under the PPS's flag, in every header but the picture's first (TEncCavlc.cpp:787-790)
      if (addr > 0) w.write((uint32_t)addr, addr_bits);
      if (!dependent) {
        w.ue(2);                                       // slice_type I
        if (!idr) { w.write((uint32_t)poc & 255u, 8); w.flag(0); w.flag(0); w.ue(0); w.ue(0); w.flag(1); }   // POC lsb, RPS coded in the header (empty), slice_temporal_mvp_enabled
        if (cfg->sao_enabled) { w.flag(1); w.flag(1); }
        w.se(cfg->qp - 26);
        if (dbk_control) { // TEncCavlc.cpp:1080-1095
          if (u.dbk_override_enabled) w.flag(u.slice.override_flag);
          if (u.slice.override_flag) { w.flag(u.slice.disabled); if (!u.slice.disabled) { w.se(u.slice.beta_offset_div2); w.se(u.slice.tc_offset_div2); } }
        }
        if (u.lf_slices && (cfg->sao_enabled || !u.slice.disabled)) w.flag(1);     // slice_loop_filter_across_slices_enabled_flag: only under the PPS's flag and when an in-loop filter is on (TEncCavlc.cpp:1097-1104)
      }
      if (tiled || wpp) { // entry points: TEncCavlc::codeTilesWPPEntryPoint :1207-1240; a size counts the emulation prevention bytes of its sub-stream
        std::vector<uint32_t> size((size_t)(s1 - s0 - 1));
        uint32_t max_size = 0;
        for (int i = s0; i + 1 < s1; i++) { size[(size_t)(i - s0)] = (uint32_t)sub[(size_t)i].n + count_emulations(sub[(size_t)i]); if (size[(size_t)(i - s0)] > max_size) max_size = size[(size_t)(i - s0)]; }
        int len_m1 = 0; while (max_size >= (1u << (len_m1 + 1))) len_m1++;
        w.ue((uint32_t)size.size());
        if (!size.empty()) { w.ue((uint32_t)len_m1); for (uint32_t v : size) w.write(v - 1, len_m1 + 1); }
      }
      w.trailing();                                    // byte_alignment()
      for (int i = s0; i < s1; i++) w.b.insert(w.b.end(), sub[(size_t)i].p, sub[(size_t)i].p + sub[(size_t)i].n);
      put_nal(au, idr ? 19 : 21, w.b, first_nal);      // IDR_W_RADL, then CRA (DecodingRefreshType 1); the first NAL unit of an access unit carries the zero_byte
      first_nal = false;
    }
  }
}

// The slice data of one picture on the host: entropy_coder.h instantiated once, for every entry point below.  One sub-stream per tile, tiles in raster order, CTUs in
// raster order inside a tile (TEncSlice.cpp:1030-1145), or one per CTU row with WaveFrontSynchro.  Every sub-stream starts from the slice-start contexts and ends with a
// terminating 1 bin (end_of_slice_segment_flag of the last CTU / end_of_subset_one_bit of the others), the coder flush and byte_alignment().  With WaveFrontSynchro a row
// starts from the contexts behind the SECOND CTU of the row above when the picture is at least two CTUs wide (:1127-1130): the sub-streams are coded in order, so those
// contexts are kept where they arise (the device, where rows run side by side, needs a first launch for them).
struct SliceCoder {
  const AuSetup &u; const int qp; EcPic p; EcCoder s;
  uint8_t ctx[EC_SYNC_BYTES], start[NUM_CTX], sync[NUM_CTX]; uint16_t absb[16]; int started = -1;
  SliceCoder(const hevcdl_stream_config *cfg, const AuSetup &setup, const hevcdl_ctu_record *records, const hevcdl_sao_blk *sao) : u(setup), qp(cfg->qp)
  {
    p.recs = records; p.sao = sao; p.W = cfg->width; p.H = cfg->height; p.ctus_x = (p.W + 63) >> 6; p.ctus_y = (p.H + 63) >> 6; p.ctus = p.ctus_x * p.ctus_y; p.tx0 = p.ty0 = 0;
    p.tools = cfg->tools; p.max_sao_offset = (1 << ((u.bd < 10 ? u.bd : 10) - 5)) - 1;
    memset(&s, 0, sizeof s);
    s.t = &ec_tables(); s.ctx = ctx; s.absb = absb;
  }
  SliceCoder(const SliceCoder &) = delete;
  int substreams() const { return u.wpp ? p.ctus_y : u.tcols * u.trows; }
  // Sub-stream k into out[0, cap): s.pos is its true length, s.overflow says that it did not fit.  Sub-streams are taken in order; the same k once more (into a larger
  // region) starts from the same contexts.  -> the CTUs of the sub-stream
  int code(int k, uint8_t *out, uint32_t cap)
  {
    int cx0, cx1, cy0, cy1;
    ec_unit_rect(u.wpp, u.tcols, u.col_bd, u.row_bd, p.ctus_x, k, cx0, cx1, cy0, cy1);
    if (!u.wpp) { p.tx0 = cx0 * 64; p.ty0 = cy0 * 64; }
    p.slice_end_ctu = ec_slice_end_ctu(ec_ends_segment(u.wpp ? 0 : u.slice_units, u.seg_units, k, substreams()), p.ctus_x, cx1, cy1);
    if (k != started) {
      if (u.wpp && k > 0 && p.ctus_x > 1) memcpy(start, sync, NUM_CTX); else ec_init_contexts(start, s.t, qp);
      started = k;
    }
    memcpy(ctx, start, NUM_CTX);
    s.out = out; s.cap = cap;
    ec_start(s);
    for (int cy = cy0; cy < cy1; cy++) for (int cx = cx0; cx < cx1; cx++) {
      ec_code_ctu(s, p, cx, cy);
      if (u.wpp && cx == 1) memcpy(sync, ctx, NUM_CTX);
    }
    ec_terminate(s, 1);                              // TEncSlice.cpp:1136
    ec_finish(s);
    return (cx1 - cx0) * (cy1 - cy0);
  }
};

// First-pass room of the packed slice data below, per CTU: two thirds of a byte per sample (content at QP 32 codes to about 70 bytes per CTU).  Never the worst case
// (EC_DEFAULT_CAPACITY_PER_CTU: 83 MB at 2160p): the coder reports the true length of a sub-stream that did not fit, and that one is coded again.
enum { HOST_FIRST_PASS_PER_CTU = 4096 };

// The sub-streams of one picture one behind the other: sub[k] points into `data`.  The memory is not initialised, so what is never written is never touched.
struct PackedSliceData { std::unique_ptr<uint8_t[]> data; std::vector<SubStream> sub; };
void code_slice_data_packed(const hevcdl_stream_config *cfg, const AuSetup &u, const hevcdl_ctu_record *records, const hevcdl_sao_blk *sao, PackedSliceData &d)
{
  SliceCoder c(cfg, u, records, sao);
  const int n = c.substreams();
  size_t room = (size_t)c.p.ctus * HOST_FIRST_PASS_PER_CTU + EC_REGION_SLACK, at = 0, left = (size_t)c.p.ctus;
  d.data.reset(new uint8_t[room]);
  std::vector<uint32_t> size((size_t)n);
  for (int k = 0; k < n; k++) {
    const int ctus = c.code(k, d.data.get() + at, (uint32_t)std::min<size_t>(room - at, 0xffffffffu));
    left -= (size_t)ctus;
    if (c.s.overflow) { // room for exactly this sub-stream and the first-pass share of those behind it; what is coded already moves
      room = at + c.s.pos + left * HOST_FIRST_PASS_PER_CTU + EC_REGION_SLACK;
      std::unique_ptr<uint8_t[]> more(new uint8_t[room]);
      memcpy(more.get(), d.data.get(), at);
      d.data.swap(more);
      c.code(k, d.data.get() + at, c.s.pos);
    }
    size[(size_t)k] = c.s.pos; at += c.s.pos;
  }
  d.sub.resize((size_t)n);
  at = 0;
  for (int k = 0; k < n; k++) { d.sub[(size_t)k].p = d.data.get() + at; d.sub[(size_t)k].n = size[(size_t)k]; at += size[(size_t)k]; }
}
} // namespace

extern "C" hevcdl_status hevcdl_write_access_unit(const hevcdl_stream_config *cfg, int poc, const hevcdl_ctu_record *records, const hevcdl_sao_blk *sao,
                                                 uint8_t *out, size_t capacity, size_t *out_len)
{
  return hevcdl_write_access_unit_dbk(cfg, poc, records, sao, nullptr, out, capacity, out_len);
}

extern "C" hevcdl_status hevcdl_write_access_unit_dbk(const hevcdl_stream_config *cfg, int poc, const hevcdl_ctu_record *records, const hevcdl_sao_blk *sao,
                                                     const hevcdl_dbk_choice *choice, uint8_t *out, size_t capacity, size_t *out_len)
{
  return hevcdl_write_access_unit_slices(cfg, nullptr, poc, records, sao, choice, out, capacity, out_len);
}

extern "C" hevcdl_status hevcdl_write_access_unit_slices(const hevcdl_stream_config *cfg, const hevcdl_slice_layout *layout, int poc, const hevcdl_ctu_record *records,
                                                        const hevcdl_sao_blk *sao, const hevcdl_dbk_choice *choice, uint8_t *out, size_t capacity, size_t *out_len)
{
  return hevcdl_write_access_unit_segments(cfg, layout, nullptr, poc, records, sao, choice, out, capacity, out_len);
}

extern "C" hevcdl_status hevcdl_write_access_unit_segments(const hevcdl_stream_config *cfg, const hevcdl_slice_layout *layout, const hevcdl_segment_layout *segments, int poc,
                                                          const hevcdl_ctu_record *records, const hevcdl_sao_blk *sao, const hevcdl_dbk_choice *choice, uint8_t *out, size_t capacity, size_t *out_len)
{
  if (!cfg || cfg->struct_size != sizeof *cfg || !records || !out || !out_len || poc < 0) return HEVCDL_ERR_INVALID_ARG;
  AuSetup u;
  if ((cfg->sao_enabled != 0) != (sao != nullptr)) return HEVCDL_ERR_INVALID_ARG;         // SAO parameters go with sample_adaptive_offset_enabled_flag
  const hevcdl_status st = au_setup(cfg, u, choice, layout, segments);
  if (st != HEVCDL_OK) return st;
  PackedSliceData d;
  code_slice_data_packed(cfg, u, records, sao, d);
  const std::vector<SubStream> &ss = d.sub;
  std::vector<uint8_t> au;
  au_assemble(cfg, u, poc, ss, au);
  *out_len = au.size();
  if (au.size() > capacity) return HEVCDL_ERR_INVALID_ARG;
  memcpy(out, au.data(), au.size());
  return HEVCDL_OK;
}

// ---- slice data coded apart from the access unit, and the access unit around slice data that exists already ---------------------------------------------

extern "C" hevcdl_status hevcdl_slice_data_layout(const hevcdl_stream_config *cfg, int capacity_per_ctu, int *n_substreams, size_t *picture_bytes,
                                                 uint32_t *offsets_opt, uint32_t *capacities_opt)
{
  return hevcdl_slice_data_layout_slices(cfg, nullptr, capacity_per_ctu, n_substreams, picture_bytes, offsets_opt, capacities_opt);
}

extern "C" hevcdl_status hevcdl_slice_data_layout_slices(const hevcdl_stream_config *cfg, const hevcdl_slice_layout *layout, int capacity_per_ctu, int *n_substreams, size_t *picture_bytes,
                                                        uint32_t *offsets_opt, uint32_t *capacities_opt)
{
  return hevcdl_slice_data_layout_segments(cfg, layout, nullptr, capacity_per_ctu, n_substreams, picture_bytes, offsets_opt, capacities_opt);
}

extern "C" hevcdl_status hevcdl_slice_data_layout_segments(const hevcdl_stream_config *cfg, const hevcdl_slice_layout *layout, const hevcdl_segment_layout *segments, int capacity_per_ctu,
                                                          int *n_substreams, size_t *picture_bytes, uint32_t *offsets_opt, uint32_t *capacities_opt)
{
  AuSetup u;
  const hevcdl_status st = au_setup(cfg, u, nullptr, layout, segments);
  if (st != HEVCDL_OK) return st;
  if (!n_substreams || !picture_bytes) return HEVCDL_ERR_INVALID_ARG;
  const int cpc = capacity_per_ctu <= 0 ? EC_DEFAULT_CAPACITY_PER_CTU : capacity_per_ctu;
  if ((cpc & 3) || cpc > (1 << 20)) return HEVCDL_ERR_INVALID_ARG;
  const int ctus_x = (cfg->width + 63) >> 6, ctus_y = (cfg->height + 63) >> 6;
  const int n = u.wpp ? ctus_y : u.tcols * u.trows;
  size_t off = 0;
  for (int k = 0; k < n; k++) {
    int cx0, cx1, cy0, cy1;
    ec_unit_rect(u.wpp, u.tcols, u.col_bd, u.row_bd, ctus_x, k, cx0, cx1, cy0, cy1);
    const size_t cap = (size_t)(cx1 - cx0) * (cy1 - cy0) * cpc + EC_REGION_SLACK;
    if (off + cap + EC_REGION_GAP > 0xfffffff0u) return HEVCDL_ERR_INVALID_ARG;
    if (offsets_opt) offsets_opt[k] = (uint32_t)off;
    if (capacities_opt) capacities_opt[k] = (uint32_t)cap;
    off += cap + EC_REGION_GAP;
  }
  *n_substreams = n; *picture_bytes = off;
  return HEVCDL_OK;
}

extern "C" hevcdl_status hevcdl_code_slice_data_host(const hevcdl_stream_config *cfg, const hevcdl_ctu_record *records, const hevcdl_sao_blk *sao_opt, int n_frames,
                                                    int capacity_per_ctu, uint8_t *out, size_t out_capacity, uint32_t *sizes, uint32_t *overflow)
{
  return hevcdl_code_slice_data_host_slices(cfg, nullptr, records, sao_opt, n_frames, capacity_per_ctu, out, out_capacity, sizes, overflow);
}

extern "C" hevcdl_status hevcdl_code_slice_data_host_slices(const hevcdl_stream_config *cfg, const hevcdl_slice_layout *layout, const hevcdl_ctu_record *records, const hevcdl_sao_blk *sao_opt,
                                                           int n_frames, int capacity_per_ctu, uint8_t *out, size_t out_capacity, uint32_t *sizes, uint32_t *overflow)
{
  return hevcdl_code_slice_data_host_segments(cfg, layout, nullptr, records, sao_opt, n_frames, capacity_per_ctu, out, out_capacity, sizes, overflow);
}

extern "C" hevcdl_status hevcdl_code_slice_data_host_segments(const hevcdl_stream_config *cfg, const hevcdl_slice_layout *layout, const hevcdl_segment_layout *segments,
                                                             const hevcdl_ctu_record *records, const hevcdl_sao_blk *sao_opt, int n_frames, int capacity_per_ctu, uint8_t *out,
                                                             size_t out_capacity, uint32_t *sizes, uint32_t *overflow)
{
  if (!records || !out || !sizes || !overflow || n_frames < 0) return HEVCDL_ERR_INVALID_ARG;
  AuSetup u;
  hevcdl_status st = au_setup(cfg, u, nullptr, layout, segments);
  if (st != HEVCDL_OK) return st;
  if ((cfg->sao_enabled != 0) != (sao_opt != nullptr)) return HEVCDL_ERR_INVALID_ARG;
  int n_sub = 0; size_t pic_bytes = 0;
  uint32_t off[512], cap[512];                      // at most 20 x 22 tiles, or 8192 / 64 CTU rows
  if (((cfg->height + 63) >> 6) > 512) return HEVCDL_ERR_UNSUPPORTED;
  st = hevcdl_slice_data_layout_segments(cfg, layout, segments, capacity_per_ctu, &n_sub, &pic_bytes, off, cap);
  if (st != HEVCDL_OK) return st;
  if (out_capacity / (pic_bytes ? pic_bytes : 1) < (size_t)n_frames) return HEVCDL_ERR_INVALID_ARG;
  const size_t ctus = (size_t)((cfg->width + 63) >> 6) * ((cfg->height + 63) >> 6);
  for (int f = 0; f < n_frames; f++) {
    SliceCoder c(cfg, u, records + (size_t)f * ctus, sao_opt ? sao_opt + (size_t)f * ctus : nullptr);
    for (int k = 0; k < n_sub; k++) {
      c.code(k, out + (size_t)f * pic_bytes + off[k], cap[k]);
      sizes[(size_t)f * n_sub + k] = c.s.pos; overflow[(size_t)f * n_sub + k] = c.s.overflow;
    }
  }
  return HEVCDL_OK;
}

extern "C" hevcdl_status hevcdl_write_access_unit_from_slice_data(const hevcdl_stream_config *cfg, int poc, const uint8_t *data, const uint32_t *sizes, int n_substreams,
                                                                 uint8_t *out, size_t capacity, size_t *out_len)
{
  return hevcdl_write_access_unit_from_slice_data_dbk(cfg, poc, data, sizes, n_substreams, nullptr, out, capacity, out_len);
}

extern "C" hevcdl_status hevcdl_write_access_unit_from_slice_data_dbk(const hevcdl_stream_config *cfg, int poc, const uint8_t *data, const uint32_t *sizes, int n_substreams,
                                                                     const hevcdl_dbk_choice *choice, uint8_t *out, size_t capacity, size_t *out_len)
{
  return hevcdl_write_access_unit_from_slice_data_slices(cfg, nullptr, poc, data, sizes, n_substreams, choice, out, capacity, out_len);
}

extern "C" hevcdl_status hevcdl_write_access_unit_from_slice_data_slices(const hevcdl_stream_config *cfg, const hevcdl_slice_layout *layout, int poc, const uint8_t *data,
                                                                        const uint32_t *sizes, int n_substreams, const hevcdl_dbk_choice *choice, uint8_t *out, size_t capacity, size_t *out_len)
{
  return hevcdl_write_access_unit_from_slice_data_segments(cfg, layout, nullptr, poc, data, sizes, n_substreams, choice, out, capacity, out_len);
}

extern "C" hevcdl_status hevcdl_write_access_unit_from_slice_data_segments(const hevcdl_stream_config *cfg, const hevcdl_slice_layout *layout, const hevcdl_segment_layout *segments, int poc,
                                                                          const uint8_t *data, const uint32_t *sizes, int n_substreams, const hevcdl_dbk_choice *choice, uint8_t *out,
                                                                          size_t capacity, size_t *out_len)
{
  if (!data || !sizes || !out || !out_len || poc < 0) return HEVCDL_ERR_INVALID_ARG;
  AuSetup u;
  const hevcdl_status st = au_setup(cfg, u, choice, layout, segments);
  if (st != HEVCDL_OK) return st;
  if (n_substreams != (u.wpp ? (cfg->height + 63) >> 6 : u.tcols * u.trows)) return HEVCDL_ERR_INVALID_ARG;
  std::vector<SubStream> ss((size_t)n_substreams);
  size_t at = 0;
  for (int i = 0; i < n_substreams; i++) { ss[(size_t)i].p = data + at; ss[(size_t)i].n = sizes[i]; at += sizes[i]; }
  std::vector<uint8_t> au;
  au_assemble(cfg, u, poc, ss, au);
  *out_len = au.size();
  if (au.size() > capacity) return HEVCDL_ERR_INVALID_ARG;
  memcpy(out, au.data(), au.size());
  return HEVCDL_OK;
}

// internal (hevcdl_dev.h): the sub-stream grid of a stream configuration and a slice layout, for the device coder's parameter block
extern "C" int hevcdl_substream_grid(const hevcdl_stream_config *cfg, const hevcdl_slice_layout *layout, const hevcdl_segment_layout *segments, int *cols, int *rows, int col_bd[21],
                                     int row_bd[23], int *slice_units, int *segment_units)
{
  AuSetup u;
  const hevcdl_status st = au_setup(cfg, u, nullptr, layout, segments);
  if (st != HEVCDL_OK) return st;
  *cols = u.tcols; *rows = u.trows; *slice_units = u.slice_units; *segment_units = u.seg_units;
  memset(col_bd, 0, 21 * sizeof(int)); memset(row_bd, 0, 23 * sizeof(int));
  memcpy(col_bd, u.col_bd, (size_t)(u.tcols + 1) * sizeof(int)); memcpy(row_bd, u.row_bd, (size_t)(u.trows + 1) * sizeof(int));
  return HEVCDL_OK;
}

// internal (hevcdl_dev.h): the packed sub-streams of one picture, coded on the host -- what the picture pipeline falls back to for a picture whose sub-stream overflowed
// its region on the device (the same coder with all the room it asks for).  Returns 0, or -1 when `capacity` is too small or `out` is null: sizes and *total are set
// either way (the coder counts what it cannot store), so a first call sizes the buffer of the second.
extern "C" int hevcdl_host_writer_slice_data(const hevcdl_stream_config *cfg, const hevcdl_slice_layout *layout, const hevcdl_segment_layout *segments, const hevcdl_ctu_record *records,
                                             const hevcdl_sao_blk *sao, uint8_t *out, size_t capacity, uint32_t *sizes, size_t *total)
{
  AuSetup u;
  if (au_setup(cfg, u, nullptr, layout, segments) != HEVCDL_OK || !records || !sizes || !total) return -2;
  if (!out) capacity = 0;
  SliceCoder c(cfg, u, records, sao);
  size_t at = 0;
  for (int k = 0; k < c.substreams(); k++) {
    const size_t room = at < capacity ? capacity - at : 0;
    c.code(k, room ? out + at : nullptr, (uint32_t)std::min<size_t>(room, 0xffffffffu));
    sizes[k] = c.s.pos; at += c.s.pos;
  }
  *total = at;
  return at > capacity || !out ? -1 : 0;
}

// ---- source and output formats on the host (csrc/source_core.h: the source the device kernels compile too; no GPU needed) -------------------------------------------
extern "C" hevcdl_status hevcdl_source_format_default(hevcdl_source_format *fmt, const hevcdl_config *cfg)
{
  if (!fmt || !cfg) return HEVCDL_ERR_INVALID_ARG;
  memset(fmt, 0, sizeof *fmt);
  fmt->struct_size = sizeof *fmt; fmt->source_width = cfg->width; fmt->source_height = cfg->height; fmt->input_bit_depth = fmt->output_bit_depth = cfg->bit_depth;
  return HEVCDL_OK;
}

extern "C" hevcdl_status hevcdl_padded_size(int source_width, int source_height, int mode, int pad_x, int pad_y, int *width, int *height)
{ // TAppEncCfg.cpp:1569-1617; the minimum CU of this path is 8 (MaxCUHeight 64 >> (MaxPartitionDepth 4 - 1))
  if (!width || !height || source_width < 2 || source_height < 2 || (source_width & 1) || (source_height & 1)) return HEVCDL_ERR_INVALID_ARG;
  if (mode == 3) return HEVCDL_ERR_UNSUPPORTED;                           // explicit ConfWin* offsets: another path
  if (mode < 0 || mode > 3) return HEVCDL_ERR_INVALID_ARG;
  int px = 0, py = 0;
  if (mode == 1) { px = (8 - source_width % 8) % 8; py = (8 - source_height % 8) % 8; }
  if (mode == 2) { px = pad_x; py = pad_y; }
  if (px < 0 || py < 0 || (px & 1) || (py & 1)) return HEVCDL_ERR_INVALID_ARG;      // the window's offsets are in chroma units
  if (px > 16384 || py > 16384 || ((source_width + px) & 7) || ((source_height + py) & 7)) return HEVCDL_ERR_INVALID_ARG;    // mode 0 with a size that is no multiple of 8; mode 2 with a padding that does not reach one
  *width = source_width + px; *height = source_height + py;
  return HEVCDL_OK;
}

// every rule of a source format against a coded size: the size and depth rules of format_fits, a known file format, the plane order, the explicit window (1 / 0)
extern "C" int hevcdl_source_format_fits(const hevcdl_source_format *fmt, int coded_width, int coded_height)
{
  if (!fmt || fmt->struct_size != sizeof *fmt) return 0;
  if (!hevcdl_src::format_fits(fmt->source_width, fmt->source_height, fmt->input_bit_depth, fmt->output_bit_depth, coded_width, coded_height)) return 0;
  if (!hevcdl_src::chroma_format_known(fmt->chroma_format) || fmt->colour_space < 0 || fmt->colour_space > 1) return 0;
  if (fmt->colour_space && hevcdl_src::chroma_format_id(fmt->chroma_format) == hevcdl_src::FMT_400) return 0;      // nothing to swap (the reference needs chroma planes for the conversion)
  if (!hevcdl_src::window_fits(coded_width, coded_height, fmt->conf_win_left, fmt->conf_win_right, fmt->conf_win_top, fmt->conf_win_bottom)) return 0;      // odd or negative offsets, a window of no samples
  const bool window = (fmt->conf_win_left | fmt->conf_win_right | fmt->conf_win_top | fmt->conf_win_bottom) != 0;
  if (window && (coded_width != fmt->source_width || coded_height != fmt->source_height)) return 0;               // ConformanceWindowMode 3 pads nothing
  return 1;
}
// no field of the file's layout is set: the functions of before this struct had them, run as they were
extern "C" int hevcdl_source_format_plain(const hevcdl_source_format *fmt)
{
  return hevcdl_src::chroma_format_id(fmt->chroma_format) == hevcdl_src::FMT_420 && !fmt->colour_space && !(fmt->conf_win_left | fmt->conf_win_right | fmt->conf_win_top | fmt->conf_win_bottom);
}
// the output frame's luma size: the source size (the coded picture minus the padding), or the explicit window
extern "C" void hevcdl_source_window_size(const hevcdl_source_format *fmt, int *ww, int *wh)
{
  *ww = fmt->source_width - fmt->conf_win_left - fmt->conf_win_right; *wh = fmt->source_height - fmt->conf_win_top - fmt->conf_win_bottom;
}

static bool source_format_ok(const hevcdl_source_format *fmt) { return fmt && hevcdl_source_format_fits(fmt, fmt->source_width, fmt->source_height); }
extern "C" size_t hevcdl_source_frame_bytes(const hevcdl_source_format *fmt)
{ return source_format_ok(fmt) ? hevcdl_src::picture_samples_fmt(fmt->source_width, fmt->source_height, fmt->chroma_format) * (fmt->input_bit_depth > 8 ? 2 : 1) : 0; }
extern "C" size_t hevcdl_output_frame_bytes(const hevcdl_source_format *fmt)
{
  if (!source_format_ok(fmt)) return 0;
  int ww, wh; hevcdl_source_window_size(fmt, &ww, &wh);
  return hevcdl_src::picture_samples(ww, wh) * (fmt->output_bit_depth > 8 ? 2 : 1);
}

extern "C" hevcdl_status hevcdl_load_source_host(const hevcdl_source_format *fmt, int coded_width, int coded_height, int internal_bit_depth, const void *src, int n_frames, void *coded_out)
{
  if (!fmt || fmt->struct_size != sizeof *fmt || !src || !coded_out || n_frames < 0 || internal_bit_depth < 8 || internal_bit_depth > 16) return HEVCDL_ERR_INVALID_ARG;
  if (!hevcdl_source_format_fits(fmt, coded_width, coded_height)) return HEVCDL_ERR_INVALID_ARG;
  const int sw = fmt->source_width, sh = fmt->source_height, id = fmt->input_bit_depth;
  if (hevcdl_src::chroma_format_id(fmt->chroma_format) != hevcdl_src::FMT_420 || fmt->colour_space) { // the file's layout (the window plays no part on the way in)
    const int f = fmt->chroma_format, sp = fmt->colour_space;
    if (id > 8 && internal_bit_depth > 8) hevcdl_src::load_pictures_fmt((const uint16_t *)src, sw, sh, f, sp, (uint16_t *)coded_out, coded_width, coded_height, n_frames, id, internal_bit_depth);
    else if (id > 8) hevcdl_src::load_pictures_fmt((const uint16_t *)src, sw, sh, f, sp, (uint8_t *)coded_out, coded_width, coded_height, n_frames, id, internal_bit_depth);
    else if (internal_bit_depth > 8) hevcdl_src::load_pictures_fmt((const uint8_t *)src, sw, sh, f, sp, (uint16_t *)coded_out, coded_width, coded_height, n_frames, id, internal_bit_depth);
    else hevcdl_src::load_pictures_fmt((const uint8_t *)src, sw, sh, f, sp, (uint8_t *)coded_out, coded_width, coded_height, n_frames, id, internal_bit_depth);
    return HEVCDL_OK;
  }
  if (id > 8 && internal_bit_depth > 8) hevcdl_src::load_pictures((const uint16_t *)src, sw, sh, (uint16_t *)coded_out, coded_width, coded_height, n_frames, id, internal_bit_depth);
  else if (id > 8) hevcdl_src::load_pictures((const uint16_t *)src, sw, sh, (uint8_t *)coded_out, coded_width, coded_height, n_frames, id, internal_bit_depth);
  else if (internal_bit_depth > 8) hevcdl_src::load_pictures((const uint8_t *)src, sw, sh, (uint16_t *)coded_out, coded_width, coded_height, n_frames, id, internal_bit_depth);
  else hevcdl_src::load_pictures((const uint8_t *)src, sw, sh, (uint8_t *)coded_out, coded_width, coded_height, n_frames, id, internal_bit_depth);
  return HEVCDL_OK;
}

extern "C" hevcdl_status hevcdl_store_output_host(const hevcdl_source_format *fmt, int coded_width, int coded_height, int internal_bit_depth, const void *pictures, int n_frames, void *out)
{
  if (!fmt || fmt->struct_size != sizeof *fmt || !pictures || !out || n_frames < 0 || internal_bit_depth < 8 || internal_bit_depth > 16) return HEVCDL_ERR_INVALID_ARG;
  if (!hevcdl_source_format_fits(fmt, coded_width, coded_height)) return HEVCDL_ERR_INVALID_ARG;
  int ww, wh; hevcdl_source_window_size(fmt, &ww, &wh);
  const int od = fmt->output_bit_depth;
  const int swap = fmt->colour_space && !fmt->output_internal_colour_space, wl = fmt->conf_win_left, wt = fmt->conf_win_top;
  if (swap || ww != fmt->source_width || wh != fmt->source_height) { // planes back in the file's order, a window with an origin
    if (internal_bit_depth > 8 && od > 8) hevcdl_src::store_pictures_fmt((const uint16_t *)pictures, coded_width, coded_height, (uint16_t *)out, ww, wh, wl, wt, swap, n_frames, internal_bit_depth, od);
    else if (internal_bit_depth > 8) hevcdl_src::store_pictures_fmt((const uint16_t *)pictures, coded_width, coded_height, (uint8_t *)out, ww, wh, wl, wt, swap, n_frames, internal_bit_depth, od);
    else if (od > 8) hevcdl_src::store_pictures_fmt((const uint8_t *)pictures, coded_width, coded_height, (uint16_t *)out, ww, wh, wl, wt, swap, n_frames, internal_bit_depth, od);
    else hevcdl_src::store_pictures_fmt((const uint8_t *)pictures, coded_width, coded_height, (uint8_t *)out, ww, wh, wl, wt, swap, n_frames, internal_bit_depth, od);
    return HEVCDL_OK;
  }
  if (internal_bit_depth > 8 && od > 8) hevcdl_src::store_pictures((const uint16_t *)pictures, coded_width, coded_height, (uint16_t *)out, ww, wh, n_frames, internal_bit_depth, od);
  else if (internal_bit_depth > 8) hevcdl_src::store_pictures((const uint16_t *)pictures, coded_width, coded_height, (uint8_t *)out, ww, wh, n_frames, internal_bit_depth, od);
  else if (od > 8) hevcdl_src::store_pictures((const uint8_t *)pictures, coded_width, coded_height, (uint16_t *)out, ww, wh, n_frames, internal_bit_depth, od);
  else hevcdl_src::store_pictures((const uint8_t *)pictures, coded_width, coded_height, (uint8_t *)out, ww, wh, n_frames, internal_bit_depth, od);
  return HEVCDL_OK;
}
