// hevcdl_parse.cpp -- HEVC stream parser for the streams this library writes: the inverse of hevcdl_bitstream.cpp and of entropy_coder.h.
// Host C++ (no GPU, no HIP header).  Annex B -> NAL units -> VPS / SPS / PPS / slice segment headers / decoded picture hash SEI -> slice data: an arithmetic
// DECODER over entropy_tables.h (ITU-T H.265 9.3.4.3) and the I-slice syntax of 7.3.8 (sao, coding_quadtree, coding_unit, transform_tree, residual_coding) ->
// hevcdl_ctu_record and hevcdl_sao_blk per CTU (hevcdl_parse.h names the record fields a stream determines).
// One function, walk_stream, owns everything in front of the slice data and hands each complete picture to a sink: hevcdl_parse_stream's sink decodes it with the decoder
// of this file, collect_units' sink cuts it into units for the shared decoder (slice_decode_core.h), which the first is tested against.
//
// Accepted: what hevcdl_write_access_unit_segments can produce.  Anything else is HEVCDL_ERR_UNSUPPORTED with a sentence (hevcdl_parse_error); a damaged stream is
// HEVCDL_ERR_INVALID_ARG.  Construction rules (a stream is untrusted input):
//   * every read goes through a reader that knows the end of its bytes: past it a sticky flag is set and zeros are returned;
//   * every loop has a bound that does not depend on stream contents beyond a checked value (64 coefficient groups, 16 positions, 32 prefix bins, the CTUs of the picture);
//   * every value that later indexes memory is checked where it is read: slice_segment_address, tile sizes, entry points against the payload, the last significant
//     position against its block, prediction modes, levels against 16 bits; a transform block's position follows from the trees and lies inside its CTU by construction;
//   * recursion only over the two quadtrees, four and five levels deep.
#include <algorithm>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "hevcdl.h"
#include "hevcdl_dev.h"
#include "entropy_tables.h"
#define EC_FN static inline
#include "entropy_coder.h"
#include "hevcdl_parse.h"
#define SD_FN static inline
#include "slice_decode_units.h"

namespace hevcdl_parse {
static thread_local char g_error[256] = "";
void set_error(const char *fmt, ...)
{
  va_list ap; va_start(ap, fmt); vsnprintf(g_error, sizeof g_error, fmt, ap); va_end(ap);
}
} // namespace hevcdl_parse

namespace {
using namespace hevcdl_ec;
using namespace hevcdl_parse;

thread_local hevcdl_qp_tally g_tally;      // what the last hevcdl_parse_stream_qp of this thread met (hevcdl_parse_qp_tally)

#define UNSUPPORTED(...) do { set_error(__VA_ARGS__); return HEVCDL_ERR_UNSUPPORTED; } while (0)
#define INVALID(...) do { set_error(__VA_ARGS__); return HEVCDL_ERR_INVALID_ARG; } while (0)

// ---- bit reader over RBSP bytes --------------------------------------------------------------------------------------------
struct BitIn {
  const uint8_t *d; size_t nbits, p; int bad;
  BitIn(const uint8_t *data, size_t n) : d(data), nbits(n * 8), p(0), bad(0) {}
  uint32_t u(int n)
  {
    uint32_t v = 0;
    for (int i = 0; i < n; i++) {
      if (p >= nbits) { bad = 1; v <<= 1; continue; }
      v = (v << 1) | ((d[p >> 3] >> (7 - (p & 7))) & 1u); p++;
    }
    return v;
  }
  uint32_t ue()
  {
    int z = 0;
    while (z < 32 && !bad && u(1) == 0) z++;
    if (z >= 32 || bad) { bad = 1; return 0; }
    return z ? ((1u << z) - 1u + u(z)) : 0;
  }
  int se() { const uint32_t k = ue(); return (k & 1) ? (int)((k + 1) >> 1) : -(int)(k >> 1); }
};

struct Nal { int type; std::vector<uint8_t> rbsp; std::vector<uint32_t> pos; size_t size; };      // rbsp: the bytes behind the two header bytes, emulation prevention removed; pos: where each came from

// Annex B: NAL units between start codes (B.2); a zero_byte in front of a start code belongs to the start code
void split_annexb(const uint8_t *b, size_t n, std::vector<std::pair<size_t, size_t>> &out)
{
  std::vector<size_t> sc;
  for (size_t i = 0; i + 2 < n; i++) if (b[i] == 0 && b[i + 1] == 0 && b[i + 2] == 1) { sc.push_back(i); i += 2; }
  for (size_t k = 0; k < sc.size(); k++) {
    size_t begin = sc[k] + 3, end = k + 1 < sc.size() ? sc[k + 1] : n;
    while (end > begin && k + 1 < sc.size() && b[end - 1] == 0) end--;      // trailing_zero_8bits / the next start code's zero_byte
    out.push_back({ begin, end });
  }
}

bool unescape(const uint8_t *b, size_t n, Nal &nal)
{
  if (n < 2 || (b[0] & 0x80)) return false;      // forbidden_zero_bit
  nal.type = (b[0] >> 1) & 63; nal.size = n;
  nal.rbsp.clear(); nal.pos.clear();
  int zeros = 0;
  for (size_t i = 2; i < n; i++) {
    if (zeros >= 2 && b[i] == 3) { zeros = 0; continue; }
    nal.rbsp.push_back(b[i]); nal.pos.push_back((uint32_t)i);
    zeros = b[i] == 0 ? zeros + 1 : 0;
  }
  return true;
}

// ---- parameter sets ----------------------------------------------------------------------------------------------------------
void profile_tier_level(BitIn &r, int &level_idc)
{
  r.u(2); r.u(1); r.u(5); r.u(32); r.u(4); r.u(32); r.u(11); r.u(1);
  level_idc = (int)r.u(8);
}

// ---- scaling lists (7.3.4, 7.4.5) ----------------------------------------------------------------------------------------------
// Table 7-6 in the order it is coded in (up-right diagonal); Table 7-5 is 16 everywhere
const uint8_t SL_DEFAULT_INTRA[64] = { 16, 16, 16, 16, 16, 16, 16, 16, 16, 16, 17, 16, 17, 16, 17, 18, 17, 18, 18, 17, 18, 21, 19, 20, 21, 20, 19, 21, 24, 22, 22, 24,
                                       24, 22, 22, 24, 25, 25, 27, 30, 27, 25, 25, 29, 31, 35, 35, 31, 29, 36, 41, 44, 41, 36, 47, 54, 54, 47, 65, 70, 65, 88, 88, 115 };
const uint8_t SL_DEFAULT_INTER[64] = { 16, 16, 16, 16, 16, 16, 16, 16, 16, 16, 17, 17, 17, 17, 17, 18, 18, 18, 18, 18, 18, 20, 20, 20, 20, 20, 20, 20, 24, 24, 24, 24,
                                       24, 24, 24, 24, 25, 25, 25, 25, 25, 25, 25, 28, 28, 28, 28, 28, 28, 33, 33, 33, 33, 33, 41, 41, 41, 41, 54, 54, 54, 71, 71, 91 };
struct ScalingLists { uint8_t list[4][6][64]; int dc[4][6]; };      // [sizeId][matrixId] in coded order; dc: the DC entry of sizeId 2 and 3

void sl_default(ScalingLists &s, int size_id, int m)
{
  for (int i = 0; i < 64; i++) s.list[size_id][m][i] = size_id == 0 ? 16 : (m < 3 ? SL_DEFAULT_INTRA[i] : SL_DEFAULT_INTER[i]);
  s.dc[size_id][m] = 16;
}
// ScanOrder[log2][0] of 6.5.3: position i of the up-right diagonal scan of a block of n x n -> raster index y * n + x
void sl_diag(int n, uint8_t *raster)
{
  int i = 0, x = 0, y = 0;
  while (i < n * n) {
    while (y >= 0) { if (x < n && y < n) raster[i++] = (uint8_t)(y * n + x); y--; x++; }
    y = x; x = 0;
  }
}
// ScalingFactor of 7.4.5 for the planes 4:2:0 has, raster order: Y 4 8 16 32, Cb 4 8 16, Cr 4 8 16 (hevcdl_scaling_info).  The inter lists (matrixId 3 .. 5) are dropped here
void sl_expand(const ScalingLists &s, uint8_t *f)
{
  uint8_t d4[16], d8[64];
  sl_diag(4, d4); sl_diag(8, d8);
  for (int c = 0; c < 3; c++) {
    uint8_t *o = f + (c == 0 ? 0 : 1360 + (c - 1) * 336);
    for (int i = 0; i < 16; i++) o[d4[i]] = s.list[0][c][i];
    for (int i = 0; i < 64; i++) o[16 + d8[i]] = s.list[1][c][i];
    for (int size_id = 2; size_id < (c == 0 ? 4 : 3); size_id++) {
      const int m = size_id == 3 ? 0 : c, n = 4 << size_id, rep = n >> 3;
      uint8_t *b = o + (size_id == 2 ? 80 : 336);
      for (int i = 0; i < 64; i++) {
        const int x8 = d8[i] & 7, y8 = d8[i] >> 3;
        for (int j = 0; j < rep; j++) for (int k = 0; k < rep; k++) b[(y8 * rep + j) * n + x8 * rep + k] = s.list[size_id][m][i];
      }
      b[0] = (uint8_t)s.dc[size_id][m];
    }
  }
}
// scaling_list_data() 7.3.4 as the reference writes it: for sizeId 3 only matrixId 0 and 3, scaling_list_pred_matrix_id_delta counting in steps of 3
hevcdl_status parse_scaling_list_data(BitIn &r, ScalingLists &s)
{
  for (int size_id = 0; size_id < 4; size_id++) {
    const int step = size_id == 3 ? 3 : 1, num = size_id == 0 ? 16 : 64;
    for (int m = 0; m < 6; m += step) {
      if (!r.u(1)) { // scaling_list_pred_mode_flag 0: the default list, or a copy of an earlier one
        const uint32_t delta = r.ue();
        if (r.bad) INVALID("the SPS ends inside its scaling lists");
        if (delta > (uint32_t)(m / step)) INVALID("scaling_list_pred_matrix_id_delta %u of list %d of size %d", delta, m, size_id);
        if (delta == 0) sl_default(s, size_id, m);
        else { const int ref = m - (int)delta * step; memcpy(s.list[size_id][m], s.list[size_id][ref], 64); s.dc[size_id][m] = s.dc[size_id][ref]; }
        continue;
      }
      int next = 8;
      s.dc[size_id][m] = 16;
      if (size_id > 1) {
        const int dc = r.se();
        if (r.bad) INVALID("the SPS ends inside its scaling lists");
        if (dc < -7 || dc > 247) INVALID("scaling_list_dc_coef_minus8 %d of list %d of size %d", dc, m, size_id);
        next = dc + 8; s.dc[size_id][m] = next;
      }
      for (int i = 0; i < num; i++) {
        const int d = r.se();
        if (r.bad) INVALID("the SPS ends inside its scaling lists");
        if (d < -128 || d > 127) INVALID("scaling_list_delta_coef %d of list %d of size %d", d, m, size_id);
        next = (next + d + 256) % 256;
        if (next == 0) INVALID("entry %d of scaling list %d of size %d is 0", i, m, size_id);
        s.list[size_id][m][i] = (uint8_t)next;
      }
    }
  }
  return HEVCDL_OK;
}

hevcdl_status parse_sps(const Nal &n, ParamSets &ps, unsigned accept)
{
  BitIn r(n.rbsp.data(), n.rbsp.size());
  r.u(4); const int max_sub = (int)r.u(3); r.u(1);
  if (max_sub != 0) UNSUPPORTED("temporal sub-layers are outside this decoder");
  profile_tier_level(r, ps.level_idc);
  r.ue();
  const uint32_t chroma = r.ue();
  if (r.bad) INVALID("the SPS ends inside its profile fields");
  if (chroma != 1) UNSUPPORTED("chroma_format_idc %u: only 4:2:0 is decoded", chroma);
  const uint32_t w = r.ue(), h = r.ue();
  if (r.bad || w < 8 || h < 8 || w > 16384 || h > 16384 || (w & 7) || (h & 7)) INVALID("picture size %u x %u in the SPS", w, h);
  ps.width = (int)w; ps.height = (int)h;
  ps.conf_left = ps.conf_right = ps.conf_top = ps.conf_bottom = 0;
  if (r.u(1)) {
    const uint32_t c[4] = { r.ue(), r.ue(), r.ue(), r.ue() };
    for (int i = 0; i < 4; i++) if (c[i] > 8192) INVALID("conformance window offset %u", c[i]);
    ps.conf_left = 2 * (int)c[0]; ps.conf_right = 2 * (int)c[1]; ps.conf_top = 2 * (int)c[2]; ps.conf_bottom = 2 * (int)c[3];
    if (ps.conf_left + ps.conf_right >= ps.width || ps.conf_top + ps.conf_bottom >= ps.height) INVALID("the conformance window leaves nothing of the picture");
  }
  const uint32_t bdl = r.ue(), bdc = r.ue();
  if (r.bad) INVALID("the SPS ends inside its bit depths");
  if (bdl != bdc || (bdl != 0 && bdl != 2)) UNSUPPORTED("bit depth %u / %u: only 8 and 10 bits (main, main10) are decoded", bdl + 8, bdc + 8);
  ps.bit_depth = 8 + (int)bdl;
  const uint32_t lp = r.ue();
  if (lp > 12) INVALID("log2_max_pic_order_cnt_lsb_minus4 %u", lp);
  ps.log2_poc = (int)lp + 4;
  r.u(1); r.ue(); r.ue(); r.ue();
  const uint32_t min_cb = r.ue(), diff_cb = r.ue(), min_tb = r.ue(), diff_tb = r.ue(), td_inter = r.ue(), td_intra = r.ue();
  (void)td_inter;
  if (r.bad) INVALID("the SPS ends inside its block sizes");
  if (min_cb != 0 || diff_cb != 3 || min_tb != 0 || diff_tb != 3 || td_intra != 2)
    UNSUPPORTED("block sizes of the SPS: only CTU 64, minimum CB 8, TU 4..32 and intra TU depth 3 are decoded");
  ps.sl_enabled = ps.sl_data_present = 0; memset(ps.sl_factor, 0, sizeof ps.sl_factor);
  if (r.u(1)) { // scaling_list_enabled_flag: the default lists, or sps_scaling_list_data_present_flag and scaling_list_data()
    if (!(accept & HEVCDL_ACCEPT_SCALING_LISTS)) UNSUPPORTED("scaling lists are outside this decoder");
    ScalingLists s;
    for (int size_id = 0; size_id < 4; size_id++) for (int m = 0; m < 6; m++) sl_default(s, size_id, m);
    ps.sl_enabled = 1; ps.sl_data_present = (int)r.u(1);
    if (ps.sl_data_present) { const hevcdl_status st = parse_scaling_list_data(r, s); if (st != HEVCDL_OK) return st; }
    sl_expand(s, ps.sl_factor);
  }
  r.u(1);                                            // amp_enabled_flag: nothing in an I slice
  ps.sao = (int)r.u(1);
  if (r.u(1)) UNSUPPORTED("PCM is outside this decoder");
  const uint32_t nrps = r.ue();
  if (r.bad || nrps > 64) INVALID("num_short_term_ref_pic_sets %u", nrps);
  ps.num_st_rps = (int)nrps;
  for (uint32_t i = 0; i < nrps; i++) {
    if (i > 0 && r.u(1)) UNSUPPORTED("inter-predicted reference picture sets are outside this decoder");
    const uint32_t nneg = r.ue(), npos = r.ue();
    if (r.bad || nneg > 16 || npos > 16) INVALID("a reference picture set of %u + %u pictures", nneg, npos);
    for (uint32_t k = 0; k < nneg + npos; k++) { r.ue(); r.u(1); }
  }
  ps.long_term = (int)r.u(1);
  if (ps.long_term) UNSUPPORTED("long-term reference pictures are outside this decoder");
  ps.temporal_mvp = (int)r.u(1);
  ps.strong_intra = (int)r.u(1);
  if (r.u(1)) UNSUPPORTED("VUI parameters are outside this decoder");
  if (r.u(1)) UNSUPPORTED("SPS extensions are outside this decoder");
  if (r.bad) INVALID("the SPS ends before its last field");
  ps.have_sps = 1;
  return HEVCDL_OK;
}

hevcdl_status parse_pps(const Nal &n, ParamSets &ps, unsigned accept)
{
  BitIn r(n.rbsp.data(), n.rbsp.size());
  r.ue(); r.ue();
  ps.dep_slices = (int)r.u(1); ps.output_flag_present = (int)r.u(1); ps.extra_bits = (int)r.u(3);
  ps.sign_hiding = (int)r.u(1); r.u(1); r.ue(); r.ue();
  ps.init_qp = 26 + r.se();
  if (r.bad || ps.init_qp < 0 || ps.init_qp > 51) INVALID("init_qp_minus26 of the PPS");
  if (r.u(1)) UNSUPPORTED("constrained intra prediction is outside this decoder");
  ps.tskip = (int)r.u(1);
  ps.cu_qp_delta = (int)r.u(1); ps.diff_cu_qp_depth = 0;
  if (ps.cu_qp_delta && !(accept & HEVCDL_ACCEPT_CU_QP)) UNSUPPORTED("cu_qp_delta_enabled_flag is outside this decoder");
  if (ps.cu_qp_delta) {
    const uint32_t d = r.ue();
    if (r.bad || d > 3) INVALID("diff_cu_qp_delta_depth %u", d);
    ps.diff_cu_qp_depth = (int)d;
  }
  const int cb = r.se(), cr = r.se();
  if ((cb != 0 || cr != 0) && !(accept & HEVCDL_ACCEPT_CU_QP)) UNSUPPORTED("chroma QP offsets are outside this decoder");
  if (cb < -12 || cb > 12 || cr < -12 || cr > 12) INVALID("chroma QP offsets %d / %d in the PPS", cb, cr);
  ps.cb_qp_offset = cb; ps.cr_qp_offset = cr;
  if (r.u(1)) UNSUPPORTED("slice-level chroma QP offsets are outside this decoder");
  r.u(1); r.u(1);                                    // weighted prediction: nothing in an I slice
  if (r.u(1)) UNSUPPORTED("transquant bypass is outside this decoder");
  ps.tiles = (int)r.u(1); ps.wpp = (int)r.u(1);
  if (r.bad) INVALID("the PPS ends inside its flags");
  if (ps.tiles && ps.wpp) UNSUPPORTED("wavefront together with tiles is outside this decoder");
  ps.tcols = ps.trows = 1; ps.uniform = 1; ps.lf_across_tiles = 1;
  if (ps.tiles) {
    const uint32_t c = r.ue(), t = r.ue();
    if (r.bad || c >= MAX_TILE_COLS || t >= MAX_TILE_ROWS) INVALID("a tile grid of %u x %u", c + 1, t + 1);
    ps.tcols = (int)c + 1; ps.trows = (int)t + 1;
    ps.uniform = (int)r.u(1);
    if (!ps.uniform) {
      for (int i = 0; i < ps.tcols - 1; i++) { const uint32_t v = r.ue(); if (r.bad || v > 1024) INVALID("column_width_minus1 %u", v); ps.col_width[i] = (int)v + 1; }
      for (int i = 0; i < ps.trows - 1; i++) { const uint32_t v = r.ue(); if (r.bad || v > 1024) INVALID("row_height_minus1 %u", v); ps.row_height[i] = (int)v + 1; }
    }
    ps.lf_across_tiles = (int)r.u(1);
  }
  ps.lf_across_slices = (int)r.u(1);
  ps.dbk_control = (int)r.u(1);
  ps.dbk_override_enabled = ps.dbk_disabled = ps.beta_div2 = ps.tc_div2 = 0;
  if (ps.dbk_control) {
    ps.dbk_override_enabled = (int)r.u(1); ps.dbk_disabled = (int)r.u(1);
    if (!ps.dbk_disabled) { ps.beta_div2 = r.se(); ps.tc_div2 = r.se(); }
    if (ps.beta_div2 < -6 || ps.beta_div2 > 6 || ps.tc_div2 < -6 || ps.tc_div2 > 6) INVALID("deblocking offsets %d / %d in the PPS", ps.beta_div2, ps.tc_div2);
  }
  if (r.u(1)) UNSUPPORTED("scaling lists are outside this decoder");
  r.u(1); r.ue();                                    // lists_modification_present_flag, log2_parallel_merge_level_minus2: nothing in an I slice
  if (r.u(1)) UNSUPPORTED("slice segment header extensions are outside this decoder");
  if (r.u(1)) UNSUPPORTED("PPS extensions are outside this decoder");
  if (r.bad) INVALID("the PPS ends before its last field");
  ps.have_pps = 1;
  return HEVCDL_OK;
}

// the grid of a picture: tile boundaries, tile scan, tile ids
struct Grid {
  int cx, cy, n, tcols, trows, col_bd[MAX_TILE_COLS + 1], row_bd[MAX_TILE_ROWS + 1];
  std::vector<int> rs2ts, ts2rs, tile_id;
};
hevcdl_status make_grid(const ParamSets &ps, Grid &g)
{
  g.cx = (ps.width + 63) >> 6; g.cy = (ps.height + 63) >> 6; g.n = g.cx * g.cy; g.tcols = ps.tcols; g.trows = ps.trows;
  if (hevcdl_tile_bounds(g.cx, g.tcols, ps.uniform, ps.col_width, 1, g.col_bd) || hevcdl_tile_bounds(g.cy, g.trows, ps.uniform, ps.row_height, 1, g.row_bd))
    INVALID("the tile sizes of the PPS do not fit a picture of %d x %d CTUs", g.cx, g.cy);
  g.rs2ts.assign((size_t)g.n, 0); g.ts2rs.assign((size_t)g.n, 0); g.tile_id.assign((size_t)g.n, 0);
  int ts = 0;
  for (int tr = 0; tr < g.trows; tr++) for (int tc = 0; tc < g.tcols; tc++)
    for (int y = g.row_bd[tr]; y < g.row_bd[tr + 1]; y++) for (int x = g.col_bd[tc]; x < g.col_bd[tc + 1]; x++) {
      const int rs = y * g.cx + x;
      g.rs2ts[(size_t)rs] = ts; g.ts2rs[(size_t)ts] = rs; g.tile_id[(size_t)rs] = tr * g.tcols + tc; ts++;
    }
  return HEVCDL_OK;
}

hevcdl_status parse_slice_header(const Nal &n, const ParamSets &ps, int n_ctus, SegmentHeader &h)
{
  BitIn r(n.rbsp.data(), n.rbsp.size());
  memset(&h, 0, sizeof h);
  h.nal_type = n.type;
  h.first = (int)r.u(1);
  if (n.type >= 16 && n.type <= 23) r.u(1);
  if (r.ue() != 0) UNSUPPORTED("several picture parameter sets are outside this decoder");
  if (!h.first) {
    if (ps.dep_slices) h.dependent = (int)r.u(1);
    int bits = 0; while (n_ctus > (1 << bits)) bits++;
    h.address = (int)r.u(bits);
    if (r.bad || h.address <= 0 || h.address >= n_ctus) INVALID("slice_segment_address %d in a picture of %d CTUs", h.address, n_ctus);
  }
  if (!h.dependent) {
    r.u(ps.extra_bits);
    const uint32_t type = r.ue();
    if (r.bad) INVALID("a slice segment header ends inside its first fields");
    if (type != 2) UNSUPPORTED("slice_type %u: P and B slices are outside this decoder", type);
    if (ps.output_flag_present) r.u(1);
    if (n.type != 19 && n.type != 20) {
      h.poc = (int)r.u(ps.log2_poc);
      if (!r.u(1)) {
        if (ps.num_st_rps > 0 && r.u(1)) UNSUPPORTED("inter-predicted reference picture sets are outside this decoder");
        const uint32_t nneg = r.ue(), npos = r.ue();
        if (r.bad || nneg > 16 || npos > 16) INVALID("a reference picture set of %u + %u pictures", nneg, npos);
        for (uint32_t k = 0; k < nneg + npos; k++) { r.ue(); r.u(1); }
      } else if (ps.num_st_rps > 1) { int b = 0; while (ps.num_st_rps > (1 << b)) b++; r.u(b); }
      if (ps.temporal_mvp) r.u(1);
    }
    if (ps.sao) { h.sao_luma = (int)r.u(1); h.sao_chroma = (int)r.u(1); }
    h.qp_delta = r.se();
    h.dbk.override_enabled = ps.dbk_override_enabled; h.dbk.disabled = ps.dbk_disabled; h.dbk.beta_offset_div2 = ps.beta_div2; h.dbk.tc_offset_div2 = ps.tc_div2;
    if (ps.dbk_override_enabled) h.dbk.override_flag = (int)r.u(1);
    if (h.dbk.override_flag) {
      h.dbk.disabled = (int)r.u(1); h.dbk.beta_offset_div2 = h.dbk.tc_offset_div2 = 0;
      if (!h.dbk.disabled) { h.dbk.beta_offset_div2 = r.se(); h.dbk.tc_offset_div2 = r.se(); }
      if (h.dbk.beta_offset_div2 < -6 || h.dbk.beta_offset_div2 > 6 || h.dbk.tc_offset_div2 < -6 || h.dbk.tc_offset_div2 > 6) INVALID("deblocking offsets %d / %d in a slice header", h.dbk.beta_offset_div2, h.dbk.tc_offset_div2);
    }
    h.lf_across_slices = ps.lf_across_slices;
    if (ps.lf_across_slices && (h.sao_luma || h.sao_chroma || !h.dbk.disabled)) h.lf_across_slices = (int)r.u(1);
  }
  if (ps.tiles || ps.wpp) {
    const uint32_t ne = r.ue();
    if (r.bad || ne >= MAX_SEGMENTS) INVALID("num_entry_point_offsets %u", ne);
    h.n_entry = (int)ne;
    if (ne) {
      const uint32_t len = r.ue();
      if (r.bad || len > 31) INVALID("offset_len_minus1 %u", len);
      for (uint32_t i = 0; i < ne; i++) { const uint32_t v = r.u((int)len + 1); if (v == 0xffffffffu) INVALID("an entry point offset of 2^32"); h.entry[i] = v + 1; }
    }
  }
  if (r.u(1) != 1) { if (!r.bad) INVALID("byte_alignment() of a slice segment header does not start with 1"); }
  while ((r.p & 7) && !r.bad) if (r.u(1)) INVALID("byte_alignment() of a slice segment header holds a 1 among its zeros");
  if (r.bad) INVALID("a slice segment header runs past the end of its NAL unit");
  h.data_byte_pos = r.p >> 3;
  return HEVCDL_OK;
}

// the decoded picture hash of a suffix SEI NAL unit (D.2.19): method 1 MD5, 2 CRC, 3 checksum; 0: the NAL unit holds no such message
hevcdl_status parse_hash_sei(const Nal &n, hevcdl_parsed_picture &pic)
{
  BitIn r(n.rbsp.data(), n.rbsp.size());
  for (int msg = 0; msg < 64 && r.p + 16 <= r.nbits; msg++) {
    uint32_t type = 0, size = 0, b;
    do { b = r.u(8); type += b; } while (b == 0xff && !r.bad);
    do { b = r.u(8); size += b; } while (b == 0xff && !r.bad);
    if (r.bad || (size_t)size * 8 > r.nbits - r.p) INVALID("an SEI message of %u bytes runs past the end of its NAL unit", size);
    if (type != 132) { r.p += (size_t)size * 8; continue; }
    const uint32_t ht = r.u(8);
    if (ht > 2) INVALID("hash_type %u of the decoded picture hash", ht);
    const int pb = ht == 0 ? 16 : (ht == 1 ? 2 : 4);
    if (size != 1u + 3u * (uint32_t)pb) UNSUPPORTED("a decoded picture hash of %u bytes: only three colour planes are decoded", size);
    pic.hash_method = (int)ht + 1; pic.hash_plane_bytes = pb;
    for (int i = 0; i < 3 * pb; i++) pic.digest[i] = (uint8_t)r.u(8);
  }
  return HEVCDL_OK;
}

// ---- the arithmetic decoding engine (9.3.4.3) over one sub-stream --------------------------------------------------------------
struct Engine {
  const EcTables *t; const uint8_t *d; size_t nbits, p; uint32_t range, offset; int bad;
  uint32_t bit() { if (p >= nbits) { bad = 1; return 0; } const uint32_t v = (d[p >> 3] >> (7 - (p & 7))) & 1u; p++; return v; }
  void start(const uint8_t *data, size_t n)
  {
    d = data; nbits = n * 8; p = 0; bad = 0; range = 510; offset = 0;
    for (int i = 0; i < 9; i++) offset = (offset << 1) | bit();
    if (offset >= 510) bad = 1;
  }
  int bin(uint8_t *ctx, int c)
  {
    if ((unsigned)c >= (unsigned)hevcdl_sd::SD_NUM_CTX) { bad = 1; return 0; }
    const uint32_t cv = ctx[c] & 127u, st = cv >> 1; int v = (int)(cv & 1);
    const uint32_t lps = t->lps[st][(range >> 6) & 3];
    range -= lps;
    if (offset >= range) { v = !v; offset -= range; range = lps; ctx[c] = t->next_lps[cv]; }
    else ctx[c] = t->next_mps[cv];
    for (int k = 0; k < 8 && range < 256; k++) { range <<= 1; offset = (offset << 1) | bit(); }
    return v;
  }
  int ep() { offset = (offset << 1) | bit(); if (offset >= range) { offset -= range; return 1; } return 0; }
  uint32_t eps(int n) { uint32_t v = 0; for (int i = 0; i < n && i < 32; i++) v = (v << 1) | (uint32_t)ep(); return v; }
  int terminate()
  {
    range -= 2;
    if (offset >= range) return 1;
    if (range < 256) { range <<= 1; offset = (offset << 1) | bit(); }
    return 0;
  }
  // behind a terminating bin of 1: the last bit read is the 1 of byte_alignment() / rbsp_slice_segment_trailing_bits(), zeros up to the byte boundary, nothing after
  bool finish()
  {
    if (bad || p == 0 || p > nbits) return false;
    if (!((d[(p - 1) >> 3] >> (7 - ((p - 1) & 7))) & 1)) return false;
    while (p & 7) if (bit()) return false;
    return p == nbits && !bad;
  }
};

// ---- one picture's slice data --------------------------------------------------------------------------------------------------
struct Picture {
  const ParamSets &ps; const Grid &g; const EcTables *t;
  hevcdl_ctu_record *recs; hevcdl_sao_blk *sao;      // [g.n]; sao may be null
  int W, H, qp, sao_on, max_sao;
  std::vector<int> slice_addr;                       // SliceAddrRs of every CTU decoded so far, -1: not yet
  Engine e; uint8_t ctx[EC_SYNC_BYTES], sync[EC_SYNC_BYTES];
  const char *why;                                   // the first syntax error
  // 8.6.1 (only with ps.cu_qp_delta, or with a map to fill): QpY per 4x4 partition of the picture [g.n][256] (null: none wanted) and of the CTU in work; qPY_PREV, qPY_PRED,
  // IsCuQpDeltaCoded and CuQpDeltaVal of the quantisation group in work
  int8_t *qp_map; int8_t qp_cur[256]; int qp_prev, qp_pred, dqp_coded, dqp_val;
  // the tally's view of the group in work: has a CU, where its prediction came from, what opened behind a reset of qPY_PREV (1 slice, 2 tile, 3 wavefront row), and the
  // CTU of the last group that closed without a delta (-1: the last one had one, or none closed yet)
  int grp_cu = 0, grp_prev_left = 0, grp_prev_up = 0, grp_reset = 0, grp_ctu = -1, none_ctu = -1;
  void close_group()
  {
    if (!grp_cu) return;
    if (dqp_coded) { g_tally.groups_with_delta++; if (none_ctu == grp_ctu) g_tally.coded_behind_uncoded_in_ctu++; none_ctu = -1; }
    else { g_tally.groups_without_delta++; none_ctu = grp_ctu; }
    grp_cu = 0;
  }
  Picture(const ParamSets &p, const Grid &grid) : ps(p), g(grid), t(&ec_tables()), recs(nullptr), sao(nullptr), why(nullptr), qp_map(nullptr), qp_prev(0), qp_pred(0), dqp_coded(0), dqp_val(0) { e.t = t; memset(qp_cur, 0, sizeof qp_cur); }

  void init_contexts()
  { // the coder's, and behind them the two of cu_qp_delta_abs (initValue 154, Table 9-24: state 0 with MPS 1 at every QP)
    ec_init_contexts(ctx, t, qp);
    const int v = hevcdl_sd::SD_DQP_INIT, slope = (v >> 4) * 5 - 45, offset = ((v & 15) << 3) - 16;
    const int st = std::min(std::max(((slope * qp) >> 4) + offset, 1), 126), mps = st >= 64;
    ctx[hevcdl_sd::SD_CTX_DQP] = ctx[hevcdl_sd::SD_CTX_DQP + 1] = (uint8_t)(((mps ? st - 64 : 63 - st) << 1) + mps);
  }
  // a quantisation group opens at the quadtree node (x0, y0)
  void start_qg(int x0, int y0)
  {
    close_group();
    dqp_coded = 0; dqp_val = 0;
    grp_prev_left = !(x0 & 63); grp_prev_up = !(y0 & 63);
    const int a = (x0 & 63) ? qp_cur[z_of(x0 - 1, y0)] : qp_prev, b = (y0 & 63) ? qp_cur[z_of(x0, y0 - 1)] : qp_prev;
    qp_pred = (a + b + 1) >> 1;
  }
  void cu_qp_delta(int in_4x4_without_luma)
  { // cu_qp_delta_abs: TU prefix (cMax 5), EG0 suffix; cu_qp_delta_sign_flag
    int v = 0;
    while (v < 5 && e.bin(ctx, hevcdl_sd::SD_CTX_DQP + (v ? 1 : 0))) v++;
    if (v == 5) {
      int k = 0;
      while (k < 32 && e.ep()) k++;
      if (k >= 8) { fail("CuQpDeltaVal outside its range"); return; }
      v += (1 << k) - 1 + (int)e.eps(k);
      g_tally.deltas_with_suffix++; if (k > 0) g_tally.suffixes_of_several_bins++;
    }
    if (v && e.ep()) v = -v;
    if (v > 0) g_tally.deltas_positive++; else if (v < 0) g_tally.deltas_negative++; else g_tally.deltas_zero++;
    if ((uint32_t)(v < 0 ? -v : v) > g_tally.max_abs_delta) g_tally.max_abs_delta = (uint32_t)(v < 0 ? -v : v);
    if (in_4x4_without_luma) g_tally.deltas_by_parent_chroma_cbf++;
    const int half = 3 * (ps.bit_depth - 8);
    if (v < -(26 + half) || v > 25 + half) { fail("CuQpDeltaVal outside its range"); return; }
    dqp_coded = 1; dqp_val = v;
  }
  void finish_cu_qp(int rs, int z, int nparts)
  {
    int q = qp;
    if (ps.cu_qp_delta && !grp_cu) {
      grp_cu = 1; grp_ctu = rs;
      if (grp_prev_left) g_tally.groups_left_from_prev++;
      if (grp_prev_up) g_tally.groups_up_from_prev++;
      if (grp_reset == 1) g_tally.groups_opening_slice++; else if (grp_reset == 2) g_tally.groups_opening_tile++; else if (grp_reset == 3) g_tally.groups_opening_wpp_row++;
      grp_reset = 0;
    }
    if (ps.cu_qp_delta) { const int off = 6 * (ps.bit_depth - 8); q = ((qp_pred + dqp_val + 52 + 2 * off) % (52 + off)) - off; qp_prev = q; }
    for (int i = 0; i < nparts; i++) { qp_cur[(z + i) & 255] = (int8_t)q; if (qp_map) qp_map[(size_t)rs * 256 + ((z + i) & 255)] = (int8_t)q; }
  }

  void fail(const char *s) { if (!why) why = s; }
  int z_of(int x, int y) const { return t->r2z[(((y >> 2) & 15) << 4) | ((x >> 2) & 15)]; }
  int ctu_of(int x, int y) const { return (y >> 6) * g.cx + (x >> 6); }
  // 6.4.1 for a left or an upper neighbour: inside the picture, in a CTU of the same tile and the same slice that is decoded already
  bool available(int cur, int xn, int yn) const
  {
    if (xn < 0 || yn < 0 || xn >= W || yn >= H) return false;
    const int rn = ctu_of(xn, yn);
    if (rn == cur) return true;
    return slice_addr[(size_t)rn] >= 0 && slice_addr[(size_t)rn] == slice_addr[(size_t)cur] && g.tile_id[(size_t)rn] == g.tile_id[(size_t)cur];
  }

  void sao_syntax(int rs)
  { // 7.3.8.3, inverse of ec_code_sao_blk
    hevcdl_sao_blk &b = sao[rs];
    const int rx = rs % g.cx, ry = rs / g.cx;
    int left = 0, up = 0;
    if (rx > 0 && available(rs, (rx - 1) << 6, ry << 6)) left = e.bin(ctx, CTX_SAO_MERGE);
    if (ry > 0 && !left && available(rs, rx << 6, (ry - 1) << 6)) up = e.bin(ctx, CTX_SAO_MERGE);
    if (left || up) { b.c[0].mode = 2; b.c[0].type = left ? 0 : 1; return; }
    int type_idx = 0, eo = 0;
    for (int c = 0; c < 3; c++) {
      if (c < 2) { type_idx = 0; if (e.bin(ctx, CTX_SAO_TYPE)) type_idx = e.ep() ? 2 : 1; }
      if (!type_idx) continue;
      int a[4];
      for (int i = 0; i < 4; i++) { a[i] = 0; while (a[i] < max_sao && e.ep()) a[i]++; }
      hevcdl_sao_offset &o = b.c[c];
      o.mode = 1;
      if (type_idx == 1) {
        int neg[4];
        for (int i = 0; i < 4; i++) neg[i] = a[i] ? e.ep() : 0;
        const int band = (int)e.eps(5);
        o.type = 4; o.aux = band;
        for (int i = 0; i < 4; i++) o.offset[(band + i) & 31] = neg[i] ? -a[i] : a[i];
      } else {
        if (c < 2) eo = (int)e.eps(2);
        o.type = eo;
        o.offset[0] = a[0]; o.offset[1] = a[1]; o.offset[3] = -a[2]; o.offset[4] = -a[3];
      }
    }
  }

  // residual_coding() 7.3.8.11: the inverse of ec_code_coeff; the block's levels go to plane[base, base + n * n)
  void residual(hevcdl_ctu_record &r, int comp, int z, int log2n, int dir_mode)
  {
    const int ch = comp ? 1 : 0;
    EcCParam cp; ec_get_cparam(t, cp, comp, log2n, dir_mode);
    if (cp.log2 != log2n) { fail("a transform block outside 4 .. 32"); return; }
    const int n = cp.n, nn = n * n;
    int16_t *plane = comp == 0 ? r.coeff_y : (comp == 1 ? r.coeff_cb : r.coeff_cr);
    const int base = (z & 255) * (comp ? 4 : 16);
    if (base + nn > (comp ? 1024 : 4096)) { fail("a transform block that leaves its CTU"); return; }
    int16_t *coef = plane + base;
    if (n == 4 && ps.tskip) r.tskip[comp][z & 255] = (uint8_t)e.bin(ctx, CTX_TSKIP + ch);
    int px, py;
    { // last_sig_coeff_{x,y}_prefix / _suffix
      const int gmax = t->group_idx[n - 1], cw = log2n - 2;
      const int off = ch ? 0 : (cw * 3 + ((cw + 1) >> 2)), shift = ch ? cw : ((cw + 3) >> 2);
      const int bx = CTX_LAST_X + (ch ? 15 : 0) + off, by = CTX_LAST_Y + (ch ? 15 : 0) + off;
      int gx = 0, gy = 0;
      while (gx < gmax && e.bin(ctx, bx + (gx >> shift))) gx++;
      while (gy < gmax && e.bin(ctx, by + (gy >> shift))) gy++;
      px = gx > 3 ? t->min_in_group[gx] + (int)e.eps((gx - 2) >> 1) : gx;
      py = gy > 3 ? t->min_in_group[gy] + (int)e.eps((gy - 2) >> 1) : gy;
      if (px >= n || py >= n) { fail("last significant position outside the block"); return; }
      if (cp.scan_type == SCAN_VER) std::swap(px, py);
    }
    const int pos_last = py * n + px;
    int scan_last = -1;
    for (int q = 0; q < nn; q++) if ((cp.scan[q] & (nn - 1)) == pos_last) { scan_last = q; break; }
    if (scan_last < 0) { fail("last significant position outside the scan"); return; }
    const int cg_off = CTX_SIG_CG + (ch ? 2 : 0), sig_off = CTX_SIG + (ch ? 28 : 0);
    const int last_set = scan_last >> 4;
    uint64_t cgf = 0;
    int c1 = 1, sp = scan_last;
    for (int subset = last_set; subset >= 0 && !e.bad; subset--) {
      int num_nz = 0, go_rice = 0, pos[16], absv[16];
      const int sub_pos = subset << 4;
      int last_nz = -1, first_nz = 16;
      if (sp == scan_last) { pos[0] = pos_last; num_nz = 1; last_nz = first_nz = sp; sp--; }
      const int cgblk = cp.scan_cg[subset] & 63, gy = cgblk >> (log2n - 2), gx = cgblk & (cp.wg - 1);
      const int right = (gx < cp.wg - 1) ? (int)((cgf >> (gy * cp.wg + gx + 1)) & 1) : 0, lower = (gy < cp.wg - 1) ? (int)((cgf >> ((gy + 1) * cp.wg + gx)) & 1) : 0;
      if (subset == last_set || subset == 0) cgf |= 1ull << cgblk;
      else if (e.bin(ctx, cg_off + ((right + lower) != 0))) cgf |= 1ull << cgblk;
      if ((cgf >> cgblk) & 1) {
        const int pat = cp.wg <= 1 ? 0 : right + (lower << 1);
        for (int q = 0; q < 16 && sp >= sub_pos; q++, sp--) {
          const int raster = cp.scan[sp] & (nn - 1);
          int sig = 1;                                                   // the group's only possible level: inferred
          if (sp > sub_pos || subset == 0 || num_nz) sig = e.bin(ctx, sig_off + ec_sig_ctx_inc(t, cp, pat, raster));
          if (sig && num_nz < 16) { pos[num_nz++] = raster; if (last_nz == -1) last_nz = sp; first_nz = sp; }
        }
      } else sp = sub_pos - 1;
      if (num_nz == 0) continue;
      const int sign_hidden = ps.sign_hiding && (last_nz - first_nz >= 4);
      const int cset = (ch ? 4 : 0) + ((!ch && subset > 0) ? 2 : 0) + (c1 == 0 ? 1 : 0);
      c1 = 1;
      const int n_c1 = num_nz < 8 ? num_nz : 8; int first_c2 = -1;
      for (int i = 0; i < num_nz; i++) absv[i] = 1;
      for (int i = 0; i < n_c1; i++) {
        const int sym = e.bin(ctx, CTX_ONE + 4 * cset + c1);
        absv[i] += sym;
        if (sym) { c1 = 0; if (first_c2 == -1) first_c2 = i; }
        else if (c1 < 3 && c1 > 0) c1++;
      }
      if (c1 == 0 && first_c2 != -1) absv[first_c2] += e.bin(ctx, CTX_ABS + cset);
      const int n_signs = num_nz - sign_hidden;
      const uint32_t signs = e.eps(n_signs);
      int first_coeff2 = 1; uint32_t sum = 0;
      for (int i = 0; i < num_nz; i++) {
        const int bse = (i < 8) ? (2 + first_coeff2) : 1;
        if (absv[i] == bse) { // coeff_abs_level_remaining: the inverse of xWriteCoefRemainExGolomb
          int q = 0;
          while (q < 32 && e.ep()) q++;
          int rem;
          if (q < 3) rem = (q << go_rice) + (int)e.eps(go_rice);
          else {
            const int len = q - 3 + go_rice;
            if (len > 17) { fail("a level outside 16 bits"); return; }
            rem = (int)e.eps(len) + (3 << go_rice) + ((1 << len) - (1 << go_rice));
          }
          absv[i] += rem;
          if (absv[i] > (3 << go_rice)) go_rice = go_rice + 1 < 4 ? go_rice + 1 : 4;
        }
        if (absv[i] >= 2) first_coeff2 = 0;
        sum += (uint32_t)absv[i];
        int neg = i < n_signs ? (int)((signs >> (n_signs - 1 - i)) & 1) : (int)(sum & 1);      // the hidden sign is the last one's: the parity of the group's sum
        const int v = neg ? -absv[i] : absv[i];
        if (v < -32768 || v > 32767) { fail("a level outside 16 bits"); return; }
        coef[pos[i]] = (int16_t)v;
      }
    }
  }

  struct Cu { int x, y, log2, z, nparts, nxn, mode_c; hevcdl_ctu_record *r; };

  // transform_tree() 7.3.8.8 and transform_unit() 7.3.8.10; pcb: the chroma flags of the parent node
  void transform_tree(const Cu &cu, int zrel, int log2, int trd, int blk, int pcb, int pcr)
  {
    if (e.bad || why) return;
    hevcdl_ctu_record &r = *cu.r;
    const int max_depth = 2 + cu.nxn;
    int split;
    if (log2 <= 5 && log2 > 2 && trd < max_depth && !(cu.nxn && trd == 0)) split = e.bin(ctx, CTX_SUBDIV + 5 - log2);
    else split = (log2 > 5 || (cu.nxn && trd == 0)) ? 1 : 0;
    const int z = cu.z + zrel, np = cu.nparts >> (2 * trd);
    int cbf_c[3] = { 0, pcb, pcr };
    if (log2 > 2) for (int c = 1; c < 3; c++) {
      cbf_c[c] = (trd == 0 || cbf_c[c]) ? e.bin(ctx, CTX_QT_CBF + 5 + trd) : 0;
      if (cbf_c[c]) for (int i = 0; i < np; i++) r.cbf[c][(z + i) & 255] |= (uint8_t)((1 << trd) | ((log2 == 3 && split) ? (2 << trd) : 0));
    }
    if (split) {
      for (int k = 0; k < 4; k++) transform_tree(cu, zrel + k * (np >> 2), log2 - 1, trd + 1, k, cbf_c[1], cbf_c[2]);
      return;
    }
    const int cbf_y = e.bin(ctx, CTX_QT_CBF + (trd == 0 ? 1 : 0));
    if (ps.cu_qp_delta && !dqp_coded && (cbf_y || cbf_c[1] || cbf_c[2])) { cu_qp_delta(log2 == 2 && !cbf_y); if (why) return; }      // (a 4x4 luma block: cbf_c[] are its parent's)
    for (int i = 0; i < np; i++) r.tr_idx[(z + i) & 255] = (uint8_t)trd;
    if (cbf_y) {
      for (int d = 0; d <= trd; d++) {
        const int nd = cu.nparts >> (2 * d), org = cu.z + (zrel & ~(nd - 1));
        for (int i = 0; i < nd; i++) r.cbf[0][(org + i) & 255] |= (uint8_t)(1 << d);
      }
      residual(r, 0, z, log2, r.luma_dir[z & 255]);
    }
    if (log2 > 2) { for (int c = 1; c < 3; c++) if (cbf_c[c] && !why) residual(r, c, z, log2 - 1, cu.mode_c); }
    else if (blk == 3) for (int c = 1; c < 3; c++) if (cbf_c[c] && !why) residual(r, c, cu.z + (zrel & ~3), 2, cu.mode_c);
  }

  // coding_unit() 7.3.8.5 with 8.4.2 / 8.4.3
  void coding_unit(int rs, int x0, int y0, int log2, int depth)
  {
    hevcdl_ctu_record &r = recs[rs];
    Cu cu; cu.x = x0; cu.y = y0; cu.log2 = log2; cu.z = z_of(x0, y0); cu.nparts = 1 << (2 * (log2 - 2)); cu.r = &r;
    cu.nxn = log2 == 3 ? !e.bin(ctx, CTX_PART_SIZE) : 0;
    for (int i = 0; i < cu.nparts; i++) { r.depth[cu.z + i] = (uint8_t)depth; r.part_size[cu.z + i] = cu.nxn ? SIZE_NxN : SIZE_2Nx2N; }
    const int npu = cu.nxn ? 4 : 1, pb = cu.nxn ? 4 : (1 << log2), ppu = cu.nparts / npu;
    int prev[4], coded[4];
    for (int j = 0; j < npu; j++) prev[j] = e.bin(ctx, CTX_INTRA_PRED);
    for (int j = 0; j < npu; j++) coded[j] = prev[j] ? (e.ep() ? 1 + e.ep() : 0) : (int)e.eps(5);
    for (int j = 0; j < npu; j++) {
      const int xp = x0 + (j & 1) * pb, yp = y0 + (j >> 1) * pb;
      int left = DC, above = DC;
      if (available(rs, xp - 1, yp)) left = recs[ctu_of(xp - 1, yp)].luma_dir[z_of(xp - 1, yp)];
      if ((yp & 63) != 0 && available(rs, xp, yp - 1)) above = recs[ctu_of(xp, yp - 1)].luma_dir[z_of(xp, yp - 1)];
      int cand[3];
      if (left == above) {
        if (left > 1) { cand[0] = left; cand[1] = ((left + 29) % 32) + 2; cand[2] = ((left - 1) % 32) + 2; }
        else { cand[0] = PLANAR; cand[1] = DC; cand[2] = VER; }
      } else {
        cand[0] = left; cand[1] = above;
        cand[2] = (left && above) ? PLANAR : ((left + above) < 2 ? VER : DC);
      }
      int mode;
      if (prev[j]) mode = cand[coded[j]];
      else {
        if (cand[0] > cand[1]) std::swap(cand[0], cand[1]);
        if (cand[0] > cand[2]) std::swap(cand[0], cand[2]);
        if (cand[1] > cand[2]) std::swap(cand[1], cand[2]);
        mode = coded[j];
        for (int i = 0; i < 3; i++) if (mode >= cand[i]) mode++;
      }
      if (mode < 0 || mode > 34) { fail("a luma prediction mode above 34"); return; }
      for (int i = 0; i < ppu; i++) r.luma_dir[cu.z + j * ppu + i] = (uint8_t)mode;
    }
    int icpm = 4;
    if (e.bin(ctx, CTX_CHROMA_PRED)) icpm = (int)e.eps(2);
    const int luma0 = r.luma_dir[cu.z];
    int rec_c = DM_CHROMA; cu.mode_c = luma0;
    if (icpm != 4) {
      static const int list[4] = { PLANAR, VER, HOR, DC };
      cu.mode_c = list[icpm] == luma0 ? 34 : list[icpm];
      rec_c = cu.mode_c;
    }
    for (int i = 0; i < cu.nparts; i++) r.chroma_dir[cu.z + i] = (uint8_t)rec_c;
    transform_tree(cu, 0, log2, 0, 0, 0, 0);
    if ((ps.cu_qp_delta || qp_map) && !why) finish_cu_qp(rs, cu.z, cu.nparts);
  }

  // coding_quadtree() 7.3.8.4
  void coding_quadtree(int rs, int x0, int y0, int log2, int depth)
  {
    if (e.bad || why) return;
    const int size = 1 << log2;
    if (ps.cu_qp_delta && log2 >= 6 - ps.diff_cu_qp_depth) start_qg(x0, y0);
    int split;
    if (x0 + size <= W && y0 + size <= H && log2 > 3) {
      int inc = 0;
      if (available(rs, x0 - 1, y0)) inc += recs[ctu_of(x0 - 1, y0)].depth[z_of(x0 - 1, y0)] > depth;
      if (available(rs, x0, y0 - 1)) inc += recs[ctu_of(x0, y0 - 1)].depth[z_of(x0, y0 - 1)] > depth;
      split = e.bin(ctx, CTX_SPLIT + inc);
    } else split = log2 > 3;
    if (!split) { coding_unit(rs, x0, y0, log2, depth); return; }
    const int half = size >> 1;
    for (int k = 0; k < 4; k++) {
      const int x1 = x0 + (k & 1) * half, y1 = y0 + (k >> 1) * half;
      if (x1 < W && y1 < H) coding_quadtree(rs, x1, y1, log2 - 1, depth + 1);
    }
  }
};

struct SegmentData { SegmentHeader h; std::vector<std::pair<const uint8_t *, size_t>> subs; };

// slice_segment_data() 7.3.8.1 of every segment of a picture, with 9.3.1 / 9.3.2: where the contexts of a CTU come from
hevcdl_status decode_picture_data(Picture &p, const std::vector<SegmentData> &segs)
{
  const Grid &g = p.g;
  p.slice_addr.assign((size_t)g.n, -1);
  int ts = 0, slice_addr = -1, have_sync = 0;
  for (size_t si = 0; si < segs.size(); si++) {
    const SegmentHeader &h = segs[si].h;
    if (ts >= g.n) INVALID("a slice segment behind the picture's last CTU");
    if (h.address != g.ts2rs[(size_t)ts]) INVALID("slice_segment_address %d, the CTU behind the segment before it is %d", h.address, g.ts2rs[(size_t)ts]);
    if (h.dependent) { if (slice_addr < 0) INVALID("a dependent slice segment opens the picture"); }
    else slice_addr = h.address;
    if (segs[si].subs.empty()) INVALID("a slice segment without data");
    size_t k = 0;
    const int first_ts = ts;
    for (;;) {
      const int rs = g.ts2rs[(size_t)ts], rx = rs % g.cx, ry = rs / g.cx;
      p.slice_addr[(size_t)rs] = slice_addr;
      const bool new_tile = ts == 0 || g.tile_id[(size_t)rs] != g.tile_id[(size_t)g.ts2rs[(size_t)ts - 1]];
      const bool new_row = p.ps.wpp && rx == 0;
      if (ts == first_ts || new_tile || new_row) {
        if (ts != first_ts) k++;
        if (k >= segs[si].subs.size()) INVALID("slice segment %d has %d sub-streams, more are needed", (int)si, (int)segs[si].subs.size());
        p.e.start(segs[si].subs[k].first, segs[si].subs[k].second);
        if (p.e.bad) INVALID("a sub-stream too short for the arithmetic decoder, or one that starts with an offset of 510 / 511");
      }
      if (new_tile) p.init_contexts();
      else if (new_row) {
        if (have_sync && p.available(rs, (rx + 1) << 6, (ry - 1) << 6)) memcpy(p.ctx, p.sync, hevcdl_sd::SD_NUM_CTX);
        else p.init_contexts();
      } else if (ts == first_ts) {
        if (h.dependent) UNSUPPORTED("a dependent slice segment that starts inside a CTU row or a tile is outside this decoder");
        p.init_contexts();
      }
      if (new_tile || new_row || (ts == first_ts && !h.dependent)) { p.qp_prev = p.qp; p.grp_reset = (ts == first_ts && !h.dependent && ts != 0 && !new_tile) ? 1 : (new_tile ? 2 : 3); }      // 8.6.1: the first quantisation group of a slice, a tile, a wavefront row
      if (p.sao_on) p.sao_syntax(rs);
      p.coding_quadtree(rs, rx << 6, ry << 6, 6, 0);
      if (p.why) INVALID("CTU %d: %s", rs, p.why);
      const int end = p.e.terminate();
      if (p.e.bad) INVALID("CTU %d: the slice data ends inside the CTU", rs);
      if (p.ps.wpp && rx == 1) { memcpy(p.sync, p.ctx, hevcdl_sd::SD_NUM_CTX); have_sync = 1; }
      ts++;
      if (end) {
        if (!p.e.finish()) INVALID("rbsp_slice_segment_trailing_bits() behind CTU %d are damaged, or bytes follow them", rs);
        break;
      }
      if (ts >= g.n) INVALID("no end_of_slice_segment_flag behind the picture's last CTU");
      const int nxt = g.ts2rs[(size_t)ts];
      if (g.tile_id[(size_t)nxt] != g.tile_id[(size_t)rs] || (p.ps.wpp && nxt % g.cx == 0)) {
        if (p.e.terminate() != 1) INVALID("end_of_subset_one_bit behind CTU %d is 0", rs);
        if (!p.e.finish()) INVALID("byte_alignment() behind CTU %d is damaged, or its entry point is wrong", rs);
      }
    }
    if (k + 1 != segs[si].subs.size()) INVALID("slice segment %d has %d sub-streams, %d were used", (int)si, (int)segs[si].subs.size(), (int)k + 1);
  }
  if (ts != g.n) INVALID("the last slice segment ends behind CTU %d of %d", ts, g.n);
  return HEVCDL_OK;
}

// the sub-streams of a slice NAL unit: its entry points count bytes of the NAL unit, emulation prevention bytes included (7.4.7.1)
hevcdl_status cut_substreams(const Nal &n, SegmentData &s)
{
  const SegmentHeader &h = s.h;
  if (h.data_byte_pos >= n.rbsp.size()) INVALID("a slice NAL unit without slice segment data");
  const size_t first = n.pos[h.data_byte_pos], payload = n.size - first;
  uint64_t sum = 0;
  for (int i = 0; i < h.n_entry; i++) sum += h.entry[i];
  if (sum >= payload) INVALID("entry points add up to %llu bytes, the slice data has %llu", (unsigned long long)sum, (unsigned long long)payload);
  size_t cut = first, at = h.data_byte_pos;
  for (int i = 0; i <= h.n_entry; i++) {
    const size_t next = i < h.n_entry ? cut + h.entry[i] : n.size;
    const size_t to = (size_t)(std::lower_bound(n.pos.begin(), n.pos.end(), (uint32_t)next) - n.pos.begin());
    s.subs.push_back({ n.rbsp.data() + at, to - at });
    at = to; cut = next;
  }
  return HEVCDL_OK;
}

// what hevcdl_write_access_unit_segments would be told to write these segments: SliceMode / SliceSegmentMode and their arguments, from the first picture; every picture must
// then consist of exactly the segments those keys give
hevcdl_status derive_layouts(const ParamSets &ps, const Grid &g, const std::vector<SegmentData> &segs, hevcdl_slice_layout &sl, hevcdl_segment_layout &sg)
{
  sl.mode = 0; sl.argument = 0; sl.lf_across_slices = segs[0].h.lf_across_slices; sg.mode = 0; sg.argument = 0;
  // units: the sub-streams the writer knows -- tiles, wavefront rows, or (SliceMode 1) whole slices of CTU rows
  std::vector<int> slice_start, seg_start;          // in tile-scan CTU addresses
  for (const SegmentData &s : segs) { seg_start.push_back(g.rs2ts[(size_t)s.h.address]); if (!s.h.dependent) slice_start.push_back(seg_start.back()); }
  const bool tiled = ps.tcols * ps.trows > 1;
  auto unit_of = [&](int ts) -> int { // the index of the tile / row that starts at ts, -1: none does
    const int rs = g.ts2rs[(size_t)ts];
    if (tiled) { if (ts > 0 && g.tile_id[(size_t)rs] == g.tile_id[(size_t)g.ts2rs[(size_t)ts - 1]]) return -1; return g.tile_id[(size_t)rs]; }
    return rs % g.cx == 0 ? rs / g.cx : -1;
  };
  for (int ts : seg_start) if (unit_of(ts) < 0) UNSUPPORTED("a slice or slice segment that does not start at a CTU row or a tile is outside this decoder");
  if (slice_start.size() > 1) {
    if (tiled) { sl.mode = 3; sl.argument = unit_of(slice_start[1]); }
    else if (ps.wpp) UNSUPPORTED("several slices a picture together with wavefront are outside this decoder");
    else { sl.mode = 1; sl.argument = slice_start[1]; }
  }
  if (seg_start.size() > slice_start.size()) {
    size_t first_dep = 0;
    while (first_dep < segs.size() && !segs[first_dep].h.dependent) first_dep++;
    const int base = seg_start[first_dep - 1], at = seg_start[first_dep];
    if (tiled) { sg.mode = 3; sg.argument = unit_of(at) - unit_of(base); }
    else if (ps.wpp) { sg.mode = 1; sg.argument = at - base; }
    else UNSUPPORTED("dependent slice segments without wavefront or tiles are outside this decoder");
  }
  return HEVCDL_OK;
}
hevcdl_status check_layouts(const ParamSets &ps, const Grid &g, const std::vector<SegmentData> &segs, const hevcdl_slice_layout &sl, const hevcdl_segment_layout &sg)
{
  const bool tiled = ps.tcols * ps.trows > 1;
  // the starts the keys give, as au_assemble walks them
  std::vector<int> unit_ts;                         // first CTU (tile scan) of every unit
  if (sl.mode == 1) { for (int a = 0; a < g.n; a += std::max(sl.argument, 1)) unit_ts.push_back(a); }
  else if (tiled) { for (int ts = 0; ts < g.n; ts++) if (ts == 0 || g.tile_id[(size_t)g.ts2rs[(size_t)ts]] != g.tile_id[(size_t)g.ts2rs[(size_t)ts - 1]]) unit_ts.push_back(ts); }
  else if (ps.wpp) { for (int y = 0; y < g.cy; y++) unit_ts.push_back(y * g.cx); }
  else unit_ts.push_back(0);
  if (sl.mode == 1 && (sl.argument < 1 || sl.argument % g.cx != 0)) UNSUPPORTED("slices that are not whole CTU rows are outside this decoder");
  if (sg.mode == 1 && (sg.argument < 1 || sg.argument % g.cx != 0)) UNSUPPORTED("slice segments that are not whole CTU rows are outside this decoder");
  if ((sl.mode == 3 && sl.argument < 1) || (sg.mode == 3 && sg.argument < 1)) UNSUPPORTED("slices of no tiles");
  const int n_sub = (int)unit_ts.size(), per = sl.mode == 3 ? sl.argument : (sl.mode == 1 ? 1 : n_sub);
  const int seg_units = sg.mode == 1 ? sg.argument / g.cx : (sg.mode == 3 ? sg.argument : 0);
  size_t i = 0;
  for (int k0 = 0; k0 < n_sub; k0 += per) {
    const int k1 = std::min(k0 + per, n_sub), seg = seg_units > 0 ? seg_units : k1 - k0;
    for (int s0 = k0; s0 < k1; s0 += seg, i++) {
      if (i >= segs.size() || g.rs2ts[(size_t)segs[i].h.address] != unit_ts[(size_t)s0] || segs[i].h.dependent != (s0 > k0))
        UNSUPPORTED("the slice segments of a picture are not those of one SliceMode / SliceSegmentMode setting: outside this decoder");
    }
  }
  if (i != segs.size()) UNSUPPORTED("the slice segments of a picture are not those of one SliceMode / SliceSegmentMode setting: outside this decoder");
  return HEVCDL_OK;
}

// ---- one walk over the stream ----------------------------------------------------------------------------------------------------
// the hevcdl_stream_config a stream's parameter sets amount to, the layouts of its first picture and what its SPS / PPS carry beyond them
void fill_config(const ParamSets &active, int level_idc, int first_qp, int count, int ps_before_second, const hevcdl_slice_layout &sl, const hevcdl_segment_layout &sg, StreamShape &out)
{
  hevcdl_stream_config c;
  hevcdl_stream_config_default(&c, active.width, active.height, 26);
  c.qp = 0; c.level_idc = level_idc; c.sao_enabled = active.sao; c.loop_filter_disable = active.dbk_disabled;
  c.tile_columns = active.tcols; c.tile_rows = active.trows; c.bit_depth = active.bit_depth; c.tile_uniform_spacing = active.uniform;
  if (!active.uniform) { for (int i = 0; i < active.tcols - 1 && i < 19; i++) c.tile_column_width[i] = active.col_width[i]; for (int i = 0; i < active.trows - 1 && i < 21; i++) c.tile_row_height[i] = active.row_height[i]; }
  c.lf_across_tiles = active.lf_across_tiles;
  c.tools = (HEVCDL_TOOLS_REFERENCE & ~(uint32_t)(HEVCDL_TOOL_TSKIP | HEVCDL_TOOL_SIGN_HIDE | HEVCDL_TOOL_STRONG_INTRA)) | (active.tskip ? HEVCDL_TOOL_TSKIP : 0) |
            (active.sign_hiding ? HEVCDL_TOOL_SIGN_HIDE : 0) | (active.strong_intra ? HEVCDL_TOOL_STRONG_INTRA : 0);
  c.lf_beta_offset_div2 = active.beta_div2; c.lf_tc_offset_div2 = active.tc_div2;
  c.rewrite_param_sets = (count == 1 || ps_before_second) ? 1 : 0;
  c.wavefront = active.wpp;
  c.conf_win_left = active.conf_left; c.conf_win_right = active.conf_right; c.conf_win_top = active.conf_top; c.conf_win_bottom = active.conf_bottom;
  c.qp = first_qp;                                   // the first picture's: a stream of one QP is then described by the configuration alone
  out.cfg = c; out.slices = sl; out.segments = sg;
  out.qp.cu_qp_delta_enabled = active.cu_qp_delta; out.qp.diff_cu_qp_delta_depth = active.diff_cu_qp_depth; out.qp.cb_qp_offset = active.cb_qp_offset; out.qp.cr_qp_offset = active.cr_qp_offset;
  out.sl.enabled = active.sl_enabled; out.sl.data_present = active.sl_data_present;
  if (active.sl_enabled) memcpy(out.sl.factor, active.sl_factor, sizeof out.sl.factor); else memset(out.sl.factor, 16, sizeof out.sl.factor);
}

// Everything in front of the slice data, once: Annex B -> NAL units -> parameter sets, SEI and slice segment headers, every check in its place.  A picture whose segments are
// complete and are those of the stream's layouts goes to sink(active, grid, slices, segments, segs, picture, index) -> status: the parser decodes it there, collect_units cuts
// it into units.  `out` is written only behind the last picture (a refusal leaves it alone).
template <class Sink>
hevcdl_status walk_stream(const uint8_t *stream, size_t bytes, unsigned accept, Sink sink, StreamShape &out)
{
  std::vector<std::pair<size_t, size_t>> units;
  split_annexb(stream, bytes, units);
  if (units.empty()) INVALID("no start code in the stream");

  ParamSets ps; memset(&ps, 0, sizeof ps);
  ParamSets active; memset(&active, 0, sizeof active);
  Grid g; bool have_grid = false;
  hevcdl_slice_layout sl = { 0, 0, 1 }; hevcdl_segment_layout sg = { 0, 0 };
  std::vector<SegmentData> segs; std::vector<Nal> seg_nals;
  hevcdl_parsed_picture cur; memset(&cur, 0, sizeof cur);
  int count = 0, level_idc = 0, first_qp = 0, ps_before_second = 0;
  bool open = false;

  // the picture whose segments are collected: check them, hand them to the sink
  auto close_picture = [&]() -> hevcdl_status {
    if (!open) return HEVCDL_OK;
    open = false;
    hevcdl_status st;
    if (count == 0) { st = derive_layouts(active, g, segs, sl, sg); if (st != HEVCDL_OK) return st; }
    st = check_layouts(active, g, segs, sl, sg);
    if (st != HEVCDL_OK) return st;
    cur.n_segments = (int)segs.size();
    st = sink(active, g, sl, sg, segs, cur, count);
    if (st != HEVCDL_OK) return st;
    if (count == 0) first_qp = cur.qp;
    count++;
    segs.clear(); seg_nals.clear();
    return HEVCDL_OK;
  };

  seg_nals.reserve(units.size());
  for (const auto &u : units) {
    Nal nal;
    if (!unescape(stream + u.first, u.second - u.first, nal)) INVALID("a NAL unit of %llu bytes, or one with forbidden_zero_bit set", (unsigned long long)(u.second - u.first));
    hevcdl_status st = HEVCDL_OK;
    if (nal.type == 32) { st = close_picture(); if (st != HEVCDL_OK) return st; continue; }      // VPS: nothing a picture depends on
    if (nal.type == 33 || nal.type == 34) {
      st = close_picture(); if (st != HEVCDL_OK) return st;
      st = nal.type == 33 ? parse_sps(nal, ps, accept) : parse_pps(nal, ps, accept);
      if (st != HEVCDL_OK) return st;
      if (nal.type == 33) level_idc = ps.level_idc;
      if (count == 1) ps_before_second = 1;
      continue;
    }
    if (nal.type == 40 || nal.type == 39) { // SEI: the hash of the picture in front of it
      if (nal.type == 40 && open) { st = parse_hash_sei(nal, cur); if (st != HEVCDL_OK) return st; }
      continue;
    }
    if (nal.type == 35 || nal.type == 36 || nal.type == 37 || nal.type == 38) { if (nal.type != 38) { st = close_picture(); if (st != HEVCDL_OK) return st; } continue; }      // AUD, EOS, EOB, filler
    if (nal.type >= 32) UNSUPPORTED("NAL unit type %d is outside this decoder", nal.type);
    if (nal.type != 19 && nal.type != 20 && nal.type != 21) UNSUPPORTED("NAL unit type %d: only intra random access pictures (IDR, CRA) are decoded", nal.type);
    if (!ps.have_sps || !ps.have_pps) INVALID("a slice NAL unit in front of the SPS and the PPS");
    if (nal.rbsp.empty()) INVALID("an empty slice NAL unit");
    if (nal.rbsp[0] & 0x80) { // first_slice_segment_in_pic_flag
      st = close_picture(); if (st != HEVCDL_OK) return st;
      if (count > 0 && memcmp(&ps, &active, sizeof ps) != 0) UNSUPPORTED("parameter sets that change inside the stream are outside this decoder");
      if (count == 0) { active = ps; st = make_grid(active, g); if (st != HEVCDL_OK) return st; have_grid = true; }
      memset(&cur, 0, sizeof cur);
      open = true;
    } else if (!open) INVALID("a slice segment without the first segment of its picture");
    if (segs.size() >= (size_t)MAX_SEGMENTS) INVALID("more than %d slice segments a picture", (int)MAX_SEGMENTS);
    seg_nals.push_back(std::move(nal));
    const Nal &kept = seg_nals.back();
    SegmentData sd;
    st = parse_slice_header(kept, active, g.n, sd.h);
    if (st != HEVCDL_OK) return st;
    if (sd.h.first != (segs.empty() ? 1 : 0)) INVALID("first_slice_segment_in_pic_flag of a slice segment");
    if (!sd.h.dependent) {
      if (sd.h.sao_luma != sd.h.sao_chroma) UNSUPPORTED("SAO for one of luma / chroma only is outside this decoder");
      const int qp = active.init_qp + sd.h.qp_delta;
      if (qp < 0 || qp > 51) INVALID("slice QP %d", qp);
      if (segs.empty()) { cur.poc = sd.h.poc; cur.nal_type = sd.h.nal_type; cur.qp = qp; cur.sao = sd.h.sao_luma; cur.dbk = sd.h.dbk; cur.lf_across_slices = sd.h.lf_across_slices; }
      else if (cur.qp != qp || cur.sao != sd.h.sao_luma || memcmp(&cur.dbk, &sd.h.dbk, sizeof cur.dbk) != 0 || cur.lf_across_slices != sd.h.lf_across_slices || cur.poc != sd.h.poc)
        UNSUPPORTED("slices of one picture that differ in QP, SAO or deblocking parameters are outside this decoder");
    } else if (segs.empty()) INVALID("a dependent slice segment opens the picture");
    if (kept.type != (segs.empty() ? kept.type : cur.nal_type)) INVALID("the slice NAL units of a picture differ in their type");
    st = cut_substreams(kept, sd);
    if (st != HEVCDL_OK) return st;
    segs.push_back(std::move(sd));
  }
  { const hevcdl_status st = close_picture(); if (st != HEVCDL_OK) return st; }
  if (count == 0 || !have_grid) INVALID("no picture in the stream");
  fill_config(active, level_idc, first_qp, count, ps_before_second, sl, sg, out);
  return HEVCDL_OK;
}

} // namespace

extern "C" const char *hevcdl_parse_error(void) { return hevcdl_parse::g_error; }

extern "C" hevcdl_status hevcdl_parse_stream_sl(const uint8_t *stream, size_t bytes, unsigned accept, hevcdl_stream_config *cfg, hevcdl_slice_layout *slices, hevcdl_segment_layout *segments,
                                               hevcdl_parsed_picture *pictures, int picture_capacity, int *n_pictures, hevcdl_ctu_record *records, hevcdl_sao_blk *sao,
                                               size_t ctu_capacity, hevcdl_qp_info *qp_info, int8_t *qp_map, hevcdl_scaling_info *scaling)
{
  memset(&g_tally, 0, sizeof g_tally);
  set_error("%s", "");
  if (n_pictures) *n_pictures = 0;
  if (!stream || !cfg || !n_pictures || picture_capacity < 0) INVALID("null stream, configuration or picture count");
  if (cfg->struct_size != sizeof *cfg) INVALID("hevcdl_stream_config.struct_size is not that of this library");
  // the sink of the walk: the picture's slice data decoded by the parser's own decoder, its header handed out
  int count = 0;
  auto decode = [&](const ParamSets &active, const Grid &g, const hevcdl_slice_layout &, const hevcdl_segment_layout &, const std::vector<SegmentData> &segs, const hevcdl_parsed_picture &cur, int index) -> hevcdl_status {
    if (records) {
      if ((size_t)(index + 1) * (size_t)g.n > ctu_capacity) INVALID("room for %llu CTUs, picture %d needs %llu", (unsigned long long)ctu_capacity, index, (unsigned long long)(index + 1) * g.n);
      Picture p(active, g);
      p.recs = records + (size_t)index * g.n; p.sao = sao ? sao + (size_t)index * g.n : nullptr;
      memset(p.recs, 0, sizeof(hevcdl_ctu_record) * (size_t)g.n);
      if (p.sao) memset(p.sao, 0, sizeof(hevcdl_sao_blk) * (size_t)g.n);
      p.W = active.width; p.H = active.height; p.qp = cur.qp; p.sao_on = cur.sao; p.max_sao = (1 << (std::min(active.bit_depth, 10) - 5)) - 1;
      if (qp_map) { p.qp_map = qp_map + (size_t)index * g.n * 256; memset(p.qp_map, 0, (size_t)g.n * 256); }
      if (cur.sao && !p.sao) INVALID("the stream carries SAO parameters and there is no room for them");
      const hevcdl_status st = decode_picture_data(p, segs);
      p.close_group();
      if (st != HEVCDL_OK) return st;
    }
    if (pictures && index < picture_capacity) pictures[index] = cur;
    count = index + 1;
    return HEVCDL_OK;
  };
  StreamShape shape;
  const hevcdl_status st = walk_stream(stream, bytes, accept, decode, shape);
  if (st != HEVCDL_OK) return st;
  *n_pictures = count;
  *cfg = shape.cfg;
  if (qp_info) *qp_info = shape.qp;
  if (scaling) *scaling = shape.sl;
  if (slices) *slices = shape.slices;
  if (segments) *segments = shape.segments;
  if (pictures && count > picture_capacity) INVALID("room for %d pictures, the stream holds %d", picture_capacity, count);
  return HEVCDL_OK;
}

extern "C" hevcdl_status hevcdl_parse_stream_qp(const uint8_t *stream, size_t bytes, unsigned accept, hevcdl_stream_config *cfg, hevcdl_slice_layout *slices, hevcdl_segment_layout *segments,
                                               hevcdl_parsed_picture *pictures, int picture_capacity, int *n_pictures, hevcdl_ctu_record *records, hevcdl_sao_blk *sao,
                                               size_t ctu_capacity, hevcdl_qp_info *qp_info, int8_t *qp_map)
{
  return hevcdl_parse_stream_sl(stream, bytes, accept, cfg, slices, segments, pictures, picture_capacity, n_pictures, records, sao, ctu_capacity, qp_info, qp_map, nullptr);
}

extern "C" void hevcdl_parse_qp_tally(hevcdl_qp_tally *out) { if (out) *out = g_tally; }

extern "C" hevcdl_status hevcdl_parse_stream(const uint8_t *stream, size_t bytes, hevcdl_stream_config *cfg, hevcdl_slice_layout *slices, hevcdl_segment_layout *segments,
                                            hevcdl_parsed_picture *pictures, int picture_capacity, int *n_pictures, hevcdl_ctu_record *records, hevcdl_sao_blk *sao,
                                            size_t ctu_capacity)
{
  return hevcdl_parse_stream_qp(stream, bytes, 0, cfg, slices, segments, pictures, picture_capacity, n_pictures, records, sao, ctu_capacity, nullptr, nullptr);
}

// ---- records a caller brings itself ----------------------------------------------------------------------------------------------
namespace {
struct Validator {
  int W, H; const hevcdl_ctu_record *r; const char *why = nullptr;
  void fail(const char *s) { if (!why) why = s; }
  void tu(int z, int zrel, int np_cu, int log2, int trd, int nxn)
  {
    if (why) return;
    const int np = np_cu >> (2 * trd), zz = z + zrel, t = r->tr_idx[zz & 255];
    const bool forced = log2 > 5 || (nxn && trd == 0);
    if (forced || (log2 > 2 && t > trd)) {
      if (log2 <= 2 || (!forced && trd >= 2 + nxn)) { fail("a transform tree deeper than the SPS allows"); return; }
      for (int k = 0; k < 4; k++) tu(z, zrel + k * (np >> 2), np_cu, log2 - 1, trd + 1, nxn);
      return;
    }
    for (int i = 0; i < np; i++) if (r->tr_idx[(zz + i) & 255] != trd) { fail("tr_idx differs inside one transform unit"); return; }
    for (int c = 0; c < 3; c++) if (r->tskip[c][zz & 255] > 1) { fail("a transform-skip flag above 1"); return; }
    // a flag of a node below the leaf does not exist: bits above the unit's depth (a 4x4 chroma block's flag sits at the depth of its four luma blocks, which is the leaf's)
    for (int c = 0; c < 3; c++) for (int i = 0; i < np; i++) if (r->cbf[c][(zz + i) & 255] >> (trd + 1)) { fail("a cbf bit below the depth of its transform unit"); return; }
  }
  void cu(int x, int y, int d, int z)
  {
    if (why || x >= W || y >= H) return;
    const int size = 64 >> d, dz = r->depth[z & 255];
    if (dz > 3) { fail("a CU depth above 3"); return; }
    const bool must = x + size > W || y + size > H;
    if (d < 3 && (dz > d || must)) {
      for (int k = 0; k < 4; k++) cu(x + (k & 1) * (size >> 1), y + (k >> 1) * (size >> 1), d + 1, z + k * (256 >> (2 * d + 2)));
      return;
    }
    if (must) { fail("an 8x8 CU that crosses the picture's edge"); return; }
    const int np = 256 >> (2 * d), part = r->part_size[z & 255];
    if (dz != d) { fail("a CU depth below the depth of its position"); return; }
    if (part != SIZE_2Nx2N && !(part == SIZE_NxN && d == 3)) { fail("a part size other than 2Nx2N, or NxN in an 8x8 CU"); return; }
    for (int i = 0; i < np; i++) {
      if (r->depth[z + i] != d || r->part_size[z + i] != part) { fail("depth or part size differs inside one CU"); return; }
      if (r->luma_dir[z + i] > 34) { fail("a luma prediction mode above 34"); return; }
      const int c = r->chroma_dir[z + i];
      if (c != r->chroma_dir[z] || !(c == PLANAR || c == DC || c == HOR || c == VER || c == 34 || c == DM_CHROMA)) { fail("a chroma prediction mode outside the five of its CU"); return; }
    }
    if (part == SIZE_2Nx2N) for (int i = 1; i < np; i++) if (r->luma_dir[z + i] != r->luma_dir[z]) { fail("luma modes differ inside a 2Nx2N CU"); return; }
    tu(z, 0, np, 6 - d, 0, part == SIZE_NxN);
  }
};
} // namespace

extern "C" hevcdl_status hevcdl_validate_records(const hevcdl_stream_config *cfg, const hevcdl_ctu_record *records, int n_frames)
{
  set_error("%s", "");
  if (!cfg || cfg->struct_size != sizeof *cfg || !records || n_frames < 0) INVALID("null configuration or records");
  if (cfg->width <= 0 || cfg->height <= 0 || (cfg->width & 7) || (cfg->height & 7) || cfg->width > 16384 || cfg->height > 16384) INVALID("picture size %d x %d", cfg->width, cfg->height);
  const int cx = (cfg->width + 63) >> 6, cy = (cfg->height + 63) >> 6;
  for (int f = 0; f < n_frames; f++) for (int a = 0; a < cx * cy; a++) {
    Validator v; v.W = cfg->width; v.H = cfg->height; v.r = records + (size_t)f * cx * cy + a;
    v.cu((a % cx) * 64, (a / cx) * 64, 0, 0);
    if (v.why) INVALID("picture %d, CTU %d: %s", f, a, v.why);
  }
  return HEVCDL_OK;
}

// ---- the same stream through the shared slice-data decoder (slice_decode_core.h) ---------------------------------------------------------------------------------
// Everything in front of the slice data is walk_stream above, the walk hevcdl_parse_stream runs -- a header refusal is the parser's, sentence and place included.  Where
// the parser's sink decodes a picture, collect_units' sink cuts it into units (slice_decode_units.h); who walks them is the caller's choice: the CPU
// (hevcdl_parse_stream_core) or hevcdl_slice_decode_kernel.
namespace {
using namespace hevcdl_sd;

// the units of one picture behind check_layouts: sub-streams start at a segment, a tile and a wavefront row; units at a tile, at a row slice, or at the picture
hevcdl_status picture_units(const ParamSets &ps, const Grid &g, const hevcdl_slice_layout &sl, const std::vector<SegmentData> &segs, const hevcdl_parsed_picture &cur, StreamUnits &out)
{
  const int pic = (int)out.pictures.size();
  const size_t byte0 = out.rbsp.size(), sub0 = out.subs.size();
  const bool tiled = ps.tcols * ps.trows > 1;
  auto new_tile = [&](int ts) { return ts == 0 || g.tile_id[(size_t)g.ts2rs[(size_t)ts]] != g.tile_id[(size_t)g.ts2rs[(size_t)ts - 1]]; };
  std::vector<int> sub_ts;                          // first CTU (tile scan) of every sub-stream of the picture
  for (size_t i = 0; i < segs.size(); i++) {
    const int a = g.rs2ts[(size_t)segs[i].h.address], b = i + 1 < segs.size() ? g.rs2ts[(size_t)segs[i + 1].h.address] : g.n;
    size_t k = 0;
    for (int ts = a; ts < b; ts++) {
      if (!(ts == a || new_tile(ts) || (ps.wpp && g.ts2rs[(size_t)ts] % g.cx == 0))) continue;
      if (k < segs[i].subs.size()) {
        const auto &sb = segs[i].subs[k];
        if (out.rbsp.size() - byte0 + sb.second > 0xffffffffull) UNSUPPORTED("a picture of more than 4 GB of slice data is outside this decoder");
        out.subs.push_back({ (uint32_t)(out.rbsp.size() - byte0), (uint32_t)sb.second, 0u, 0u });
        out.rbsp.insert(out.rbsp.end(), sb.first, sb.first + sb.second);
        sub_ts.push_back(ts);
      }
      k++;
    }
    if (k != segs[i].subs.size()) INVALID("slice segment %d has %d sub-streams, %d are needed", (int)i, (int)segs[i].subs.size(), (int)k);
    out.subs.back().ends_segment = 1;
  }
  int slice_addr = 0;
  size_t si = 0, k = 0;
  for (int ts = 0; ts < g.n; ) {
    while (si < segs.size() && g.rs2ts[(size_t)segs[si].h.address] <= ts) { if (!segs[si].h.dependent) slice_addr = segs[si].h.address; si++; }
    int end = g.n;                                  // the unit [ts, end)
    if (tiled) { end = ts + 1; while (end < g.n && !new_tile(end)) end++; }
    else if (sl.mode == 1) { for (size_t j = 0; j < segs.size(); j++) { const int a = g.rs2ts[(size_t)segs[j].h.address]; if (a > ts && a < end) end = a; } }
    SdUnit u; memset(&u, 0, sizeof u);
    u.pic = pic; u.first_ts = ts; u.n_ctus = end - ts; u.slice_addr = slice_addr; u.qp = cur.qp; u.sao_on = cur.sao;
    u.sub0 = (int)(sub0 + k);
    while (k < sub_ts.size() && sub_ts[k] < end) { k++; u.n_subs++; }
    const int a = g.ts2rs[(size_t)ts], b = g.ts2rs[(size_t)end - 1];
    u.cx0 = a % g.cx; u.cy0 = a / g.cx; u.cx1 = b % g.cx + 1; u.cy1 = b / g.cx + 1;
    out.units.push_back(u);
    ts = end;
  }
  for (size_t j = out.pic_unit.back(); j < out.units.size(); j++) out.units[j].rbsp_bytes = (uint32_t)(out.rbsp.size() - byte0);
  out.pictures.push_back(cur);
  out.pic_byte.push_back(out.rbsp.size()); out.pic_sub.push_back(out.subs.size()); out.pic_unit.push_back(out.units.size());
  return HEVCDL_OK;
}

// collect_units' sink of the walk: where the parser decodes a picture, it is cut into units (headers only: just kept)
hevcdl_status collect_loop(const uint8_t *stream, size_t bytes, int want_slice_data, int have_sao, size_t ctu_capacity, StreamUnits &out, unsigned accept)
{
  auto cut = [&](const ParamSets &active, const Grid &g, const hevcdl_slice_layout &sl, const hevcdl_segment_layout &, const std::vector<SegmentData> &segs, const hevcdl_parsed_picture &cur, int index) -> hevcdl_status {
    if (index == 0) out.ctus = g.n;
    if (!want_slice_data) { out.pictures.push_back(cur); return HEVCDL_OK; }
    if ((size_t)(index + 1) * (size_t)g.n > ctu_capacity) INVALID("room for %llu CTUs, picture %d needs %llu", (unsigned long long)ctu_capacity, index, (unsigned long long)(index + 1) * g.n);
    if (cur.sao && !have_sao) INVALID("the stream carries SAO parameters and there is no room for them");
    if (index == 0) {
      SdStream &d = out.sd;
      d.W = active.width; d.H = active.height; d.ctus_x = g.cx; d.ctus_y = g.cy; d.wpp = active.wpp; d.tskip = active.tskip; d.sign_hiding = active.sign_hiding;
      d.max_sao = (1 << (std::min(active.bit_depth, 10) - 5)) - 1; d.row_slices = sl.mode == 1;
      d.cu_qp = active.cu_qp_delta; d.log2_qg = 6 - active.diff_cu_qp_depth; d.qp_bd_offset = 6 * (active.bit_depth - 8);
    }
    for (const SegmentData &s : segs) if (s.subs.empty()) INVALID("a slice segment without data");
    return picture_units(active, g, sl, segs, cur, out);
  };
  return walk_stream(stream, bytes, accept, cut, out);
}

// the units of pictures [0, n) on the CPU, in the parser's order: the first error met is the lowest picture's first
hevcdl_status walk_units_host(void *, const StreamUnits &su, int n, hevcdl_ctu_record *records, hevcdl_sao_blk *sao, int8_t *qp_map, int *bad_pic, SdResult *res)
{
  uint8_t ctx[EC_SYNC_BYTES], sync[EC_SYNC_BYTES], dry_depth[512], dry_dir[512]; uint16_t cg_pos[16]; int16_t cg_val[16]; int8_t qp_cur[256] = { 0 };
  SdState s; memset(&s, 0, sizeof s);
  s.t = &ec_tables(); s.s = &su.sd; s.ctx = ctx; s.sync = sync; s.cg_pos = cg_pos; s.cg_val = cg_val; s.dry_depth = dry_depth; s.dry_dir = dry_dir; s.qp_cur = qp_cur;
  *bad_pic = -1;
  for (size_t i = 0; i < su.pic_unit[(size_t)n]; i++) {
    SdUnit u = su.units[i];
    u.rbsp0 = 0;
    s.recs = records + (size_t)u.pic * su.ctus; s.sao = sao ? sao + (size_t)u.pic * su.ctus : nullptr; s.qp_map = qp_map ? qp_map + (size_t)u.pic * su.ctus * 256 : nullptr;
    const SdResult r = sd_decode_unit(s, u, su.subs.data(), (int)su.subs.size(), su.rbsp.data() + su.pic_byte[(size_t)u.pic], su.pic_byte[(size_t)u.pic + 1] - su.pic_byte[(size_t)u.pic]);
    if (r.code != SD_OK) { *bad_pic = u.pic; *res = r; return HEVCDL_OK; }
  }
  return HEVCDL_OK;
}
} // namespace

namespace hevcdl_parse {
void set_slice_error(int pic, const SdResult &res)
{
  if (res.ctu >= 0) set_error("picture %d, CTU %d: %s", pic, res.ctu, sd_error_sentence(res.code));
  else set_error("picture %d: %s", pic, sd_error_sentence(res.code));
}

hevcdl_status collect_units(const uint8_t *stream, size_t bytes, int want_slice_data, int have_sao, size_t ctu_capacity, StreamUnits &out, unsigned accept)
{
  out.pic_byte.assign(1, 0); out.pic_sub.assign(1, 0); out.pic_unit.assign(1, 0);
  const hevcdl_status st = collect_loop(stream, bytes, want_slice_data, have_sao, ctu_capacity, out, accept);
  if (st == HEVCDL_OK) return st;
  // (a picture that was refused half way through its units leaves nothing behind)
  out.rbsp.resize(out.pic_byte.back()); out.subs.resize(out.pic_sub.back()); out.units.resize(out.pic_unit.back());
  if (!want_slice_data || out.pictures.empty()) return st;
  out.pending = st; snprintf(out.pending_sentence, sizeof out.pending_sentence, "%s", g_error);
  return HEVCDL_OK;
}

hevcdl_status batch_tables(const StreamUnits &su, int first, int count, std::vector<SdUnit> &units, size_t &sub0, size_t &n_subs, size_t &byte0, size_t &n_bytes)
{
  if (first < 0 || count < 1 || (size_t)first + (size_t)count > su.pictures.size()) INVALID("a batch outside the stream's pictures");
  sub0 = su.pic_sub[(size_t)first]; n_subs = su.pic_sub[(size_t)first + count] - sub0;
  byte0 = su.pic_byte[(size_t)first]; n_bytes = su.pic_byte[(size_t)first + count] - byte0;
  if (n_bytes > 0xffffffffull) UNSUPPORTED("a batch of more than 4 GB of slice data: decode fewer pictures a batch");
  units.assign(su.units.begin() + (ptrdiff_t)su.pic_unit[(size_t)first], su.units.begin() + (ptrdiff_t)su.pic_unit[(size_t)first + count]);
  for (SdUnit &u : units) { u.rbsp0 = (uint32_t)(su.pic_byte[(size_t)u.pic] - byte0); u.sub0 -= (int)sub0; u.pic -= first; }
  return HEVCDL_OK;
}

hevcdl_status parse_stream_with(UnitWalker walk, void *user, const uint8_t *stream, size_t bytes, hevcdl_stream_config *cfg, hevcdl_slice_layout *slices, hevcdl_segment_layout *segments,
                                hevcdl_parsed_picture *pictures, int picture_capacity, int *n_pictures, hevcdl_ctu_record *records, hevcdl_sao_blk *sao, size_t ctu_capacity,
                                unsigned accept, hevcdl_qp_info *qp_info, int8_t *qp_map, hevcdl_scaling_info *scaling)
{
  set_error("%s", "");
  if (n_pictures) *n_pictures = 0;
  if (!stream || !cfg || !n_pictures || picture_capacity < 0) INVALID("null stream, configuration or picture count");
  if (cfg->struct_size != sizeof *cfg) INVALID("hevcdl_stream_config.struct_size is not that of this library");
  StreamUnits su;
  hevcdl_status st = collect_units(stream, bytes, records != nullptr, sao != nullptr, ctu_capacity, su, accept);
  if (st != HEVCDL_OK) return st;
  const int count = (int)su.pictures.size();
  for (int i = 0; i < count && pictures && i < picture_capacity; i++) pictures[i] = su.pictures[(size_t)i];
  if (records) {
    int bad_pic = -1; SdResult res = { SD_OK, -1 };
    st = walk(user, su, count, records, sao, qp_map, &bad_pic, &res);
    if (st != HEVCDL_OK) return st;
    if (bad_pic >= 0) { set_slice_error(bad_pic, res); return HEVCDL_ERR_INVALID_ARG; }
  }
  if (su.pending != HEVCDL_OK) { set_error("%s", su.pending_sentence); return su.pending; }
  *n_pictures = count;
  *cfg = su.cfg;
  if (qp_info) *qp_info = su.qp;
  if (scaling) *scaling = su.sl;
  if (slices) *slices = su.slices;
  if (segments) *segments = su.segments;
  if (pictures && count > picture_capacity) INVALID("room for %d pictures, the stream holds %d", picture_capacity, count);
  return HEVCDL_OK;
}
} // namespace hevcdl_parse

extern "C" hevcdl_status hevcdl_parse_stream_core(const uint8_t *stream, size_t bytes, hevcdl_stream_config *cfg, hevcdl_slice_layout *slices, hevcdl_segment_layout *segments,
                                                 hevcdl_parsed_picture *pictures, int picture_capacity, int *n_pictures, hevcdl_ctu_record *records, hevcdl_sao_blk *sao,
                                                 size_t ctu_capacity)
{
  return parse_stream_with(walk_units_host, nullptr, stream, bytes, cfg, slices, segments, pictures, picture_capacity, n_pictures, records, sao, ctu_capacity);
}

extern "C" hevcdl_status hevcdl_parse_stream_core_qp(const uint8_t *stream, size_t bytes, unsigned accept, hevcdl_stream_config *cfg, hevcdl_slice_layout *slices, hevcdl_segment_layout *segments,
                                                    hevcdl_parsed_picture *pictures, int picture_capacity, int *n_pictures, hevcdl_ctu_record *records, hevcdl_sao_blk *sao,
                                                    size_t ctu_capacity, hevcdl_qp_info *qp_info, int8_t *qp_map)
{
  return parse_stream_with(walk_units_host, nullptr, stream, bytes, cfg, slices, segments, pictures, picture_capacity, n_pictures, records, sao, ctu_capacity, accept, qp_info, qp_map);
}

extern "C" hevcdl_status hevcdl_parse_stream_core_sl(const uint8_t *stream, size_t bytes, unsigned accept, hevcdl_stream_config *cfg, hevcdl_slice_layout *slices, hevcdl_segment_layout *segments,
                                                    hevcdl_parsed_picture *pictures, int picture_capacity, int *n_pictures, hevcdl_ctu_record *records, hevcdl_sao_blk *sao,
                                                    size_t ctu_capacity, hevcdl_qp_info *qp_info, int8_t *qp_map, hevcdl_scaling_info *scaling)
{
  return parse_stream_with(walk_units_host, nullptr, stream, bytes, cfg, slices, segments, pictures, picture_capacity, n_pictures, records, sao, ctu_capacity, accept, qp_info, qp_map, scaling);
}
