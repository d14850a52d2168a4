// hevcdl_parse.h -- what the stream parser (hevcdl_parse.cpp, host C++ without a HIP header) shares with the rest of the library.
//
// hevcdl_parse_stream reads the streams hevcdl_write_access_unit* produces (and the reference encoder's of the same configuration) back into the structures the
// writer takes.  Of a hevcdl_ctu_record it fills every field the stream determines:
//   depth, part_size            of every 4x4 partition of a coded CU (partitions outside the picture stay 0)
//   luma_dir                    per prediction block (four of an NxN CU)
//   chroma_dir                  the CU's mode; DM_CHROMA (36) for intra_chroma_pred_mode 4, 34 where the coded mode equals the luma mode
//   tr_idx                      the depth of the transform unit a partition lies in
//   cbf[3]                      bit d: the flag of the partition's transform-tree node of depth d (luma: every depth down to its leaf, as the reference keeps it; a 4x4 chroma block
//                               repeats its flag at the depth of its four luma blocks)
//   tskip[3]                    transform_skip_flag at the first partition of a 4x4 block that has one in the stream (a 4x4 chroma block: at the first of its four partitions)
//   coeff_y, coeff_cb, coeff_cr the levels, hidden signs resolved
// bits, dist and cost are 0: a stream does not carry the encoder's statistics.
// Scaling lists (HEVCDL_ACCEPT_SCALING_LISTS, hevcdl_parse_stream_sl) change no record either: the factors are one block of the stream, hevcdl_scaling_info.
// QpY is NOT a field of the record: with HEVCDL_ACCEPT_CU_QP (hevcdl_parse_stream_qp) it goes into a map beside the records, int8 [pictures][ctus][256] in z-order.
#ifndef HEVCDL_PARSE_H
#define HEVCDL_PARSE_H
#include <stddef.h>
#include <stdint.h>
#include "hevcdl.h"

namespace hevcdl_parse {

enum { MAX_TILE_COLS = 20, MAX_TILE_ROWS = 22, MAX_SEGMENTS = 512 };

// sequence and picture parameter sets, as far as a stream of the accepted surface uses them
struct ParamSets {
  int have_sps, have_pps;
  int width, height, bit_depth, level_idc, log2_poc, sao, strong_intra, num_st_rps, long_term, temporal_mvp;
  int conf_left, conf_right, conf_top, conf_bottom;      // luma samples
  int dep_slices, output_flag_present, extra_bits, sign_hiding, init_qp, tskip, tiles, wpp, tcols, trows, uniform, lf_across_tiles, lf_across_slices;
  int col_width[MAX_TILE_COLS], row_height[MAX_TILE_ROWS];
  int dbk_control, dbk_override_enabled, dbk_disabled, beta_div2, tc_div2;
  int cu_qp_delta, diff_cu_qp_depth, cb_qp_offset, cr_qp_offset;      // all 0 unless the caller accepts them (HEVCDL_ACCEPT_CU_QP)
  // scaling lists of the SPS (HEVCDL_ACCEPT_SCALING_LISTS, else all 0): the flags and, with sl_enabled, ScalingFactor of 7.4.5 in the layout of hevcdl_scaling_info
  int sl_enabled, sl_data_present; uint8_t sl_factor[HEVCDL_SCALING_FACTOR_BYTES];
};

// one slice segment header
struct SegmentHeader {
  int nal_type, first, dependent, address, poc, sao_luma, sao_chroma, qp_delta;
  hevcdl_dbk_choice dbk;
  int lf_across_slices;
  int n_entry; uint32_t entry[MAX_SEGMENTS];
  size_t data_byte_pos;          // first byte of slice_segment_data() in the unescaped NAL unit
};

void set_error(const char *fmt, ...);

} // namespace hevcdl_parse
#endif
