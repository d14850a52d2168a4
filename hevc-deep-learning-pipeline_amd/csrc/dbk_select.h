// dbk_select.h -- the host side of the per-picture deblocking parameters (cfg key DeblockingFilterMetric): pure functions, no HIP header, so that a stand-alone
// harness compiles them with any compiler and sanitizer (tests/dbk_select_harness.cpp).  The device side is csrc/dbk_select_kernel.hip.
//
// Replaces the tail of TEncGOP::applyDeblockingFilterMetric (TEncGOP.cpp:3259-3301): the picture's two sums -> one offset for beta and tc, override on or off.
#ifndef HEVCDL_DBK_SELECT_H
#define HEVCDL_DBK_SELECT_H
#include <stdint.h>

// deblocking tables (TComLoopFilter.cpp:59-67)
static const unsigned char HEVCDL_DBK_TC[54] = { 0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,1,1,1,1,1,1,1,1,1,2,2,2,2,3,3,3,3,4,4,4,5,5,6,6,7,8,9,10,11,13,14,16,18,20,22,24 };
static const unsigned char HEVCDL_DBK_BETA[52] = { 0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,0,6,7,8,9,10,11,12,13,14,15,16,17,18,20,22,24,26,28,30,32,34,36,38,40,42,44,46,48,50,52,54,56,58,60,62,64 };

// The two thresholds a line's second derivative must lie strictly between (TEncGOP.cpp:3206-3211): beta is TComLoopFilter::getBeta(qp), the table entry of the slice QP
// without any offset.
static inline void hevcdl_dbk_metric_thresholds(int qp, int bit_depth, int *thr1, int *thr2)
{
  const int scale = 1 << (bit_depth - 8), beta = HEVCDL_DBK_BETA[qp < 0 ? 0 : (qp > 51 ? 51 : qp)] * scale;
  *thr1 = 2 * scale; *thr2 = beta >> 2;
}

// Edges that count: the first (size >> 5) - 1 of the edges at multiples of 32 (TEncGOP.cpp:3196-3197, 3261-3268) -- at a size that is no multiple of 32 the last edge is
// computed by the reference and dropped.  0 or less: the reference asserts (and would divide by zero).
static inline int hevcdl_dbk_metric_edges(int size) { return (size >> 5) - 1; }

// TEncGOP.cpp:3270-3283, line for line: -> the offset (2 .. 6) of an override, or 0: no override.
static inline int hevcdl_dbk_metric_offset(int width, int height, int bit_depth, uint64_t col_sum, uint64_t row_sum)
{
  const uint64_t no_col = (uint64_t)(width >> 5), no_rows = (uint64_t)(height >> 5);
  col_sum <<= 10; row_sum <<= 10;
  col_sum /= (no_col - 1); col_sum /= (uint64_t)height;
  row_sum /= (no_rows - 1); row_sum /= (uint64_t)width;
  uint64_t avg = (col_sum + row_sum) >> 1;
  avg >>= (bit_depth - 8);
  if (avg <= 2048) return 0;
  avg >>= 9;
  return avg < 2 ? 2 : (avg > 6 ? 6 : (int)avg);
}

// ---- DeblockingFilterMetric 2: the walk of TEncGOP::applyDeblockingFilterParameterSelection (TEncGOP.cpp:3335-3420) over a table of trial distortions ----------------
// The carried state is the reference's m_DBParam[0] (an all-intra sequence has one quality layer): whether a picture has been searched, and its best.
typedef struct hevcdl_dbk_walk_state { int32_t available, disabled, beta_offset_div2, tc_offset_div2; } hevcdl_dbk_walk_state;
typedef struct hevcdl_dbk_walk_result { int32_t override_flag, disabled, beta_offset_div2, tc_offset_div2; } hevcdl_dbk_walk_result;
static inline int hevcdl_dbk_clip3(int lo, int hi, int v) { return v < lo ? lo : (v > hi ? hi : v); }
// table[7 (b + 3) + (t + 3)]: the distortion of the picture filtered with slice_beta_offset_div2 b and slice_tc_offset_div2 t.  Windows of +-1 (beta) and +-2 (tc) round
// the previous best once there is one, descending order, strict comparisons, both early breaks, the final override / no-override rule.  Only entries the reference would
// have computed are read.  state is advanced in place.
static inline hevcdl_dbk_walk_result hevcdl_dbk_walk(const uint64_t *table, int pps_beta_offset_div2, int pps_tc_offset_div2, hevcdl_dbk_walk_state *state)
{
  const int lo = -3, hi = 3;
  const int narrow = state->available && !state->disabled;                                     // bNoFiltering, :3335
  const int max_b = narrow ? hevcdl_dbk_clip3(lo, hi, state->beta_offset_div2 + 1) : hi, min_b = narrow ? hevcdl_dbk_clip3(lo, hi, state->beta_offset_div2 - 1) : lo;
  const int max_t = narrow ? hevcdl_dbk_clip3(lo, hi, state->tc_offset_div2 + 2) : hi, min_t = narrow ? hevcdl_dbk_clip3(lo, hi, state->tc_offset_div2 - 2) : lo;
  uint64_t dist_beta_prev = UINT64_MAX, dist_min = UINT64_MAX;
  int disabled_best = 1, beta_best = 0, tc_best = 0;
  for (int b = max_b; b >= min_b; b--) {
    uint64_t dist_tc_min = UINT64_MAX;
    for (int t = max_t; t >= min_t; t--) {
      const uint64_t dist = table[7 * (b + 3) + (t + 3)];
      if (dist < dist_min) { dist_min = dist; disabled_best = 0; beta_best = b; tc_best = t; }
      if (dist < dist_tc_min) dist_tc_min = dist;
      else if (t < -2) break;
    }
    if (b < -1 && dist_tc_min >= dist_beta_prev) break;
    dist_beta_prev = dist_tc_min;
  }
  state->available = 1; state->disabled = disabled_best; state->beta_offset_div2 = beta_best; state->tc_offset_div2 = tc_best;      // :3386-3389
  hevcdl_dbk_walk_result r;
  if (disabled_best) { r.override_flag = 1; r.disabled = 1; r.beta_offset_div2 = 0; r.tc_offset_div2 = 0; }
  else if (beta_best == pps_beta_offset_div2 && tc_best == pps_tc_offset_div2) { r.override_flag = 0; r.disabled = 0; r.beta_offset_div2 = pps_beta_offset_div2; r.tc_offset_div2 = pps_tc_offset_div2; }
  else { r.override_flag = 1; r.disabled = 0; r.beta_offset_div2 = beta_best; r.tc_offset_div2 = tc_best; }
  return r;
}
#endif
