// slice_grid.h -- what a configuration's slice keys make of the grid a context runs.  A pure function of the configuration (plain C++, no HIP: hevcdl_create calls it,
// tests/slices_harness.cpp runs it on a CPU).
//
// SliceMode 1 over whole CTU rows IS a tile grid of one column in everything a context computes (decisions, deblocking, SAO statistics and merge candidates; DESIGN.md
// section 5f): the grid configuration carries that grid in its tile fields and lf_across_slices in lf_across_tiles' place.  Its one column may be narrower than the four
// CTUs a tile column needs: that is a limit of tiles, not of slices.  SliceMode 3 keeps the cfg's tiles: only the stream changes.
#ifndef HEVCDL_SLICE_GRID_H
#define HEVCDL_SLICE_GRID_H
#include "hevcdl.h"

// Dependent slice segments (SliceSegmentMode 1 over WaveFrontSynchro rows, 3 over tiles) change nothing a context computes: they are checked here and
// then taken OUT of the grid configuration, so that launch plan, workspace and parameter blocks cannot see them; the context keeps them for the stream alone.
static inline hevcdl_status hevcdl_segment_keys(const hevcdl_config *cfg, const char **why)
{
  *why = "";
  if (cfg->slice_segment_mode == 0) return HEVCDL_OK;
  const int cx = (cfg->width + 63) >> 6, tiled = cfg->tile_columns * cfg->tile_rows > 1;
#define SEGMENT_REFUSE(status, text) do { *why = text; return status; } while (0)
  if (cfg->slice_segment_mode == 2) SEGMENT_REFUSE(HEVCDL_ERR_UNSUPPORTED, "SliceSegmentMode 2 (slice segments by bytes) is not supported: the segment borders would depend on the coded bytes");
  if (cfg->slice_segment_mode != 1 && cfg->slice_segment_mode != 3) SEGMENT_REFUSE(HEVCDL_ERR_INVALID_ARG, "SliceSegmentMode is 0, 1 or 3");
  if (cfg->deblocking_metric != 0) SEGMENT_REFUSE(HEVCDL_ERR_UNSUPPORTED, "slice segments together with DeblockingFilterMetric are not supported");
  if (cfg->slice_segment_mode == 1) {
    if (tiled) SEGMENT_REFUSE(HEVCDL_ERR_UNSUPPORTED, "SliceSegmentMode 1 together with tiles is not supported (SliceSegmentMode 3 cuts a picture of tiles into segments)");
    if (cfg->slice_mode != 0) SEGMENT_REFUSE(HEVCDL_ERR_UNSUPPORTED, "SliceSegmentMode 1 together with slices is not supported (row slices are refused with WaveFrontSynchro, which these segments need)");
    if (!cfg->wavefront)
      SEGMENT_REFUSE(HEVCDL_ERR_UNSUPPORTED, "SliceSegmentMode 1 needs WaveFrontSynchro: without it a segment starts in the middle of a coder chain and the reference's decisions change from its first CTU on");
    if (cfg->slice_segment_argument < 1 || cfg->slice_segment_argument % cx != 0)
      SEGMENT_REFUSE(HEVCDL_ERR_UNSUPPORTED, "SliceSegmentMode 1 needs a SliceSegmentArgument that is a positive multiple of the picture's width in CTUs: a segment that starts inside a CTU row changes the reference's decisions");
    return HEVCDL_OK;
  }
  if (!tiled) SEGMENT_REFUSE(HEVCDL_ERR_INVALID_ARG, "SliceSegmentMode 3 (segments of whole tiles) needs tiles");
  if (cfg->slice_segment_argument < 1) SEGMENT_REFUSE(HEVCDL_ERR_INVALID_ARG, "SliceSegmentMode 3 needs a SliceSegmentArgument of at least 1 tile");
#undef SEGMENT_REFUSE
  return HEVCDL_OK;
}

// cfg (valid but for its slice and segment keys) -> *grid, or the status of the refusal and, in *why, its sentence
static inline hevcdl_status hevcdl_slice_grid(const hevcdl_config *cfg, hevcdl_config *grid, const char **why)
{
  *grid = *cfg;
  { const hevcdl_status ss = hevcdl_segment_keys(cfg, why); if (ss != HEVCDL_OK) return ss; }
  grid->slice_segment_mode = grid->slice_segment_argument = 0;
  if (cfg->slice_mode == 0) return HEVCDL_OK;
  const int cx = (cfg->width + 63) >> 6, cy = (cfg->height + 63) >> 6, tiled = cfg->tile_columns * cfg->tile_rows > 1;
#define SLICE_REFUSE(status, text) do { *why = text; return status; } while (0)
  if (cfg->slice_mode == 2) SLICE_REFUSE(HEVCDL_ERR_UNSUPPORTED, "SliceMode 2 (slices by bytes) is not supported: the slice borders would depend on the coded bytes");
  if (cfg->slice_mode != 1 && cfg->slice_mode != 3) SLICE_REFUSE(HEVCDL_ERR_INVALID_ARG, "SliceMode is 0, 1 or 3");
  if (cfg->deblocking_metric != 0) SLICE_REFUSE(HEVCDL_ERR_UNSUPPORTED, "slices together with DeblockingFilterMetric are not supported");
  if (cfg->slice_mode == 1) {
    if (tiled) SLICE_REFUSE(HEVCDL_ERR_UNSUPPORTED, "SliceMode 1 together with tiles is not supported (SliceMode 3 cuts a picture of tiles into slices)");
    if (cfg->wavefront) SLICE_REFUSE(HEVCDL_ERR_UNSUPPORTED, "slices together with WaveFrontSynchro are not supported");
    if (cfg->slice_argument < 1 || cfg->slice_argument % cx != 0)
      SLICE_REFUSE(HEVCDL_ERR_UNSUPPORTED, "SliceMode 1 needs a SliceArgument that is a positive multiple of the picture's width in CTUs: only slices of whole CTU rows are supported");
    const int rows = cfg->slice_argument / cx, n = (cy + rows - 1) / rows;
    if (n > 22) SLICE_REFUSE(HEVCDL_ERR_UNSUPPORTED, "SliceMode 1: at most 22 slices a picture are supported");
    grid->tile_columns = 1; grid->tile_rows = n; grid->tile_uniform_spacing = 0; grid->lf_across_tiles = cfg->lf_across_slices != 0;
    for (int i = 0; i < 21; i++) grid->tile_row_height[i] = i < n - 1 ? rows : 0;
    return HEVCDL_OK;
  }
  if (!tiled) SLICE_REFUSE(HEVCDL_ERR_INVALID_ARG, "SliceMode 3 (slices of whole tiles) needs tiles");
  if (cfg->slice_argument < 1) SLICE_REFUSE(HEVCDL_ERR_INVALID_ARG, "SliceMode 3 needs a SliceArgument of at least 1 tile");
  // A border between two slices is crossed when both flags say so (tests/golden/slices_t512_a1_lf0.npz); a tile border inside a slice follows lf_across_tiles alone
  // (tools/gen_slice_fixtures.py checks it).  The filter kernels have one flag for all tile borders: the one combination that needs two is refused.
  if (cfg->slice_argument > 1 && cfg->lf_across_tiles != 0 && cfg->lf_across_slices == 0)
    SLICE_REFUSE(HEVCDL_ERR_UNSUPPORTED, "SliceMode 3 with more than one tile a slice, LFCrossTileBoundaryFlag 1 and LFCrossSliceBoundaryFlag 0 is not supported: the in-loop filters would cross the tile borders inside a slice and stop at those between slices");
#undef SLICE_REFUSE
  grid->lf_across_tiles = cfg->lf_across_tiles != 0 && cfg->lf_across_slices != 0;
  return HEVCDL_OK;
}
#endif
