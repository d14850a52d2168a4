// slice_grid.h -- what a configuration's slice keys make of the grid a context runs.  A pure function of the configuration (plain C++, no HIP: hevcdl_create calls it,
// tests/slices_harness.cpp runs it on a CPU).
//
// SliceMode 1 over whole CTU rows IS a tile grid of one column in everything a context computes (decisions, deblocking, SAO statistics and merge candidates; DESIGN.md
// section 5f): the grid configuration carries that grid in its tile fields and lf_across_slices in lf_across_tiles' place.  Its one column may be narrower than the four
// CTUs a tile column needs: that is a limit of tiles, not of slices.  SliceMode 3 keeps the cfg's tiles: only the stream changes.
#ifndef HEVCDL_SLICE_GRID_H
#define HEVCDL_SLICE_GRID_H
#include "hevcdl.h"

// cfg (valid but for its slice keys) -> *grid, or the status of the refusal and, in *why, its sentence
static inline hevcdl_status hevcdl_slice_grid(const hevcdl_config *cfg, hevcdl_config *grid, const char **why)
{
  *grid = *cfg; *why = "";
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
