// rd_launch_plan.h -- the launch plan of the decision kernel: which of its four builds a launch runs, on how many workgroups, in which form.  A pure function of what
// the context was created with and of the call's arguments (plain C++, no HIP: hevcdl_api.hip launches what it returns, tests/rd_plan_harness.cpp prints it on a CPU).
#ifndef HEVCDL_RD_LAUNCH_PLAN_H
#define HEVCDL_RD_LAUNCH_PLAN_H
#include <stddef.h>
#include <stdio.h>
#include <algorithm>
#include "hevcdl.h"

enum { RD_NARROW, RD_WIDE, RD_TOOLS, RD_BD10, RD_BUILDS };      // rows of hevcdl_api.hip's rd_builds
static const char *const rd_build_names[RD_BUILDS] = { "hevcdl_rd_frame_kernel", "hevcdl_rd_frame_kernel_wide", "hevcdl_rd_frame_kernel_tools", "hevcdl_rd_frame_kernel_bd10" };      // as hevcdl_last_rd_launch reports them

// what the plan reads of a context
struct RdPlanContext {
  int n_cus = 0, max_frames = 1, bit_depth = 8; unsigned tools = HEVCDL_TOOLS_REFERENCE; int exec_flags = 0, wavefront = 0;
  int tile_columns = 1, tile_rows = 1, ctus_x = 1, ctus_y = 1;
  int waves[RD_BUILDS] = { 0, 0, 0, 0 };      // wavefronts per workgroup of each build
  long long max_units() const { return (long long)max_frames * (wavefront ? ctus_y : tile_columns * tile_rows); }
  // workgroups of a launch: one per CU, fewer when the context cannot hold that many units
  int rd_groups() const { return (int)std::min<long long>(n_cus, max_units()); }
  // (launches of few units run on every CU: the workgroups without a unit take second luma passes from the others -- they need a workspace too)
  int remote_groups() const { return (bit_depth == 8 && !(exec_flags & HEVCDL_EXEC_NO_UNIT_HANDOVER) && n_cus >= 8 && n_cus <= 1024) ? n_cus : 0; }
};

// The plan's view of a context: `grid` is the configuration the context RUNS (with SliceMode 1 a column of row slices in the tile fields: slice_grid.h), so a slice
// context plans exactly like the tile context with the same grid.  waves: wavefronts per workgroup of each build.
static inline RdPlanContext rd_plan_context_of(const hevcdl_config &grid, int n_cus, const int *waves)
{
  RdPlanContext pc;
  pc.n_cus = n_cus; pc.max_frames = grid.max_frames; pc.bit_depth = grid.bit_depth; pc.tools = grid.tools; pc.exec_flags = grid.exec_flags; pc.wavefront = grid.wavefront;
  pc.tile_columns = grid.tile_columns; pc.tile_rows = grid.tile_rows; pc.ctus_x = (grid.width + 63) >> 6; pc.ctus_y = (grid.height + 63) >> 6;
  for (int b = 0; b < RD_BUILDS; b++) pc.waves[b] = waves[b];
  return pc;
}

// the arguments of one launch.  ctu_end / tile_count < 0: all of them; session_frame >= 0: the per-CTU session's frame (hevcdl_compress_ctu)
struct RdLaunchArgs { int n_frames = 0, ctu_begin = 0, ctu_end = -1; bool cabac_in = false, cabac_out = false; int tile_begin = 0, tile_count = -1, session_frame = -1; };

struct RdLaunchPlan {
  hevcdl_status status = HEVCDL_OK;      // HEVCDL_ERR_UNSUPPORTED: WaveFrontSynchro with a partial launch
  int build = RD_NARROW, waves = 0, n_units = 0, tile_count = 0;
  int groups = 0, grid = 0;              // workgroups that hold units; workgroups launched: `groups`, or every CU's in the few-units form
  long long walkers = 0; int master_groups = 0;
  int wpp = 0; bool wpp_session = false; // 0: no WaveFrontSynchro, 1: rows on waves of their own, 2: a wave walks a frame's rows in order -- for the per-CTU session: the rows' contexts stay from call to call
  int wpp_masters = 0, migrate = 0, remote = 0;
  size_t sched_clear = 0;                // bytes of the hand-over area the launch wants zeroed (unit hand-over: then seeded with the dealing; few units: counter, queue, ring)
  size_t scratch_blocks() const { return (size_t)grid * (size_t)waves; }      // the workspace: one block per wave of every workgroup of the launch
  bool cooperative() const { return migrate || remote || wpp == 1; }          // workgroups that wait for each other
};

// Which build of the decision kernel a launch runs: `walkers` units under way on `groups` workgroups, few_units = the few-units form (hevcdl_rd_params.remote).
// Measured at 2160p on 256 CUs, eight- / ten-wave build (rd_kernel_wide.hip: 168 registers per lane instead of 256, no look-ahead
// region): 200 frames 3.53 / 4.21 s, 300 frames 4.16 / 4.59 s, 450 frames 5.17 / 5.21 s, 600 frames 6.24 / 6.11 s, 1024 frames 10.33 / 9.50 s, 2048 frames
// 16.08 / 15.66 s, 2560 frames 21.47 / 18.14 s -- but the ten-wave build moves three times the bytes (600 frames: 5.8 MB per CTU through the L2s against 1.85 MB:
// register spills at 168 registers, the CU walk's snapshots in HBM).  It is chosen where it clearly pays: from three units per workgroup on (round 5; four before).  Launches in the
// few-units form keep the eight-wave build.
static inline int rd_build_of(const RdPlanContext &c, bool few_units, long long walkers, int groups)
{
  if (c.bit_depth != 8) return RD_BD10;
  if (c.tools != HEVCDL_TOOLS_REFERENCE) return RD_TOOLS;      // a context with other tool switches than the reference cfg's runs the build that reads them: rd_kernel_tools.hip, eight waves
  if (c.exec_flags & HEVCDL_EXEC_RD_NARROW) return RD_NARROW;
  if (c.exec_flags & HEVCDL_EXEC_RD_WIDE) return RD_WIDE;
  return (!few_units && walkers >= 3LL * groups) ? RD_WIDE : RD_NARROW;      // round 5, eight- / ten-wave build on 256 CUs: 450 frames 4.80 / 4.87 s, 600 frames 5.76 / 5.70 s, 768 frames 7.00 / 6.87 s, 1024 frames 9.44 / 8.78 s
}

static inline RdLaunchPlan rd_launch_plan(const RdPlanContext &c, const RdLaunchArgs &a)
{
  RdLaunchPlan p;
  const int ctus = c.ctus_x * c.ctus_y, ctu_end = a.ctu_end < 0 ? ctus : a.ctu_end, remote_groups = c.remote_groups();
  const bool whole_ctus = !a.cabac_in && !a.cabac_out && a.ctu_begin == 0 && ctu_end == ctus, whole_tiles = a.tile_begin == 0 && a.tile_count < 0;
  p.tile_count = a.tile_count < 0 ? c.tile_columns * c.tile_rows : a.tile_count;
  // WaveFrontSynchro: a unit is one CTU row of a frame (rows of a frame run two CTUs apart on different waves, which wait for each other: a cooperative launch), or -- where
  // the grid cannot be co-resident, or the caller shares the device (HEVCDL_EXEC_NO_UNIT_HANDOVER) -- a whole frame whose rows one wave walks in order
  if (c.wavefront) {
    if (a.session_frame >= 0 && a.n_frames == 1 && whole_tiles) {
      // the per-CTU session (hevcdl_compress_ctu): one CTU a launch in the one-wave form; the contexts behind the second CTU of every row stay in the session frame's part of
      // d_wpp from call to call (hevcdl_begin_frames cleared it), so a row's first CTU finds what the row above left -- whatever state the caller hands in for that CTU
      p.wpp = 2; p.wpp_session = true; p.tile_count = 1;
    } else {
      if (!(whole_ctus && whole_tiles)) { p.status = HEVCDL_ERR_UNSUPPORTED; return p; }
      p.wpp = (c.exec_flags & HEVCDL_EXEC_NO_UNIT_HANDOVER) ? 2 : 1; p.tile_count = p.wpp == 1 ? c.ctus_y : 1;
    }
  }
  // One workgroup (waves[build] wavefronts, the whole LDS) per CU; the units (frame x tile) are dealt round-robin to the
  // workgroups, a wave per unit; waves left without a unit help the others (rd_kernel.hip).
  p.n_units = a.n_frames * p.tile_count;
  // WaveFrontSynchro, rows on waves of their own: rows are claimed as they become startable, so what sizes the launch is not the number of rows but how many of them can be
  // under way at once -- a row starts two CTUs behind the row above, i.e. at most (ctus_x + 1) / 2 rows of a frame (+ 1: one being claimed) -- `walkers`
  p.walkers = p.wpp == 1 ? (long long)a.n_frames * std::min(c.ctus_y, (c.ctus_x + 1) / 2 + 1) : (long long)p.n_units;
  p.groups = (int)std::min<long long>(p.walkers, c.rd_groups());
  p.master_groups = (int)std::min<long long>(p.walkers, 1 << 30);
  // Uneven dealing (e.g. 600 frames on 256 workgroups): the surplus units travel round the ring of workgroups so that every workgroup --
  // and every frame -- is crowded for the same share of the time (rd_kernel.hip, process_unit).  Only for whole-unit launches of a few units
  // per workgroup.
  p.migrate = (!p.wpp && p.n_units > p.groups && p.n_units % p.groups != 0 && p.n_units / p.groups <= 3 && p.groups <= 1024 && p.groups >= 8 && whole_ctus &&
               !(c.exec_flags & HEVCDL_EXEC_NO_UNIT_HANDOVER)) ? 1 : 0;
  if (p.migrate) p.sched_clear = 8192 + (size_t)p.groups * 192;
  // Few units (one frame, ten, a GPU's share of a sharded job): a frame is bound by the work of its CU's eight waves while most CUs have nothing to do -> the
  // kernel runs on ALL CUs and the workgroups without a unit take the second luma passes the others post (rd_kernel.hip, remote_post / remote_serve)
  p.remote = (!p.migrate && p.wpp != 2 && remote_groups && 3 * p.walkers <= 2 * remote_groups && whole_ctus) ? 1 : 0;
  // more units than takers (up to two units per taker; measured on 256 CUs: 150 frames 3.89 -> 3.79 s, 200 frames 3.92 -> 4.00 s, hence the limit): a pass is
  // posted only while a taker is free (rd_kernel.hip, remote_room)
  if (p.remote && 2 * p.walkers > remote_groups) p.remote = 3;
  // very few units: enough idle workgroups for the chroma modes of every master as well (eleven jobs per unit in flight).  Measured on 256 CUs, chroma jobs posted /
  // kept in the unit's own workgroup: 1 frame 2.84 / 3.10 s, 10 frames 2.95 / 3.17 s, 16 frames 3.38 / 3.18 s -- hence a twenty-second of the CUs, not a sixteenth
  if (p.remote && 22 * p.walkers <= remote_groups) p.remote = 2;
  // the ring of posted jobs has 2048 entries (rd_kernel.hip RQ_SIZE): a unit has at most two passes and the ten component jobs of its chroma modes posted
  if (p.remote && 12 * p.walkers > 2048) p.remote = 0;
  if (p.remote) p.sched_clear = 4096 + 2048 * 8;      // finished counter, queue head / tail, the ring (2048 pointers behind byte 4096)
  p.build = rd_build_of(c, p.remote != 0, p.walkers, p.groups);
  if (p.build == RD_WIDE) p.remote = 0;      // (the ten-wave build together with the hand-over of units: launches of more than three and fewer than four units per workgroup, or exec_flags; tests/test_rd_gpu.py::test_units_handed_over_between_workgroups_give_the_same_result runs the pair)
  p.waves = c.waves[p.build];
  p.grid = p.remote ? remote_groups : p.groups;
  // Waves of a workgroup that claim rows (the rest help them).  A frame's rows form a chain of ctus_x + 2 (ctus_y - 1) CTU steps; a step takes a claimer ~1.5 ms with seven
  // helpers and ~8 ms without any (t(m) ~ 0.75 + 0.75 m ms at m claimers per workgroup, measured on 600-frame launches: profiles/r06d_wavefront_masters.txt), while the
  // chip's rate grows with m (216 k CTU/s at 2 ... 313 k at 10).  A launch is bound by that chain until the work per claimer exceeds it: m = 0.7 x (CTUs of the launch) /
  // (workgroups x chain), at least 1, at most every wave.  Measured at 2160p, 75 frames: m = 3 0.79 s, m = 10 0.98 s; 150 frames: flat from 6 up (1.32 - 1.34 s); 600 frames:
  // m = 10 3.91 s, m = 6 4.54 s, m = 3 5.06 s.
  if (p.wpp == 1) { const long long chain = c.ctus_x + 2LL * (c.ctus_y - 1);
                    p.wpp_masters = p.remote ? 1 : (int)std::max<long long>(1, std::min<long long>(p.waves, (7LL * a.n_frames * ctus) / (10LL * p.groups * chain))); }
  return p;
}

// what hevcdl_last_rd_launch reports of a launch (after the launch: a cooperative launch the runtime refused has lost its migrate / remote)
static inline void rd_launch_report(const RdLaunchPlan &p, char *dst, size_t n)
{
  snprintf(dst, n, "%s form=%s workgroups=%d waves=%d units=%d", rd_build_names[p.build],
           p.wpp == 1 ? (p.remote ? "wavefront-rows+few-units" : "wavefront-rows") : p.wpp == 2 ? "wavefront(one wave per frame)" : p.migrate ? "unit-handover" : (p.remote == 1 ? "few-units(passes)" : (p.remote == 2 ? "few-units(passes+chroma)" : (p.remote == 3 ? "few-units(passes while takers idle)" : "independent"))),
           p.grid, p.waves, p.n_units);
}

// The most workspace blocks any whole launch of the context asks for: launches of 1 .. max_frames frames (hevcdl_reserve_workspace)
static inline size_t rd_largest_scratch_blocks(const RdPlanContext &c)
{
  size_t most = 0;
  RdLaunchArgs a;
  for (a.n_frames = 1; a.n_frames <= c.max_frames; a.n_frames++) most = std::max(most, rd_launch_plan(c, a).scratch_blocks());
  return most;
}
#endif
