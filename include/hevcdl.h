/* include/hevcdl.h -- C ABI of the MI355X-native all-intra CU-partition hot path.
 *
 * Drop-in boundary: the reference's
 *     Void TEncCu::compressCtu(Int m_iFrame, TComDataCU* pCtu)
 *       HM_dl/source/Lib/TLibEncoder/TEncCu.h:120, TEncCu.cpp:234, single call site TEncSlice.cpp:879
 * together with the label producer it busy-waits for (use_model.py / gen_frames.py, file IPC at
 * TEncCu.cpp:244-253).  The reference walks CTUs one at a time on one CPU thread; CTUs of one slice
 * are strictly serial (reconstructed neighbours + adaptive CABAC state), frames of an all-intra
 * sequence are independent, so the GPU entry points are per BATCH OF FRAMES.  Everything crossing this
 * boundary is plain pointers and sizes; no torch / C++ types.
 *
 * Threading: one hevcdl_ctx per device; a ctx is not thread-safe; different ctxs are independent.
 * Ownership: the caller owns every buffer it passes; the library owns only its internal workspace.
 * Errors: every function returns a status code; nothing aborts or waits forever (the reference hangs at
 * TEncCu.cpp:245 when the label file never appears).
 */
#ifndef HEVCDL_H
#define HEVCDL_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  HEVCDL_OK = 0,
  HEVCDL_ERR_INVALID_ARG = 1,
  HEVCDL_ERR_UNSUPPORTED = 2,   /* a cfg key that would change the path and is not implemented */
  HEVCDL_ERR_NO_DEVICE = 3,
  HEVCDL_ERR_HIP = 4,
  HEVCDL_ERR_OOM = 5
} hevcdl_status;

/* tool flags (reference cfg: encoder_intra_main.cfg:37-38,53-54 + TAppEncCfg.cpp defaults :978,950,1007) */
#define HEVCDL_TOOL_RDOQ            (1u << 0)
#define HEVCDL_TOOL_RDOQTS          (1u << 1)
#define HEVCDL_TOOL_TSKIP           (1u << 2)
#define HEVCDL_TOOL_TSKIP_FAST      (1u << 3)
#define HEVCDL_TOOL_SIGN_HIDE       (1u << 4)
#define HEVCDL_TOOL_STRONG_INTRA    (1u << 5)
#define HEVCDL_TOOL_FAST_UDI_MPM    (1u << 6)
#define HEVCDL_TOOLS_REFERENCE      0x7fu
/* Every one of them may be turned off (cfg keys RDOQ, RDOQTS, TransformSkip, TransformSkipFast, SignHideFlag, StrongIntraSmoothing, FastUDIUseMPMEnabled; each pinned by a run of
 * the reference encoder with the switch on its command line: tests/golden/rd_k*.npz).  Without RDOQ the quantiser is the dead-zone rounding of TComTrQuant::xQuant with
 * signBitHidingHDQ behind it (RDOQTS: the same choice for transform-skipped blocks); without TransformSkipFast every 4x4 block is tried both ways, not only those of NxN CUs
 * (TEncSearch.cpp:1502-1505, 1965-1990).  Bits outside HEVCDL_TOOLS_REFERENCE are rejected. */
#define HEVCDL_TOOLS_SWITCHABLE     HEVCDL_TOOLS_REFERENCE
#define HEVCDL_TOOLS_SUPPORTED(t)   ((((t) | HEVCDL_TOOLS_SWITCHABLE) == HEVCDL_TOOLS_REFERENCE) && ((t) & ~HEVCDL_TOOLS_REFERENCE) == 0)

#define HEVCDL_CNN_INPUT_RGB601 0   /* BT.601 limited-range YUV -> RGB, nearest chroma (defined by this project) */
#define HEVCDL_CNN_INPUT_LUMA   1   /* R = G = B = Y */
#define HEVCDL_BN_REFERENCE     0   /* training-mode BatchNorm, as use_model.py:61-63 runs it (the reference never calls model.eval()) */
#define HEVCDL_BN_EVAL          1   /* BatchNorm with the checkpoint's running statistics (what model.eval() would give; NOT the reference pipeline's labels) */
/* HEVCDL_BOUNDARY_CLAMP: every label is raised to the smallest depth at which the CU containing its 16x16 cell lies inside the picture;
 * then exactly what the reference's walk READS is made valid and nothing else is touched.  The walk (TEncCu.cpp:496-520) looks at one label per CU, the one of its
 * top-left cell: a CTU inside the picture whose first label is 0 is ONE 64x64 CU whatever the other 15 labels say (use_model.py:101-119 does write such files, and HM
 * codes them that way -- so does this library); otherwise a visited 32x32 quadrant whose first label is 0 gets 1 and the cells of a split quadrant at least 2. */
#define HEVCDL_BOUNDARY_CLAMP   0

#define HEVCDL_WEIGHT_FLOATS 637712 /* state_dict order of rec/hevc_encoder_model.pt, fp32 tensors only */

typedef struct hevcdl_config {
  uint32_t struct_size;          /* sizeof(hevcdl_config) */
  int32_t  width, height;        /* luma samples, multiples of 8 (min CU) */
  int32_t  bit_depth;            /* 8, or 10: InputBitDepth = InternalBitDepth = 10 (Profile main10); samples are then uint16,
                                    little endian, in every yuv / recon / picture buffer (decision path and in-loop filters); the CNN
                                    stage sees sample >> 2 */
  int32_t  chroma_format;        /* 420 */
  int32_t  qp;                   /* slice QP, 0..51 */
  int32_t  ctu_size;             /* 64   (MaxCUWidth/Height)          */
  int32_t  max_partition_depth;  /* 4    (MaxPartitionDepth)          */
  int32_t  tu_log2_min, tu_log2_max, tu_max_depth_intra;   /* 2, 5, 3 */
  uint32_t tools;                /* HEVCDL_TOOL_* : any subset of HEVCDL_TOOLS_REFERENCE (the reference cfg's value) */
  int32_t  bn_mode, boundary_policy, cnn_input;
  int32_t  device;               /* HIP device ordinal */
  int32_t  max_frames;           /* frames per call the workspace is sized for */
  /* decision constants computed ON THE HOST in IEEE double exactly as the reference does
   * (TEncSlice.cpp:112-140,433-527; TComTrQuant.cpp:3096-3126,2532-2535) and passed as bits: */
  double   lambda, sqrt_lambda, chroma_weight, lambda_chroma;
  double   err_scale[2][4];      /* [luma/chroma][log2(TU)-2] */
  int64_t  sbh_rd_factor[2];     /* [luma/chroma] */
  int32_t  qp_chroma;
  /* uniformly spaced tiles (cfg keys TileUniformSpacing 1, NumTileColumnsMinus1 + 1, NumTileRowsMinus1 + 1; TAppEncCfg.cpp:1024-1028);
   * 1 x 1 = no tiles.  Every tile is at least 4 CTUs wide (the reference's own limit, TComPicSym.cpp:388).  Tiles are independent
   * units of the decision path: one wavefront per (frame, tile). */
  int32_t  tile_columns, tile_rows;
  /* Execution options of the decision kernel (0 = default; formerly a reserved field that had to be 0).
   * HEVCDL_EXEC_NO_UNIT_HANDOVER: never let a frame travel between workgroups.  With more frames than compute units and an uneven split (600 frames on
   * 256 CUs) the kernel hands frames round a ring of workgroups so that every CU is crowded for the same share of the time; workgroups then wait for
   * each other, which needs ALL of them resident at once.  The library therefore launches that form cooperatively (the runtime refuses the launch when
   * it cannot co-schedule the grid -- another context holding CUs or LDS, a CU mask -- and the library falls back to the independent form by itself);
   * set this bit to use the independent form always, e.g. when several contexts / processes share the device by design.  The same holds for launches of at most
   * two thirds as many frames (x tiles) as CUs, which run on ALL CUs so that the empty ones take second luma passes (and, below a twenty-second, chroma modes) from the
   * others: cooperative as well, same fall-back, switched off by this bit (the context then also allocates workspace for its own frames only). */
  int32_t  exec_flags;
#define HEVCDL_EXEC_NO_UNIT_HANDOVER 1
  /* The 8-bit decision kernel exists in two builds: 8 wavefronts per workgroup with the look-ahead of the few-units form, and 10 (csrc/rd_kernel_wide.hip) for
   * launches of three or more units per workgroup; the library picks by the shape of the launch.  HEVCDL_EXEC_RD_WIDE forces the second for every launch of the context (the few-units form is then
   * never used), HEVCDL_EXEC_RD_NARROW the first.  Results do not depend on the choice.  Contexts whose `tools` are not the reference cfg's and 10-bit contexts have
   * one build each (eight waves): both bits are without effect there. */
#define HEVCDL_EXEC_RD_WIDE 2
#define HEVCDL_EXEC_RD_NARROW 4
  /* TileUniformSpacing 0: explicit sizes in CTUs of every tile column / row but the last (TileColumnWidthArray, TileRowHeightArray,
   * TAppEncCfg.cpp:1026-1028); ignored when tile_uniform_spacing != 0 (the default) */
  int32_t  tile_uniform_spacing;
  int32_t  tile_column_width[19], tile_row_height[21];
  int32_t  lf_across_tiles;      /* LFCrossTileBoundaryFlag (default 1): 0 = deblocking and SAO stop at tile borders */
  /* LoopFilterBetaOffset_div2 / LoopFilterTcOffset_div2 (-6 .. 6, default 0; with LoopFilterOffsetInPPS 1, the cfg's value): added twice to the QP the deblocking filter's
   * beta / tc tables are read with (TComLoopFilter.cpp:623-624, 804) */
  int32_t  lf_beta_offset_div2, lf_tc_offset_div2;
  /* WaveFrontSynchro (cfg key of that name, TAppEncCfg.cpp:975; default 0).  1: entropy_coding_sync_enabled_flag -- the coder is re-initialised at the first CTU of every
   * CTU row and takes over the contexts behind the second CTU of the row above (TEncSlice.cpp:783-830, 925-928).  The decisions then differ from the default cfg's (every
   * RD cost is priced with other context states), exactly as the reference's do with the key set; the CTU chain of a frame (2040 steps at 2160p) becomes ctus_y chains two
   * CTUs apart (126 steps), which the decision kernel walks on different waves.  Not together with tiles (the reference refuses the pair in the main profiles).  The per-CTU
   * session (hevcdl_compress_ctu) works on such a context too: the contexts behind the second CTU of every row are kept per session frame, a row's first CTU starts from them
   * whatever state the caller hands in (that IS the reference's behaviour: resetEntropy + loadContexts in front of compressCtu, TEncSlice.cpp:808-823). */
  int32_t  wavefront;
  /* Per-picture deblocking parameters (section "deblocking parameters chosen per picture" below).  deblocking_metric = DeblockingFilterMetric (default 0): 1 = the blockiness
   * metric of TEncGOP::applyDeblockingFilterMetric picks one offset for beta and tc per picture; 2 = the trial search of applyDeblockingFilterParameterSelection:
   * up to 49 pairs (beta, tc) in -3 .. 3 are tried on every picture and the one with the least distortion is signalled.  lf_offset_in_pps = LoopFilterOffsetInPPS (default 1); 0 = the slice header repeats the offsets (deblocking_filter_override_flag 1), the filter
   * itself runs as before.  A non-zero metric needs lf_offset_in_pps 0 and the filter on, as in the reference (TAppEncCfg.cpp:2143), and metric 1 a picture of at least
   * 64 luma samples either way (the reference divides by the number of 32-sample columns and rows minus one).  hevcdl_create_error names what was refused. */
  int32_t  deblocking_metric, lf_offset_in_pps;
  /* Slices (cfg keys SliceMode, SliceArgument, LFCrossSliceBoundaryFlag).  slice_mode 0 (the default; a zeroed tail means it): one slice a picture, and the
   * other two fields are not looked at (the reference sets LFCrossSliceBoundaryFlag to 1 then, TAppEncTop.cpp:278-281).  1: slices of slice_argument CTUs in raster order; only
   * whole CTU rows -- slice_argument a positive multiple of the picture's width in CTUs -- at most 22 slices a picture, not together with tiles or wavefront.  Such slices are the
   * reference's tile rows of full width in everything but the syntax (same decisions, same filters): the context runs them as a unit grid of one column, which may be narrower
   * than the four CTUs a tile column needs.  3: slices of slice_argument tiles in raster order of the tile grid (the last one takes the rest); needs tiles; changes nothing
   * but the stream.  2 (slices by bytes) is refused.  lf_across_slices = LFCrossSliceBoundaryFlag: 0 = deblocking and SAO stop at slice borders.  In mode 3 every slice border is
   * a tile border and the in-loop filters cross it only when BOTH lf_across_tiles and lf_across_slices are set (tests/golden/slices_t512_a1_lf0.npz), while a tile border inside
   * a slice follows lf_across_tiles alone: more than one tile a slice with lf_across_tiles 1 and lf_across_slices 0 is refused (the filters have one flag).  Not together
   * with deblocking_metric, and the per-CTU session refuses such a context.  hevcdl_create_error names what was refused. */
  int32_t  slice_mode, slice_argument, lf_across_slices;
  /* Dependent slice segments (cfg keys SliceSegmentMode, SliceSegmentArgument).  slice_segment_mode 0 (the default; a zeroed tail means it): none, and
   * the argument is not looked at.  1: segments of slice_segment_argument CTUs; needs wavefront 1, no tiles, slice_mode 0 and an argument that is a positive multiple of the
   * picture's width in CTUs -- segments of argument / width whole CTU rows, the last one shorter; a picture one CTU wide makes every CTU a segment.  3: segments of
   * slice_segment_argument tiles in raster order of the tile grid, the last one taking the rest; needs tiles and an argument of at least 1; may be combined with slice_mode 3,
   * and a segment never runs past the end of its slice.  Both change nothing but the stream -- every segment is a NAL unit of its own with a short header, and a sub-stream
   * that ends a segment ends with end_of_slice_segment_flag 1: launch plan, workspace, decisions, filters and the per-CTU session are those of the context without the keys.
   * Refused: 2 (segments by bytes); mode 1 without wavefront or with segments that are not whole CTU rows (the reference's decisions change where a segment starts in the
   * middle of a coder chain), mode 1 with tiles or slices, mode 3 without tiles, either mode with deblocking_metric.  hevcdl_create_error names what was refused. */
  int32_t  slice_segment_mode, slice_segment_argument;
  /* DeltaQpRD (cfg key of that name, "slice-based multi-QP optimization").  0 (the default; a zeroed tail means it): none -- everything behaves as
   * without the field.  N = 1 .. HEVCDL_QP_RD_MAX_N: every picture is decided 2N+1 times, at qp, qp - 1, qp + 1, ... qp + N with the same labels (the CNN runs once), and
   * the candidate with the least picture cost dist + bits * frameLambda is kept (TEncSlice::precompressSlice, TEncSlice.cpp:572-661): its records, reconstruction and
   * statistics are what the call returns, its QP and lambdas what deblocking, SAO, the slice header (slice_qp_delta; init_qp_minus26 stays 0) and the entropy coder's
   * contexts use.  Pictures of one batch may end at different QPs: hevcdl_get_qp_rd.  A candidate outside 0 .. 51 is coded at the clipped QP with the lambda of the
   * unclipped one, as in the reference.  Tiles and wavefront are allowed (a picture is still one slice).  Refused: with slice_mode or slice_segment_mode (the reference
   * optimises per slice), with deblocking_metric, N above the bound, at 10 bits qp - N < 0 (the reference would code at a negative QP); the per-CTU session
   * (hevcdl_begin_frames) and hevcdl_compress_tiles_dev refuse such a context.  hevcdl_create_error names what was refused. */
  int32_t  delta_qp_rd;
} hevcdl_config;

/* ---- DeltaQpRD: the slice QP of a picture picked among 2N+1 candidate encodes (csrc/qp_rd.h, csrc/qp_rd_kernel.hip) -----------------------------------------------
 * The largest N a context takes: 13 candidates, offsets -6 .. +6 -- one doubling of the quantiser step either way.  Every candidate is a whole decision launch, so a
 * picture costs 2N+1 times its decisions. */
#define HEVCDL_QP_RD_MAX_N 6
#define HEVCDL_QP_RD_MAX_CANDIDATES (2 * HEVCDL_QP_RD_MAX_N + 1)
/* One candidate: its offset (0, -1, +1, -2, +2, ...: TEncSlice.cpp:294), the QP it is coded at (:523) and the decision constants of hevcdl_config for it, field for field. */
typedef struct hevcdl_qp_rd_candidate {
  int32_t  offset, qp;
  double   lambda, sqrt_lambda, chroma_weight, lambda_chroma;
  double   err_scale[2][4];
  int64_t  sbh_rd_factor[2];
  int32_t  qp_chroma, pad;
} hevcdl_qp_rd_candidate;
/* One picture's row of the trial table: what the device keeps per picture while the candidates run, and what hevcdl_get_qp_rd hands out. */
typedef struct hevcdl_qp_rd_row {
  uint64_t bits[HEVCDL_QP_RD_MAX_CANDIDATES], dist[HEVCDL_QP_RD_MAX_CANDIDATES];      /* m_uiPicTotalBits / m_uiPicDist of every candidate (TEncSlice.cpp:959-961): the sums of hevcdl_ctu_record.bits / .dist */
  double   best_cost;            /* dPicRdCostBest */
  int32_t  best_idx;             /* uiQpIdxBest: the candidate the picture was coded with */
  int32_t  take;                 /* (device bookkeeping: the last candidate summed was a new best) */
} hevcdl_qp_rd_row;

/* One CTU of decisions: what compressCtu leaves in the picture's CTU record (TEncCu.cpp:1091 copyToPic).
 * 256 entries = 4x4 luma partitions in z-scan order (TComRom.cpp:284-352).  Coefficients use the
 * reference's TComDataCU::m_pcTrCoeff layout: the TU whose first partition is p starts at 16*p (luma)
 * or 4*p (chroma) and is stored row-major with its own width as stride. */
typedef struct hevcdl_ctu_record {
  uint8_t  depth[256], part_size[256], luma_dir[256], chroma_dir[256], tr_idx[256];
  uint8_t  cbf[3][256], tskip[3][256];
  uint32_t bits, dist;           /* pCtu->getTotalBits() / getTotalDistortion() (TEncSlice.cpp:959-961) */
  double   cost;                 /* pCtu->getTotalCost() */
  int16_t  coeff_y[4096], coeff_cb[1024], coeff_cr[1024];
} hevcdl_ctu_record;             /* 15120 bytes */

typedef struct hevcdl_frame_stats {
  uint64_t sse[3];               /* reconstruction SSE per plane before in-loop filters */
  uint64_t est_bits;             /* CABAC-estimated bits of the state-advancing encode (TEncSlice.cpp:886-893) */
  uint32_t ctus, pad;
} hevcdl_frame_stats;

typedef struct hevcdl_profile {
  double   cnn_ms, rd_ms;        /* accumulated kernel time measured with HIP events on the launch stream */
  uint32_t cnn_launches, rd_launches;
  double   cnn_conv_ms;          /* of cnn_ms: the convolution kernel alone (the rest is the fully connected head), summed over the same launches */
} hevcdl_profile;

typedef struct hevcdl_ctx hevcdl_ctx;

/* Fill cfg from (width, height, qp) with the reference configuration (encoder_intra_main.cfg) and the
 * host-computed lambda family.  Replaces TEncSlice::setUpLambda / calculateLambda for this path. */
hevcdl_status hevcdl_config_default(hevcdl_config *cfg, int width, int height, int qp);
/* The same for a given sample bit depth (8 or 10): quantiser QP offset 6 per extra bit, distortion kept at 8-bit scale
 * (the reference's FULL_NBIT 0 build, TypeDef.h:162-172), lambda unchanged (TEncSlice.cpp:433-527). */
hevcdl_status hevcdl_config_default_bd(hevcdl_config *cfg, int width, int height, int qp, int bit_depth);
/* DeltaQpRD, host only (no GPU needed; csrc/qp_rd.h): the candidate table of a configuration -- cfg->qp, cfg->delta_qp_rd and cfg->bit_depth are read.  out[idx], idx = 0 ..
 * 2N: the candidate's offset, the QP it is coded at and its constants, computed by the code hevcdl_config_default* fills a configuration with; *count = 2N+1;
 * *frame_lambda = 0.68 * 2^((qp - 12) / 3), the lambda of the picture cost (TEncSlice.cpp:615-623).  delta_qp_rd 0 gives the one candidate a plain context runs.
 * HEVCDL_ERR_INVALID_ARG: null pointers, capacity below 2N+1, N outside 0 .. HEVCDL_QP_RD_MAX_N, qp outside 0 .. 51; HEVCDL_ERR_UNSUPPORTED: a bit depth other
 * than 8 or 10, or 10 bits with qp - N < 0. */
hevcdl_status hevcdl_qp_rd_candidates(const hevcdl_config *cfg, hevcdl_qp_rd_candidate *out, int capacity, int *count, double *frame_lambda);
/* ... and the pick rule (TEncSlice.cpp:646-652): the index of the candidate kept, from the n pairs of picture sums in candidate order -- cost = dist + bits * frame_lambda in
 * IEEE double, multiply and add separate, strict `<`: a tie keeps the earlier index.  -1 for null pointers or n < 1.  The device runs the same source. */
int           hevcdl_qp_rd_pick_index(const uint64_t *bits, const uint64_t *dist, int n, double frame_lambda);

/* weights: flat fp32 blob, HEVCDL_WEIGHT_FLOATS values (replaces torch.load at use_model.py:62). */
hevcdl_status hevcdl_create(const hevcdl_config *cfg, const float *weights, size_t n_floats, hevcdl_ctx **out);
/* Why the calling thread's last hevcdl_create refused its configuration: there is no context to ask yet.  ONLY the refusals of the deblocking keys (deblocking_metric,
 * lf_offset_in_pps), of the slice keys (slice_mode, slice_argument, lf_across_slices) and of the segment keys (slice_segment_mode, slice_segment_argument) leave a message so far; every other failure of hevcdl_create, and a success, leave "" -- the status is then all there is. */
const char   *hevcdl_create_error(void);
void          hevcdl_destroy(hevcdl_ctx *ctx);
const char   *hevcdl_last_error(const hevcdl_ctx *ctx);

/* ---- host-buffer entry points (copy in, run, copy out) ------------------------------------- */
/* Replaces gen_frames.py + use_model.py: planar 4:2:0 frames (uint8, or uint16 at bit_depth 10) -> labels[n_frames][ctus][16]
 * (clamped to the picture); logits_opt[n_frames][ctus][4][16] may be NULL. */
hevcdl_status hevcdl_predict_depth(hevcdl_ctx *ctx, const uint8_t *yuv, int n_frames, uint8_t *labels, float *logits_opt);
/* Fixture entry: n_ctus RGB CTUs [n][64][64][3] (the tensor the reference feeds ConvNet2) -> raw labels
 * (use_model.py:101-119, no clamping) and logits[n][4][16]. */
hevcdl_status hevcdl_predict_depth_rgb(hevcdl_ctx *ctx, const uint8_t *ctu_rgb, int n_ctus, uint8_t *labels, float *logits_opt);
/* The label stage alone: logits[n_ctus][4][16] (the four forwards of a CTU, use_model.py:100) -> labels[n_ctus][16] by the 4x argmax and the
 * fix-ups of use_model.py:101-119, run by the same device code that follows the fully connected head.  clamp != 0 also applies the boundary
 * policy, taking CTU i as CTU (i mod ctus-per-frame) of the context's picture. */
hevcdl_status hevcdl_labels_from_logits(hevcdl_ctx *ctx, const float *logits, int n_ctus, int clamp, uint8_t *labels);
/* Replaces the compressCtu loop of TEncSlice::compressSlice for n_frames independent frames.
 * labels_opt == NULL -> labels come from the on-device CNN.  recon_opt / stats_opt may be NULL. */
hevcdl_status hevcdl_compress_frames(hevcdl_ctx *ctx, const uint8_t *yuv, int n_frames, const uint8_t *labels_opt,
                                     hevcdl_ctu_record *records, uint8_t *recon_opt, hevcdl_frame_stats *stats_opt);

/* The same two entry points for pictures that are NOT packed: three planes with their own row pitch, as an encoder's picture buffers hold them
 * (HM: TComPicYuv = one Pel (int16) plane per component with a margin of 80 samples round the picture, stride = width + 160,
 * TComPicYuv.cpp:81-104; getAddr(compID) / getStride(compID) give exactly plane[] / row_stride[]).  Strides are in BYTES.  sample_bytes: 1
 * (uint8 samples, bit_depth 8), or 2 (16-bit containers: the samples of a bit_depth 10 context, or 8-bit samples in int16 as HM keeps them --
 * narrowed on the device).  frame_stride[c]: distance from plane c of frame i to plane c of frame i + 1 (ignored for n_frames 1). */
typedef struct hevcdl_planes {
  const void *plane[3];          /* first sample of Y, Cb, Cr of frame 0 */
  size_t      row_stride[3];     /* bytes from one row to the next, >= the plane's width * sample_bytes */
  size_t      frame_stride[3];   /* bytes from frame i to frame i + 1, per plane */
  int32_t     sample_bytes;      /* 1 or 2 */
} hevcdl_planes;
hevcdl_status hevcdl_predict_depth_planes(hevcdl_ctx *ctx, const hevcdl_planes *src, int n_frames, uint8_t *labels, float *logits_opt);
hevcdl_status hevcdl_compress_frames_planes(hevcdl_ctx *ctx, const hevcdl_planes *src, int n_frames, const uint8_t *labels_opt,
                                            hevcdl_ctu_record *records, uint8_t *recon_opt, hevcdl_frame_stats *stats_opt);

/* ---- deblocking filter (first in-loop filter of the reference) -------------------------------------
 * Replaces TComLoopFilter::loopFilterPic(TComPic*) (TLibCommon/TComLoopFilter.cpp:130, called at TEncGOP.cpp:1742) for
 * the pictures this library decides: recon = what hevcdl_compress_frames returned, records = its CTU records (the
 * TU grid), out = the picture the reference hands to SAO (may alias recon in the device variant). */
hevcdl_status hevcdl_deblock_frames(hevcdl_ctx *ctx, const uint8_t *recon, int n_frames, const hevcdl_ctu_record *records, uint8_t *out);
hevcdl_status hevcdl_deblock_frames_dev(hevcdl_ctx *ctx, const void *d_recon, int n_frames, const void *d_records, void *d_out, void *stream);

/* ---- deblocking parameters chosen per picture (cfg keys DeblockingFilterMetric, LoopFilterOffsetInPPS; csrc/dbk_select_kernel.hip, csrc/dbk_select.h) -------------
 * What the slice header says about the deblocking filter of ONE picture and what the filter ran with (TEncCavlc.cpp:1080-1095).  Without override_flag the picture uses the
 * PPS's values, and the other three fields hold exactly those. */
typedef struct hevcdl_dbk_choice {
  int32_t override_enabled;                    /* deblocking_filter_override_enabled_flag of the PPS the picture is coded under: DeblockingFilterMetric != 0 or
                                                  LoopFilterOffsetInPPS 0 (TEncTop.cpp:1007-1016).  A property of the STREAM carried with every picture: it must be the
                                                  same for all pictures of a stream (hevcdl_get_dbk_choice gives it so); the writers put it into the PPS in front of the
                                                  picture they are called for, so with rewrite_param_sets 0 picture 0's value is the one a decoder sees */
  int32_t override_flag;                       /* deblocking_filter_override_flag */
  int32_t disabled;                            /* slice_deblocking_filter_disabled_flag */
  int32_t beta_offset_div2, tc_offset_div2;    /* slice_beta_offset_div2 / slice_tc_offset_div2 */
} hevcdl_dbk_choice;
/* DeblockingFilterMetric 1, the measurement: for n_frames reconstructions BEFORE deblocking (coded size, padding included) the two exact sums of
 * TEncGOP::applyDeblockingFilterMetric (TEncGOP.cpp:3216-3268), sums[i][0] over the vertical edges at multiples of 32 and sums[i][1] over the horizontal ones: |p0 - q0| of
 * every line whose a = (|p2 - 2 p1 + p0| + |q0 - 2 q1 + q2|) << 1 lies strictly between 2 << (bit depth - 8) and (beta(QP) << (bit depth - 8)) >> 2.  Of the edges only the
 * first (width >> 5) - 1 and (height >> 5) - 1 count, as in the reference: at a size that is no multiple of 32 the last edge is dropped.  A picture under 64 samples
 * either way is HEVCDL_ERR_INVALID_ARG.  The device variant is asynchronous on `stream`; d_sums: [n_frames][2] uint64. */
hevcdl_status hevcdl_dbk_metric_frames(hevcdl_ctx *ctx, const void *recon, int n_frames, uint64_t *sums);
hevcdl_status hevcdl_dbk_metric_frames_dev(hevcdl_ctx *ctx, const void *d_recon, int n_frames, void *d_sums, void *stream);
/* ... and the decision (TEncGOP.cpp:3270-3301; host only, no GPU needed): the two sums of a width x height picture -> the picture's choice.  Above the threshold: override
 * with one offset 2 .. 6 for beta and tc; otherwise no override and the PPS's values (pps_beta_offset_div2, pps_tc_offset_div2).  override_enabled is 1 either way. */
hevcdl_status hevcdl_dbk_metric_choice(int width, int height, int bit_depth, uint64_t col_sum, uint64_t row_sum, int pps_beta_offset_div2, int pps_tc_offset_div2,
                                       hevcdl_dbk_choice *out);
/* hevcdl_deblock_frames with parameters per picture: choices[i] = what picture i is filtered with (disabled: the picture is copied; override_flag is not looked at).
 * choices == NULL is hevcdl_deblock_frames itself.  The device variant takes the choices from HOST memory too and synchronises nothing; d_out may alias d_recon.  The rows
 * are staged in the context (one host copy, one device buffer): like every launch of a context, one such call at a time -- a second call must not be issued before the
 * first has finished on the device, on whatever stream. */
hevcdl_status hevcdl_deblock_frames_choice(hevcdl_ctx *ctx, const uint8_t *recon, int n_frames, const hevcdl_ctu_record *records, const hevcdl_dbk_choice *choices, uint8_t *out);
hevcdl_status hevcdl_deblock_frames_choice_dev(hevcdl_ctx *ctx, const void *d_recon, int n_frames, const void *d_records, const hevcdl_dbk_choice *choices, void *d_out, void *stream);
/* DeblockingFilterMetric 2, the trials: for n_frames pictures one launch fills tables[i][49], entry 7 (b + 3) + (t + 3) = the distortion (xFindDistortionFrame,
 * TEncGOP.cpp:2172-2200: all three components, (d * d) >> 2 (bit depth - 8) per sample) of the original against the reconstruction deblocked with slice_beta_offset_div2 b
 * and slice_tc_offset_div2 t, b, t in -3 .. 3 -- every entry, also those the reference's walk would not visit.  No trial picture is written to memory.  The device variant is
 * asynchronous on `stream`; d_tables: [n_frames][49] uint64. */
hevcdl_status hevcdl_dbk_trial_frames(hevcdl_ctx *ctx, const void *org, const void *recon, int n_frames, const hevcdl_ctu_record *records, uint64_t *tables);
hevcdl_status hevcdl_dbk_trial_frames_dev(hevcdl_ctx *ctx, const void *d_org, const void *d_recon, int n_frames, const void *d_records, void *d_tables, void *stream);
/* ... and the walk (TEncGOP.cpp:3335-3420; host only, no GPU needed; csrc/dbk_select.h): one table and the carried state -- state4 = the reference's m_DBParam[0]:
 * available, disabled, beta, tc; all zero at the start of a sequence -- -> the picture's choice; state4 is advanced.  The search windows are +-1 (beta) and +-2 (tc) round
 * the previous picture's best, so the result depends on the ORDER of the pictures. */
hevcdl_status hevcdl_dbk_walk_table(const uint64_t *table, int pps_beta_offset_div2, int pps_tc_offset_div2, int32_t *state4, hevcdl_dbk_choice *out);
/* With deblocking_metric 2 the picture pipelines keep that state in the context and advance it picture by picture ACROSS calls: the pictures of a sequence must reach one
 * context in POC order, call after call.  A caller that deals pictures out of order, or over several contexts, gets other choices than the reference; that is the caller's
 * problem, the library cannot see it.  hevcdl_dbk_select_reset starts a new sequence (the state of a fresh context). */
hevcdl_status hevcdl_dbk_select_reset(hevcdl_ctx *ctx);
/* The choices of pictures [first, first + count) of the LAST hevcdl_encode_pictures / _chunked / _stream call -- valid inside the chunk callback and after the call returns,
 * like hevcdl_get_slice_data; they feed hevcdl_write_access_unit_dbk / hevcdl_write_access_unit_from_slice_data_dbk.  With deblocking_metric 1 the pipeline measures the
 * reconstruction behind the decisions, fetches two sums a picture, decides on the host and deblocks every picture with its own parameters; the metric keeps no state, so
 * pictures may be dealt to contexts, devices and calls in any way; with deblocking_metric 2 it runs the trial launch, fetches 49 words a picture and walks them in
 * order (see above).  Without the metric every picture carries the cfg's values (override_enabled = override_flag =
 * !lf_offset_in_pps). */
hevcdl_status hevcdl_get_dbk_choice(hevcdl_ctx *ctx, int first, int count, hevcdl_dbk_choice *out);

/* ---- sample adaptive offset (second in-loop filter) ---------------------------------------------------
 * Replaces TEncSampleAdaptiveOffset::SAOProcess (TLibEncoder/TEncSampleAdaptiveOffset.cpp:244, called at TEncGOP.cpp:1797):
 * statistics, per-CTU parameter decision (new / merge-left / merge-up / off, edge or band offsets) and the offset
 * reconstruction.  org = the original frames, deblocked = output of hevcdl_deblock_frames; params receives the coded
 * parameters of every CTU (what TEncSbac::codeSAOBlkParam writes), out the final reconstruction. */
typedef struct hevcdl_sao_offset {
  int32_t mode;        /* 0 off, 1 new, 2 merge (SAOMode, TypeDef.h:539-545) */
  int32_t type;        /* new: 0..3 edge offset 0/90/135/45 degrees, 4 band offset; merge: 0 left, 1 above */
  int32_t aux;         /* band position */
  int32_t offset[32];  /* per class: edge classes 0..4 (2 = plain, always 0) or bands 0..31 */
} hevcdl_sao_offset;
typedef struct hevcdl_sao_blk { hevcdl_sao_offset c[3]; } hevcdl_sao_blk;      /* Y, Cb, Cr */
hevcdl_status hevcdl_sao_frames(hevcdl_ctx *ctx, const uint8_t *org, const uint8_t *deblocked, int n_frames, hevcdl_sao_blk *params, uint8_t *out);
hevcdl_status hevcdl_sao_frames_dev(hevcdl_ctx *ctx, const void *d_org, const void *d_deblocked, int n_frames, void *d_params, void *d_out, void *stream);

/* SAO with GIVEN parameters -- what a decoder runs behind the deblocking filter: deblocked pictures + the [n_frames][ctus] parameters of a stream (hevcdl_parse_stream;
 * the layout hevcdl_sao_frames returns and hevcdl_write_access_unit takes: a merged CTU is mode 2 with the direction in component 0) -> the output pictures.  No original and
 * no decision: hevcdl_sao_apply*_kernel alone.  params is HOST memory in both forms: the call checks it (HEVCDL_ERR_INVALID_ARG: a mode outside 0 .. 2, a type outside
 * 0 .. 4, a band position outside 0 .. 31, an offset outside +-31, a merge whose candidate lies outside the picture or across a tile / row-slice border of the context),
 * resolves the merges and stages the result in the context -- one such call at a time.
 * THE CONTEXT MUST DESCRIBE THE STREAM: picture size, bit depth, tiles, lf_across_tiles and the slice keys (slice_mode, slice_argument, lf_across_slices) decide where the
 * filter stops, and the call takes them from the context -- it is not given the stream's configuration and cannot compare.  A context created from the parsed
 * hevcdl_stream_config and hevcdl_slice_layout field by field filters as the stream's encoder did; parameters of a SliceMode 1 stream with lf_across_slices 0 run through a
 * context without the slice keys are filtered across the slice borders, and no error is reported.  The device form is asynchronous on `stream`; d_out must not be d_deblocked.  A CTU of mode 0 is copied. */
hevcdl_status hevcdl_sao_apply_frames(hevcdl_ctx *ctx, const void *deblocked, int n_frames, const hevcdl_sao_blk *params, void *out);
hevcdl_status hevcdl_sao_apply_frames_dev(hevcdl_ctx *ctx, const void *d_deblocked, int n_frames, const hevcdl_sao_blk *params, void *d_out, void *stream);

/* ---- the whole picture pipeline in one call (host buffers): CNN labels (labels_opt == NULL) -> decisions -> deblocking (deblock != 0) -> SAO
 * (sao_opt != NULL; with deblock == 0 -- LoopFilterDisable 1 -- it works on the unfiltered reconstruction, as the reference does) with the pictures staying in HBM between the stages.  records + picture_out (the output picture: after the
 * enabled filters; uint16 samples at 10 bits) + sao_opt feed hevcdl_write_access_unit / hevcdl_write_picture_hash_sei.  stats_opt: SSE before
 * the in-loop filters and estimated bits, as hevcdl_compress_frames.  Replaces TEncGOP::compressGOP's per-picture stages (TEncGOP.cpp:1560-1800). */
hevcdl_status hevcdl_encode_pictures(hevcdl_ctx *ctx, const void *yuv, int n_frames, const uint8_t *labels_opt, int deblock, hevcdl_ctu_record *records,
                                     void *picture_out, hevcdl_sao_blk *sao_opt, hevcdl_frame_stats *stats_opt);
/* The same pipeline with the results handed over CHUNK BY CHUNK instead of into caller buffers for the whole batch: the device works on all n_frames at once (a
 * frame is a serial chain of CTUs, so a call costs about the same from 1 to ~250 pictures: large batches are what the GPU wants), then `fn` is called on the
 * calling thread for pictures [first, first + count) -- records, output pictures, SAO parameters (NULL when want_sao == 0) and statistics of the chunk, in
 * page-locked memory owned by the library and valid only during the call -- while the next chunk is copied from HBM behind it.  The host work per picture
 * (hevcdl_write_access_unit, hashes, PSNR: TEncGOP.cpp:1895-1935, 2420-2447) thus overlaps the copies, and the host never holds more than two chunks
 * (a 2160p picture is 43 MB of results).  chunk_frames <= 0: a default (64).  A non-zero return of fn stops the hand-over: HEVCDL_ERR_INVALID_ARG. */
typedef int (*hevcdl_chunk_fn)(void *user, int first, int count, const hevcdl_ctu_record *records, const void *pictures, const hevcdl_sao_blk *sao_opt,
                               const hevcdl_frame_stats *stats);
hevcdl_status hevcdl_encode_pictures_chunked(hevcdl_ctx *ctx, const void *yuv, int n_frames, const uint8_t *labels_opt, int deblock, int want_sao,
                                             int chunk_frames, hevcdl_chunk_fn fn, void *user);

/* ---- slice data coded on the device (opt-in; csrc/entropy_kernel.hip) ----------------------------------------------------------------------------
 * hevcdl_enable_device_entropy(ctx, 1): every hevcdl_encode_pictures / _chunked / _stream call also codes the slice data of its pictures on the device, from the records
 * and SAO parameters still in HBM (one wave per sub-stream; wavefront rows in two launches, nothing waits).  The call reserves the whole workspace -- sub-stream regions
 * of up to 512 MB worth of pictures (larger batches go through it in passes), as much again for the packed bytes -- and returns HEVCDL_ERR_OOM when the device refuses;
 * (ctx, 0) synchronises the device and frees it.  Off (the default): nothing is launched or allocated, hevcdl_get_slice_data and hevcdl_encode_pictures_stream return
 * HEVCDL_ERR_INVALID_ARG.
 * hevcdl_get_slice_data: the packed sub-streams of pictures [first, first + count) of the LAST such call (valid inside the chunk callback and until the next call):
 * *data, the lengths (*sizes)[count][*n_substreams_per_picture]; picture by picture they feed hevcdl_write_access_unit_from_slice_data.  A picture with a sub-stream that
 * did not fit its region (capacity: 40 960 bytes per CTU + 64) is coded on the host from its records instead, by the same coder source (csrc/entropy_coder.h); the caller sees no difference. */
hevcdl_status hevcdl_enable_device_entropy(hevcdl_ctx *ctx, int on);
hevcdl_status hevcdl_get_slice_data(hevcdl_ctx *ctx, int first, int count, const uint8_t **data, const uint32_t **sizes, int *n_substreams_per_picture);
/* The picture pipeline for a caller that writes the stream from slice data: as hevcdl_encode_pictures_chunked, but the callback gets the slice data of the chunk (as
 * hevcdl_get_slice_data) and the statistics; the output pictures only with want_pictures, the records only with want_records (NULL otherwise) -- without the two
 * flags neither leaves HBM (43 MB a 2160p picture; its slice data is about 0.1 MB).  Needs hevcdl_enable_device_entropy(ctx, 1).  SAO parameters are in the slice
 * data already. */
typedef int (*hevcdl_stream_fn)(void *user, int first, int count, const uint8_t *slice_data, const uint32_t *sizes, int n_substreams_per_picture,
                                const hevcdl_frame_stats *stats, const void *pictures_opt, const hevcdl_ctu_record *records_opt);
hevcdl_status hevcdl_encode_pictures_stream(hevcdl_ctx *ctx, const void *yuv, int n_frames, const uint8_t *labels_opt, int deblock, int want_sao,
                                            int want_pictures, int want_records, int chunk_frames, hevcdl_stream_fn fn, void *user);
/* TEST AND DIAGNOSTIC entry points of the switch.
 * hevcdl_set_entropy_capacity: the capacity per CTU the NEXT hevcdl_enable_device_entropy(ctx, 1) lays its sub-stream regions out with (<= 0: the default; otherwise a
 * multiple of 4).  A small value makes sub-streams overflow, so that the host codes those pictures: that is what it is for.  HEVCDL_ERR_INVALID_ARG while the
 * switch is on.
 * hevcdl_get_entropy_info: about the last hevcdl_encode_pictures* call with the switch on -- *fallbacks_opt: pictures the host coded; kernel_ms_opt[3]: HIP-event
 * times of the wavefront phase-1 launch (0 without wavefront), the coding launch and the pack launch, summed over the passes; measured only with
 * hevcdl_profile_enable(ctx, 1), zeros otherwise. */
hevcdl_status hevcdl_set_entropy_capacity(hevcdl_ctx *ctx, int capacity_per_ctu);
hevcdl_status hevcdl_get_entropy_info(hevcdl_ctx *ctx, int *fallbacks_opt, double *kernel_ms_opt);

/* ---- picture quality: the reference's PrintMSSSIM / PrintFrameMSE / PrintSequenceMSE numbers, computed on the device --------------
 * Replaces TEncGOP::xCalculateMSSSIM (TEncGOP.cpp:2559-2727: 11 x 11 Gaussian window in f64 at every sample position of up to five scales) and the SSD
 * loop of xCalculateAddPSNR (:2380-2390).  org / pic: n_frames packed planar 4:2:0 pictures of the context's size and bit depth (uint16 samples at 10 bits).
 * sse is exact.  Every block SSIM value is computed by the reference's operations in the reference's order and is bit-identical to it; the mean over a
 * scale's blocks is a fixed reduction tree instead of the reference's serial sum, so msssim may differ from the reference by a few units of the last
 * place (it is the same bits on every run, for every batch size and position in the batch).  A plane smaller than the window (8 x 8 chroma of a
 * 16 x 16 picture) gives what the reference's expression gives: 0 / totalBlocks.
 * The device variant is asynchronous on `stream`; d_out must not overlap the pictures (HEVCDL_ERR_INVALID_ARG); d_org == d_pic is allowed. */
typedef struct hevcdl_quality {
  uint64_t sse[3];               /* sum of squared sample differences per plane (Y, Cb, Cr) */
  double   msssim[3];            /* MS-SSIM per plane */
} hevcdl_quality;
hevcdl_status hevcdl_picture_quality(hevcdl_ctx *ctx, const void *org, const void *pic, int n_frames, hevcdl_quality *out);
hevcdl_status hevcdl_picture_quality_dev(hevcdl_ctx *ctx, const void *d_org, const void *d_pic, int n_frames, void *d_out, void *stream);
/* TEST AND DIAGNOSTIC entry point, not for a hot path (it allocates and frees its device buffers on every call): the same for ONE plane of any size from
 * 1 x 1 to 16384 x 16384 and any bit depth from 8 to 16 (host buffers; uint16 samples above 8 bits), without a context.  A context's picture sizes are
 * multiples of 8, so its planes never have the odd sizes and the sizes next to the scale cut-offs (21, 43, 87, 175) that the kernels' tests need; this runs the
 * same kernels on them. */
hevcdl_status hevcdl_plane_quality(int device, const void *org, const void *pic, int width, int height, int bit_depth, uint64_t *sse, double *msssim);
/* The picture pipeline can measure its own output while original and output picture are still in HBM: after hevcdl_enable_quality(ctx, 1) every
 * hevcdl_encode_pictures / hevcdl_encode_pictures_chunked call also computes the hevcdl_quality of its output pictures (after the enabled in-loop
 * filters) against the originals, and hevcdl_get_quality returns those of pictures [first, first + count) of the LAST such call -- valid inside the chunk
 * callback and after the call returns.  Off (the default): nothing is launched or allocated, hevcdl_get_quality returns HEVCDL_ERR_INVALID_ARG.
 * hevcdl_enable_quality(ctx, 1) allocates everything the pass needs (pyramids of up to 16 pictures: 33 MB a picture at 2160p) and returns HEVCDL_ERR_OOM when
 * the device refuses -- call it where the batch is sized, beside hevcdl_reserve_workspace; hevcdl_enable_quality(ctx, 0) synchronises the device and frees it. */
hevcdl_status hevcdl_enable_quality(hevcdl_ctx *ctx, int on);
hevcdl_status hevcdl_get_quality(hevcdl_ctx *ctx, int first, int count, hevcdl_quality *out);

/* ---- picture report: what the log line and the hash SEI of a picture are made of, computed on the device (opt-in; csrc/report_kernel.hip) ----------
 * Replaces, for pictures that are in HBM, the SSD loop of xCalculateAddPSNR (TEncGOP.cpp:2380-2390) and calcMD5 / calcCRC / calcChecksum (TComPicYuvMD5.cpp:88-180;
 * on the host: hevcdl_picture_hash below).  org / pic: n_frames packed planar 4:2:0 pictures of the context's size and bit depth (uint16 samples at 10 bits).
 * sse: the output picture against the original, exact; org == NULL leaves it 0.  digest: the plane digests of `method` (SEIDecodedPictureHash: 0 none -- the digest
 * stays zero --, 1 MD5, 2 CRC, 3 checksum; anything else is HEVCDL_ERR_INVALID_ARG) side by side, plane_bytes each (16 / 2 / 4), exactly as hevcdl_picture_hash leaves
 * them: they feed hevcdl_write_hash_sei.  Everything is integer arithmetic: the same bits as the host's, for every batch size and position in the batch.
 * The device variant is asynchronous on `stream`; d_out (8-byte aligned) must not overlap the pictures (HEVCDL_ERR_INVALID_ARG).
 * Cost at 2160p (profiles/report_time.txt): SSE, CRC and checksum take well under a millisecond a picture at any batch size; an MD5 chain is serial, one lane per plane:
 * a batch costs about 0.14 s whatever it holds, which beats one host core from 5 pictures and 16 host threads from about 75. */
typedef struct hevcdl_picture_report {
  uint64_t sse[3];               /* output picture against the original, per plane; exact */
  uint8_t  digest[48];           /* plane digests side by side, plane_bytes each (16 / 2 / 4), as hevcdl_picture_hash leaves them */
  int32_t  method;               /* 0 none, 1 MD5, 2 CRC, 3 checksum */
  int32_t  plane_bytes;
} hevcdl_picture_report_t;       /* 80 bytes (C gives a function and a typedef one name space: the type's name carries _t, the struct tag is the plain name) */
hevcdl_status hevcdl_picture_report(hevcdl_ctx *ctx, const void *org_opt, const void *pic, int n_frames, int method, hevcdl_picture_report_t *out);
hevcdl_status hevcdl_picture_report_dev(hevcdl_ctx *ctx, const void *d_org_opt, const void *d_pic, int n_frames, int method, void *d_out, void *stream);
/* The picture pipeline can report on its own output while original and output picture are still in HBM: after hevcdl_enable_picture_report(ctx, 1, method) every
 * hevcdl_encode_pictures / _chunked / _stream call also computes the report of its output pictures (after the enabled in-loop filters) against the originals, and
 * hevcdl_get_picture_report returns those of pictures [first, first + count) of the LAST such call -- valid inside the chunk callback and after the call returns.  A
 * hevcdl_encode_pictures_stream call without want_pictures then yields stream, PSNR and hash SEI while only the slice data leaves HBM.  Off (the default): nothing is
 * launched or allocated, hevcdl_get_picture_report returns HEVCDL_ERR_INVALID_ARG.  Enabling allocates the whole workspace for the context's max_frames (records, partials
 * and the SSE words: a few KB a picture) and returns HEVCDL_ERR_OOM when the device refuses; (ctx, 0, 0) synchronises the device and frees it. */
hevcdl_status hevcdl_enable_picture_report(hevcdl_ctx *ctx, int on, int method);
hevcdl_status hevcdl_get_picture_report(hevcdl_ctx *ctx, int first, int count, hevcdl_picture_report_t *out);
/* TEST AND DIAGNOSTIC entry points, not for a hot path.
 * hevcdl_plane_hash: the digest of ONE plane of any size from 1 x 1 (at most 2^20 samples a side and 2^28 in all: a w x 1 plane reaches any byte length) and any bit depth from 8 to 16 (host buffers; uint16 samples above 8 bits), without a
 * context, by the same kernels (it allocates and frees its device buffers on every call): a context's planes never have the odd sizes and the tails the kernels' tests need.
 * digest16 receives 16 / 2 / 4 bytes (method 1 / 2 / 3), the rest is zeroed.
 * hevcdl_plane_hash_host: the shared source (csrc/picture_hash_core.h) on the CPU, no GPU needed, with an explicit chunk size for the CRC / checksum partials
 * (chunk_bytes <= 0: the default).
 * hevcdl_report_chunk_bytes: the default chunk size.
 * hevcdl_get_report_info: HIP-event times of the last report launches of the context -- kernel_ms[3]: the SSE launch (0 without originals), the partial or MD5 launch, the
 * finish launch; measured only with hevcdl_profile_enable(ctx, 1) (the call then synchronises), zeros otherwise. */
hevcdl_status hevcdl_plane_hash(int device, const void *plane, int width, int height, int bit_depth, int method, uint8_t *digest16);
hevcdl_status hevcdl_plane_hash_host(const void *plane, int width, int height, int bit_depth, int method, int chunk_bytes, uint8_t *digest16);
int           hevcdl_report_chunk_bytes(void);
hevcdl_status hevcdl_get_report_info(hevcdl_ctx *ctx, double *kernel_ms);

/* ---- source pictures of any size and bit depth: padding, conformance window, bit-depth conversion (csrc/source_core.h, csrc/source_kernel.hip) ----------------
 * A context is created with the CODED size (multiples of 8) and the internal bit depth, as ever.  A source format describes what the caller's pictures look like
 * instead: source_width x source_height (even, at most the coded size; the difference is the padding, even as well) at input_bit_depth, and at which depth output
 * frames are wanted.  Replaces the reference's file boundary: TVideoIOYuv.cpp readPlane :363-381 (a column past the source width takes the row's last source sample, a
 * row past the source height the row above), scalePlane :70-95 (up: a left shift; down: a rounding right shift clipped to the target depth; no Rec.709 clip), write
 * :755-830 (the window = the coded picture minus the right and lower padding, scaled from the internal to the output depth).  Samples above 8 bits are two bytes,
 * little endian; a picture is its Y, Cb, Cr planes back to back without a pitch.  Input samples must lie inside input_bit_depth. */
typedef struct hevcdl_source_format {
  uint32_t struct_size;          /* sizeof(hevcdl_source_format) */
  int32_t  source_width, source_height;      /* luma samples, even, >= 2 */
  int32_t  input_bit_depth, output_bit_depth;      /* 8 .. 16 */
  /* The file's layout; zero in every field below is a planar 4:2:0 file with Cb before Cr and no explicit window.  The CODED picture is 4:2:0 whatever the file is. */
  int32_t  chroma_format;        /* InputChromaFormat: 400 / 420 / 422 / 444 (0 = 420).  A frame is Y, then both chroma planes at the file's own chroma size (4:0:0: none).  A
                                    coded chroma sample is the nearest (top-left) file sample, no filter: file_c(min(x, sw/2 - 1) << (1 - csx), min(y, sh/2 - 1) << (1 - csy)), the
                                    clamp in coded coordinates (readPlane, TVideoIOYuv.cpp:249-384); 4:0:0: both coded chroma planes are 1 << (input_bit_depth - 1), scaled
                                    like any sample.  Output frames are never converted back: they are 4:2:0 */
  int32_t  colour_space;         /* InputColourSpaceConvert: 0 unchanged, 1 YCbCrtoYCrCb -- file planes 1 and 2 change places on the way in (ColourSpaceConvert, :981-1041);
                                    not with chroma_format 400 */
  int32_t  output_internal_colour_space;      /* OutputInternalColourSpace: 0 output frames get the two planes back in the file's order, 1 they keep the coded order */
  int32_t  snr_internal_colour_space;         /* SNRInternalColourSpace: 0 hevcdl_get_quality / hevcdl_get_picture_report carry U and V (SSE, MS-SSIM) in the file's order,
                                                 1 in the coded order.  Digests are always those of the coded picture */
  int32_t  conf_win_left, conf_win_right, conf_win_top, conf_win_bottom;      /* ConformanceWindowMode 3: an explicit window in luma samples, all even, something left
                                    of the picture.  Only without padding (source size == coded size); output frames are the window (write, :811-826), while quality, the
                                    report and the digests stay over the WHOLE coded picture.  hevcdl_stream_config carries the same four offsets into the SPS */
} hevcdl_source_format;
/* the context's own size and depth: a format that changes nothing */
hevcdl_status hevcdl_source_format_default(hevcdl_source_format *fmt, const hevcdl_config *cfg);
/* The coded size of a source size (TAppEncCfg.cpp:1569-1617).  mode = ConformanceWindowMode: 0 no padding (a size that is no multiple of 8 is HEVCDL_ERR_INVALID_ARG),
 * 1 pad every dimension that is no multiple of the minimum CU (8) up to the next one, 2 pad by pad_x / pad_y (HorizontalPadding / VerticalPadding; the result must be a
 * multiple of 8), 3 (explicit window offsets) HEVCDL_ERR_UNSUPPORTED: that mode pads nothing, so there is no size to derive -- the coded size is the source size
 * (a multiple of 8) and the window goes into hevcdl_source_format.conf_win_*.  Odd padding or an odd source size is HEVCDL_ERR_INVALID_ARG (4:2:0). */
hevcdl_status hevcdl_padded_size(int source_width, int source_height, int mode, int pad_x, int pad_y, int *width, int *height);
size_t        hevcdl_source_frame_bytes(const hevcdl_source_format *fmt);      /* one source-format frame; 0 for an invalid format */
size_t        hevcdl_output_frame_bytes(const hevcdl_source_format *fmt);      /* one output-format frame (window size, output depth) */
/* With a source format set (fmt == NULL clears it; HEVCDL_ERR_INVALID_ARG when it does not fit the context's size), hevcdl_encode_pictures / _chunked / _stream read
 * `yuv` as source-format frames: those bytes are uploaded (an 8-bit source of a 10-bit context is half the bytes of its coded form) and hevcdl_source_load_kernel
 * converts and pads them in HBM in front of the CNN and the decisions.  Records, pictures and slice data stay what they are: coded format, so every consumer keeps
 * working, and the hash SEI / the report's digests cover the whole coded picture.  hevcdl_get_quality and hevcdl_get_picture_report carry SSE and MS-SSIM of the WINDOW
 * (TEncGOP.cpp:2302-2303, 2375-2376, 2413-2414), and so does hevcdl_frame_stats.sse when the picture is padded.  The per-CTU session and the *_dev entry points take
 * coded-format input, as before.  With no format set every entry point behaves exactly as before.
 * The file's layout (chroma_format, colour_space, conf_win_*): hevcdl_source_frame_bytes is the file's own frame (Y plus chroma planes at the file's size) and only those
 * bytes are uploaded; hevcdl_output_frame_bytes is a 4:2:0 frame of the window.  With padding (source size < coded size) quality, report and stats cover the coded picture
 * minus the padding, as above; with an explicit window they cover the WHOLE coded picture.  HEVCDL_ERR_INVALID_ARG: an unknown chroma_format, colour_space outside 0 / 1 or
 * together with chroma_format 400, odd or negative window offsets, a window of no samples, window offsets together with padding. */
hevcdl_status hevcdl_set_source_format(hevcdl_ctx *ctx, const hevcdl_source_format *fmt);
/* source-format frames -> coded-format frames of the context (host buffers: upload, kernel, download; device buffers: asynchronous on `stream`, pointers sample aligned) */
hevcdl_status hevcdl_load_source(hevcdl_ctx *ctx, const void *src, int n_frames, void *coded_out);
hevcdl_status hevcdl_load_source_dev(hevcdl_ctx *ctx, const void *d_src, int n_frames, void *d_coded, void *stream);
/* coded-format pictures -> output-format frames (window size, output depth) */
hevcdl_status hevcdl_store_output(hevcdl_ctx *ctx, const void *pictures, int n_frames, void *out);
hevcdl_status hevcdl_store_output_dev(hevcdl_ctx *ctx, const void *d_pictures, int n_frames, void *d_out, void *stream);
/* Output-format frames of pictures [first, first + count) of the LAST hevcdl_encode_pictures / _chunked / _stream call of a context with a source format, cropped and scaled on
 * the device from the pictures still in HBM -- valid inside the chunk callback and after the call returns.  A run that needs its pictures for the reconstruction file only
 * (hevcdl_encode_pictures_stream without want_pictures, the report on) fetches the window at the output depth this way instead of the coded pictures. */
hevcdl_status hevcdl_get_output_frames(hevcdl_ctx *ctx, int first, int count, void *out);
/* The same on the CPU, by the same source (csrc/source_core.h), without a context or a GPU: coded_width x coded_height at internal_bit_depth (8 .. 16) is the coded format. */
hevcdl_status hevcdl_load_source_host(const hevcdl_source_format *fmt, int coded_width, int coded_height, int internal_bit_depth, const void *src, int n_frames, void *coded_out);
hevcdl_status hevcdl_store_output_host(const hevcdl_source_format *fmt, int coded_width, int coded_height, int internal_bit_depth, const void *pictures, int n_frames, void *out);

/* ---- bitstream writer (host side; no GPU needed) ---------------------------------------------------
 * One access unit per picture exactly as the reference emits it for its all-intra configuration: VPS, SPS, PPS
 * (ReWriteParamSetsFlag 1), then one slice NAL (IDR_W_RADL for POC 0, CRA afterwards), Annex B start codes.
 * Replaces TEncGOP::compressGOP's parameter-set / slice writing (TEncGOP.cpp:1751-1756, 1895-1935), TEncCavlc::codeVPS /
 * codeSPS / codePPS / codeSliceHeader (TEncCavlc.cpp:677, 500, 189, 755), TEncSlice::encodeSlice (TEncSlice.cpp:985) and
 * the arithmetic coder TEncBinCABAC (TEncBinCoderCABAC.cpp:187-446) for the CTU records hevcdl_compress_frames
 * returns.  sao == NULL (cfg.sao_enabled 0): sample_adaptive_offset_enabled_flag 0; otherwise the [ctus] parameters
 * hevcdl_sao_frames returned are coded in front of every CTU. */
typedef struct hevcdl_stream_config {
  uint32_t struct_size;          /* sizeof(hevcdl_stream_config) */
  int32_t  width, height, qp;    /* as in hevcdl_config */
  int32_t  level_idc;            /* general_level_idc = 30 x Level (cfg key Level, TAppEncCfg.cpp:850): 6.2 -> 186, 3.1 -> 93 */
  int32_t  sao_enabled;          /* 1 iff SAO parameters are passed to hevcdl_write_access_unit */
  int32_t  loop_filter_disable;  /* LoopFilterDisable: 1 = pps_deblocking_filter_disabled_flag (the pictures are then NOT to be passed through hevcdl_deblock_frames) */
  int32_t  tile_columns, tile_rows; /* as in hevcdl_config: PPS tile syntax (loop_filter_across_tiles_enabled_flag 1), CTUs in tile scan,
                                       one sub-stream per tile with entry points in the slice header */
  int32_t  bit_depth;            /* 8 (Profile main) or 10 (Profile main10): profile_tier_level, SPS bit depths, SAO offset range */
  int32_t  tile_uniform_spacing; /* as in the hevcdl_config field, default 1; 0: column_width_minus1 / row_height_minus1 are written */
  int32_t  tile_column_width[19], tile_row_height[21];
  int32_t  lf_across_tiles;      /* loop_filter_across_tiles_enabled_flag of the PPS (default 1) */
  uint32_t tools;                /* as in hevcdl_config: transform_skip_enabled_flag / sign_data_hiding_enabled_flag of the PPS, strong_intra_smoothing_enabled_flag of the SPS,
                                    and the residual syntax that goes with the first two */
  int32_t  lf_beta_offset_div2, lf_tc_offset_div2;   /* as in hevcdl_config: pps_beta_offset_div2 / pps_tc_offset_div2 (deblocking_filter_control_present_flag is set when
                                    either is non-zero or the filter is disabled: TEncTop.cpp:1007-1035) */
  int32_t  rewrite_param_sets;   /* ReWriteParamSetsFlag (default 1: VPS / SPS / PPS in front of every picture, all of them IRAPs here); 0: in front of the first picture only
                                    (TEncGOP.cpp:1751) */
  int32_t  wavefront;            /* WaveFrontSynchro (default 0): 1 = entropy_coding_sync_enabled_flag, one sub-stream per CTU row with entry points in the slice header, every row
                                    starting from the contexts behind the second CTU of the row above (TEncSlice.cpp:1047-1145); the records must come from a context with
                                    hevcdl_config.wavefront 1.  Not together with tiles (the reference refuses the pair in the main profiles) */
  int32_t  conf_win_right, conf_win_bottom;   /* conformance window in LUMA samples (default 0): the right and lower padding of a picture whose source size is no multiple of
                                    the minimum CU (hevcdl_source_format); both even.  The SPS carries them in chroma units, conf_win_right_offset = right / 2
                                    (TEncCavlc.cpp:526-535); a decoder then outputs width - right by height - bottom */
  int32_t  conf_win_left, conf_win_top;       /* the other two offsets (default 0; ConformanceWindowMode 3, hevcdl_source_format.conf_win_*): even, and something must be left
                                    of the picture */
                                 /* (LFCrossSliceBoundaryFlag has no field here: without slices -- SliceMode 0, a NULL hevcdl_slice_layout -- the reference sets it to 1 whatever the cfg
                                    says, TAppEncTop.cpp:278-281; tests/golden/stream_c192_q32.npz pins that.  With slices it is hevcdl_slice_layout.lf_across_slices) */
} hevcdl_stream_config;
hevcdl_status hevcdl_stream_config_default(hevcdl_stream_config *cfg, int width, int height, int qp);
size_t        hevcdl_access_unit_bound(int width, int height);
/* records: the [ctus] records of picture `poc` (= frame index; POC lsb is 8 bits).  out_len is set even when the
 * buffer is too small (HEVCDL_ERR_INVALID_ARG), so the call can be repeated.  The slice data is coded by csrc/entropy_coder.h, the source the
 * device kernel compiles too: garbage records give garbage bytes, never an access outside the records. */
hevcdl_status hevcdl_write_access_unit(const hevcdl_stream_config *cfg, int poc, const hevcdl_ctu_record *records, const hevcdl_sao_blk *sao,
                                       uint8_t *out, size_t capacity, size_t *out_len);

/* The same for a stream whose slice headers carry deblocking parameters (DeblockingFilterMetric, LoopFilterOffsetInPPS 0): choice = what hevcdl_get_dbk_choice returned
 * for the picture.  The stream configuration has no field for the two keys; everything they change in the stream is in the choice: override_enabled sets
 * deblocking_filter_override_enabled_flag in the PPS (which keeps cfg's loop_filter_disable and offsets), and the slice header then carries
 * deblocking_filter_override_flag and, behind a 1, the picture's own values (TEncTop.cpp:1007-1035, TEncCavlc.cpp:1080-1095).  LoopFilterOffsetInPPS 0 alone: every slice
 * repeats the cfg's values (TEncSlice.cpp:388-404), loop_filter_disable included.  NULL is hevcdl_write_access_unit itself.  A choice the PPS cannot carry --
 * override_flag without override_enabled, or no override_flag with values that are not the PPS's -- is HEVCDL_ERR_INVALID_ARG. */
hevcdl_status hevcdl_write_access_unit_dbk(const hevcdl_stream_config *cfg, int poc, const hevcdl_ctu_record *records, const hevcdl_sao_blk *sao,
                                           const hevcdl_dbk_choice *choice, uint8_t *out, size_t capacity, size_t *out_len);

/* ---- slice data coded apart from the access unit (csrc/entropy_coder.h: one coder source for the host and the device) -------------------
 * The slice data of a picture is its sub-streams back to back: one per tile in raster order of the tile grid, one per CTU row with wavefront, otherwise one; each
 * is the arithmetic coder's bytes of its CTUs followed by byte_alignment().  hevcdl_write_access_unit_from_slice_data writes everything around that payload exactly as
 * hevcdl_write_access_unit does -- parameter sets, slice segment header with the entry points (counted with their emulation prevention bytes), NAL packing -- so
 * that for the same decisions the two give the same bytes (the slice data of both comes from that one source).  data: the n_substreams sub-streams of picture `poc`, packed; sizes: their lengths. */
hevcdl_status hevcdl_write_access_unit_from_slice_data(const hevcdl_stream_config *cfg, int poc, const uint8_t *data, const uint32_t *sizes, int n_substreams,
                                                       uint8_t *out, size_t capacity, size_t *out_len);
hevcdl_status hevcdl_write_access_unit_from_slice_data_dbk(const hevcdl_stream_config *cfg, int poc, const uint8_t *data, const uint32_t *sizes, int n_substreams,
                                                           const hevcdl_dbk_choice *choice, uint8_t *out, size_t capacity, size_t *out_len);      /* choice: as hevcdl_write_access_unit_dbk */
/* TEST AND DIAGNOSTIC entry points (host buffers in and out; the picture pipeline's form is hevcdl_enable_device_entropy above).
 * hevcdl_slice_data_layout: where the coder puts the sub-streams of ONE picture in a slice-data buffer.  Sub-stream k owns the region [offsets[k], offsets[k] +
 * capacities[k]), capacities[k] = (its CTUs) x capacity_per_ctu + 64, and the regions lie 64 bytes apart: the coder writes nothing but the regions, so a caller may keep a
 * pattern in the gaps (the tests do).  Picture i of a call starts at i x picture_bytes.  capacity_per_ctu <= 0: the default, 40 960: above the derived worst case of a CTU, 38 582 bytes (csrc/entropy_coder.h);
 * otherwise a multiple of 4 (a small value makes sub-streams overflow: that is what it is for).  offsets_opt / capacities_opt: [n_substreams], may be NULL.
 * hevcdl_code_slice_data_host: the coder on the CPU (no GPU needed) for n_frames pictures: records [n_frames][ctus], sao_opt [n_frames][ctus] or NULL as
 * cfg->sao_enabled says, out as laid out above, sizes / overflow [n_frames][n_substreams].  A sub-stream that does not fit its region sets its overflow word; its size is
 * still the true length, and nothing outside the region is written.
 * hevcdl_code_slice_data: the same by the device kernels (csrc/entropy_kernel.hip) on `device`: uploads (the out buffer too, so that what the kernels leave untouched comes
 * back as it went), runs them and downloads. */
hevcdl_status hevcdl_slice_data_layout(const hevcdl_stream_config *cfg, int capacity_per_ctu, int *n_substreams, size_t *picture_bytes,
                                       uint32_t *offsets_opt, uint32_t *capacities_opt);
hevcdl_status hevcdl_code_slice_data_host(const hevcdl_stream_config *cfg, const hevcdl_ctu_record *records, const hevcdl_sao_blk *sao_opt, int n_frames,
                                          int capacity_per_ctu, uint8_t *out, size_t out_capacity, uint32_t *sizes, uint32_t *overflow);
hevcdl_status hevcdl_code_slice_data(int device, const hevcdl_stream_config *cfg, const hevcdl_ctu_record *records, const hevcdl_sao_blk *sao_opt, int n_frames,
                                     int capacity_per_ctu, uint8_t *out, size_t out_capacity, uint32_t *sizes, uint32_t *overflow);

/* ---- slices (cfg keys SliceMode, SliceArgument, LFCrossSliceBoundaryFlag) -----------------------------------------------------------------------------
 * hevcdl_stream_config does not grow (recorded digests hash its bytes): what slices change in a stream is this small block, taken by siblings of the writer's entry points.
 * A NULL layout, or mode 0, is the function without the suffix.  mode 1: slices of `argument` CTUs, whole CTU rows only (a positive multiple of the width in CTUs, at most
 * 22 slices), cfg without tiles and wavefront -- the slice data is then one sub-stream per SLICE (n_substreams = the number of slices), no entry points, and nothing in the
 * stream speaks of tiles.  mode 3: slices of `argument` tiles of cfg's tile grid; sub-streams are the tiles as ever, a slice header carries the entry points of its own tiles.
 * Every slice is a NAL unit of its own with first_slice_segment_in_pic_flag / slice_segment_address and the whole header repeated (TEncCavlc.cpp:755-1109, TEncGOP's slice
 * loop); pps_loop_filter_across_slices_enabled_flag and slice_loop_filter_across_slices_enabled_flag are lf_across_slices.  Anything else is HEVCDL_ERR_INVALID_ARG,
 * mode 2 HEVCDL_ERR_UNSUPPORTED. */
typedef struct hevcdl_slice_layout {
  int32_t mode;                  /* SliceMode 0, 1, 3 */
  int32_t argument;              /* SliceArgument: CTUs (mode 1) or tiles (mode 3) a slice */
  int32_t lf_across_slices;      /* LFCrossSliceBoundaryFlag */
} hevcdl_slice_layout;
/* hevcdl_write_access_unit_dbk / hevcdl_write_access_unit_from_slice_data_dbk (choice may be NULL as there) */
hevcdl_status hevcdl_write_access_unit_slices(const hevcdl_stream_config *cfg, const hevcdl_slice_layout *layout, int poc, const hevcdl_ctu_record *records,
                                              const hevcdl_sao_blk *sao, const hevcdl_dbk_choice *choice, uint8_t *out, size_t capacity, size_t *out_len);
hevcdl_status hevcdl_write_access_unit_from_slice_data_slices(const hevcdl_stream_config *cfg, const hevcdl_slice_layout *layout, int poc, const uint8_t *data,
                                                              const uint32_t *sizes, int n_substreams, const hevcdl_dbk_choice *choice, uint8_t *out, size_t capacity, size_t *out_len);
/* hevcdl_slice_data_layout / hevcdl_code_slice_data_host / hevcdl_code_slice_data: in mode 1 the sub-streams are the slices; in every mode a sub-stream that ends a slice
 * ends with the terminating bin alone, without end_of_slice_segment_flag 0 in front of it */
hevcdl_status hevcdl_slice_data_layout_slices(const hevcdl_stream_config *cfg, const hevcdl_slice_layout *layout, int capacity_per_ctu, int *n_substreams, size_t *picture_bytes,
                                              uint32_t *offsets_opt, uint32_t *capacities_opt);
hevcdl_status hevcdl_code_slice_data_host_slices(const hevcdl_stream_config *cfg, const hevcdl_slice_layout *layout, const hevcdl_ctu_record *records, const hevcdl_sao_blk *sao_opt,
                                                 int n_frames, int capacity_per_ctu, uint8_t *out, size_t out_capacity, uint32_t *sizes, uint32_t *overflow);
hevcdl_status hevcdl_code_slice_data_slices(int device, const hevcdl_stream_config *cfg, const hevcdl_slice_layout *layout, const hevcdl_ctu_record *records,
                                            const hevcdl_sao_blk *sao_opt, int n_frames, int capacity_per_ctu, uint8_t *out, size_t out_capacity, uint32_t *sizes, uint32_t *overflow);
/* hevcdl_access_unit_bound plus the headers of the slice NAL units (at most 22 in mode 1, 440 in mode 3) */
size_t        hevcdl_access_unit_bound_slices(int width, int height, const hevcdl_slice_layout *layout);
/* The layout a context's pictures are written with (mode 0 for a context without slices). */
hevcdl_status hevcdl_get_slice_layout(const hevcdl_ctx *ctx, hevcdl_slice_layout *out);

/* ---- dependent slice segments (cfg keys SliceSegmentMode, SliceSegmentArgument) -----------------------------------------------------------------------------------------
 * Neither hevcdl_stream_config nor hevcdl_slice_layout grows (recorded digests hash the first; callers pass the second without a size): the segments of a stream are this
 * block, taken beside the slice layout by siblings of the _slices entry points.  A NULL block, or mode 0, is the _slices function.  mode 1: segments of `argument` CTUs --
 * cfg with wavefront and without tiles, no slices, `argument` a positive multiple of the width in CTUs: argument / width CTU rows a segment.  mode 3: segments of `argument`
 * tiles of cfg's tile grid, counted from the start of each slice of a mode-3 slice layout (a segment ends where its slice ends).  The sub-streams are those of the stream
 * without segments (CTU rows, tiles).  Every segment is a NAL unit of its own: the PPS says dependent_slice_segments_enabled_flag 1; a header that does not start a slice is
 * dependent_slice_segment_flag 1, slice_segment_address, the entry points of the segment's own rows or tiles, and the alignment (TEncCavlc.cpp:755-1109); a sub-stream that
 * ends a segment ends with end_of_slice_segment_flag 1 alone.  Anything else is HEVCDL_ERR_INVALID_ARG, mode 2 HEVCDL_ERR_UNSUPPORTED. */
typedef struct hevcdl_segment_layout {
  int32_t mode;                  /* SliceSegmentMode 0, 1, 3 */
  int32_t argument;              /* SliceSegmentArgument: CTUs (mode 1) or tiles (mode 3) a segment */
} hevcdl_segment_layout;
hevcdl_status hevcdl_write_access_unit_segments(const hevcdl_stream_config *cfg, const hevcdl_slice_layout *layout, const hevcdl_segment_layout *segments, int poc,
                                                const hevcdl_ctu_record *records, const hevcdl_sao_blk *sao, const hevcdl_dbk_choice *choice, uint8_t *out, size_t capacity, size_t *out_len);
hevcdl_status hevcdl_write_access_unit_from_slice_data_segments(const hevcdl_stream_config *cfg, const hevcdl_slice_layout *layout, const hevcdl_segment_layout *segments, int poc,
                                                                const uint8_t *data, const uint32_t *sizes, int n_substreams, const hevcdl_dbk_choice *choice, uint8_t *out,
                                                                size_t capacity, size_t *out_len);
/* (the regions of a slice-data buffer do not depend on the segments; the function is there so that a caller passes one set of arguments everywhere) */
hevcdl_status hevcdl_slice_data_layout_segments(const hevcdl_stream_config *cfg, const hevcdl_slice_layout *layout, const hevcdl_segment_layout *segments, int capacity_per_ctu,
                                                int *n_substreams, size_t *picture_bytes, uint32_t *offsets_opt, uint32_t *capacities_opt);
hevcdl_status hevcdl_code_slice_data_host_segments(const hevcdl_stream_config *cfg, const hevcdl_slice_layout *layout, const hevcdl_segment_layout *segments,
                                                   const hevcdl_ctu_record *records, const hevcdl_sao_blk *sao_opt, int n_frames, int capacity_per_ctu, uint8_t *out, size_t out_capacity,
                                                   uint32_t *sizes, uint32_t *overflow);
hevcdl_status hevcdl_code_slice_data_segments(int device, const hevcdl_stream_config *cfg, const hevcdl_slice_layout *layout, const hevcdl_segment_layout *segments,
                                              const hevcdl_ctu_record *records, const hevcdl_sao_blk *sao_opt, int n_frames, int capacity_per_ctu, uint8_t *out, size_t out_capacity,
                                              uint32_t *sizes, uint32_t *overflow);
/* hevcdl_access_unit_bound_slices plus the headers of the segment NAL units (one per CTU row or tile at the most) */
size_t        hevcdl_access_unit_bound_segments(int width, int height, const hevcdl_slice_layout *layout, const hevcdl_segment_layout *segments);
/* The segments a context's pictures are written with (mode 0 for a context without them). */
hevcdl_status hevcdl_get_segment_layout(const hevcdl_ctx *ctx, hevcdl_segment_layout *out);

/* Decoded picture hash (cfg key SEIDecodedPictureHash 1 = MD5): the suffix SEI NAL the reference appends to the access unit
 * (TEncGOP.cpp:1938-1960), computed from `picture` = the final reconstruction (planar 4:2:0; uint16 samples at 10 bits).  At most
 * 128 bytes.  A decoder uses it to verify its output bit for bit. */
hevcdl_status hevcdl_write_picture_hash_sei(const hevcdl_stream_config *cfg, const void *picture, uint8_t *out, size_t capacity, size_t *out_len);
/* The three 16-byte MD5 digests (Y, Cb, Cr) themselves, as the reference prints them behind a picture's line (TEncGOP.cpp:2529-2540). */
hevcdl_status hevcdl_picture_md5(const hevcdl_stream_config *cfg, const void *picture, uint8_t digest[48]);
/* The same SEI NAL from digests already computed by hevcdl_picture_md5 (an application that also prints them hashes the picture once). */
hevcdl_status hevcdl_write_digest_sei(const uint8_t digest[48], uint8_t *out, size_t capacity, size_t *out_len);
/* The other two hashes of the key (SEIDecodedPictureHash 2 = CRC, 3 = checksum; 1 = MD5 as above): hevcdl_picture_hash leaves the plane digests of `method` side by side in
 * `digest` (16 / 2 / 4 bytes a plane: *plane_bytes; TComPicYuvMD5.cpp:88-180), hevcdl_write_hash_sei writes the SEI (hash_type = method - 1, SEIwrite.cpp). */
hevcdl_status hevcdl_picture_hash(const hevcdl_stream_config *cfg, const void *picture, int method, uint8_t digest[48], int *plane_bytes);
hevcdl_status hevcdl_write_hash_sei(int method, const uint8_t *digest, uint8_t *out, size_t capacity, size_t *out_len);

/* ---- per-CTU session: the semantic drop-in for the reference's call pair ------------------------
 *   TEncCu::compressCtu(Int m_iFrame, TComDataCU* pCtu)   TEncCu.h:120, called at TEncSlice.cpp:879
 *   TEncCu::encodeCtu(TComDataCU* pCtu)                   TEncCu.h:123, called at TEncSlice.cpp:893
 * One call = both (decide the CTU, then advance the true CABAC state over it).  For CPU-side diff testing against
 * the reference's loop; the batched entry points above are what feeds the GPU.
 *   hevcdl_begin_frames   uploads the frames, takes / predicts their labels (labels_out_opt may be NULL) and clears
 *                         reconstruction and records: the replacement of the label-file poll at TEncCu.cpp:244-253.
 *   hevcdl_compress_ctu   CTUs of a frame must arrive in coding order (neighbours' reconstruction and records live
 *                         in the context).  state_in_opt == NULL: continue from the state the previous call left
 *                         (CTU 0: slice-start contexts of the QP, ContextModel.cpp:56-66); otherwise the caller's
 *                         TEncSbac state (TEncSlice.cpp:826-832).  state_out_opt receives the state after encodeCtu.
 *                         Never hangs and never aborts: ordering / range errors come back as HEVCDL_ERR_INVALID_ARG. */
typedef struct hevcdl_cabac_state {
  uint8_t  ctx[160];    /* (state << 1) | mps of the 159 I-slice contexts in TEncSbac.cpp:62-92 order, 1 pad byte */
  uint64_t frac;        /* TEncBinCABACCounter fractional bit accumulator (15 fractional bits) */
} hevcdl_cabac_state;
hevcdl_status hevcdl_begin_frames(hevcdl_ctx *ctx, const uint8_t *yuv, int n_frames, const uint8_t *labels_opt, uint8_t *labels_out_opt);
hevcdl_status hevcdl_compress_ctu(hevcdl_ctx *ctx, int frame, int ctu_addr, const hevcdl_cabac_state *state_in_opt,
                                  hevcdl_ctu_record *record, hevcdl_cabac_state *state_out_opt);
hevcdl_status hevcdl_get_recon(hevcdl_ctx *ctx, int frame, uint8_t *recon);

/* Page-locked host memory for the yuv / records / picture buffers handed to the host-pointer entry points (optional; ordinary memory works,
 * page-locked memory is copied at the DMA rate).  NULL when no GPU runtime is available. */
/* free / total bytes of a device's memory (hipMemGetInfo): what a front end sizes cfg.max_frames by -- a picture of a call holds about 3 frame buffers, its CTU
 * records (15 120 B per CTU), labels / logits and SAO parameters in HBM */
hevcdl_status hevcdl_device_memory(int device, size_t *free_bytes, size_t *total_bytes);
void *hevcdl_host_alloc(size_t bytes);
void hevcdl_host_free(void *p);

/* ---- device-buffer entry points (inputs/outputs already resident in HBM, asynchronous on `stream`) ---- */
/* All pointers are device pointers; stream is a hipStream_t (NULL = default stream). */
hevcdl_status hevcdl_predict_depth_dev(hevcdl_ctx *ctx, const void *d_yuv, int n_frames, void *d_labels, void *d_logits_opt, void *stream);
/* Labels that do NOT come from hevcdl_predict_depth* (e.g. the unclamped label files of the reference's use_model.py, TEncCu.cpp:244-287):
 * boundary policy HEVCDL_BOUNDARY_CLAMP (see there: label sets that are valid for the reference's walk pass unchanged), in place; a depth above 3 is
 * HEVCDL_ERR_INVALID_ARG.  The host-pointer
 * entry points (labels_opt of hevcdl_compress_frames / hevcdl_encode_pictures / hevcdl_begin_frames) do this themselves; the device
 * entry points below take d_labels as they are and require them to satisfy the policy.  Synchronises `stream`.
 * One context = one launch in flight: the context owns the kernels' workspace, so calls on different streams of the same context must
 * not overlap (use one context per concurrent stream). */
hevcdl_status hevcdl_clamp_labels_dev(hevcdl_ctx *ctx, void *d_labels, int n_frames, void *stream);
hevcdl_status hevcdl_compress_frames_dev(hevcdl_ctx *ctx, const void *d_yuv, int n_frames, const void *d_labels,
                                         void *d_records, void *d_recon, void *d_stats, void *stream);
/* The same for tiles [tile_begin, tile_begin + tile_count) of every frame only (raster order of the cfg's tile grid): the unit of
 * work when the tiles of a picture are spread over several GPUs.  Buffers are whole-frame buffers; only the records, reconstruction
 * samples and statistics (partial sums) of the named tiles are written.  Tiles never read each other's results, so the launches of
 * different ranks need no ordering; the in-loop filters need the assembled picture (hevc-deep-learning-pipeline_amd/sharding.py). */
hevcdl_status hevcdl_compress_tiles_dev(hevcdl_ctx *ctx, const void *d_yuv, int n_frames, const void *d_labels,
                                        void *d_records, void *d_recon, void *d_stats, int tile_begin, int tile_count, void *stream);
/* CNN + RD search back to back: the whole hot path for one batch of frames. */
hevcdl_status hevcdl_encode_frames_dev(hevcdl_ctx *ctx, const void *d_yuv, int n_frames, void *d_labels,
                                       void *d_records, void *d_recon, void *d_stats, void *stream);

/* Which build of the decision kernel and which launch form the context's last decision launch took, as text:
 * "hevcdl_rd_frame_kernel[_wide|_tools|_bd10] form=independent|unit-handover|few-units(...) workgroups=N waves=N units=N" ("" before the first launch).  The selection
 * rule lives in one place (launch_rd); bench.py reports this instead of restating the rule. */
const char   *hevcdl_last_rd_launch(const hevcdl_ctx *ctx);
/* The decision kernel's workspace is allocated by the first launch that needs it (megabytes for a frame in the independent form, 3.4 - 4.3 GB for a launch on every
 * CU) and a launch that cannot get it returns HEVCDL_ERR_OOM; the first launch of a larger shape also synchronises the device while the workspace grows.  This call
 * allocates the largest workspace any launch of the context (1 .. max_frames frames) can ask for, so that a lack of memory shows up here -- the CLI calls it right
 * behind hevcdl_create and retries with a smaller batch -- and no later launch allocates or synchronises. */
hevcdl_status hevcdl_reserve_workspace(hevcdl_ctx *ctx);

/* ---- DeltaQpRD on a context (cfg.delta_qp_rd = N > 0) ----------------------------------------------------------------------------------------------------------------------
 * Every decision call for whole frames -- hevcdl_compress_frames*, hevcdl_encode_frames_dev and the picture pipelines -- runs the label CNN once (where it runs it at all)
 * and then the decision launch 2N+1 times on the caller's stream, each with that candidate's constants and each with the launch plan of the same call without the key.
 * Candidate 0 writes into the call's own records / reconstruction / statistics; later candidates write into one trial set the context owns (records, reconstruction and
 * statistics of max_frames pictures, allocated by the first such call or by hevcdl_reserve_workspace; a refusal is HEVCDL_ERR_OOM).  Behind every launch
 * hevcdl_qp_rd_sum_kernel adds up the picture's bits and dist and compares, and hevcdl_qp_rd_keep_kernel copies the trial set's outputs over the call's own for the
 * pictures whose candidate is the best so far.  The search is deterministic, so the winning trial IS the reference's final compress at the winning QP: it is kept, not
 * run again.  The device entry points need d_records and d_recon 16-byte aligned and d_stats 8-byte aligned (HEVCDL_ERR_INVALID_ARG otherwise).
 * The picture pipelines then fetch the rows (a few words a picture) and run deblocking, the SAO decision and the device entropy coder with every picture's own QP and
 * lambdas.  The host writer takes the picture's QP in hevcdl_stream_config.qp of the call that writes its access unit: slice_qp_delta = qp - 26, and no parameter set
 * depends on it.
 * hevcdl_get_qp_rd: rows [first, first + count) of the LAST decision call of the context (it waits for the device first) and, in qps_opt, the QP every picture was coded
 * with.  On a context without the key: HEVCDL_ERR_INVALID_ARG. */
hevcdl_status hevcdl_get_qp_rd(hevcdl_ctx *ctx, int first, int count, hevcdl_qp_rd_row *rows, int32_t *qps_opt);
/* The stages behind the decisions for pictures with QPs of their own: idx[i] = the candidate (0 .. 2N of the context's table, hevcdl_qp_rd_candidates) picture i was coded
 * with.  idx == NULL is the function without the suffix; an index outside the table is HEVCDL_ERR_INVALID_ARG.  choices_opt: as hevcdl_deblock_frames_choice. */
hevcdl_status hevcdl_deblock_frames_qp(hevcdl_ctx *ctx, const uint8_t *recon, int n_frames, const hevcdl_ctu_record *records, const hevcdl_dbk_choice *choices_opt, const int32_t *idx, uint8_t *out);
hevcdl_status hevcdl_deblock_frames_qp_dev(hevcdl_ctx *ctx, const void *d_recon, int n_frames, const void *d_records, const hevcdl_dbk_choice *choices_opt, const int32_t *idx, void *d_out, void *stream);
hevcdl_status hevcdl_sao_frames_qp(hevcdl_ctx *ctx, const uint8_t *org, const uint8_t *deblocked, int n_frames, const int32_t *idx, hevcdl_sao_blk *params, uint8_t *out);
hevcdl_status hevcdl_sao_frames_qp_dev(hevcdl_ctx *ctx, const void *d_org, const void *d_deblocked, int n_frames, const int32_t *idx, void *d_params, void *d_out, void *stream);
/* TEST AND DIAGNOSTIC entry points.
 * hevcdl_get_qp_rd_info: bytes of the trial set the context holds (0: none allocated) and how many sum / keep kernel launches it has made so far; kernel_ms_opt[2] (may be
 * NULL): HIP-event times of the sum launches and of the keep launches of the LAST search, each summed over its candidates -- measured only with
 * hevcdl_profile_enable(ctx, 1) (the call then synchronises and the events are released), zeros otherwise.
 * hevcdl_qp_rd_step: the two kernels alone, without a context, for candidate `idx` of n_frames pictures of ctus_per_frame CTUs and frame_bytes bytes of reconstruction
 * (a multiple of 16): the sum launch over trial_records and, for idx > 0, the keep launch from the trial set into records / recon / stats.  Host buffers in and out; rows is
 * read (idx > 0: the state the candidates before left) and written.  The three destinations are passed WITH a margin of guard_bytes (a multiple of 16) in front of and
 * behind the payload, uploaded and downloaded whole: what the kernels leave untouched comes back as it went. */
hevcdl_status hevcdl_get_qp_rd_info(hevcdl_ctx *ctx, size_t *trial_bytes, uint64_t *kernel_launches, double *kernel_ms_opt);
hevcdl_status hevcdl_qp_rd_step(int device, int ctus_per_frame, size_t frame_bytes, int n_frames, int idx, double frame_lambda, const hevcdl_ctu_record *trial_records,
                                const void *trial_recon, const hevcdl_frame_stats *trial_stats, hevcdl_qp_rd_row *rows, void *records, void *recon, void *stats, size_t guard_bytes);
/* ---- A QP per picture (cfg keys dQPFile, QPIncrementFrame, IntraQPOffset, LambdaModifierI / LambdaModifier0; csrc/frame_qp.h) -------------------------
 * hevcdl_set_frame_qps: picture i of every following decision, in-loop filter or picture-pipeline call of the context is coded at qp[i], for i < n; pictures past n take the
 * context's QP (the list is copied).  qp == NULL or n == 0 returns to the context's one QP exactly.  A value outside 0 .. 51 is HEVCDL_ERR_INVALID_ARG and leaves the list
 * as it was.  The front ends compute the list from the keys with the rule of csrc/frame_qp.h (TEncCfg::getQPForPicture, TEncTop.cpp:1396-1451) and set the slice of every
 * batch; a sweep sets e.g. 22 27 32 37 on four copies of a picture.
 * hevcdl_set_lambda_modifier: the factor the lambda of every picture is multiplied by before anything is derived from it (LambdaModifierI, else LambdaModifier0:
 * TEncSlice.cpp:512-520).  1.0 (the default) changes no bit.
 * The decisions of a call then run as ONE decision launch per run of equal QP, each with the lambda family of its QP (hevcdl_frame_qp_families) and with the launch plan
 * of a plain call of that many frames.  Where every QP is one contiguous run of the list (32 32 30 30) nothing is copied: the launches take offsets into the caller's
 * buffers.  Otherwise (32 30 32) hevcdl_frame_permute_kernel gathers source pictures and labels into a set sorted by QP, the launches write into a second sorted set, and
 * the kernel scatters records, reconstruction and statistics back in picture order, all on the caller's stream.  Both sets (originals, labels, records, reconstruction
 * and statistics of max_frames pictures) are allocated, all or nothing, by the first call that needs them or by hevcdl_reserve_workspace while a list is set; a refusal is
 * HEVCDL_ERR_OOM.  Deblocking, the SAO decision, the device entropy coder and its host fallback run with every picture's own QP and lambdas; the host writer takes the
 * picture's QP in hevcdl_stream_config.qp of the call that writes its access unit (slice_qp_delta = qp - 26; no parameter set depends on it).
 * Tiles, WaveFrontSynchro, slices and slice segments are allowed (a picture's slices share its QP).  Refused, with a sentence in hevcdl_last_error: a list or a modifier
 * other than 1.0 on a context with delta_qp_rd or deblocking_metric (HEVCDL_ERR_UNSUPPORTED, by the setters); hevcdl_begin_frames and hevcdl_compress_tiles_dev while either is set.
 * hevcdl_get_frame_qps: the QPs of pictures [first, first + count) of the LAST decision call (every picture's, also without a list). */
hevcdl_status hevcdl_set_frame_qps(hevcdl_ctx *ctx, const int *qp, int n);
hevcdl_status hevcdl_set_lambda_modifier(hevcdl_ctx *ctx, double lambda_modifier);
hevcdl_status hevcdl_get_frame_qps(hevcdl_ctx *ctx, int first, int count, int32_t *qp);
/* Host only (no GPU needed): what the two setters would answer on a context of cfg -- HEVCDL_OK, or the status with *why the sentence (a string constant). */
hevcdl_status hevcdl_frame_qp_check(const hevcdl_config *cfg, const int *qp, int n, double lambda_modifier, const char **why);
/* Host only: the rule.  hevcdl_frame_qp_list: out[poc] = Clip3(-6 (bit_depth - 8), 51, base_qp + dqp[poc] + intra_qp_offset) for poc < n (dqp NULL: zeros); a result
 * below 0 is HEVCDL_ERR_INVALID_ARG (10 bits: this path has no negative QP).  hevcdl_frame_qp_offsets: dqp[0 .. n) of a sequence -- zeros, ones from the switching POC of
 * QPIncrementFrame on (qpif < 0: absent; frame_skip, temporal_subsample_ratio as the cfg's), then the integers of the file dqp_file (NULL or "": none), which overwrite;
 * *file_values (may be NULL): how many the file set.  A file that cannot be opened or holds anything but integers of -64 .. 64 is HEVCDL_ERR_INVALID_ARG.
 * hevcdl_frame_qp_families: the decision constants of a picture coded at qp with the modifier.  hevcdl_frame_qp_grouping: perm[n] (sorted place -> picture, stable),
 * run_qp / run_first / run_count (room for 52 each) and *contiguous (1: every QP is one contiguous run of the list as given, nothing would be copied); returns the number
 * of runs, -1 for a QP outside 0 .. 51. */
hevcdl_status hevcdl_frame_qp_list(int base_qp, const int *dqp, int n, int intra_qp_offset, int bit_depth, int *out);
hevcdl_status hevcdl_frame_qp_offsets(int n, int qpif, int frame_skip, int temporal_subsample_ratio, const char *dqp_file, int *dqp, int *file_values);
hevcdl_status hevcdl_frame_qp_families(int qp, int bit_depth, double lambda_modifier, hevcdl_qp_rd_candidate *out);
int hevcdl_frame_qp_grouping(const int *qp, int n, int *perm, int *run_qp, int *run_first, int *run_count, int *contiguous);
/* TEST AND DIAGNOSTIC entry points.
 * hevcdl_get_frame_qp_info: bytes of the two sorted sets the context holds (0: none allocated), decision launches and permute-kernel launches of the LAST decision call;
 * kernel_ms_opt[2] (may be NULL): HIP-event times of its gather and scatter launches -- measured only with hevcdl_profile_enable(ctx, 1), zeros otherwise.
 * hevcdl_frame_permute_step: the kernel alone, without a context, on host buffers: n_ranges (1 .. 4) ranges of bytes[k] bytes a picture, n_frames pictures, picture
 * perm[i] of src[k] to picture i of dst[k] (scatter 0) or picture i to picture perm[i] (scatter 1).  Every destination is passed WITH a margin of guard_bytes in front of and
 * behind the payload, uploaded and downloaded whole: what the kernel leaves untouched comes back as it went.  perm must be a permutation of 0 .. n_frames - 1
 * (HEVCDL_ERR_INVALID_ARG otherwise). */
hevcdl_status hevcdl_get_frame_qp_info(hevcdl_ctx *ctx, size_t *set_bytes, int *rd_launches, int *permute_launches, double *kernel_ms_opt);
hevcdl_status hevcdl_frame_permute_step(int device, int n_ranges, const size_t *bytes, int n_frames, const int *perm, int scatter, const void *const *src, void *const *dst, size_t guard_bytes);
/* ---- stream parser (host side; no GPU needed; csrc/hevcdl_parse.cpp, csrc/hevcdl_parse.h) ----------------------------------------------------------------------------------
 * The inverse of the bitstream writer: an Annex-B stream of the kind hevcdl_write_access_unit_segments produces -- and the reference encoder's streams of the same
 * configurations -- back into what the writer took.  Parsed: start codes and emulation prevention, VPS / SPS / PPS, every slice_segment_header() (entry points, dependent
 * segments, deblocking override and offsets, slice_qp_delta, SAO flags), the decoded picture hash of a suffix SEI (MD5, CRC, checksum), and the slice data of I slices by
 * an arithmetic decoder over csrc/entropy_tables.h: SAO syntax, coding quadtree, part mode, luma and chroma modes, transform tree, cbf, residual_coding with transform skip
 * and sign data hiding, end_of_slice_segment_flag / end_of_subset_one_bit and the byte alignment of every sub-stream (tiles, wavefront rows).
 * One picture of the stream: */
typedef struct hevcdl_parsed_picture {
  int32_t poc;                   /* slice_pic_order_cnt_lsb (0 for an IDR picture) */
  int32_t nal_type;              /* of its slice NAL units: 19 IDR_W_RADL, 20 IDR_N_LP, 21 CRA */
  int32_t qp;                    /* 26 + init_qp_minus26 + slice_qp_delta */
  int32_t sao;                   /* slice_sao_luma_flag (= slice_sao_chroma_flag): the picture's CTUs carry SAO parameters */
  hevcdl_dbk_choice dbk;         /* what its slice headers say about the deblocking filter, as hevcdl_get_dbk_choice gives it */
  int32_t lf_across_slices;      /* slice_loop_filter_across_slices_enabled_flag (the PPS's flag where the header has none) */
  int32_t n_segments;            /* slice segments (NAL units) of the picture */
  int32_t hash_method;           /* decoded picture hash SEI behind the picture: 0 none, 1 MD5, 2 CRC, 3 checksum */
  int32_t hash_plane_bytes;      /* 16 / 2 / 4 */
  uint8_t digest[48];            /* the plane digests side by side, as hevcdl_picture_hash leaves them */
} hevcdl_parsed_picture;
/* cfg (struct_size set by the caller), slices_opt, segments_opt: what hevcdl_write_access_unit_segments would be told to write this stream (cfg->qp: the first picture's;
 * of cfg->tools only the three bits a stream carries -- transform skip, sign hiding, strong intra smoothing -- are the stream's, the others are set).  *n_pictures: pictures
 * in the stream.  pictures_opt[picture_capacity], records_opt / sao_opt [ctu_capacity]: picture i's CTUs at i x hevcdl_ctus_per_frame(cfg->width, cfg->height).  With
 * records_opt NULL only the headers are parsed: call once for the counts, once more with the buffers.  Of a record every field the stream determines is filled (named in
 * csrc/hevcdl_parse.h), bits / dist / cost are 0; sao_opt is needed when a picture has SAO on and holds zeros for the others.
 * Accepted is exactly what this library's writer can produce: I slices, main or main10, 4:2:0, CTU 64, minimum CB 8, TU 4 .. 32, any picture size (multiples of 8) with a
 * conformance window, tiles or wavefront rows, slices of CTU rows or tiles, dependent segments, every tool switch, the deblocking filter on or off.  Anything else is
 * HEVCDL_ERR_UNSUPPORTED -- P and B slices, PCM, scaling lists in the PPS, scaling lists in the SPS, cu_qp_delta_enabled_flag and PPS chroma QP offsets (the last three unless accepted: hevcdl_parse_stream_qp / _sl below), transquant bypass, other chroma formats or bit depths, slices that do not start at
 * a CTU row or a tile, ... -- and a damaged stream is HEVCDL_ERR_INVALID_ARG, never a crash: every value that addresses memory is checked where it is read.  Either way
 * hevcdl_parse_error() is a sentence saying what (per thread; "" after a success). */
hevcdl_status hevcdl_parse_stream(const uint8_t *stream, size_t bytes, hevcdl_stream_config *cfg, hevcdl_slice_layout *slices_opt, hevcdl_segment_layout *segments_opt,
                                  hevcdl_parsed_picture *pictures_opt, int picture_capacity, int *n_pictures, hevcdl_ctu_record *records_opt, hevcdl_sao_blk *sao_opt,
                                  size_t ctu_capacity);
const char   *hevcdl_parse_error(void);
/* The same contract with the slice data decoded by the shared decoder csrc/slice_decode_core.h -- one source for the host and for gfx950, the mirror image of
 * csrc/entropy_coder.h -- instead of the parser's own.  Parameter sets, slice headers, SEI, emulation prevention and the sub-streams are read by the parser's code, so
 * a refusal of the headers is the parser's, sentence included; the slice data of every picture is cut into units (a tile, a row slice, or a picture: the longest run of
 * CTUs one decoder must walk serially) and a unit is decoded by one walker.  Arguments, outputs and statuses are hevcdl_parse_stream's; records and SAO blocks are the
 * same bytes.  An error inside slice data is HEVCDL_ERR_INVALID_ARG with "picture P, CTU A: ..." in hevcdl_parse_error() -- the CTU the parser names.
 * hevcdl_parse_stream_core: the units on the CPU; no GPU needed (TEST AND DIAGNOSTIC).  hevcdl_parse_stream_dev: the units by hevcdl_slice_decode_kernel
 * (csrc/slice_decode_kernel.hip) on `device`, one wave a unit, the pictures of up to a GB of records a launch; records and SAO blocks are downloaded into the caller's
 * buffers (TEST AND DIAGNOSTIC: the decoder's form is hevcdl_enable_device_parse below).  Nothing is launched for a stream the headers refuse.
 * hevcdl_slice_decode_launches: launches of the kernel this process has made (TEST AND DIAGNOSTIC). */
hevcdl_status hevcdl_parse_stream_core(const uint8_t *stream, size_t bytes, hevcdl_stream_config *cfg, hevcdl_slice_layout *slices_opt, hevcdl_segment_layout *segments_opt,
                                       hevcdl_parsed_picture *pictures_opt, int picture_capacity, int *n_pictures, hevcdl_ctu_record *records_opt, hevcdl_sao_blk *sao_opt,
                                       size_t ctu_capacity);
hevcdl_status hevcdl_parse_stream_dev(int device, const uint8_t *stream, size_t bytes, hevcdl_stream_config *cfg, hevcdl_slice_layout *slices_opt,
                                      hevcdl_segment_layout *segments_opt, hevcdl_parsed_picture *pictures_opt, int picture_capacity, int *n_pictures,
                                      hevcdl_ctu_record *records_opt, hevcdl_sao_blk *sao_opt, size_t ctu_capacity);
unsigned long long hevcdl_slice_decode_launches(void);
/* ---- a QP per CU: OFF unless the call accepts it ----------------------------------------------------------------------------------------
 * The entry points above refuse a PPS with cu_qp_delta_enabled_flag or with pps_cb_qp_offset / pps_cr_qp_offset other than 0, sentence for sentence as ever.  The _qp
 * forms take `accept`: with HEVCDL_ACCEPT_CU_QP they read cu_qp_delta_enabled_flag, diff_cu_qp_delta_depth (0 .. 3) and the two offsets (-12 .. 12) into *qp_info_opt,
 * the slice data with cu_qp_delta_abs / cu_qp_delta_sign_flag (7.3.8.14; the two contexts of the prefix stand behind the coder's 161), and derive QpY per 8.6.1: qPY_PREV
 * is SliceQpY at the first quantisation group of a slice, a tile and a wavefront row, else the QpY of the last CU decoded; qPY_A / qPY_B come from inside the CTB only.
 * A CuQpDeltaVal outside -(26 + QpBdOffset / 2) .. 25 + QpBdOffset / 2 is HEVCDL_ERR_INVALID_ARG with its CTU.  pps_slice_chroma_qp_offsets_present_flag stays refused.
 * qp_map_opt: int8 [pictures][ctus][256] BESIDE the records (hevcdl_ctu_record keeps its size): QpY of every 4x4 partition in z-order, every partition of a coded CU
 * filled -- a CU without a cbf has the predicted value -- and 0 outside the picture; a stream without the flag gives its slice QP everywhere.  Room for ctu_capacity CTUs.
 * With accept 0 and no map the three are the entry points above.  _core_qp: the shared decoder on the CPU; _dev_qp: the kernel, which writes the map across its lanes. */
#define HEVCDL_ACCEPT_CU_QP 1u
typedef struct hevcdl_qp_info { int32_t cu_qp_delta_enabled, diff_cu_qp_delta_depth, cb_qp_offset, cr_qp_offset; } hevcdl_qp_info;
hevcdl_status hevcdl_parse_stream_qp(const uint8_t *stream, size_t bytes, unsigned accept, hevcdl_stream_config *cfg, hevcdl_slice_layout *slices_opt,
                                     hevcdl_segment_layout *segments_opt, hevcdl_parsed_picture *pictures_opt, int picture_capacity, int *n_pictures,
                                     hevcdl_ctu_record *records_opt, hevcdl_sao_blk *sao_opt, size_t ctu_capacity, hevcdl_qp_info *qp_info_opt, int8_t *qp_map_opt);
/* What the slice data of the last hevcdl_parse_stream_qp of this thread met (TEST AND DIAGNOSTIC: tools/gen_cu_qp_fixtures.py prints it per fixture).  A group is a
 * quantisation group with at least one CU.  deltas_by_parent_chroma_cbf: read in a 4x4 luma block with cbf_luma 0, i.e. for its parent's chroma cbf;
 * groups_left_from_prev / groups_up_from_prev: qPY_A / qPY_B replaced by qPY_PREV (the group touches its CTB's edge); groups_opening_*: the first group behind a reset of
 * qPY_PREV to SliceQpY (picture start counts as a tile's); coded_behind_uncoded_in_ctu: a group with a delta behind one without in the same CTU. */
typedef struct hevcdl_qp_tally {
  uint32_t groups_with_delta, groups_without_delta, deltas_positive, deltas_negative, deltas_zero, max_abs_delta, deltas_with_suffix, suffixes_of_several_bins,
           deltas_by_parent_chroma_cbf, groups_left_from_prev, groups_up_from_prev, groups_opening_tile, groups_opening_slice, groups_opening_wpp_row, coded_behind_uncoded_in_ctu;
} hevcdl_qp_tally;
void hevcdl_parse_qp_tally(hevcdl_qp_tally *out);
hevcdl_status hevcdl_parse_stream_core_qp(const uint8_t *stream, size_t bytes, unsigned accept, hevcdl_stream_config *cfg, hevcdl_slice_layout *slices_opt,
                                          hevcdl_segment_layout *segments_opt, hevcdl_parsed_picture *pictures_opt, int picture_capacity, int *n_pictures,
                                          hevcdl_ctu_record *records_opt, hevcdl_sao_blk *sao_opt, size_t ctu_capacity, hevcdl_qp_info *qp_info_opt, int8_t *qp_map_opt);
hevcdl_status hevcdl_parse_stream_dev_qp(int device, const uint8_t *stream, size_t bytes, unsigned accept, hevcdl_stream_config *cfg, hevcdl_slice_layout *slices_opt,
                                         hevcdl_segment_layout *segments_opt, hevcdl_parsed_picture *pictures_opt, int picture_capacity, int *n_pictures,
                                         hevcdl_ctu_record *records_opt, hevcdl_sao_blk *sao_opt, size_t ctu_capacity, hevcdl_qp_info *qp_info_opt, int8_t *qp_map_opt);
/* ---- scaling lists: OFF unless the call accepts them -----------------------------------------------------------------------------------------
 * The _sl forms are the _qp forms with one more output; the _qp forms are the _sl forms with scaling_opt NULL.  With HEVCDL_ACCEPT_SCALING_LISTS in `accept` the SPS may set
 * scaling_list_enabled_flag: without sps_scaling_list_data_present_flag the default lists hold (Table 7-5, the intra list of Table 7-6, DC 16), with it scaling_list_data()
 * of 7.3.4 is read -- sizeId 0 .. 3, matrixId 0 .. 5 (0 and 3 for sizeId 3, whose scaling_list_pred_matrix_id_delta counts in steps of 3); the inter lists are parsed and
 * dropped.  HEVCDL_ERR_INVALID_ARG with a sentence: a scaling_list_pred_matrix_id_delta above its matrixId, scaling_list_dc_coef_minus8 outside -7 .. 247, a
 * scaling_list_delta_coef outside -128 .. 127, a list entry of 0, an SPS that ends inside its lists.  pps_scaling_list_data_present_flag stays refused.  Without the bit
 * the flag is refused as ever.  The slice data, the records and the QP map are what they are without lists.
 * hevcdl_scaling_info.factor: ScalingFactor of 7.4.5 as bytes in raster order (y * n + x), plane behind plane: Y 4x4, 8x8, 16x16, 32x32, then Cb 4x4, 8x8, 16x16, then Cr
 * likewise -- 3 * (16 + 64 + 256) + 1024 bytes.  16x16 and 32x32 repeat their 8x8 list by 2 and by 4 and carry their DC entry at [0].  A stream without the flag gives
 * enabled 0 and 16 everywhere. */
#define HEVCDL_ACCEPT_SCALING_LISTS 2u
#define HEVCDL_SCALING_FACTOR_BYTES 2032
typedef struct hevcdl_scaling_info { int32_t enabled, data_present; uint8_t factor[HEVCDL_SCALING_FACTOR_BYTES]; } hevcdl_scaling_info;
hevcdl_status hevcdl_parse_stream_sl(const uint8_t *stream, size_t bytes, unsigned accept, hevcdl_stream_config *cfg, hevcdl_slice_layout *slices_opt,
                                     hevcdl_segment_layout *segments_opt, hevcdl_parsed_picture *pictures_opt, int picture_capacity, int *n_pictures,
                                     hevcdl_ctu_record *records_opt, hevcdl_sao_blk *sao_opt, size_t ctu_capacity, hevcdl_qp_info *qp_info_opt, int8_t *qp_map_opt,
                                     hevcdl_scaling_info *scaling_opt);
hevcdl_status hevcdl_parse_stream_core_sl(const uint8_t *stream, size_t bytes, unsigned accept, hevcdl_stream_config *cfg, hevcdl_slice_layout *slices_opt,
                                          hevcdl_segment_layout *segments_opt, hevcdl_parsed_picture *pictures_opt, int picture_capacity, int *n_pictures,
                                          hevcdl_ctu_record *records_opt, hevcdl_sao_blk *sao_opt, size_t ctu_capacity, hevcdl_qp_info *qp_info_opt, int8_t *qp_map_opt,
                                          hevcdl_scaling_info *scaling_opt);
hevcdl_status hevcdl_parse_stream_dev_sl(int device, const uint8_t *stream, size_t bytes, unsigned accept, hevcdl_stream_config *cfg, hevcdl_slice_layout *slices_opt,
                                         hevcdl_segment_layout *segments_opt, hevcdl_parsed_picture *pictures_opt, int picture_capacity, int *n_pictures,
                                         hevcdl_ctu_record *records_opt, hevcdl_sao_blk *sao_opt, size_t ctu_capacity, hevcdl_qp_info *qp_info_opt, int8_t *qp_map_opt,
                                         hevcdl_scaling_info *scaling_opt);
/* Records a caller brings itself (n_frames pictures of cfg's size), checked as the parser's own are by construction: depths that form a quadtree with the forced splits
 * at the picture's edge, NxN only in 8x8 CUs, prediction modes in range and constant over their block, tr_idx a transform tree within TU 4 .. 32 and depth 3, no cbf
 * bit below the depth of the partition's transform unit, transform-skip flags 0 / 1.  HEVCDL_ERR_INVALID_ARG with a sentence in hevcdl_parse_error() otherwise.  NOT
 * looked at: levels (any 16-bit value is one), and whether the cbf bits of a unit agree with its levels or with the bits of the depths above it. */
hevcdl_status hevcdl_validate_records(const hevcdl_stream_config *cfg, const hevcdl_ctu_record *records, int n_frames);

/* ---- reconstruction from records (csrc/recon_kernel.hip, csrc/recon_core.h): the unfiltered reconstruction of intra pictures -- what hevcdl_compress_frames returns
 * beside its records -- from records alone: per transform unit in coding order the reference samples with availability and substitution (bounded by picture, slice and
 * tile), the [1 2 1] filter and strong smoothing, all 35 prediction modes with the DC and edge filters, dequantisation at the picture's QP, inverse DST / DCT / transform
 * skip, clipping.  The standard's integer arithmetic: no tolerance.  Context-free, like hevcdl_code_slice_data: cfg (width, height, bit_depth 8 / 10, qp, the tile grid,
 * the strong-intra bit of tools) and slices_opt (NULL: one slice a picture) say where a neighbour stops being available; qps_opt (HOST memory, NULL: cfg->qp) a QP per
 * picture.  records [n_frames][ctus], recon: n_frames planar 4:2:0 pictures (uint16 samples at 10 bits).  The sentence of a refusal is in hevcdl_parse_error().
 * hevcdl_reconstruct_frames: host buffers -- records that fail hevcdl_validate_records return its status and nothing is launched -- upload, the kernel hevcdl_recon_kernel, download; a wave
 * rebuilds a CTU row, rows are claimed in order from one ticket, a row stays two CTUs behind the one above.  _dev: device buffers (d_records 16-byte aligned); the records are the
 * caller's word, having passed hevcdl_validate_records before they were uploaded (the kernel clamps every index all the same); launches on `stream` and WAITS for it (the
 * row counts are allocated and freed by the call; hevcdl_decode_stream runs the same launch on a buffer the context owns and fetches the error word with the batch).  _host: the same source on the CPU, no GPU needed (TEST AND DIAGNOSTIC: one sample at a time).
 * hevcdl_recon_launches: launches of the kernel this process has made (TEST AND DIAGNOSTIC). */
hevcdl_status hevcdl_reconstruct_frames(int device, const hevcdl_stream_config *cfg, const hevcdl_slice_layout *slices_opt, const int32_t *qps_opt,
                                        const hevcdl_ctu_record *records, int n_frames, void *recon);
hevcdl_status hevcdl_reconstruct_frames_dev(int device, const hevcdl_stream_config *cfg, const hevcdl_slice_layout *slices_opt, const int32_t *qps_opt,
                                            const void *d_records, int n_frames, void *d_recon, void *stream);
hevcdl_status hevcdl_reconstruct_frames_host(const hevcdl_stream_config *cfg, const hevcdl_slice_layout *slices_opt, const int32_t *qps_opt,
                                             const hevcdl_ctu_record *records, int n_frames, void *recon);
unsigned long long hevcdl_recon_launches(void);
/* The same three with a QP map (hevcdl_parse_stream_qp: int8 [n_frames][ctus][256], HOST memory for the first and the third, DEVICE memory for _dev) and the PPS chroma
 * offsets of *qp_info: a transform unit is dequantised with its CU's QpY; Cb with qPi = Clip3(-QpBdOffset, 57, QpY + pps_cb_qp_offset) through Table 8-10, Cr with
 * pps_cr_qp_offset.  Map values are clamped to -QpBdOffset .. 51 before they are used.  A second instantiation of the kernel: the launch above is the one it was. */
hevcdl_status hevcdl_reconstruct_frames_qp(int device, const hevcdl_stream_config *cfg, const hevcdl_slice_layout *slices_opt, const hevcdl_qp_info *qp_info,
                                           const int8_t *qp_map, const hevcdl_ctu_record *records, int n_frames, void *recon);
hevcdl_status hevcdl_reconstruct_frames_qp_dev(int device, const hevcdl_stream_config *cfg, const hevcdl_slice_layout *slices_opt, const hevcdl_qp_info *qp_info,
                                               const void *d_qp_map, const void *d_records, int n_frames, void *d_recon, void *stream);
hevcdl_status hevcdl_reconstruct_frames_qp_host(const hevcdl_stream_config *cfg, const hevcdl_slice_layout *slices_opt, const hevcdl_qp_info *qp_info,
                                                const int8_t *qp_map, const hevcdl_ctu_record *records, int n_frames, void *recon);
/* The same three with scaling factors on top of the QP map (hevcdl_parse_stream_sl gives both; a stream of one QP has a constant map): scaling->factor as described above,
 * HOST memory in all three -- the 2032 bytes are uploaded by the call.  A coefficient is level * factor * levelScale[qP % 6] << (qP / 6), rounded, shifted by bdShift and
 * clipped to 16 bits (8.6.4.2); a transform-skipped 4x4 block is scaled with its factors too.  A factor of 0 is refused.  A third instantiation of the kernel. */
hevcdl_status hevcdl_reconstruct_frames_sl(int device, const hevcdl_stream_config *cfg, const hevcdl_slice_layout *slices_opt, const hevcdl_qp_info *qp_info,
                                           const int8_t *qp_map, const hevcdl_scaling_info *scaling, const hevcdl_ctu_record *records, int n_frames, void *recon);
hevcdl_status hevcdl_reconstruct_frames_sl_dev(int device, const hevcdl_stream_config *cfg, const hevcdl_slice_layout *slices_opt, const hevcdl_qp_info *qp_info,
                                               const void *d_qp_map, const hevcdl_scaling_info *scaling, const void *d_records, int n_frames, void *d_recon, void *stream);
hevcdl_status hevcdl_reconstruct_frames_sl_host(const hevcdl_stream_config *cfg, const hevcdl_slice_layout *slices_opt, const hevcdl_qp_info *qp_info,
                                                const int8_t *qp_map, const hevcdl_scaling_info *scaling, const hevcdl_ctu_record *records, int n_frames, void *recon);

/* ---- the decoder: a stream of this library's writer, or of the reference encoder in the same configuration, to pictures ------------------------
 * hevcdl_config_from_stream: the configuration of a context that can decode a parsed stream (hevcdl_parse_stream with records_opt NULL gives cfg, the slice layout and
 * the picture count): size, bit depth, QP of the first picture, tiles, loop-filter flags and offsets, the slice keys; max_frames = pictures a batch, device as given.
 * hevcdl_decode_stream: parses on the host, then per batch of cfg.max_frames pictures, in HBM on the context's own buffers: the records are uploaded,
 * the reconstruction kernel rebuilds the pictures, the deblocking filter runs with every picture's own QP and slice-header parameters, SAO with the stream's parameters,
 * and the report kernels compute the digests of the pictures where the stream carries a decoded picture hash SEI (MD5, CRC or checksum).  pictures_opt: picture_capacity
 * pictures in CODED format (the conformance window is not cut: cfg.conf_win_* of the parsed stream say what to show; uint16 samples at 10 bits); info_opt
 * [picture_capacity]: what the headers said; hash_ok_opt [picture_capacity]: 1 the device's digest equals the SEI's, 0 it does not, -1 the picture has no SEI.
 * *n_pictures is set as soon as the headers are parsed, also when there is too little room (HEVCDL_ERR_INVALID_ARG).  The context must describe the stream
 * (HEVCDL_ERR_INVALID_ARG otherwise: size, depth, tiles, slices, loop-filter flags are compared).  A refusal of the parser comes back with its status and its sentence
 * in hevcdl_last_error(ctx).  Parsed on the host, the host holds the whole stream's records while it runs (15 120 bytes a CTU); with hevcdl_enable_device_parse it
 * holds the stream's bytes, its headers and the unit tables, whatever the picture count.
 * hevcdl_enable_device_parse(ctx, 1): hevcdl_decode_stream reads only the headers on the host and cuts the sub-streams; per batch the RBSP bytes and the unit tables go
 * up, hevcdl_slice_decode_kernel writes the records where the reconstruction reads them and the SAO blocks beside them, the error slots come back -- an error is
 * HEVCDL_ERR_INVALID_ARG with picture, CTU and sentence in hevcdl_last_error(ctx), before any reconstruction of the batch is launched -- and of the kernel's output only
 * the SAO blocks (420 bytes a CTU) are downloaded, for the merge resolution of hevcdl_sao_apply_frames_dev.  The buffers (RBSP bytes, tables, error slots, SAO blocks)
 * are sized for cfg.max_frames pictures, grown when a batch needs more, and freed by (ctx, 0).  Off by default: without the call nothing changes. */
hevcdl_status hevcdl_config_from_stream(const hevcdl_stream_config *stream_cfg, const hevcdl_slice_layout *slices_opt, int max_frames, int device, hevcdl_config *out);
hevcdl_status hevcdl_decode_stream(hevcdl_ctx *ctx, const uint8_t *stream, size_t bytes, void *pictures_opt, int picture_capacity, int *n_pictures,
                                   hevcdl_parsed_picture *info_opt, int32_t *hash_ok_opt);
hevcdl_status hevcdl_enable_device_parse(hevcdl_ctx *ctx, int on);
/* hevcdl_enable_cu_qp(ctx, 1): hevcdl_decode_stream accepts streams with cu_qp_delta_enabled_flag or PPS chroma QP offsets (HEVCDL_ACCEPT_CU_QP above).  The QP map of
 * a batch lies in HBM beside the records -- uploaded behind a host parse, written there by hevcdl_slice_decode_kernel with device parse -- and the QP-map instantiations of
 * hevcdl_recon_kernel and hevcdl_deblock_fused_kernel read it; SAO and the report kernels are what they were.  A stream without the flag and with zero offsets takes the
 * constant-QP launches, also when enabled.  Off by default: such a stream is refused with the parser's sentence; (ctx, 0) turns it off again and frees the map.
 * hevcdl_deblock_frames_map: the deblocking filter with a QP per edge on host buffers (TEST AND DIAGNOSTIC) -- per 4-sample edge segment qPL = (QpQ + QpP + 1) >> 1, beta and
 * tC from qPL and the picture's offsets (choices_opt, NULL: the context's), per chroma plane QpC from qPL + the plane's PPS offset; qp_map [n_frames][ctus][256]. */
hevcdl_status hevcdl_enable_cu_qp(hevcdl_ctx *ctx, int on);
/* launches of the QP-map instantiations this process has made: of the reconstruction kernel's -- they count in hevcdl_recon_launches too -- and of the deblocking pair (TEST AND DIAGNOSTIC) */
unsigned long long hevcdl_recon_qp_launches(void);
unsigned long long hevcdl_deblock_qp_launches(void);
/* hevcdl_enable_scaling_lists(ctx, 1): hevcdl_decode_stream parses with HEVCDL_ACCEPT_SCALING_LISTS, with host parse and with device parse.  For a stream with
 * scaling_list_enabled_flag the factor block is uploaded once, the QP map of a batch lies in HBM as with hevcdl_enable_cu_qp (a constant one for a stream of one QP), and the
 * scaling-list instantiation of hevcdl_recon_kernel runs; the deblocking filter, SAO and the report kernels are what they were.  A stream without the flag takes exactly the
 * launches it takes without the switch.  A stream with lists AND cu_qp_delta / chroma QP offsets needs both switches and is refused with the missing one's sentence.
 * Off by default; (ctx, 0) turns it off again and frees the block.  hevcdl_recon_sl_launches: launches of that instantiation by this process -- they count in
 * hevcdl_recon_launches too (TEST AND DIAGNOSTIC). */
hevcdl_status hevcdl_enable_scaling_lists(hevcdl_ctx *ctx, int on);
unsigned long long hevcdl_recon_sl_launches(void);
hevcdl_status hevcdl_deblock_frames_map(hevcdl_ctx *ctx, const void *recon, int n_frames, const hevcdl_ctu_record *records, const hevcdl_dbk_choice *choices_opt,
                                        const hevcdl_qp_info *qp_info, const int8_t *qp_map, void *out);

/* kernel timing with HIP events recorded on the launch stream */
hevcdl_status hevcdl_profile_enable(hevcdl_ctx *ctx, int enable);
hevcdl_status hevcdl_profile_get(hevcdl_ctx *ctx, hevcdl_profile *out);   /* synchronises, returns and resets */

/* sizes */
int      hevcdl_ctus_per_frame(int width, int height);
size_t   hevcdl_frame_bytes(int width, int height);                       /* 8-bit samples */
size_t   hevcdl_frame_bytes_bd(int width, int height, int bit_depth);    /* 2 bytes per sample above 8 bits */

#ifdef __cplusplus
}
#endif
#endif
