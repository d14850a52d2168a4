/* oracle/hm_oracle.h -- TEST INFRASTRUCTURE (CPU oracle), not product code.
 *
 * Plain-C restatement of the reference's depth-pruned all-intra CTU decision path
 * (TEncSlice::compressSlice -> TEncCu::compressCtu -> xCompressCU -> xCheckRDCostIntra
 *  -> TEncSearch::estIntraPredLumaQT / estIntraPredChromaQT).
 * Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may use it.
 * Pinned against the reference itself: oracle/_ref (built by oracle/build_ref.sh) through
 * oracle/gen_fixtures.py -> tests/golden/rd_*.npz.
 */
#ifndef HM_ORACLE_H
#define HM_ORACLE_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* Same layout as hevcdl_ctu_record (include/hevcdl.h): 15120 bytes. */
typedef struct {
  uint8_t  depth[256], part_size[256], luma_dir[256], chroma_dir[256], tr_idx[256];
  uint8_t  cbf[3][256], tskip[3][256];
  uint32_t bits, dist;
  double   cost;
  int16_t  coeff_y[4096], coeff_cb[1024], coeff_cr[1024];
} hm_ctu_record;

typedef struct {
  uint64_t sse[3];      /* reconstruction SSE per plane (before in-loop filters) */
  uint64_t est_bits;    /* sum over CTUs of the CABAC-estimated bits of the final encode */
  uint32_t ctus;
  uint32_t pad;
} hm_frame_stats;

/* Encode n_frames independent all-intra frames (8-bit 4:2:0 planar, Y then U then V per frame).
 * labels: [n_frames][ctus][16] depth labels (already clamped/valid).  out_recs: [n_frames][ctus].
 * recon: same layout as yuv (may be NULL).  stats: [n_frames] (may be NULL).  Returns 0 on success. */
int hm_oracle_encode_frames(const uint8_t *yuv, int width, int height, int n_frames, int qp,
                            const uint8_t *labels, hm_ctu_record *out_recs, uint8_t *recon,
                            hm_frame_stats *stats);
/* The same with tile_cols x tile_rows uniformly spaced tiles (one slice; TileUniformSpacing 1): each tile is coded from a fresh
 * coder state and sees nothing of the other tiles.  Records stay in raster CTU order. */
int hm_oracle_encode_frames_tiles(const uint8_t *yuv, int width, int height, int n_frames, int qp,
                                  const uint8_t *labels, hm_ctu_record *out_recs, uint8_t *recon,
                                  hm_frame_stats *stats, int tile_cols, int tile_rows);
/* bit_depth 8 (uint8 samples) or 10 (uint16 samples, InputBitDepth = InternalBitDepth = 10, Profile main10). */
int hm_oracle_encode_frames_ex(const void *yuv, int width, int height, int n_frames, int qp,
                               const uint8_t *labels, hm_ctu_record *out_recs, void *recon,
                               hm_frame_stats *stats, int tile_cols, int tile_rows, int bit_depth);
/* explicit tile boundaries in CTUs: col_bd[0] = 0 < ... < col_bd[tile_cols] = CTU columns (TileUniformSpacing 0 with width / height arrays) */
int hm_oracle_encode_frames_tb(const void *yuv, int width, int height, int n_frames, int qp,
                               const uint8_t *labels, hm_ctu_record *out_recs, void *recon,
                               hm_frame_stats *stats, int tile_cols, int tile_rows, const int *col_bd, const int *row_bd, int bit_depth);

/* Deblocking (oracle/hm_deblock.c): filters one planar 4:2:0 frame in place, given the frame's CTU records. */
int hm_oracle_deblock_frame(uint8_t *frame, int width, int height, int qp, const hm_ctu_record *recs);
int hm_oracle_deblock_frame16(uint16_t *frame, int width, int height, int qp, const hm_ctu_record *recs, int bit_depth);   /* uint16 samples, bit_depth 8 or 10 */
/* col_bd / row_bd (tile boundaries in CTUs) non-NULL = LFCrossTileBoundaryFlag 0: no filtering across tile borders */
int hm_oracle_deblock_frame16_tb(uint16_t *frame, int width, int height, int qp, const hm_ctu_record *recs, int bit_depth,
                                 int tile_cols, int tile_rows, const int *col_bd, const int *row_bd);

/* Sample adaptive offset (oracle/hm_sao.c).  mode 0 off / 1 new / 2 merge; type: new -> 0..3 edge offset 0/90/135/45 degrees,
 * 4 band offset; merge -> 0 left, 1 above; aux = band position; offset[class] (edge classes 0..4, bands 0..31). */
typedef struct { int32_t mode, type, aux; int32_t offset[32]; } hm_sao_offset;
typedef struct { hm_sao_offset c[3]; } hm_sao_blk;
/* org, deblocked, out: planar 4:2:0 frames; params: [ctus] coded parameters (as written to the bitstream). */
int hm_oracle_sao_frame(const uint8_t *org, const uint8_t *deblocked, int width, int height, int qp, hm_sao_blk *params, uint8_t *out);
/* uint16 sample planes, bit_depth 8 or 10 (offset range 7 / 31, band shift bit_depth - 5, distortion at 8-bit scale) */
int hm_oracle_sao_frame16(const uint16_t *org, const uint16_t *deblocked, int width, int height, int qp, hm_sao_blk *params, uint16_t *out, int tile_cols, int tile_rows, int bit_depth);
int hm_oracle_sao_frame16_tb(const uint16_t *org, const uint16_t *deblocked, int width, int height, int qp, hm_sao_blk *params, uint16_t *out, int tile_cols, int tile_rows, const int *col_bd, const int *row_bd, int bit_depth);
void hm_oracle_sao_set_lf_across_tiles(int flag);   /* LFCrossTileBoundaryFlag for the next hm_oracle_sao_* calls (default 1) */
int hm_oracle_sao_frame_tiles(const uint8_t *org, const uint8_t *deblocked, int width, int height, int qp, hm_sao_blk *params, uint8_t *out, int tile_cols, int tile_rows);

/* Leaf entries (tests/test_rd_leaf.py, tests/test_rd_leaf_gpu.py): the routines of a TU coding and of the intra prediction on blocks of the caller's, the same
 * static functions the frame path runs.  Both return 0, or -1 for arguments outside what the frame path can reach.
 *
 * hm_oracle_tu_leaf: n_blocks blocks of n x n (4..32; chroma up to 16) values, raster, through the chain of code_tu_block from `entry`:
 *   0 `in` = residual: forward transform (DST for 4x4 luma) or, with tskip (4x4 only), the transform-skip scaling
 *   1 `in` = coefficients: the quantiser -- rdoq() or plain_quant(), chosen by tools and tskip as code_tu_block does -- from the coder state ctx_in[b][160]
 *     (context bytes, [159] = 0; fractional bit counter 0), then, when abs_sum > 0, code_coeff_nxn on that state
 *   2 `in` = levels: dequantiser and inverse transform only (abs_sum = sum of |level|; the coder does not run)
 * Outputs per block: coef (behind the transform; zeros for entry 2), lvl, abs_sum, frac and ctx_out (the coder behind code_coeff_nxn, or as it came in), deq
 * (dequantised), resi (reconstructed residual); with abs_sum == 0 (entries 0, 1) lvl, deq and resi are zeros, as code_tu_block leaves them.
 * stage1 (may be NULL; entry 0 without tskip): the forward transform's first-stage intermediate [frequency][row]. */
int hm_oracle_tu_leaf(int qp, int bit_depth, unsigned tools, int comp, int n, int dir_mode, int tskip, int cbf_ctx, int entry, int n_blocks,
                      const int32_t *in, const uint8_t *ctx_in, int32_t *coef, int32_t *lvl, uint32_t *abs_sum, uint64_t *frac, uint8_t *ctx_out,
                      int32_t *deq, int32_t *resi, int32_t *stage1);
/* hm_oracle_pred_leaf: n_cases reference lines of 4n+1 samples (bottom-left ... corner ... top-right) and, for luma, original blocks of n x n.
 * Luma n 4..64, chroma 4..16.  fline (luma): filter_refs of the line (strong smoothing at n >= 32 under tool bit 0x20); pred [case][35][n * n] (n <= 32):
 * predict_intra of every mode from the line use_filtered_refs selects; satd [case][35] (luma): the rough mode decision's SATD against the original block
 * (Hadamard 8x8, 4x4 for a 4x4 block, with the distortion shift of bit_depth 10).  fline / pred / satd may be NULL. */
int hm_oracle_pred_leaf(int bit_depth, unsigned tools, int comp, int n, int n_cases, const int16_t *lines, const int16_t *org,
                        int16_t *fline, int16_t *pred, uint32_t *satd_out);

/* Debug: if non-NULL, every RD cost evaluation appends (bits, dist) to this FILE (text). */
void hm_oracle_set_trace(const char *path);

#ifdef __cplusplus
}
#endif
#endif
