// qp_rd.h -- the slice QP of a picture picked among 2N+1 candidate encodes (cfg key DeltaQpRD, "slice-based multi-QP optimization"): pure functions, no HIP header, so
// that a stand-alone harness compiles them with any compiler and sanitizer (tests/deltaqprd_harness.cpp).  The device side is csrc/qp_rd_kernel.hip, which compiles the
// pick rule below for the GPU; the host runs the same source.
//
// Replaces TEncSlice::initEncSlice's candidate loop (TEncSlice.cpp:288-305), calculateLambda (:433-527), setUpLambda (:112-140) and the comparison of
// TEncSlice::precompressSlice (:572-661) with TComRdCost::calcRdCost(bits, dist, DF_SSE_FRAME) (TComRdCost.cpp:62-107).
#ifndef HEVCDL_QP_RD_H
#define HEVCDL_QP_RD_H
#include <math.h>
#include <stdint.h>
#include "hevcdl.h"      // HEVCDL_QP_RD_MAX_N, hevcdl_qp_rd_row, hevcdl_qp_rd_candidate

#if defined(__HIPCC__)
#define HEVCDL_QP_RD_FN __host__ __device__ static inline
#else
#define HEVCDL_QP_RD_FN static inline
#endif

// TEncSlice.cpp:294: candidate idx of 0 .. 2N is offset ((idx + 1) >> 1) * (idx odd ? -1 : +1): 0, -1, +1, -2, +2, ...
HEVCDL_QP_RD_FN int hevcdl_qp_rd_offset(int idx) { return ((idx + 1) >> 1) * ((idx & 1) ? -1 : 1); }
// TEncSlice.cpp:523: the QP a candidate is coded at -- iQP = max(-QpBDOffset, min(51, floor(dQP + 0.5))); its lambda is that of the UNCLIPPED dQP
HEVCDL_QP_RD_FN int hevcdl_qp_rd_clip_qp(int dqp, int bit_depth)
{
  const int lo = -6 * (bit_depth - 8);
  return dqp > 51 ? 51 : (dqp < lo ? lo : dqp);
}

#define HEVCDL_QP_RD_MAX_DOUBLE 1.7e+308      /* MAX_DOUBLE, TypeDef.h */

// The comparison of precompressSlice (TEncSlice.cpp:646-652) for one candidate: cost = dist + bits * frameLambda, the multiply and the add two separate IEEE operations
// (the library is built with contraction off; the pragma says so again where a compiler knows it); strict `<` against the best so far, so that a tie keeps the EARLIER
// index.  Returns 1 when candidate `idx` is the new best and updates *best_cost.
HEVCDL_QP_RD_FN int hevcdl_qp_rd_better(uint64_t bits, uint64_t dist, double frame_lambda, double *best_cost)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double prod = (double)bits * frame_lambda;
  const double cost = (double)dist + prod;
  if (cost < *best_cost) { *best_cost = cost; return 1; }
  return 0;
}

// The pick rule over whole rows of sums: the index precompressSlice ends with for n candidates in order.
HEVCDL_QP_RD_FN int hevcdl_qp_rd_pick(const uint64_t *bits, const uint64_t *dist, int n, double frame_lambda)
{
  double best = HEVCDL_QP_RD_MAX_DOUBLE;
  int best_idx = 0;
  for (int i = 0; i < n; i++) if (hevcdl_qp_rd_better(bits[i], dist[i], frame_lambda, &best)) best_idx = i;
  return best_idx;
}

// ---- host only: the lambda family (hevcdl_qp_rd_candidate, include/hevcdl.h) of a (lambda QP, coded QP) pair ---------------------------------------------------------------------------------------------------------
static const int HEVCDL_CHROMA_SCALE_420[58] = { 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16, 17, 18, 19, 20, 21, 22, 23, 24, 25, 26, 27, 28, 29,
  29, 30, 31, 32, 33, 33, 34, 34, 35, 35, 36, 36, 37, 37, 38, 39, 40, 41, 42, 43, 44, 45, 46, 47, 48, 49, 50, 51 };   // TComRom.cpp:536
static const int HEVCDL_QUANT_SCALES[6] = { 26214, 23302, 20560, 18396, 16384, 14564 };   // TComRom.cpp:354-357
static const int HEVCDL_INV_QUANT_SCALES[6] = { 40, 45, 51, 57, 64, 72 };                  // TComRom.cpp:359-362

// TEncSlice::calculateLambda (TEncSlice.cpp:433-527) for an all-intra GOP of 1 at lambda_qp (the unclipped dQP), then setUpLambda (:112-140) and the quantiser's tables at
// the coded QP `qp` (>= 0): what hevcdl_config_default* fills a configuration with (lambda_qp == qp there) and what every candidate of the QP search runs with.
static inline void hevcdl_lambda_family_of(int lambda_qp, int qp, int bit_depth, hevcdl_qp_rd_candidate *f)
{
  f->qp = qp;
  f->lambda = 0.57 * 1.0 * pow(2.0, (lambda_qp - 12) / 3.0);
  f->sqrt_lambda = sqrt(f->lambda);                         // TComRdCost::setLambda TComRdCost.cpp:109-122
  f->qp_chroma = HEVCDL_CHROMA_SCALE_420[qp];
  f->chroma_weight = pow(2.0, (qp - f->qp_chroma) / 3.0);
  f->lambda_chroma = f->lambda / f->chroma_weight;
  for (int ch = 0; ch < 2; ch++) {
    // quantiser QP = QP + qpBdOffset (6 per extra bit, TComTrQuant.cpp:71-100); distortion is kept at 8-bit scale (FULL_NBIT 0:
    // DISTORTION_PRECISION_ADJUSTMENT, TypeDef.h:170), hence the 1 << 2(bd-8) divisors
    const int q = (ch ? f->qp_chroma : qp) + 6 * (bit_depth - 8), rem = q % 6, per = q / 6, dadj = 2 * (bit_depth - 8);
    for (int l = 0; l < 4; l++) {                               // TComTrQuant::setErrScaleCoeff TComTrQuant.cpp:3096-3126
      const int tshift = 15 - bit_depth - (l + 2);
      double s = (double)(1 << 15);
      s = s * pow(2.0, -2.0 * tshift);
      f->err_scale[ch][l] = s / HEVCDL_QUANT_SCALES[rem] / HEVCDL_QUANT_SCALES[rem] / (1 << dadj);
    }
    const double inv = (double)HEVCDL_INV_QUANT_SCALES[rem], lam = ch ? f->lambda_chroma : f->lambda;
    f->sbh_rd_factor[ch] = (int64_t)(inv * inv * (1 << (2 * per)) / lam / 16 / (1 << dadj) + 0.5);   // TComTrQuant.cpp:2532-2535
  }
}

// The candidate table of a configuration (TEncSlice.cpp:288-305): for idx 0 .. 2 n: cand[idx], its offset and constants (coded at the clipped QP with the lambda of the unclipped one),
// and the frame lambda of precompressSlice (:615-623, GOP size 1): 0.68 * 2^((iQP[0] - 12) / 3).  Returns the number of candidates, or -1 for arguments outside
// 0 <= n <= HEVCDL_QP_RD_MAX_N, 0 <= qp <= 51, or a candidate below QP 0 (10 bits: the reference would code at a negative QP, which this path does not have).
static inline int hevcdl_qp_rd_table(int qp, int n, int bit_depth, hevcdl_qp_rd_candidate *cand, double *frame_lambda)
{
  if (n < 0 || n > HEVCDL_QP_RD_MAX_N || qp < 0 || qp > 51 || (bit_depth != 8 && bit_depth != 10)) return -1;
  for (int idx = 0; idx < 2 * n + 1; idx++) {
    const int dqp = qp + hevcdl_qp_rd_offset(idx), iqp = hevcdl_qp_rd_clip_qp(dqp, bit_depth);
    if (iqp < 0) return -1;
    cand[idx].offset = hevcdl_qp_rd_offset(idx); cand[idx].pad = 0;
    hevcdl_lambda_family_of(dqp, iqp, bit_depth, &cand[idx]);
  }
  *frame_lambda = 0.68 * pow(2.0, (qp - 12) / 3.0);
  return 2 * n + 1;
}

// What hevcdl_create refuses of a configuration with the key, in the words hevcdl_create_error gives (and the command line prints): HEVCDL_OK, or the status and *why.
static inline hevcdl_status hevcdl_qp_rd_keys(const hevcdl_config *cfg, const char **why)
{
  *why = "";
  if (cfg->delta_qp_rd == 0) return HEVCDL_OK;
#define QP_RD_REFUSE(status, text) do { *why = text; return status; } while (0)
  if (cfg->delta_qp_rd < 0 || cfg->delta_qp_rd > HEVCDL_QP_RD_MAX_N) QP_RD_REFUSE(HEVCDL_ERR_INVALID_ARG, "DeltaQpRD is 0 .. 6: every picture is decided 2 DeltaQpRD + 1 times, and six steps either way double or halve the quantiser step");
  if (cfg->slice_mode != 0) QP_RD_REFUSE(HEVCDL_ERR_UNSUPPORTED, "DeltaQpRD together with slices is not supported: the reference picks a QP per slice, this path per picture");
  if (cfg->slice_segment_mode != 0) QP_RD_REFUSE(HEVCDL_ERR_UNSUPPORTED, "DeltaQpRD together with slice segments is not supported: the reference picks a QP per slice, this path per picture");
  if (cfg->deblocking_metric != 0) QP_RD_REFUSE(HEVCDL_ERR_UNSUPPORTED, "DeltaQpRD together with DeblockingFilterMetric is not supported");
  if (cfg->bit_depth > 8 && cfg->qp - cfg->delta_qp_rd < 0) QP_RD_REFUSE(HEVCDL_ERR_UNSUPPORTED, "DeltaQpRD at 10 bits needs QP - DeltaQpRD >= 0: the reference would code a candidate at a negative QP, which this path does not have");
#undef QP_RD_REFUSE
  return HEVCDL_OK;
}
#endif
