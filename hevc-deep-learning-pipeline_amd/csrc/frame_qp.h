// frame_qp.h -- a QP per picture (cfg keys dQPFile, QPIncrementFrame, IntraQPOffset, LambdaModifierI / LambdaModifier0): the rule that turns the keys into the QP and the
// lambda family of every picture, the grouping of a batch's pictures by QP, and what is refused -- pure functions, no HIP header, shared by the library
// (csrc/hevcdl_api.hip) and the command line (csrc/hevcdl_app.cpp) and compiled by a stand-alone harness with any compiler and sanitizer (tests/frame_qp_harness.cpp).
// The device side is csrc/frame_permute_kernel.hip.
//
// Replaces TEncCfg::getQPForPicture (TEncTop.cpp:1396-1451) for an I slice, the m_aidQP table of TAppEncCfg::xCheckParameter (TAppEncCfg.cpp:1663-1681, 1735-1753) and the
// lambda modifier of TEncSlice::calculateLambda (TEncSlice.cpp:510-521).
#ifndef HEVCDL_FRAME_QP_H
#define HEVCDL_FRAME_QP_H
#include <stdio.h>
#include <stdlib.h>
#include "hevcdl.h"
#include "qp_rd.h"      // hevcdl_lambda_family_of, hevcdl_qp_rd_clip_qp

// The QP of the picture at `poc`: qp = Clip3(-QpBDOffset, 51, base + dqp[poc] + IntraQPOffset) (TEncTop.cpp:1409-1423, 1449; every picture of this path is an I slice).
// Returns the QP, which is negative where the reference would code below QP 0 (10 bits): this path has no negative QP, the callers refuse it.
static inline int hevcdl_frame_qp_of(int base_qp, int dqp, int intra_qp_offset, int bit_depth) { return hevcdl_qp_rd_clip_qp(base_qp + dqp + intra_qp_offset, bit_depth); }

// The lambda family of a picture coded at `qp`: hevcdl_lambda_family_of(qp, qp) with dLambda *= lambdaModifier (TEncSlice.cpp:520) before setLambda takes its square root
// (TComRdCost.cpp:109-122), before setUpLambda divides it by the chroma weight (TEncSlice.cpp:112-140) and before the sign-hiding factors (TComTrQuant.cpp:2532-2535).
// The family's own lambda is 0.57 * 1.0 * 2^((qp - 12) / 3), the product the reference forms first; one more multiply by 1.0 changes no bit.
static inline void hevcdl_frame_qp_family(int qp, int bit_depth, double lambda_modifier, hevcdl_qp_rd_candidate *f)
{
  hevcdl_lambda_family_of(qp, qp, bit_depth, f);
  f->offset = 0; f->pad = 0;
  if (lambda_modifier == 1.0) return;
  f->lambda = f->lambda * lambda_modifier;
  f->sqrt_lambda = sqrt(f->lambda);
  f->lambda_chroma = f->lambda / f->chroma_weight;
  for (int ch = 0; ch < 2; ch++) {
    const int q = (ch ? f->qp_chroma : qp) + 6 * (bit_depth - 8), rem = q % 6, per = q / 6, dadj = 2 * (bit_depth - 8);
    const double inv = (double)HEVCDL_INV_QUANT_SCALES[rem], lam = ch ? f->lambda_chroma : f->lambda;
    f->sbh_rd_factor[ch] = (int64_t)(inv * inv * (1 << (2 * per)) / lam / 16 / (1 << dadj) + 0.5);
  }
}

// QPIncrementFrame (TAppEncCfg.cpp:1667-1681): the POC from which every picture's offset is 1.
static inline int hevcdl_qp_switching_poc(unsigned value, unsigned frame_skip, unsigned temporal_subsample_ratio)
{
  return value > frame_skip ? (int)((value - frame_skip) / (temporal_subsample_ratio ? temporal_subsample_ratio : 1)) : 0;
}
// The offsets of a sequence of n POCs: zeros; with the increment (qpif_present) ones from the switching POC on.  dQPFile is read afterwards and overwrites.
static inline void hevcdl_dqp_increment(int *dqp, int n, int qpif_present, unsigned value, unsigned frame_skip, unsigned temporal_subsample_ratio)
{
  for (int i = 0; i < n; i++) dqp[i] = 0;
  if (!qpif_present) return;
  for (int i = hevcdl_qp_switching_poc(value, frame_skip, temporal_subsample_ratio); i < n; i++) dqp[i] = 1;
}
// dQPFile (TAppEncCfg.cpp:1735-1753): whitespace-separated integers, one a POC, for at most n POCs; a short file leaves the rest as they were, values past the n-th are
// not read.  Returns how many offsets the file set, -1 when it cannot be opened, -2 when it holds something that is not an integer (the reference's fscanf loop would
// then store an undefined value in every remaining POC: refused here), -3 for a value outside -64 .. 64 (no QP is that far from another).
static inline int hevcdl_dqp_read_file(const char *path, int *dqp, int n)
{
  FILE *f = fopen(path, "r");
  if (!f) return -1;
  int poc = 0, bad = 0;
  while (poc < n) {
    long v = 0;
    const int got = fscanf(f, "%ld", &v);
    if (got == EOF) break;
    if (got != 1) { bad = -2; break; }
    if (v < -64 || v > 64) { bad = -3; break; }
    dqp[poc++] = (int)v;
  }
  fclose(f);
  return bad ? bad : poc;
}

// ---- the grouping: pictures of one QP form one decision launch --------------------------------------------------------------------------------------------------------
typedef struct hevcdl_qp_run { int qp, first, count; } hevcdl_qp_run;      // pictures [first, first + count) of the SORTED order share `qp`
// From qp[0 .. n): perm[i] = the picture that stands at place i when the pictures are sorted by QP, equal QPs in picture order (a stable counting sort over 0 .. 51);
// runs[] = the runs of equal QP in that order, increasing QP.  Returns the number of runs (0 for n == 0), or -1 for a QP outside 0 .. 51.  runs needs room for
// min(n, 52) entries.  *contiguous (may be NULL): 1 when perm is the identity -- every QP is one contiguous run of the list, in increasing order -- and nothing needs copying.
static inline int hevcdl_frame_qp_group(const int *qp, int n, int *perm, hevcdl_qp_run *runs, int *contiguous)
{
  int count[53];
  for (int q = 0; q < 53; q++) count[q] = 0;
  for (int i = 0; i < n; i++) { if (qp[i] < 0 || qp[i] > 51) return -1; count[qp[i] + 1]++; }
  int n_runs = 0;
  for (int q = 0; q < 52; q++) {
    if (count[q + 1]) { runs[n_runs].qp = q; runs[n_runs].first = count[q]; runs[n_runs].count = count[q + 1]; n_runs++; }
    count[q + 1] += count[q];      // count[q] = first place of QP q
  }
  for (int i = 0; i < n; i++) perm[count[qp[i]]++] = i;
  if (contiguous) { *contiguous = 1; for (int i = 0; i < n; i++) if (perm[i] != i) *contiguous = 0; }
  return n_runs;
}
// The list as the no-copy path wants it: every QP one contiguous run, in ANY order of QPs (32 32 30 30 is fine, 32 30 32 is not).  Fills runs[] in list order with `first`
// the run's first PICTURE; returns the number of runs, 0 when a QP comes back after another (then hevcdl_frame_qp_group's permutation is needed), -1 for a bad QP.
static inline int hevcdl_frame_qp_contiguous_runs(const int *qp, int n, hevcdl_qp_run *runs)
{
  unsigned char seen[52];
  for (int q = 0; q < 52; q++) seen[q] = 0;
  int n_runs = 0;
  for (int i = 0; i < n; i++) {
    if (qp[i] < 0 || qp[i] > 51) return -1;
    if (i && qp[i] == qp[i - 1]) { runs[n_runs - 1].count++; continue; }
    if (seen[qp[i]]) return 0;
    seen[qp[i]] = 1;
    runs[n_runs].qp = qp[i]; runs[n_runs].first = i; runs[n_runs].count = 1; n_runs++;
  }
  return n_runs;
}
// inv[perm[i]] = i: the scatter permutation of a gather permutation
static inline void hevcdl_frame_qp_inverse(const int *perm, int n, int *inv) { for (int i = 0; i < n; i++) inv[perm[i]] = i; }

// ---- what is refused, in the words hevcdl_set_frame_qps / hevcdl_set_lambda_modifier leave in hevcdl_last_error and the command line prints ----------------------------
#define HEVCDL_FRAME_QP_REFUSE_QP_RD      "a QP per picture (dQPFile, QPIncrementFrame, IntraQPOffset, LambdaModifier) together with DeltaQpRD is not supported: the search would run 2N+1 candidates round every picture's own QP"
#define HEVCDL_FRAME_QP_REFUSE_DBK_METRIC "a QP per picture (dQPFile, QPIncrementFrame, IntraQPOffset, LambdaModifier) together with DeblockingFilterMetric is not supported: the metric's thresholds and trials are taken at the context's QP"
#define HEVCDL_FRAME_QP_REFUSE_SESSION    "the per-CTU session codes every picture at the context's QP: a QP per picture is not supported there; use hevcdl_compress_frames"
#define HEVCDL_FRAME_QP_REFUSE_TILES      "compress_tiles: a QP per picture is not supported on a range of tiles (the ranks of a tile-sharded run would each have to group the same pictures); use hevcdl_compress_frames_dev"
#define HEVCDL_FRAME_QP_REFUSE_RANGE      "a picture's QP lies outside 0 .. 51"
#define HEVCDL_FRAME_QP_REFUSE_NEGATIVE   "a picture's QP is below 0: at 10 bits the reference would code it at a negative QP, which this path does not have"
#define HEVCDL_FRAME_QP_REFUSE_MODIFIER   "the lambda modifier is a finite number above 0"

// A list of n QPs (NULL / 0: none) and a lambda modifier on a context of `cfg`: HEVCDL_OK, or the status and *why.
static inline hevcdl_status hevcdl_frame_qp_keys(const hevcdl_config *cfg, const int *qp, int n, double lambda_modifier, const char **why)
{
  *why = "";
#define FRAME_QP_REFUSE(status, text) do { *why = text; return status; } while (0)
  if (!(lambda_modifier > 0.0) || !(lambda_modifier < 1.0e30)) FRAME_QP_REFUSE(HEVCDL_ERR_INVALID_ARG, HEVCDL_FRAME_QP_REFUSE_MODIFIER);
  for (int i = 0; qp && i < n; i++) {
    if (qp[i] < 0 && qp[i] >= -6 * (cfg->bit_depth - 8)) FRAME_QP_REFUSE(HEVCDL_ERR_INVALID_ARG, HEVCDL_FRAME_QP_REFUSE_NEGATIVE);
    if (qp[i] < 0 || qp[i] > 51) FRAME_QP_REFUSE(HEVCDL_ERR_INVALID_ARG, HEVCDL_FRAME_QP_REFUSE_RANGE);
  }
  if ((!qp || n <= 0) && lambda_modifier == 1.0) return HEVCDL_OK;
  if (cfg->delta_qp_rd != 0) FRAME_QP_REFUSE(HEVCDL_ERR_UNSUPPORTED, HEVCDL_FRAME_QP_REFUSE_QP_RD);
  if (cfg->deblocking_metric != 0) FRAME_QP_REFUSE(HEVCDL_ERR_UNSUPPORTED, HEVCDL_FRAME_QP_REFUSE_DBK_METRIC);
#undef FRAME_QP_REFUSE
  return HEVCDL_OK;
}
#endif
