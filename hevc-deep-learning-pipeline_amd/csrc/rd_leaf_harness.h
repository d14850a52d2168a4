// rd_leaf_harness.h -- TEST-ONLY leaf harness of the decision kernel (lib/libhevcdl_hip_leaf.so; tests/test_rd_leaf_gpu.py; never in the product library).
//
// Included BEHIND rd_kernel.hip by the four translation units rd_leaf.hip / rd_leaf_bd10.hip / rd_leaf_wide.hip / rd_leaf_tools.hip (one per build of the kernel: the build's
// macros, RD_SYM among them, are still defined here), so that the leaf routines of a TU coding and of the intra prediction can be run on blocks of the caller's, every
// intermediate written out, for a word-by-word comparison with the leaf entries of the plain-C restatement the tests keep.  rd_kernel.hip itself is
// compiled as it is, unchanged: its hash keys the committed counter files (profiles/r*_issue.json, r*_traffic.json).  One wave per block / case; a launch is at most
// LEAF_GROUPS workgroups whose waves stride over the blocks.  Every index below is bounded by n, comp, entry, the mode and the counts the host runners check before
// they launch.
//
// The two transform-skip scaling lines of code_tu_block_n (rd_kernel.hip) are inline there and repeated in hevcdl_leaf_tu_kernel: THE TWO PLACES MOVE TOGETHER.
#ifndef HEVCDL_LEAF_TEST
#error "rd_leaf_harness.h is part of the -DHEVCDL_LEAF_TEST build only"
#endif
constexpr int LEAF_GROUPS = 32, LEAF_MAX_BLOCKS = 1 << 16;
struct LeafTuArgs {
  const int16_t *in; const uint8_t *ctx_in;          // [n_blocks][n * n] residual / coefficients / levels (by entry), [n_blocks][160] context bytes
  int16_t *coef, *lvl, *deq, *resi;                  // [n_blocks][n * n] each
  uint32_t *abs_sum; unsigned long long *frac; uint8_t *ctx_out;
  int n_blocks, n, comp, mode, tskip, cbf_ctx, entry, pad_;
};
struct LeafPredArgs {
  const int16_t *lines; const pel_t *org;            // [n_cases][4 n + 1] reference lines, [n_cases][n * n] original blocks (luma)
  int16_t *fline; pel_t *pred; uint32_t *satd;       // [n_cases][4 n + 1] (luma), [n_cases][35][n * n] (n <= 32), [n_cases][35] (luma)
  int n_cases, n, comp, pad_;
};
namespace {
// the context of a wave as hevcdl_micro_kernel sets it up: scratch pointers, tables, K from the launch parameters
DEV void leaf_setup(const hevcdl_rd_params &p)
{
  LSmem &s = lds();
  const int lane = lane_id(), wave = wave_id();
  {
    GLB unsigned char *scr = (GLB unsigned char *)p.scratch + ((size_t)blockIdx.x * NW + wave) * p.scratch_per_wave;
    s.my_coef = (GLB int16_t *)scr; s.my_rec = (GLB pel_t *)(scr + 4 * 6144 * 2); s.my_ovl = s.my_rec + 5 * 6144; s.my_save = (GLB unsigned long long *)(s.my_ovl + 6144);
    s.my_log = s.my_save + N_SAVE * (SAVE_BYTES / 8);
    s.my_qcost = (GLB double *)(scr + SCR_LAYERS); s.my_qrate = (GLB int32_t *)(scr + SCR_LAYERS + 16384);
    s.my_slots = scr + SCR_LAYERS + SCR_RDOQ;
  }
  if (wave == 0) init_tables(wg_shared().tab);
  __syncthreads();
  LDS K &k = s.k;
  if (lane == 0) { s.bound_reg = 0; s.bound_child = -1; }
  k.q_cost = s.my_qcost; k.q_rate = s.my_qrate;
  k.lambda = p.k.lambda; k.sqrt_lambda = p.k.sqrt_lambda; k.cweight = p.k.chroma_weight; k.lambda_c = p.k.lambda_chroma;
  for (int a = 0; a < 2; a++) { for (int b = 0; b < 4; b++) k.err_scale[a][b] = p.k.err_scale[a][b]; k.sbh[a] = p.k.sbh_rd_factor[a]; }
  k.qp = p.k.qp; k.qp_c = p.k.qp_chroma; k.dbg = 0; k.dbgbuf = nullptr; k.tools = p.k.tools;
  wsync();
}
// the copy of rdoq_wave code_tu_block picks for the size (code_tu_block_n<NFIX> calls rdoq_wave<NFIX>, NFIX = the size up to 16x16, 0 above)
DEV uint32_t leaf_rdoq(KR k, const LCabac *cab, int comp, int n, int mode, int cbf_ctx)
{
  if (n == 4) return rdoq_wave<4>(k, cab, comp, n, mode, cbf_ctx);
  if (n == 8) return rdoq_wave<8>(k, cab, comp, n, mode, cbf_ctx);
  if (n == 16) return rdoq_wave<16>(k, cab, comp, n, mode, cbf_ctx);
  return rdoq_wave<0>(k, cab, comp, n, mode, cbf_ctx);
}
} // namespace

extern "C" __global__ __launch_bounds__(NW * 64)
void RD_SYM(hevcdl_leaf_tu_kernel)(hevcdl_rd_params p, LeafTuArgs a)
{
  leaf_setup(p);
  LSmem &s = lds();
  LDS K &k = s.k;
  const int lane = lane_id();
  const int n = uni(a.n), log2n = ilog2(n), nn = n * n, comp = uni(a.comp), mode = uni(a.mode), tskip = uni(a.tskip), cbf_ctx = uni(a.cbf_ctx), entry = uni(a.entry);
  const int n_blocks = uni(a.n_blocks), stride = (int)gridDim.x * NW;
  const int use_rdoq = tools_of(k) & (int)(tskip ? HEVCDL_TOOL_RDOQTS : HEVCDL_TOOL_RDOQ);        // as code_tu_block_n chooses the quantiser
  GLB const int16_t *in = (GLB const int16_t *)a.in; GLB const uint8_t *ctx_in = (GLB const uint8_t *)a.ctx_in;
  GLB int16_t *o_coef = (GLB int16_t *)a.coef, *o_lvl = (GLB int16_t *)a.lvl, *o_deq = (GLB int16_t *)a.deq, *o_resi = (GLB int16_t *)a.resi;
  GLB uint32_t *o_abs = (GLB uint32_t *)a.abs_sum; GLB unsigned long long *o_frac = (GLB unsigned long long *)a.frac; GLB uint8_t *o_ctx = (GLB uint8_t *)a.ctx_out;
#pragma unroll 1
  for (int b = (int)blockIdx.x * NW + wave_id(); b < n_blocks; b += stride) {
    const size_t bo = (size_t)b * nn;
    wsync();
    for (int i = lane; i < 160; i += 64) s.go.ctx[i] = i < NUM_CTX ? ctx_in[(size_t)b * 160 + i] : (uint8_t)0;
    if (lane == 0) s.go.frac = 0;
    if (entry == 0) { for (int i = lane; i < nn; i += 64) s.resi[(i >> log2n) * RS(n) + (i & (n - 1))] = in[bo + i]; }
    else if (entry == 1) { for (int i = lane; i < nn; i += 64) s.tc[i] = in[bo + i]; }
    else { for (int i = lane; i < nn; i += 64) s.lvl[i] = in[bo + i]; }
    wsync();
    if (entry == 0) {
      // (the transform-skip scaling of code_tu_block_n, inline there: the two places move together)
      if (tskip) { for (int i = lane; i < nn; i += 64) s.tc[i] = (int16_t)((int)s.resi[(i >> log2n) * RS(n) + (i & (n - 1))] << (13 - BD)); wsync(); }   // n == 4: one pass, every lane reads before any writes
      else fwd_transform(k, n, !comp && n == 4);
    }
    for (int i = lane; i < nn; i += 64) o_coef[bo + i] = entry <= 1 ? s.tc[i] : (int16_t)0;
    wsync();
    uint32_t abs_sum;
    if (entry <= 1) {
      if (use_rdoq) abs_sum = leaf_rdoq(k, &s.go, comp, n, mode, cbf_ctx);
      else abs_sum = plain_quant_wave(k, comp, n, mode);
      wsync();
    } else {
      int v = 0;
      for (int i = lane; i < nn; i += 64) v += abs((int)s.lvl[i]);
      abs_sum = (uint32_t)wave_sum_i(v);
    }
    const bool coded = entry == 2 || abs_sum > 0;
    for (int i = lane; i < nn; i += 64) o_lvl[bo + i] = coded ? s.lvl[i] : (int16_t)0;
    wsync();
    if (entry <= 1 && abs_sum > 0) code_coeff_wave(k, &s.go, comp, n, mode, tskip);
    wsync();
    for (int i = lane; i < 160; i += 64) o_ctx[(size_t)b * 160 + i] = s.go.ctx[i];
    if (lane == 0) { o_frac[b] = s.go.frac; o_abs[b] = abs_sum; }
    if (coded) {
      dequant(k, comp, n);
      for (int i = lane; i < nn; i += 64) o_deq[bo + i] = s.tc[i];
      wsync();
      // (the inverse of the transform-skip scaling, inline in code_tu_block_n: moves together with it)
      if (tskip) { for (int i = lane; i < nn; i += 64) s.resi[(i >> log2n) * RS(n) + (i & (n - 1))] = (int16_t)((s.tc[i] + (1 << (12 - BD))) >> (13 - BD)); wsync(); }
      else inv_transform(k, n, !comp && n == 4);
      for (int i = lane; i < nn; i += 64) o_resi[bo + i] = s.resi[(i >> log2n) * RS(n) + (i & (n - 1))];
    } else {
      for (int i = lane; i < nn; i += 64) { o_deq[bo + i] = 0; o_resi[bo + i] = 0; }
    }
    wsync();
  }
}

extern "C" __global__ __launch_bounds__(NW * 64)
void RD_SYM(hevcdl_leaf_pred_kernel)(hevcdl_rd_params p, LeafPredArgs a)
{
  leaf_setup(p);
  LSmem &s = lds();
  LDS K &k = s.k;
  const int lane = lane_id();
  const int n = uni(a.n), nn = n * n, len = 4 * n + 1, comp = uni(a.comp), n_cases = uni(a.n_cases), stride = (int)gridDim.x * NW;
  GLB const int16_t *lines = (GLB const int16_t *)a.lines; GLB const pel_t *org = (GLB const pel_t *)a.org;
  GLB int16_t *o_fline = (GLB int16_t *)a.fline; GLB pel_t *o_pred = (GLB pel_t *)a.pred; GLB uint32_t *o_satd = (GLB uint32_t *)a.satd;
#pragma unroll 1
  for (int cs = (int)blockIdx.x * NW + wave_id(); cs < n_cases; cs += stride) {
    wsync();
    LDS int16_t *line = ref_line(comp);
    for (int i = lane; i < len; i += 64) line[i] = lines[(size_t)cs * len + i];
    if (lane == 0) { s.ref_key[comp] = cs + 1; if (!comp) s.fline_key = -1; }          // (filter_refs keeps a line it has filtered: a new key per case)
    wsync();
    if (!comp) {
      filter_refs(k, n);
      for (int i = lane; i < len; i += 64) o_fline[(size_t)cs * len + i] = s.fline[i];
      wsync();
    }
    if (n <= 32) {                                   // predict_block's range (a 64x64 PU is only ever predicted by rmd_block)
#pragma unroll 1
      for (int mode = 0; mode < 35; mode++) {
        predict_block(k, comp, mode, n);
        for (int i = lane; i < nn; i += 64) o_pred[((size_t)cs * 35 + mode) * nn + i] = s.pred[i];
        wsync();
      }
    }
    if (!comp) { // the rough mode decision as rmd_satd runs it without helpers: one wave, all rounds
      if (lane < 36) s.satd[lane] = 0;
      if (lane == 0) { k.org[0] = org + (size_t)cs * nn; k.W = n; }
      wsync();
      const int dcv = dc_value(k, s.line, n);
      wsync();
      const int nbx = n >> (n >= 8 ? 3 : 2), nrounds = (35 * nbx * nbx + 63) >> 6;
      rmd_rounds(k, s.satd, 0, 0, n, dcv, 0, nrounds);
      if (lane < 35) o_satd[(size_t)cs * 35 + lane] = s.satd[lane] >> HAD_SH;
      wsync();
    }
  }
}

namespace {
unsigned char *g_leaf_scratch = nullptr;          // LEAF_GROUPS * NW waves' workspace, kept for the life of the (test) process
int leaf_params(hevcdl_rd_params &p, const double *consts, const long long *sbh, int qp, int qp_c, int tools)
{
  if (!consts || !sbh || qp < 0 || qp > 51 || qp_c < 0 || qp_c > 51) return -1;
  p.k.lambda = consts[0]; p.k.sqrt_lambda = consts[1]; p.k.chroma_weight = consts[2]; p.k.lambda_chroma = consts[3];
  for (int a = 0; a < 2; a++) for (int b = 0; b < 4; b++) p.k.err_scale[a][b] = consts[4 + 4 * a + b];
  p.k.sbh_rd_factor[0] = sbh[0]; p.k.sbh_rd_factor[1] = sbh[1]; p.k.qp = qp; p.k.qp_chroma = qp_c; p.k.tools = tools & 0x7f;
  p.scratch_per_wave = SCR_WAVE;
  if (!g_leaf_scratch && hipMalloc(&g_leaf_scratch, (size_t)LEAF_GROUPS * NW * SCR_WAVE) != hipSuccess) { g_leaf_scratch = nullptr; return -2; }
  p.scratch = g_leaf_scratch;
  return 0;
}
} // namespace

extern "C" void RD_SYM(hevcdl_leaf_info)(int *bit_depth, int *waves, int *tools_rt) { *bit_depth = BD; *waves = NW; *tools_rt = HEVCDL_TOOLS_RT ? 1 : 0; }

// host side.  consts = { lambda, sqrt_lambda, chroma_weight, lambda_chroma, err_scale[2][4] }, sbh[2] (hevcdl_config's values for the QP).  Returns 0, -1 for an
// argument outside what the kernels index with (nothing is launched), -2 out of memory, -3 a HIP error.
extern "C" int RD_SYM(hevcdl_leaf_tu_run)(const double *consts, const long long *sbh, int qp, int qp_c, int tools, int comp, int n, int mode, int tskip, int cbf_ctx, int entry,
                                          int n_blocks, const int16_t *in, const uint8_t *ctx_in, int16_t *coef, int16_t *lvl, uint32_t *abs_sum, unsigned long long *frac,
                                          uint8_t *ctx_out, int16_t *deq, int16_t *resi)
{
  if (comp < 0 || comp > 2 || (n != 4 && n != 8 && n != 16 && n != 32) || (comp && n > 16)) return -1;          // a chroma TU is at most 16 wide
  if (mode < 0 || mode > 34 || (tskip != 0 && tskip != 1) || (tskip && n != 4) || cbf_ctx < 0 || cbf_ctx > 4 || entry < 0 || entry > 2) return -1;
  if (n_blocks < 1 || n_blocks > LEAF_MAX_BLOCKS || !in || !ctx_in || !coef || !lvl || !abs_sum || !frac || !ctx_out || !deq || !resi) return -1;
  for (size_t i = 0; i < (size_t)n_blocks * 160; i++) if (ctx_in[i] > 125 || (i % 160 == 159 && ctx_in[i])) return -1;      // a context state indexes the 128-entry rate / transition tables
  hevcdl_rd_params p = {};
  const int rc = leaf_params(p, consts, sbh, qp, qp_c, tools);
  if (rc) return rc;
  const size_t nb = (size_t)n_blocks, blk = nb * n * n * 2, o_ctx = 5 * blk, o_abs = o_ctx + 2 * nb * 160, o_frac = (o_abs + nb * 4 + 7) & ~(size_t)7, total = o_frac + nb * 8;
  unsigned char *d = nullptr;
  if (hipMalloc(&d, total) != hipSuccess) return -2;
  LeafTuArgs a = {};
  a.in = (const int16_t *)d; a.coef = (int16_t *)(d + blk); a.lvl = (int16_t *)(d + 2 * blk); a.deq = (int16_t *)(d + 3 * blk); a.resi = (int16_t *)(d + 4 * blk);
  a.ctx_in = d + o_ctx; a.ctx_out = d + o_ctx + nb * 160; a.abs_sum = (uint32_t *)(d + o_abs); a.frac = (unsigned long long *)(d + o_frac);
  a.n_blocks = n_blocks; a.n = n; a.comp = comp; a.mode = mode; a.tskip = tskip; a.cbf_ctx = cbf_ctx; a.entry = entry;
  bool ok = hipMemcpy(d, in, blk, hipMemcpyHostToDevice) == hipSuccess && hipMemcpy(d + o_ctx, ctx_in, nb * 160, hipMemcpyHostToDevice) == hipSuccess;
  if (ok) {
    const size_t smem = (size_t)NW * sizeof(RdSmem) + sizeof(WgShared);
    const int groups = (n_blocks + NW - 1) / NW < LEAF_GROUPS ? (n_blocks + NW - 1) / NW : LEAF_GROUPS;
    ok = hipFuncSetAttribute((const void *)RD_SYM(hevcdl_leaf_tu_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem) == hipSuccess;
    if (ok) {
      hipLaunchKernelGGL(RD_SYM(hevcdl_leaf_tu_kernel), dim3(groups), dim3(NW * 64), smem, 0, p, a);
      ok = hipGetLastError() == hipSuccess && hipDeviceSynchronize() == hipSuccess;
    }
  }
  ok = ok && hipMemcpy(coef, a.coef, blk, hipMemcpyDeviceToHost) == hipSuccess && hipMemcpy(lvl, a.lvl, blk, hipMemcpyDeviceToHost) == hipSuccess
          && hipMemcpy(deq, a.deq, blk, hipMemcpyDeviceToHost) == hipSuccess && hipMemcpy(resi, a.resi, blk, hipMemcpyDeviceToHost) == hipSuccess
          && hipMemcpy(ctx_out, a.ctx_out, nb * 160, hipMemcpyDeviceToHost) == hipSuccess && hipMemcpy(abs_sum, a.abs_sum, nb * 4, hipMemcpyDeviceToHost) == hipSuccess
          && hipMemcpy(frac, a.frac, nb * 8, hipMemcpyDeviceToHost) == hipSuccess;
  hipFree(d);
  return ok ? 0 : -3;
}

// lines [n_cases][4 n + 1] and org [n_cases][n * n] (luma) hold samples of the build's bit depth as 16-bit values; fline (luma), pred (n <= 32) and satd (luma) as LeafPredArgs
extern "C" int RD_SYM(hevcdl_leaf_pred_run)(int tools, int comp, int n, int n_cases, const int16_t *lines, const uint16_t *org, int16_t *fline, uint16_t *pred, uint32_t *satd)
{
  if (comp < 0 || comp > 2 || (n != 4 && n != 8 && n != 16 && n != 32 && !(n == 64 && !comp)) || (comp && n > 16)) return -1;
  if (n_cases < 1 || n_cases > LEAF_MAX_BLOCKS || !lines || (!comp && (!org || !fline || !satd)) || (n <= 32 && !pred)) return -1;
  const size_t nc = (size_t)n_cases, len = 4 * (size_t)n + 1, nn = (size_t)n * n;
  for (size_t i = 0; i < nc * len; i++) if (lines[i] < 0 || lines[i] > PEL_MAX) return -1;
  if (!comp) for (size_t i = 0; i < nc * nn; i++) if (org[i] > PEL_MAX) return -1;
  hevcdl_rd_params p = {};
  const double consts[12] = { 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1 }; const long long sbh[2] = { 0, 0 };          // (no routine of this harness reads the lambda family)
  const int rc = leaf_params(p, consts, sbh, 32, 32, tools);
  if (rc) return rc;
  const size_t b_line = (nc * len * 2 + 15) & ~(size_t)15, b_org = (nc * nn * sizeof(pel_t) + 15) & ~(size_t)15, b_pred = n <= 32 ? (nc * 35 * nn * sizeof(pel_t) + 15) & ~(size_t)15 : 0;
  const size_t o_org = b_line, o_fline = o_org + b_org, o_pred = o_fline + b_line, o_satd = o_pred + b_pred, total = o_satd + nc * 35 * 4;
  unsigned char *d = nullptr;
  if (hipMalloc(&d, total) != hipSuccess) return -2;
  pel_t *h = (pel_t *)malloc(b_org > b_pred ? b_org : b_pred);
  if (!h) { hipFree(d); return -2; }
  LeafPredArgs a = {};
  a.lines = (const int16_t *)d; a.org = (const pel_t *)(d + o_org); a.fline = (int16_t *)(d + o_fline); a.pred = (pel_t *)(d + o_pred); a.satd = (uint32_t *)(d + o_satd);
  a.n_cases = n_cases; a.n = n; a.comp = comp;
  bool ok = hipMemcpy(d, lines, nc * len * 2, hipMemcpyHostToDevice) == hipSuccess;
  if (ok && !comp) { for (size_t i = 0; i < nc * nn; i++) h[i] = (pel_t)org[i]; ok = hipMemcpy(d + o_org, h, nc * nn * sizeof(pel_t), hipMemcpyHostToDevice) == hipSuccess; }
  if (ok) {
    const size_t smem = (size_t)NW * sizeof(RdSmem) + sizeof(WgShared);
    const int groups = (n_cases + NW - 1) / NW < LEAF_GROUPS ? (n_cases + NW - 1) / NW : LEAF_GROUPS;
    ok = hipFuncSetAttribute((const void *)RD_SYM(hevcdl_leaf_pred_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem) == hipSuccess;
    if (ok) {
      hipLaunchKernelGGL(RD_SYM(hevcdl_leaf_pred_kernel), dim3(groups), dim3(NW * 64), smem, 0, p, a);
      ok = hipGetLastError() == hipSuccess && hipDeviceSynchronize() == hipSuccess;
    }
  }
  if (ok && !comp) ok = hipMemcpy(fline, a.fline, nc * len * 2, hipMemcpyDeviceToHost) == hipSuccess && hipMemcpy(satd, a.satd, nc * 35 * 4, hipMemcpyDeviceToHost) == hipSuccess;
  if (ok && n <= 32) {
    ok = hipMemcpy(h, a.pred, nc * 35 * nn * sizeof(pel_t), hipMemcpyDeviceToHost) == hipSuccess;
    if (ok) for (size_t i = 0; i < nc * 35 * nn; i++) pred[i] = (uint16_t)h[i];
  }
  free(h); hipFree(d);
  return ok ? 0 : -3;
}
