// slice_decode_kernel.hip -- the slice data of I pictures DECODED on the device (gfx950): slice_decode_core.h instantiated for one wave per unit.
//
// hevcdl_slice_decode_kernel: a wave takes one unit (picture x tile, picture x row slice, or picture: slice_decode_core.h) and runs the shared decoder over its CTUs:
// the arithmetic decoder over the unit's sub-streams in the batch's RBSP blob, records and SAO blocks written into HBM where hevcdl_recon_kernel, the in-loop filters and
// the report kernels read them.  Control flow is wave-uniform, as in hevcdl_entropy_kernel: every lane computes the same decoder (the wave index is made uniform, so the
// compiler keeps the state in scalar registers where it can); the context bytes, the saved wavefront contexts, the coefficient group in work and the launch's stream
// parameters live in the wave's own LDS.  Stores are spread over the lanes where there is a run to spread: the clearing of a CTU's record (16 bytes a lane), the levels of
// a coefficient group (a level a lane), runs of depth, part_size, luma_dir, chroma_dir, tr_idx and cbf (a partition a lane); a single value is stored by lane 0.
//
// depth and luma_dir are read back from the records -- split contexts and candidate modes -- behind the wave's own stores, other lanes' among them.  The records pointer is
// neither const nor restrict, so those reads are vector loads behind the wave's vector stores in program order; a read-only restrict pointer would invite the scalar
// cache, which does not see them.  The RBSP bytes, the tables and the unit table are only ever read.
//
// No wave waits for another: no spin loop, no flag another wave sets, no cooperative launch, no barrier.  The rows of a wavefront picture are decoded one after the other
// by the picture's one wave.
//
// Safety: plain C++; every loop of slice_decode_core.h has a bound that does not depend on stream contents, every value that addresses memory is checked where it is
// read, the bit reader knows the end of its sub-stream, a unit's rectangle, sub-streams and bytes are checked against the picture, the table and the blob before the
// first CTU.  A wave writes the records and SAO blocks of its unit's CTUs and its own result slot, nothing else.
#include <hip/hip_runtime.h>
#include <atomic>
#include <stdint.h>
#include "hevcdl.h"
#include "hevcdl_dev.h"
#define HEVCDL_SD_LANES 1
#define EC_FN __device__ inline
#define SD_FN __device__ inline
#include "slice_decode_units.h"

using namespace hevcdl_sd;

namespace {
constexpr int SD_WAVES = 4;                  // waves (= units) per workgroup
struct WaveLds { uint8_t ctx[EC_SYNC_BYTES], sync[EC_SYNC_BYTES]; uint16_t cg_pos[16]; int16_t cg_val[16]; uint8_t dry_depth[512], dry_dir[512]; int8_t qp_cur[256]; SdStream sd; };
std::atomic<unsigned long long> g_launches{ 0 };
__device__ inline int sd_lane() { return (int)(threadIdx.x & 63u); }
}

__device__ void hevcdl_sd::sd_fill8(uint8_t *p, int n, int v) { for (int i = sd_lane(); i < n; i += 64) p[i] = (uint8_t)v; }
__device__ void hevcdl_sd::sd_or8(uint8_t *p, int n, int v) { for (int i = sd_lane(); i < n; i += 64) p[i] |= (uint8_t)v; }
__device__ void hevcdl_sd::sd_clear32(void *p, int dwords)
{
  if (((uintptr_t)p & 15) == 0 && (dwords & 3) == 0) { uint4 *q = (uint4 *)p; for (int i = sd_lane(); i < (dwords >> 2); i += 64) q[i] = make_uint4(0, 0, 0, 0); }
  else { uint32_t *q = (uint32_t *)p; for (int i = sd_lane(); i < dwords; i += 64) q[i] = 0; }
}
__device__ void hevcdl_sd::sd_put8(uint8_t *p, int v) { if (sd_lane() == 0) *p = (uint8_t)v; }
__device__ void hevcdl_sd::sd_put32(int32_t *p, int v) { if (sd_lane() == 0) *p = v; }
__device__ void hevcdl_sd::sd_put_levels(int16_t *coef, const uint16_t *pos, const int16_t *val, int n) { const int l = sd_lane(); if (l < n && l < 16) coef[pos[l]] = val[l]; }

extern "C" __global__ __launch_bounds__(SD_WAVES * 64) void hevcdl_slice_decode_kernel(hevcdl_slice_decode_params p)
{
  __shared__ __attribute__((aligned(16))) WaveLds lds[SD_WAVES];
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const long long i = (long long)blockIdx.x * SD_WAVES + wave;
  if (i >= p.n_units) return;
  WaveLds &l = lds[wave];
  const SdUnit u = p.units[i];
  SdResult res = { SD_E_UNIT, -1 };
  if ((unsigned)u.pic < (unsigned)p.n_pics) {
    l.sd = p.sd;                                                        // (every lane writes the same words: nothing a lane reads from LDS was written by another lane alone)
    SdState s;
    s.t = (const EcTables *)p.tables; s.s = &l.sd; s.ctx = l.ctx; s.sync = l.sync; s.cg_pos = l.cg_pos; s.cg_val = l.cg_val; s.dry_depth = l.dry_depth; s.dry_dir = l.dry_dir;
    s.recs = (hevcdl_ctu_record *)p.records + (size_t)u.pic * p.ctus;
    s.sao = p.sao ? (hevcdl_sao_blk *)p.sao + (size_t)u.pic * p.ctus : nullptr;
    s.qp_cur = l.qp_cur; s.qp_map = p.qp_map ? p.qp_map + (size_t)u.pic * p.ctus * 256 : nullptr;      // the map: written across the lanes like depth (sd_fill8)
    s.slice_qp = s.last_qp = s.qg_pred = s.is_coded = s.delta_val = 0;
    s.cx0 = s.cx1 = s.cy0 = s.cy1 = s.cur_cx = s.cur_cy = s.dry = 0; s.d = p.blob; s.size = s.pos = 0; s.win = 0; s.nwin = 0; s.last = 0; s.range = 510; s.offset = 0; s.bad = s.err = 0;
    res = sd_decode_unit(s, u, p.subs, p.n_subs, p.blob, p.blob_bytes);
  }
  if (sd_lane() == 0) p.results[i] = res;
}

int hevcdl_launch_slice_decode(const hevcdl_slice_decode_params *p, void *stream)
{
  if (!p || p->n_units <= 0 || p->n_subs <= 0 || p->n_pics <= 0 || !p->blob || !p->subs || !p->units || !p->records || !p->results || !p->tables) return 0;
  if (p->sd.ctus_x < 1 || p->sd.ctus_y < 1 || (long long)p->sd.ctus_x * p->sd.ctus_y != p->ctus || ((uintptr_t)p->records & 15)) return 0;
  if ((p->sd.cu_qp && (!p->qp_map || p->sd.log2_qg < 3 || p->sd.log2_qg > 6)) || ((uintptr_t)p->qp_map & 3)) return 0;
  hipLaunchKernelGGL(hevcdl_slice_decode_kernel, dim3((unsigned)((p->n_units + SD_WAVES - 1) / SD_WAVES)), dim3(SD_WAVES * 64), 0, (hipStream_t)stream, *p);
  g_launches++;
  return 1;
}

extern "C" unsigned long long hevcdl_slice_decode_launches(void) { return g_launches.load(); }

int hevcdl_slice_decode_first_error(const std::vector<SdUnit> &units, const SdResult *results, SdResult *res)
{
  for (size_t i = 0; i < units.size(); i++) if (results[i].code != SD_OK) { *res = results[i]; return units[i].pic; }      // units are in picture order, and in the parser's order inside a picture
  return -1;
}

// ---- hevcdl_parse_stream_dev: hevcdl_parse_stream's contract, the slice data through the kernel (TEST AND DIAGNOSTIC: host buffers in and out) ---------------------------
namespace {
struct DevMem { void *p = nullptr; ~DevMem() { if (p) (void)hipFree(p); } hipError_t get(size_t n) { return hipMalloc(&p, n ? n : 4); } };
#define SD_HIP(call) do { if ((call) != hipSuccess) { (void)hipGetLastError(); hevcdl_parse::set_error("hevcdl_parse_stream_dev: %s failed", #call); return HEVCDL_ERR_HIP; } } while (0)

hevcdl_status walk_units_dev(void *user, const hevcdl_parse::StreamUnits &su, int n, hevcdl_ctu_record *records, hevcdl_sao_blk *sao, int8_t *qp_map, int *bad_pic, SdResult *res)
{
  const int device = *(const int *)user;
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) != hipSuccess || device < 0 || device >= n_dev) { (void)hipGetLastError(); hevcdl_parse::set_error("hevcdl_parse_stream_dev: no such device"); return HEVCDL_ERR_NO_DEVICE; }
  SD_HIP(hipSetDevice(device));
  *bad_pic = -1;
  const size_t rec_b = sizeof(hevcdl_ctu_record) * (size_t)su.ctus, sao_b = sizeof(hevcdl_sao_blk) * (size_t)su.ctus;
  const int per = (int)std::max<size_t>(1, ((size_t)1 << 30) / rec_b);      // pictures a launch: a GB of records
  DevMem d_tables;
  SD_HIP(d_tables.get(sizeof(EcTables)));
  SD_HIP(hipMemcpy(d_tables.p, &ec_tables(), sizeof(EcTables), hipMemcpyHostToDevice));
  for (int first = 0; first < n; first += per) {
    const int cnt = std::min(per, n - first);
    std::vector<SdUnit> units; size_t sub0, n_subs, byte0, n_bytes;
    const hevcdl_status st = hevcdl_parse::batch_tables(su, first, cnt, units, sub0, n_subs, byte0, n_bytes);
    if (st != HEVCDL_OK) return st;
    DevMem d_blob, d_subs, d_units, d_res, d_rec, d_sao, d_map;
    const size_t map_b = (size_t)su.ctus * 256;
    if (qp_map) SD_HIP(d_map.get(map_b * cnt));
    SD_HIP(d_blob.get(n_bytes)); SD_HIP(d_subs.get(n_subs * sizeof(SdSub))); SD_HIP(d_units.get(units.size() * sizeof(SdUnit))); SD_HIP(d_res.get(units.size() * sizeof(SdResult)));
    SD_HIP(d_rec.get(rec_b * cnt));
    if (sao) SD_HIP(d_sao.get(sao_b * cnt));
    if (n_bytes) SD_HIP(hipMemcpy(d_blob.p, su.rbsp.data() + byte0, n_bytes, hipMemcpyHostToDevice));
    SD_HIP(hipMemcpy(d_subs.p, su.subs.data() + sub0, n_subs * sizeof(SdSub), hipMemcpyHostToDevice));
    SD_HIP(hipMemcpy(d_units.p, units.data(), units.size() * sizeof(SdUnit), hipMemcpyHostToDevice));
    hevcdl_slice_decode_params k;
    k.sd = su.sd; k.blob = (const uint8_t *)d_blob.p; k.blob_bytes = n_bytes; k.subs = (const SdSub *)d_subs.p; k.units = (const SdUnit *)d_units.p; k.n_subs = (int)n_subs; k.n_units = (int)units.size();
    k.records = d_rec.p; k.sao = d_sao.p; k.ctus = su.ctus; k.n_pics = cnt; k.results = (SdResult *)d_res.p; k.tables = d_tables.p; k.qp_map = (int8_t *)d_map.p;
    if (!hevcdl_launch_slice_decode(&k, nullptr)) { hevcdl_parse::set_error("hevcdl_parse_stream_dev: the unit tables of pictures %d .. %d do not fit a launch", first, first + cnt - 1); return HEVCDL_ERR_INVALID_ARG; }
    SD_HIP(hipGetLastError());
    std::vector<SdResult> results(units.size());
    SD_HIP(hipMemcpy(results.data(), d_res.p, units.size() * sizeof(SdResult), hipMemcpyDeviceToHost));
    const int bad = hevcdl_slice_decode_first_error(units, results.data(), res);
    if (bad >= 0) { *bad_pic = first + bad; return HEVCDL_OK; }
    SD_HIP(hipMemcpy(records + (size_t)first * su.ctus, d_rec.p, rec_b * cnt, hipMemcpyDeviceToHost));
    if (sao) SD_HIP(hipMemcpy(sao + (size_t)first * su.ctus, d_sao.p, sao_b * cnt, hipMemcpyDeviceToHost));
    if (qp_map) SD_HIP(hipMemcpy(qp_map + (size_t)first * map_b, d_map.p, map_b * cnt, hipMemcpyDeviceToHost));
  }
  return HEVCDL_OK;
}
} // namespace

extern "C" hevcdl_status hevcdl_parse_stream_dev(int device, const uint8_t *stream, size_t bytes, hevcdl_stream_config *cfg, hevcdl_slice_layout *slices, hevcdl_segment_layout *segments,
                                                hevcdl_parsed_picture *pictures, int picture_capacity, int *n_pictures, hevcdl_ctu_record *records, hevcdl_sao_blk *sao,
                                                size_t ctu_capacity)
{
  return hevcdl_parse::parse_stream_with(walk_units_dev, &device, stream, bytes, cfg, slices, segments, pictures, picture_capacity, n_pictures, records, sao, ctu_capacity);
}

extern "C" hevcdl_status hevcdl_parse_stream_dev_qp(int device, const uint8_t *stream, size_t bytes, unsigned accept, hevcdl_stream_config *cfg, hevcdl_slice_layout *slices,
                                                   hevcdl_segment_layout *segments, hevcdl_parsed_picture *pictures, int picture_capacity, int *n_pictures, hevcdl_ctu_record *records,
                                                   hevcdl_sao_blk *sao, size_t ctu_capacity, hevcdl_qp_info *qp_info, int8_t *qp_map)
{
  return hevcdl_parse::parse_stream_with(walk_units_dev, &device, stream, bytes, cfg, slices, segments, pictures, picture_capacity, n_pictures, records, sao, ctu_capacity, accept, qp_info, qp_map);
}

extern "C" hevcdl_status hevcdl_parse_stream_dev_sl(int device, const uint8_t *stream, size_t bytes, unsigned accept, hevcdl_stream_config *cfg, hevcdl_slice_layout *slices,
                                                   hevcdl_segment_layout *segments, hevcdl_parsed_picture *pictures, int picture_capacity, int *n_pictures, hevcdl_ctu_record *records,
                                                   hevcdl_sao_blk *sao, size_t ctu_capacity, hevcdl_qp_info *qp_info, int8_t *qp_map, hevcdl_scaling_info *scaling)
{
  return hevcdl_parse::parse_stream_with(walk_units_dev, &device, stream, bytes, cfg, slices, segments, pictures, picture_capacity, n_pictures, records, sao, ctu_capacity, accept, qp_info, qp_map, scaling);
}
