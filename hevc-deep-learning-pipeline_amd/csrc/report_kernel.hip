// report_kernel.hip -- the decoded-picture hash of pictures that are in HBM, for gfx950 (MI355X): the digests of SEIDecodedPictureHash 1 / 2 / 3.
//
// Replaces the host's hevcdl_picture_hash (hevcdl_bitstream.cpp; the reference: TComPicYuvMD5.cpp:88-180) for the picture pipeline's output pictures, so that a run
// that writes a hash SEI does not download its pictures.  The arithmetic is csrc/picture_hash_core.h, the source the host compiles too; everything is exact.
//
// Kernels (plain launches on one stream, in order; no cooperative launch, no flag another wave sets, no atomics; every loop bound is a launch parameter):
//   hevcdl_report_partial_kernel<PEL>   CRC and checksum.  Grid (chunks, planes, pictures), 256 lanes: a workgroup reduces one chunk of chunk_bytes bytes of a plane to
//                                       one 32-bit partial.  A lane reads pieces of 16 bytes (one dwordx4 where the address allows, bytes otherwise -- planes of odd
//                                       sizes, the short piece at the front); pieces are counted from the END of the chunk, piece j = the 16 bytes in front of the last
//                                       16 j: then exactly 128 j bits lie behind it.  Lane t takes pieces t, t + 256, ...: neighbouring lanes read neighbouring 16 bytes.
//                                       CRC: the lane's pieces by Horner's rule over x^(128 * 256), times x^(128 t), xor over the lanes.  Checksum: a sum.
//   hevcdl_report_md5_kernel<PEL>       MD5.  One lane per (picture, plane) chain; the 64 lanes of a wave hold the same plane of consecutive pictures, so the chains
//                                       are equally long and the wave does not diverge.  State: four registers; the message block: sixteen registers read straight from
//                                       the plane (four dwordx4), the next block requested before the current block's 64 steps.
//   hevcdl_report_finish_kernel         one thread per (picture, plane): folds the partials in chunk order (picture_hash_core.h crc_fold / a sum), writes the digest
//                                       bytes, copies the plane's SSE from the SSE launch's output, fills method / plane_bytes.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "hevcdl.h"
#include "hevcdl_dev.h"
#include "picture_hash_core.h"

namespace {

using namespace hevcdl_ph;

enum { REPORT_LANES = 256 };

// byte i (0 .. 15) of a piece held in four registers
__device__ __forceinline__ uint32_t piece_byte(const uint32_t w[4], int i) { return (w[i >> 2] >> (8 * (i & 3))) & 0xff; }

template <typename PEL> __global__ __launch_bounds__(REPORT_LANES) void hevcdl_report_partial_kernel(hevcdl_report_params p)
{
  const int chunk = blockIdx.x, plane = blockIdx.y, pic = blockIdx.z, tid = threadIdx.x;
  const uint32_t width = (uint32_t)p.plane_w[plane];
  const uint64_t n = (uint64_t)width * (uint32_t)p.plane_h[plane] * sizeof(PEL), at = (uint64_t)chunk * (uint32_t)p.chunk_bytes;
  if (at >= n) return;                                                   // (the whole workgroup: the grid is sized by the largest plane)
  const uint32_t len = n - at < (uint64_t)p.chunk_bytes ? (uint32_t)(n - at) : (uint32_t)p.chunk_bytes;
  const uint8_t *c = (const uint8_t *)p.pic + (size_t)pic * p.frame_bytes + p.plane_off[plane] + at;      // the chunk's first byte; [c, c + len) lies inside the plane
  const int pieces = (int)((len + PH_PIECE - 1) / PH_PIECE), rounds = (p.chunk_bytes / PH_PIECE + REPORT_LANES - 1) / REPORT_LANES;
  const bool crc = p.method == 2;
  const uint32_t xs = crc ? crc_xpow((uint64_t)8 * PH_PIECE * REPORT_LANES) : 0;
  uint32_t acc = 0;
  for (int r = rounds - 1; r >= 0; r--) {                                // the pieces furthest from the chunk's end first
    const int j = tid + REPORT_LANES * r;
    uint32_t part = 0;
    if (j < pieces) {
      const int hi = (int)len - PH_PIECE * j, lo = hi > PH_PIECE ? hi - PH_PIECE : 0, cnt = hi - lo;      // bytes [lo, hi) of the chunk
      const uint8_t *q = c + lo;
      uint32_t w[4] = { 0, 0, 0, 0 };
      if (cnt == PH_PIECE && ((uintptr_t)q & 15) == 0) { const uint4 v = *(const uint4 *)q; w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w; }
      else {
#pragma unroll
        for (int i = 0; i < PH_PIECE; i++) if (i < cnt) w[i >> 2] |= (uint32_t)q[i] << (8 * (i & 3));
      }
      if (crc) {
#pragma unroll
        for (int i = 0; i < PH_PIECE; i++) if (i < cnt) part = crc_feed(part, piece_byte(w, i));
      } else {
        const uint64_t g = at + (uint32_t)lo, s = g / sizeof(PEL);       // the piece's first byte in the plane, its sample
        uint32_t y = (uint32_t)(s / width), x = (uint32_t)(s - (uint64_t)y * width), sub = (uint32_t)(g - s * sizeof(PEL));
#pragma unroll
        for (int i = 0; i < PH_PIECE; i++) if (i < cnt) {
          part += (piece_byte(w, i) ^ checksum_mask(x, y)) & 0xff;
          if (++sub == sizeof(PEL)) { sub = 0; if (++x == width) { x = 0; y++; } }
        }
      }
    }
    acc = crc ? (crc_mulmod(acc, xs) ^ part) : acc + part;
  }
  if (crc) acc = crc_mulmod(acc, crc_xpow((uint64_t)8 * PH_PIECE * tid));      // 128 tid bits lie behind the lane's last piece
  __shared__ uint32_t red[REPORT_LANES];
  red[tid] = acc;
  __syncthreads();
  for (int s = REPORT_LANES / 2; s > 0; s >>= 1) { if (tid < s) red[tid] = crc ? (red[tid] ^ red[tid + s]) : red[tid] + red[tid + s]; __syncthreads(); }
  if (tid == 0) p.partials[((size_t)pic * 3 + plane) * p.chunk_stride + chunk] = red[0];
}

__device__ __forceinline__ void load_block(const uint8_t *q, bool aligned, uint32_t w[16])
{
  if (aligned) {
#pragma unroll
    for (int i = 0; i < 4; i++) { const uint4 v = ((const uint4 *)q)[i]; w[4 * i] = v.x; w[4 * i + 1] = v.y; w[4 * i + 2] = v.z; w[4 * i + 3] = v.w; }
  } else md5_words(q, w);
}

// grid (pictures / 64, planes), 64 lanes: lane = picture
template <typename PEL> __global__ __launch_bounds__(64) void hevcdl_report_md5_kernel(hevcdl_report_params p)
{
  const int plane = blockIdx.y, pic = blockIdx.x * 64 + threadIdx.x;
  if (pic >= p.n_pics) return;
  const uint64_t n = (uint64_t)(uint32_t)p.plane_w[plane] * (uint32_t)p.plane_h[plane] * sizeof(PEL), whole = n / 64;
  const uint8_t *base = (const uint8_t *)p.pic + (size_t)pic * p.frame_bytes + p.plane_off[plane];
  const bool aligned = ((uintptr_t)base & 15) == 0;                       // a context's planes are; a test plane of any size starts on an allocation
  Md5State s; md5_init(&s);
  uint32_t cur[16], nxt[16] = { 0 };
  if (whole) load_block(base, aligned, cur);
  for (uint64_t b = 0; b < whole; b++) {
    if (b + 1 < whole) load_block(base + 64 * (b + 1), aligned, nxt);    // in flight during the 64 steps below
    md5_block(&s, cur);
#pragma unroll
    for (int i = 0; i < 16; i++) cur[i] = nxt[i];
  }
  uint8_t dg[16];
  md5_tail(&s, base + 64 * whole, (int)(n - 64 * whole), n, dg);
  uint8_t *rec = (uint8_t *)p.out + (size_t)(p.out_first + pic) * sizeof(hevcdl_picture_report_t) + offsetof(hevcdl_picture_report_t, digest) + 16 * plane;
  for (int i = 0; i < 16; i++) rec[i] = dg[i];
}

// one thread per (picture, plane)
__global__ __launch_bounds__(64) void hevcdl_report_finish_kernel(hevcdl_report_params p)
{
  const int t = blockIdx.x * 64 + threadIdx.x, pic = t / 3, plane = t - 3 * pic;
  if (pic >= p.n_pics || plane >= p.n_planes) return;
  hevcdl_picture_report_t *rec = (hevcdl_picture_report_t *)p.out + (p.out_first + pic);
  if (p.sse) rec->sse[plane] = ((const hevcdl_quality *)p.sse)[pic].sse[plane];
  const int pb = p.method == 1 ? 16 : (p.method == 2 ? 2 : (p.method == 3 ? 4 : 0));
  if (plane == 0) { rec->method = p.method; rec->plane_bytes = pb; }
  if (p.method != 2 && p.method != 3) return;
  const uint64_t n = (uint64_t)(uint32_t)p.plane_w[plane] * (uint32_t)p.plane_h[plane] * (uint32_t)p.sample_bytes;
  const size_t chunks = report_chunks(n, (uint64_t)p.chunk_bytes);
  const uint32_t *part = p.partials + ((size_t)pic * 3 + plane) * p.chunk_stride;
  if (p.method == 2) {
    const uint32_t v = crc_fold(part, chunks, n, (uint64_t)p.chunk_bytes);
    rec->digest[2 * plane] = (uint8_t)(v >> 8); rec->digest[2 * plane + 1] = (uint8_t)v;
  } else {
    uint32_t sum = 0;
    for (size_t k = 0; k < chunks; k++) sum += part[k];
    for (int k = 0; k < 4; k++) rec->digest[4 * plane + k] = (uint8_t)(sum >> (24 - 8 * k));
  }
}

template <typename PEL> void launch(const hevcdl_report_params &p, hipStream_t st, hipEvent_t *ev)
{
  if (ev) hipEventRecord(ev[0], st);
  if (p.method == 1) hipLaunchKernelGGL(hevcdl_report_md5_kernel<PEL>, dim3((p.n_pics + 63) / 64, p.n_planes), dim3(64), 0, st, p);
  else if (p.method == 2 || p.method == 3) {
    uint64_t max_n = 0;
    for (int c = 0; c < p.n_planes; c++) { const uint64_t n = (uint64_t)p.plane_w[c] * p.plane_h[c] * sizeof(PEL); max_n = max_n > n ? max_n : n; }
    hipLaunchKernelGGL(hevcdl_report_partial_kernel<PEL>, dim3((unsigned)report_chunks(max_n, (uint64_t)p.chunk_bytes), p.n_planes, p.n_pics), dim3(REPORT_LANES), 0, st, p);
  }
  if (ev) hipEventRecord(ev[1], st);
  hipLaunchKernelGGL(hevcdl_report_finish_kernel, dim3((p.n_pics * 3 + 63) / 64), dim3(64), 0, st, p);
  if (ev) hipEventRecord(ev[2], st);
}

}  // namespace

extern "C" void hevcdl_launch_report(const hevcdl_report_params *pp, void *stream, void **events_opt)
{
  if (pp->sample_bytes == 1) launch<uint8_t>(*pp, (hipStream_t)stream, (hipEvent_t *)events_opt);
  else launch<uint16_t>(*pp, (hipStream_t)stream, (hipEvent_t *)events_opt);
}
