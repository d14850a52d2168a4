// source_kernel.hip -- source-format pictures into the codec's format and coded pictures into output-format frames, for gfx950 (MI355X).
//
// Replaces, for pictures that are in HBM, the reference's file boundary (TVideoIOYuv.cpp: readPlane :363-381, scalePlane :70-95, write :755-830): padding to the coded
// size and the bit-depth change in front of the CNN and the decision kernel, the crop to the conformance window and the change to the output depth behind the filters.
// The arithmetic is csrc/source_core.h, the source the host compiles too; everything is exact.  Both directions move every sample once: the kernels are HBM bound.
//
// Kernels (plain launches on one stream; no cooperative launch, no flag another wave sets, no atomics, no LDS; every loop bound is a launch parameter):
//   hevcdl_source_load_kernel<IN, PEL>    grid (row groups, planes, pictures), 256 lanes: a workgroup converts rows_per_group rows of one plane.  A row is cut into
//   hevcdl_source_store_kernel<PEL, OUT>  pieces of 16 samples counted from the 16-byte boundary at or in front of the row's first DESTINATION byte, so that every whole
//                                         piece is stored as dwordx4 (two for 16-bit samples); the pieces that hang over the row's ends are stored sample by sample.  A
//                                         piece is read as dwordx4 where its source address allows and it lies inside the source row, sample by sample otherwise (rows of
//                                         odd chroma widths, the replicated columns, a source pointer that is only sample aligned).  Neighbouring lanes take neighbouring pieces.
//   The load kernel clamps the source coordinates (the padding rule of source_core.h); the store kernel reads the window's samples only.
//   hevcdl_source_load_fmt_kernel<IN, PEL>   the same for a file that is not planar 4:2:0 with Cb before Cr (4:0:0 / 4:2:2 / 4:4:4, swapped chroma planes) and for a
//   hevcdl_source_store_fmt_kernel<PEL, OUT> window with an origin: kernels and a parameter block of their own behind the two above, which stay the code they were and
//                                         are what a format without those fields launches.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "hevcdl.h"
#include "hevcdl_dev.h"
#include "source_core.h"

namespace {

using namespace hevcdl_src;

enum { SOURCE_LANES = 256, SOURCE_PIECE = 16 };

// sixteen samples from 16-byte aligned memory
__device__ __forceinline__ void read_piece(const uint8_t *q, int32_t v[SOURCE_PIECE])
{
  const uint4 a = *(const uint4 *)q;
  const uint32_t w[4] = { a.x, a.y, a.z, a.w };
#pragma unroll
  for (int i = 0; i < SOURCE_PIECE; i++) v[i] = (int32_t)((w[i >> 2] >> (8 * (i & 3))) & 0xff);
}
__device__ __forceinline__ void read_piece(const uint16_t *q, int32_t v[SOURCE_PIECE])
{
  const uint4 a = ((const uint4 *)q)[0], b = ((const uint4 *)q)[1];
  const uint32_t w[8] = { a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w };
#pragma unroll
  for (int i = 0; i < SOURCE_PIECE; i++) v[i] = (int32_t)((w[i >> 1] >> (16 * (i & 1))) & 0xffff);
}
__device__ __forceinline__ void write_piece(uint8_t *q, const int32_t v[SOURCE_PIECE])
{
  uint32_t w[4] = { 0, 0, 0, 0 };
#pragma unroll
  for (int i = 0; i < SOURCE_PIECE; i++) w[i >> 2] |= ((uint32_t)v[i] & 0xff) << (8 * (i & 3));
  *(uint4 *)q = make_uint4(w[0], w[1], w[2], w[3]);
}
__device__ __forceinline__ void write_piece(uint16_t *q, const int32_t v[SOURCE_PIECE])
{
  uint32_t w[8] = { 0, 0, 0, 0, 0, 0, 0, 0 };
#pragma unroll
  for (int i = 0; i < SOURCE_PIECE; i++) w[i >> 1] |= ((uint32_t)v[i] & 0xffff) << (16 * (i & 1));
  ((uint4 *)q)[0] = make_uint4(w[0], w[1], w[2], w[3]); ((uint4 *)q)[1] = make_uint4(w[4], w[5], w[6], w[7]);
}

// Rows [row0, row0 + rows_per_group) of plane `plane` of picture `pic`: destination sample (x, y) = scale(source sample (min(x, sw - 1), min(y, sh - 1))).
// The load kernel's source is smaller than its destination (the clamp is the padding); the store kernel's is larger (the clamp never acts).
template <typename S, typename D> __device__ __forceinline__ void convert_rows(const hevcdl_source_params &p)
{
  const int plane = blockIdx.y, pic = blockIdx.z, tid = threadIdx.x;
  const int sw = plane_width(p.src_w, plane), sh = plane_height(p.src_h, plane), dw = plane_width(p.dst_w, plane), dh = plane_height(p.dst_h, plane);
  const int row0 = (int)blockIdx.x * p.rows_per_group;
  if (row0 >= dh) return;                                                  // (the whole workgroup: the grid is sized by the luma plane)
  const int rows = dh - row0 < p.rows_per_group ? dh - row0 : p.rows_per_group;
  const S *sp = (const S *)p.src + picture_samples(p.src_w, p.src_h) * (size_t)pic + plane_offset(p.src_w, p.src_h, plane);
  D *dp = (D *)p.dst + picture_samples(p.dst_w, p.dst_h) * (size_t)pic + plane_offset(p.dst_w, p.dst_h, plane);
  const int slots = (dw + 2 * SOURCE_PIECE - 2) / SOURCE_PIECE + 1;        // pieces a row can take, whatever its alignment (a launch parameter's function: the same for every row)
  for (int it = tid; it < rows * slots; it += SOURCE_LANES) {
    const int y = row0 + it / slots, k = it - (it / slots) * slots;
    const S *srow = sp + (size_t)(y < sh ? y : sh - 1) * sw;
    D *drow = dp + (size_t)y * dw;
    const int lead = (int)(((uintptr_t)drow / sizeof(D)) & (16 / sizeof(D) - 1));       // samples between the 16-byte boundary in front of the row and the row
    const int x0 = k * SOURCE_PIECE - lead, x1 = x0 + SOURCE_PIECE;
    if (x1 <= 0 || x0 >= dw) continue;
    int32_t v[SOURCE_PIECE];
    if (x0 >= 0 && x1 <= sw && (((uintptr_t)(srow + x0)) & 15) == 0) read_piece(srow + x0, v);
    else {
#pragma unroll
      for (int i = 0; i < SOURCE_PIECE; i++) { const int x = x0 + i; v[i] = (x >= 0 && x < dw) ? (int32_t)srow[x < sw ? x : sw - 1] : 0; }
    }
#pragma unroll
    for (int i = 0; i < SOURCE_PIECE; i++) v[i] = scale_sample(v[i], p.from_depth, p.to_depth);
    if (x0 >= 0 && x1 <= dw) write_piece(drow + x0, v);                    // 16-byte aligned by the choice of `lead`
    else {
#pragma unroll
      for (int i = 0; i < SOURCE_PIECE; i++) { const int x = x0 + i; if (x >= 0 && x < dw) drow[x] = (D)v[i]; }
    }
  }
}

template <typename IN, typename PEL> __global__ __launch_bounds__(SOURCE_LANES) void hevcdl_source_load_kernel(hevcdl_source_params p) { convert_rows<IN, PEL>(p); }
template <typename PEL, typename OUT> __global__ __launch_bounds__(SOURCE_LANES) void hevcdl_source_store_kernel(hevcdl_source_params p) { convert_rows<PEL, OUT>(p); }

template <typename S, typename D> void launch(const hevcdl_source_params &p, hipStream_t st, bool store)
{
  const dim3 grid((unsigned)((p.dst_h + p.rows_per_group - 1) / p.rows_per_group), 3, (unsigned)p.n_pics);
  if (store) hipLaunchKernelGGL((hevcdl_source_store_kernel<S, D>), grid, dim3(SOURCE_LANES), 0, st, p);
  else hipLaunchKernelGGL((hevcdl_source_load_kernel<S, D>), grid, dim3(SOURCE_LANES), 0, st, p);
}

void launch_any(const hevcdl_source_params *pp, void *stream, bool store)
{
  hevcdl_source_params p = *pp;
  if (p.n_pics <= 0) return;
  // rows of a workgroup: about 8192 samples, 32 a lane; a picture's z index is bounded by the grid (65535 pictures a launch: far above any batch a context holds)
  p.rows_per_group = p.dst_w >= 8192 ? 1 : 8192 / p.dst_w;
  if (p.rows_per_group > p.dst_h) p.rows_per_group = p.dst_h;
  hipStream_t st = (hipStream_t)stream;
  if (p.src_bytes == 1 && p.dst_bytes == 1) launch<uint8_t, uint8_t>(p, st, store);
  else if (p.src_bytes == 1) launch<uint8_t, uint16_t>(p, st, store);
  else if (p.dst_bytes == 1) launch<uint16_t, uint8_t>(p, st, store);
  else launch<uint16_t, uint16_t>(p, st, store);
}

// ---- the file's layout: 4:0:0 / 4:2:2 / 4:4:4 sources, swapped chroma planes, a window with an origin (source_core.h plane_ref) ---------------------------------------
// Kernels of their own, so that convert_rows above stays the code it was.  The destination side is the same: 16-sample pieces from the 16-byte boundary of the
// destination row, whole pieces stored as dwordx4.  The source side goes by the plane's description:
//   constant (a 4:0:0 file's chroma)   no read: the piece is the scaled constant -- a fill
//   step 1                             a dwordx4 read (two for 16-bit samples) where the piece lies inside the clamp limit and its first source sample is 16-byte aligned
//   step 2 (a 4:4:4 file's chroma)     32 source samples as two such reads where all of them are inside the source row and aligned; the even ones are kept
//   otherwise                          sample by sample through the clamp (row ends, replicated columns, pointers that are only sample aligned: a window's origin)
// A vertical step of 2 is row addressing alone: the odd source rows are never read.

// thirty-two samples from 16-byte aligned memory, the even ones kept
__device__ __forceinline__ void read_piece_even(const uint8_t *q, int32_t v[SOURCE_PIECE])
{
  const uint4 a = ((const uint4 *)q)[0], b = ((const uint4 *)q)[1];
  const uint32_t w[8] = { a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w };
#pragma unroll
  for (int i = 0; i < SOURCE_PIECE; i++) v[i] = (int32_t)((w[i >> 1] >> (16 * (i & 1))) & 0xff);
}
__device__ __forceinline__ void read_piece_even(const uint16_t *q, int32_t v[SOURCE_PIECE])
{
  const uint4 a = ((const uint4 *)q)[0], b = ((const uint4 *)q)[1], c = ((const uint4 *)q)[2], d = ((const uint4 *)q)[3];
  const uint32_t w[16] = { a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w, d.x, d.y, d.z, d.w };
#pragma unroll
  for (int i = 0; i < SOURCE_PIECE; i++) v[i] = (int32_t)(w[i] & 0xffff);
}

template <typename S, typename D> __device__ __forceinline__ void convert_rows_fmt(const hevcdl_source_fmt_params &q, bool store)
{
  const hevcdl_source_params &p = q.b;
  const int plane = blockIdx.y, pic = blockIdx.z, tid = threadIdx.x;
  const int dw = plane_width(p.dst_w, plane), dh = plane_height(p.dst_h, plane);
  const int row0 = (int)blockIdx.x * p.rows_per_group;
  if (row0 >= dh) return;                                                  // (the whole workgroup: the grid is sized by the luma plane)
  const int rows = dh - row0 < p.rows_per_group ? dh - row0 : p.rows_per_group;
  const plane_ref r = store ? store_plane_ref(p.src_w, p.src_h, p.dst_w, p.dst_h, q.win_x, q.win_y, q.swap, plane) : load_plane_ref(p.src_w, p.src_h, q.chroma_format, q.swap, plane, p.from_depth);
  const S *sp = (const S *)p.src + picture_samples_fmt(p.src_w, p.src_h, store ? (int)FMT_420 : q.chroma_format) * (size_t)pic + r.offset;
  D *dp = (D *)p.dst + picture_samples(p.dst_w, p.dst_h) * (size_t)pic + plane_offset(p.dst_w, p.dst_h, plane);
  const int32_t fill = r.constant ? scale_sample(r.value, p.from_depth, p.to_depth) : 0;
  const int slots = (dw + 2 * SOURCE_PIECE - 2) / SOURCE_PIECE + 1;        // pieces a row can take, whatever its alignment
  for (int it = tid; it < rows * slots; it += SOURCE_LANES) {
    const int y = row0 + it / slots, k = it - (it / slots) * slots;
    D *drow = dp + (size_t)y * dw;
    const int lead = (int)(((uintptr_t)drow / sizeof(D)) & (16 / sizeof(D) - 1));       // samples between the 16-byte boundary in front of the row and the row
    const int x0 = k * SOURCE_PIECE - lead, x1 = x0 + SOURCE_PIECE;
    if (x1 <= 0 || x0 >= dw) continue;
    int32_t v[SOURCE_PIECE];
    if (r.constant) {
#pragma unroll
      for (int i = 0; i < SOURCE_PIECE; i++) v[i] = fill;
    } else {
      const S *srow = sp + ((size_t)(y < r.lim_h ? y : r.lim_h - 1) << r.sy) * (size_t)r.pitch;
      const bool inside = x0 >= 0 && x1 <= r.lim_w;                        // no clamped column in the piece: its source samples are (x0 .. x1 - 1) << sx, all inside the source row
      if (inside && r.sx == 0 && (((uintptr_t)(srow + x0)) & 15) == 0) read_piece(srow + x0, v);
      else if (inside && r.sx == 1 && (((uintptr_t)(srow + 2 * (size_t)x0)) & 15) == 0) read_piece_even(srow + 2 * (size_t)x0, v);      // reads samples 2 x0 .. 2 x0 + 31 <= 2 lim_w - 1: inside the row of 2 lim_w samples
      else {
#pragma unroll
        for (int i = 0; i < SOURCE_PIECE; i++) { const int x = x0 + i; v[i] = (x >= 0 && x < dw) ? (int32_t)srow[(size_t)(x < r.lim_w ? x : r.lim_w - 1) << r.sx] : 0; }
      }
#pragma unroll
      for (int i = 0; i < SOURCE_PIECE; i++) v[i] = scale_sample(v[i], p.from_depth, p.to_depth);
    }
    if (x0 >= 0 && x1 <= dw) write_piece(drow + x0, v);                    // 16-byte aligned by the choice of `lead`
    else {
#pragma unroll
      for (int i = 0; i < SOURCE_PIECE; i++) { const int x = x0 + i; if (x >= 0 && x < dw) drow[x] = (D)v[i]; }
    }
  }
}

template <typename IN, typename PEL> __global__ __launch_bounds__(SOURCE_LANES) void hevcdl_source_load_fmt_kernel(hevcdl_source_fmt_params q) { convert_rows_fmt<IN, PEL>(q, false); }
template <typename PEL, typename OUT> __global__ __launch_bounds__(SOURCE_LANES) void hevcdl_source_store_fmt_kernel(hevcdl_source_fmt_params q) { convert_rows_fmt<PEL, OUT>(q, true); }

template <typename S, typename D> void launch_fmt(const hevcdl_source_fmt_params &q, hipStream_t st, bool store)
{
  const dim3 grid((unsigned)((q.b.dst_h + q.b.rows_per_group - 1) / q.b.rows_per_group), 3, (unsigned)q.b.n_pics);
  if (store) hipLaunchKernelGGL((hevcdl_source_store_fmt_kernel<S, D>), grid, dim3(SOURCE_LANES), 0, st, q);
  else hipLaunchKernelGGL((hevcdl_source_load_fmt_kernel<S, D>), grid, dim3(SOURCE_LANES), 0, st, q);
}

void launch_any_fmt(const hevcdl_source_fmt_params *qq, void *stream, bool store)
{
  hevcdl_source_fmt_params q = *qq;
  hevcdl_source_params &p = q.b;
  if (p.n_pics <= 0) return;
  p.rows_per_group = p.dst_w >= 8192 ? 1 : 8192 / p.dst_w;                 // as launch_any
  if (p.rows_per_group > p.dst_h) p.rows_per_group = p.dst_h;
  hipStream_t st = (hipStream_t)stream;
  if (p.src_bytes == 1 && p.dst_bytes == 1) launch_fmt<uint8_t, uint8_t>(q, st, store);
  else if (p.src_bytes == 1) launch_fmt<uint8_t, uint16_t>(q, st, store);
  else if (p.dst_bytes == 1) launch_fmt<uint16_t, uint8_t>(q, st, store);
  else launch_fmt<uint16_t, uint16_t>(q, st, store);
}

}  // namespace

extern "C" void hevcdl_launch_source_load_fmt(const hevcdl_source_fmt_params *p, void *stream) { launch_any_fmt(p, stream, false); }
extern "C" void hevcdl_launch_source_store_fmt(const hevcdl_source_fmt_params *p, void *stream) { launch_any_fmt(p, stream, true); }
extern "C" void hevcdl_launch_source_load(const hevcdl_source_params *p, void *stream) { launch_any(p, stream, false); }
extern "C" void hevcdl_launch_source_store(const hevcdl_source_params *p, void *stream) { launch_any(p, stream, true); }
