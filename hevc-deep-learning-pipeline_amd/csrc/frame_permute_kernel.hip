// frame_permute_kernel.hip -- device side of a QP per picture (hevcdl_set_frame_qps; csrc/frame_qp.h): the decision kernel reads its constants once per launch, so the
// pictures of one QP have to form one launch.  Where a batch's QPs are not already contiguous runs, this kernel brings source pictures and labels together by QP in front of
// the decision launches (gather) and takes records, reconstruction and statistics back to picture order behind them (scatter).
//
// Plain launches in stream order: nothing here waits for another wave, no flag is polled, no atomics.  Every loop bound is a launch parameter.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "hevcdl_dev.h"

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));      // one dwordx4 load or store

// field `f` of range k, k uniform over the workgroup: selects, not an indexed read of the kernel's arguments
#define RANGE_FIELD(p, k, f) ((k) == 0 ? (p).r[0].f : (k) == 1 ? (p).r[1].f : (k) == 2 ? (p).r[2].f : (p).r[3].f)

template <class T> static __device__ __forceinline__ void copy_narrow(const unsigned char *src, unsigned char *dst, unsigned long long units, int iters, int lane)
{
  for (int it = 0; it < iters; it++) {
    const unsigned long long a = (unsigned long long)it * 256 + lane;
    if (a < units) ((T *)dst)[a] = ((const T *)src)[a];
  }
}

// Grid (chunk, picture).  The permutation entry of the picture is read through readfirstlane: a wave-uniform value, so every address below is a scalar base plus the lane's
// offset.  A range whose picture size and bases are multiples of 16 is a run of 16-byte units cut into chunks of chunk_iters x 1024 units; a workgroup copies one chunk of
// one range, four units a lane in flight (dwordx4 loads, then dwordx4 stores; consecutive lanes take consecutive units).  The last chunk of a range is cut short by the
// range's own unit count: nothing is read or written past a picture.  The other ranges (the 40 bytes of statistics a picture: bases 8-byte aligned only) are copied by
// workgroup (0, picture) with loads and stores of the range's own width.
extern "C" __global__ __launch_bounds__(256) void hevcdl_frame_permute_kernel(hevcdl_frame_permute_params p, int pic_first)
{
  const int pic = pic_first + (int)blockIdx.y, lane = (int)threadIdx.x;
  if (pic >= p.n_frames) return;
  const int e = __builtin_amdgcn_readfirstlane(p.perm[pic]);
  if (e < 0 || e >= p.n_frames) return;      // (the host hands over a checked permutation; an entry outside the batch moves nothing)
  const unsigned long long sp = (unsigned long long)(p.scatter ? pic : e), dp = (unsigned long long)(p.scatter ? e : pic);
  const unsigned int c = blockIdx.x;
  if (c < p.chunk_first[4]) {
    const int k = (c >= p.chunk_first[1]) + (c >= p.chunk_first[2]) + (c >= p.chunk_first[3]);
    const unsigned long long bytes = RANGE_FIELD(p, k, bytes), units = RANGE_FIELD(p, k, units);
    const u32x4 *__restrict__ src = (const u32x4 *)(RANGE_FIELD(p, k, src) + sp * bytes);
    u32x4 *__restrict__ dst = (u32x4 *)(RANGE_FIELD(p, k, dst) + dp * bytes);
    const unsigned int first = k == 0 ? 0u : k == 1 ? p.chunk_first[1] : k == 2 ? p.chunk_first[2] : p.chunk_first[3];
    const unsigned long long begin = (unsigned long long)(c - first) * 1024ull * (unsigned long long)p.chunk_iters;
    for (int it = 0; it < p.chunk_iters; it++) {
      const unsigned long long u0 = begin + (unsigned long long)it * 1024 + lane;
      u32x4 v[4];
#pragma unroll
      for (int j = 0; j < 4; j++) { const unsigned long long u = u0 + 256ull * j; v[j] = src[u < units ? u : units - 1]; }      // unconditional (a lane past the end re-reads the range's last unit): a load under a branch would wait for the one before it
#pragma unroll
      for (int j = 0; j < 4; j++) { const unsigned long long u = u0 + 256ull * j; if (u < units) dst[u] = v[j]; }
    }
  }
  if (c != 0) return;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    if (k >= p.n_ranges || p.r[k].unit_bytes == 16) continue;
    const unsigned char *src = p.r[k].src + sp * p.r[k].bytes;
    unsigned char *dst = p.r[k].dst + dp * p.r[k].bytes;
    if (p.r[k].unit_bytes == 8) copy_narrow<unsigned long long>(src, dst, p.r[k].units, p.narrow_iters, lane);
    else if (p.r[k].unit_bytes == 4) copy_narrow<unsigned int>(src, dst, p.r[k].units, p.narrow_iters, lane);
    else copy_narrow<unsigned char>(src, dst, p.r[k].units, p.narrow_iters, lane);
  }
}

extern "C" void hevcdl_launch_frame_permute(const hevcdl_frame_permute_params *pp, void *stream)
{
  if (pp->n_frames <= 0 || pp->n_ranges < 1 || pp->n_ranges > 4 || !pp->perm) return;
  hevcdl_frame_permute_params p = *pp;
  unsigned long long widest = 0, narrowest = 0;
  for (int k = 0; k < 4; k++) {
    hevcdl_frame_permute_range &r = p.r[k];
    if (k >= p.n_ranges) { r.src = nullptr; r.dst = nullptr; r.bytes = 0; r.unit_bytes = 16; r.units = 0; r.pad = 0; continue; }
    const unsigned long long all = r.bytes | (unsigned long long)(uintptr_t)r.src | (unsigned long long)(uintptr_t)r.dst;
    r.unit_bytes = !(all & 15) ? 16 : !(all & 7) ? 8 : !(all & 3) ? 4 : 1; r.pad = 0;
    r.units = r.bytes / (unsigned long long)r.unit_bytes;
    if (r.unit_bytes == 16) widest = r.units > widest ? r.units : widest; else narrowest = r.units > narrowest ? r.units : narrowest;
  }
  // 128 KB a workgroup (8 rounds of 256 lanes x 4 units), fewer rounds when the largest range is smaller: the records and reconstruction of a 2160p picture are 336 workgroups
  const unsigned long long rounds = (widest + 1023) / 1024;
  p.chunk_iters = (int)(rounds < 8 ? (rounds ? rounds : 1) : 8);
  p.narrow_iters = (int)((narrowest + 255) / 256);
  const unsigned long long chunk16 = 1024ull * (unsigned long long)p.chunk_iters;
  unsigned long long at = 0;
  for (int k = 0; k < 4; k++) { p.chunk_first[k] = (unsigned int)at; if (p.r[k].unit_bytes == 16) at += (p.r[k].units + chunk16 - 1) / chunk16; }
  p.chunk_first[4] = (unsigned int)at;
  if (at > 0x7fffffffull) return;      // (2^31 chunks of 16 KB at the least a picture: no picture is that large)
  for (int first = 0; first < p.n_frames; first += 65535) {      // (gridDim.y holds 65535 pictures)
    const int cnt = p.n_frames - first < 65535 ? p.n_frames - first : 65535;
    hipLaunchKernelGGL(hevcdl_frame_permute_kernel, dim3((unsigned)(at ? at : 1), (unsigned)cnt), dim3(256), 0, (hipStream_t)stream, p, first);
  }
}
