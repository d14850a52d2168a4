// recon_launch.h -- recon_kernel.hip's launch on work memory the caller owns (nothing allocated, freed or waited for), for the host code of the library
// (hevcdl_api.hip: hevcdl_decode_stream keeps the work memory in its context).  See recon_kernel.hip.
#ifndef HEVCDL_RECON_LAUNCH_H
#define HEVCDL_RECON_LAUNCH_H
#include <stddef.h>
#include <stdint.h>
#include <vector>
#include "hevcdl.h"
extern "C" size_t hevcdl_recon_work_bytes(int width, int height, int n_frames);
hevcdl_status hevcdl_recon_enqueue(const hevcdl_stream_config *cfg, const hevcdl_slice_layout *slices_opt, const int32_t *qps_opt, const void *d_records, int n_frames,
                                   void *d_recon, void *d_work, size_t work_bytes, void *stream, std::vector<uint32_t> &keep, const uint32_t **d_error);
// the instantiation with a QP per CU: d_qp_map int8 [n_frames][ctus][256] in device memory, the PPS chroma offsets of *qp_info; the same work memory
hevcdl_status hevcdl_recon_enqueue_qp(const hevcdl_stream_config *cfg, const hevcdl_slice_layout *slices_opt, const hevcdl_qp_info *qp_info, const void *d_qp_map, const void *d_records,
                                      int n_frames, void *d_recon, void *d_work, size_t work_bytes, void *stream, std::vector<uint32_t> &keep, const uint32_t **d_error);
// the instantiation with scaling lists on top of the QP map: d_factor HEVCDL_SCALING_FACTOR_BYTES non-zero bytes in device memory (hevcdl_scaling_info.factor); the same work memory
hevcdl_status hevcdl_recon_enqueue_sl(const hevcdl_stream_config *cfg, const hevcdl_slice_layout *slices_opt, const hevcdl_qp_info *qp_info, const void *d_qp_map, const void *d_factor,
                                      const void *d_records, int n_frames, void *d_recon, void *d_work, size_t work_bytes, void *stream, std::vector<uint32_t> &keep, const uint32_t **d_error);
#endif
