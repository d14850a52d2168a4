// slice_decode_units.h -- what the host builds for the shared slice-data decoder (slice_decode_core.h) and who runs it: hevcdl_parse.cpp builds the tables in the one
// walk over the stream that the parser runs too (walk_stream),hevcdl_parse_stream_core walks them on the CPU, slice_decode_kernel.hip and hevcdl_decode_stream (hevcdl_api.hip) on the device.
#ifndef HEVCDL_SLICE_DECODE_UNITS_H
#define HEVCDL_SLICE_DECODE_UNITS_H
#include <stddef.h>
#include <stdint.h>
#include <vector>
#include "hevcdl.h"
#include "hevcdl_parse.h"
#include "slice_decode_core.h"

namespace hevcdl_parse {

// What the walk over a stream (walk_stream, hevcdl_parse.cpp) leaves behind its last picture, as hevcdl_parse_stream gives it; a refused stream leaves it unset.
struct StreamShape {
  hevcdl_stream_config cfg; hevcdl_slice_layout slices; hevcdl_segment_layout segments;
  hevcdl_qp_info qp = { 0, 0, 0, 0 };            // the PPS fields a QP map goes with (all 0 unless accepted)
  hevcdl_scaling_info sl;                        // the SPS's scaling lists as factors (enabled 0 unless accepted)
};
// The pictures of a stream with their headers parsed and their slice data cut into units: what the walk's second sink makes of a picture where hevcdl_parse_stream's
// decodes it.  A refusal of the headers does not end the collection with nothing: the pictures in front of it stay, and the refusal waits in `pending` --
// hevcdl_parse_stream decodes a picture before it reads the next one's headers, so an error in the slice data of an earlier picture is the one it reports, and so
// do the walkers of these tables.  (The StreamShape part only without a pending refusal.)
struct StreamUnits : StreamShape {
  hevcdl_sd::SdStream sd;
  int ctus = 0;
  std::vector<hevcdl_parsed_picture> pictures;
  std::vector<uint8_t> rbsp;                     // the slice data of every picture, emulation prevention removed, sub-stream behind sub-stream
  std::vector<hevcdl_sd::SdSub> subs;            // offsets count from the first byte of their picture
  std::vector<hevcdl_sd::SdUnit> units;          // pic: index into pictures; sub0: index into subs; rbsp0: 0 (a batch sets it when it is cut out: batch_tables)
  std::vector<size_t> pic_byte, pic_sub, pic_unit;      // [pictures + 1]: where picture i's bytes, sub-streams and units start
  hevcdl_status pending = HEVCDL_OK; char pending_sentence[256] = "";
};
// want_slice_data 0: headers only (no tables).  have_sao / ctu_capacity: the caller's room, checked per picture as hevcdl_parse_stream does.  Returns HEVCDL_OK also with a
// pending refusal; anything else is a refusal in front of the first picture's end (the sentence is in hevcdl_parse_error()).
// accept: HEVCDL_ACCEPT_* bits (hevcdl.h) -- 0: cu_qp_delta_enabled_flag, chroma QP offsets and scaling lists are refused as ever; su.qp says what the PPS carries, su.sl what the SPS.
hevcdl_status collect_units(const uint8_t *stream, size_t bytes, int want_slice_data, int have_sao, size_t ctu_capacity, StreamUnits &out, unsigned accept = 0);
// the tables of pictures [first, first + count) as one launch takes them: units and sub-streams renumbered from 0, rbsp0 from the first byte of picture `first`
hevcdl_status batch_tables(const StreamUnits &su, int first, int count, std::vector<hevcdl_sd::SdUnit> &units, size_t &sub0, size_t &n_subs, size_t &byte0, size_t &n_bytes);

// Walks the units of pictures [0, n) into records / sao ([n][ctus]; sao may be null when no picture has SAO on).  HEVCDL_OK: *bad_pic < 0, or the lowest picture with an error and its
// first error in *res; anything else: the walker itself failed (a HIP error; the sentence set).  qp_map: [n][ctus][256] or null (hevcdl_parse_stream_qp).
typedef hevcdl_status (*UnitWalker)(void *user, const StreamUnits &su, int n, hevcdl_ctu_record *records, hevcdl_sao_blk *sao, int8_t *qp_map, int *bad_pic, hevcdl_sd::SdResult *res);
// hevcdl_parse_stream's contract with the slice data decoded by `walk`
hevcdl_status parse_stream_with(UnitWalker walk, void *user, const uint8_t *stream, size_t bytes, hevcdl_stream_config *cfg, hevcdl_slice_layout *slices, hevcdl_segment_layout *segments,
                                hevcdl_parsed_picture *pictures, int picture_capacity, int *n_pictures, hevcdl_ctu_record *records, hevcdl_sao_blk *sao, size_t ctu_capacity,
                                unsigned accept = 0, hevcdl_qp_info *qp_info = nullptr, int8_t *qp_map = nullptr, hevcdl_scaling_info *scaling = nullptr);
// "picture 3, CTU 17: <sentence of the code>" into hevcdl_parse_error()
void set_slice_error(int pic, const hevcdl_sd::SdResult &res);

} // namespace hevcdl_parse

// ---- the launch (slice_decode_kernel.hip) ------------------------------------------------------------------------------------------------------------------
// One wave per unit.  All pointers are device memory: blob [blob_bytes] RBSP bytes of the batch, subs [n_subs], units [n_units] (batch_tables), tables an EcTables block,
// records [n_pics][ctus] (16-byte aligned) and sao [n_pics][ctus] (may be null when no unit has SAO on) are written -- every CTU of every unit is cleared, then decoded --
// and results [n_units] receives a code and a CTU per unit.
struct hevcdl_slice_decode_params {
  hevcdl_sd::SdStream sd;
  const uint8_t *blob; unsigned long long blob_bytes;
  const hevcdl_sd::SdSub *subs; const hevcdl_sd::SdUnit *units; int n_subs, n_units;
  void *records; void *sao; int ctus, n_pics;
  hevcdl_sd::SdResult *results;
  const void *tables;
  int8_t *qp_map;                                // [n_pics][ctus][256] QpY per 4x4 partition, or null: not wanted (must not be null when sd.cu_qp is set)
};
// launches nothing and returns 0 when the parameters do not fit each other (no units, a grid that is not `ctus` CTUs, null pointers); 1 behind a launch
int hevcdl_launch_slice_decode(const hevcdl_slice_decode_params *p, void *stream);
// the first unit with an error in results [n_units] of a batch -> its picture in the batch (units[].pic) and *res; -1: none
int hevcdl_slice_decode_first_error(const std::vector<hevcdl_sd::SdUnit> &units, const hevcdl_sd::SdResult *results, hevcdl_sd::SdResult *res);
#endif
