"""oracle/slice_spec.py -- TEST INFRASTRUCTURE, not product code.

An independent DECODER of the slice data of an I slice, written from the text of ITU-T H.265 for the configuration the product writes: pictures of
one or several slices and dependent slice segments (a NAL unit each), 4:2:0, CTB 64, minimum CB 8, transform blocks 4 .. 32, no PCM / transquant
bypass / scaling lists / cu_qp_delta, tiles or entropy_coding_sync (wavefront rows), SAO on or off, 8 and 10 bits.  Clauses restated:

  7.3.6.1 (in oracle/hevc_parse.py), 7.4.7.1     slice_segment_header: first_slice_segment_in_pic_flag, dependent_slice_segment_flag, slice_segment_address,
                                                 the dependent header, the deblocking override fields, the entry points; SliceAddrRs
  7.3.8.1-7.3.8.5, 7.3.8.8, 7.3.8.10, 7.3.8.11   slice_segment_data (per segment), coding_tree_unit, sao, coding_quadtree, coding_unit, transform_tree,
                                                 transform_unit, residual_coding, with the semantics of 7.4.9 (inferred values, scanIdx, hidden signs)
  9.3.1-9.3.4                                    initialisation, storage and synchronisation of the context variables (tile start, wavefront row start,
                                                 start of a dependent segment, start of a slice: in that order), the binarisations, the ctxInc
                                                 derivations, the arithmetic decoding engine (decision, bypass, terminate)
  6.5.1-6.5.5                                    CTB raster <-> tile scan, TileId, MinTbAddrZs, the up-right diagonal, horizontal and vertical scans
  6.4.1                                          z-scan order availability (picture, decoding order, tile, slice)
  8.4.2, 8.4.3                                   the candidate list of the luma prediction mode, rem_intra_luma_pred_mode, the chroma mode

SLICES AND SEGMENTS.  decode_access_unit takes every slice NAL unit of the access unit in order and cuts each one's sub-streams at its own entry points
against its own payload.  SliceAddrRs (the address of the independent segment a CTB's slice began with) is the slice term of availability and of the SAO
merge candidates.  A picture of row slices (SliceMode 1) has NO tiles in its PPS and is decoded with one tile and slice availability alone -- the product
computes the same thing as a tile grid of one column (csrc/slice_grid.h); the two stay two derivations, the coder's grid is never passed in.  Not
covered: slices or segments that start inside a CTU row or inside a tile (the product refuses those layouts, so the restore of 9.3.2.2's TableStateIdxDs
is implemented and its tally entry stays 0), P and B slices, wavefront together with tiles, SAO for luma or chroma alone.

It is deliberately NOT a restatement of csrc/entropy_coder.h or of the host writer: coding_quadtree and transform_tree are the recursive functions of
the standard (the product walks both trees iteratively), every scan, the last-position prefix / suffix split and the z-order are GENERATED from the
clauses, availability goes through MinTbAddrZs and TileId, and it reads bits where the product writes them.  The round trip
records -> coder -> bytes -> this decoder -> records is what tests/test_entropy_roundtrip.py holds the coder to.

CONSTANT TABLES.  The tables of the arithmetic coder that cannot be derived are handled as follows: transIdxLps (Table 9-41) and the 4x4 ctxIdxMap
(9.3.4.2.5) are typed in below from the standard and a CPU test asserts that they equal the product's; transIdxMps is the standard's rule (state + 1,
62 stays 62).  rangeTabLps (Table 9-40) and the initValue of every context of an I slice (Tables 9-5 .. 9-37, initType 0) are READ OUT OF
csrc/entropy_tables.h at import by a small parser (LPS_TABLE; CTX_INIT cut per syntax element at the enum offsets found there).  The contents of
those two tables are therefore pinned by the reference-encoder streams this decoder reproduces the records of (tests/golden/rd_*.npz, slices_*.npz,
segments_*.npz), NOT by the
round trip: an arithmetic coder round-trips with any table that the coder and the decoder share.

END CONDITIONS are demanded, not reported: end_of_slice_segment_flag is 1 behind the last CTU of every slice segment and nowhere else (the last CTU is
the one before the next segment's slice_segment_address; the last segment ends the picture), end_of_subset_one_bit (1) stands behind the last CTU of
every tile / CTU row that does not end its segment, byte_alignment() follows (a 1 and zeros up to the byte boundary) and then the sub-stream has no
byte left.  A violation, a read past the end of a sub-stream, a level outside 16 bits or an ivlOffset of 510 / 511 raises SliceError.

Besides records and SAO parameters the decoder returns a TALLY of the branches taken (as oracle/filter_spec.py does), so that a corpus can be held to
"this path was reached".  Nothing here is imported by the product package.
"""
import bisect
import os
import re

import numpy as np

REC_DTYPE = np.dtype([
    ("depth", "u1", 256), ("part_size", "u1", 256), ("luma_dir", "u1", 256), ("chroma_dir", "u1", 256),
    ("tr_idx", "u1", 256), ("cbf", "u1", (3, 256)), ("tskip", "u1", (3, 256)),
    ("bits", "<u4"), ("dist", "<u4"), ("cost", "<f8"),
    ("coeff_y", "<i2", 4096), ("coeff_cb", "<i2", 1024), ("coeff_cr", "<i2", 1024)])          # hevcdl_ctu_record
SAO_DTYPE = np.dtype([("mode", "<i4"), ("type", "<i4"), ("aux", "<i4"), ("offset", "<i4", 32)])   # hevcdl_sao_offset
TOOL_TSKIP, TOOL_SIGN_HIDE = 0x04, 0x10                                                       # HEVCDL_TOOL_* bits that change the slice-data syntax
DM_CHROMA = 36                                                                               # the record's value for intra_chroma_pred_mode 4


class SliceError(Exception):
    pass


# ---- constant tables ------------------------------------------------------------------------------------------------------------------------------
# Table 9-41, typed in from the standard
TRANS_IDX_LPS = [0, 0, 1, 2, 2, 4, 4, 5, 6, 7, 8, 9, 9, 11, 11, 12, 13, 13, 15, 15, 16, 16, 18, 18, 19, 19, 21, 21, 22, 22, 23, 24,
                 24, 25, 26, 26, 27, 27, 28, 29, 29, 30, 30, 30, 31, 32, 32, 33, 33, 33, 34, 34, 35, 35, 35, 36, 36, 36, 37, 37, 37, 38, 38, 63]
TRANS_IDX_MPS = [min(s + 1, 62) for s in range(63)] + [63]
# 9.3.4.2.5: ctxIdxMap[i] for log2TrafoSize 2, i = (yC << 2) + xC (the standard lists 15 entries; position 15 continues the 8s)
CTX_IDX_MAP = [0, 1, 4, 5, 2, 3, 4, 5, 6, 6, 8, 8, 7, 7, 8, 8]


def _parse_tables_header(path=None):
    """-> (enum name -> value, array name -> flat list of ints) of csrc/entropy_tables.h."""
    if path is None:
        root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
        hits = [os.path.join(root, d, "csrc", "entropy_tables.h") for d in sorted(os.listdir(root)) if os.path.exists(os.path.join(root, d, "csrc", "entropy_tables.h"))]
        path = hits[0]
    text = re.sub(r"//[^\n]*", "", open(path).read())
    enums = {}
    for body in re.findall(r"enum\s*\{([^}]*)\}", text):
        for name, val in re.findall(r"(\w+)\s*=\s*(\d+)", body):
            enums[name] = int(val)
    arrays = {}
    for name, body in re.findall(r"static const uint8_t (\w+)(?:\[[^\]]*\])+\s*=\s*\{(.*?)\};", text, re.S):
        arrays[name] = [int(v) for v in re.findall(r"\d+", body)]
    return enums, arrays


_ENUMS, _ARRAYS = _parse_tables_header()
RANGE_TAB_LPS = [_ARRAYS["LPS_TABLE"][4 * i:4 * i + 4] for i in range(64)]
assert len(_ARRAYS["LPS_TABLE"]) == 256 and len(_ARRAYS["CTX_INIT"]) == _ENUMS["NUM_CTX"]


def _init_slice(name, count, skip=0):
    at = _ENUMS[name] + skip
    return _ARRAYS["CTX_INIT"][at:at + count]


# initValue per syntax element (initType 0), in the standard's ctxIdx order.  The header keeps 28 + 16 slots for sig_coeff_flag and 15 + 15 for each
# last_sig_coeff prefix; the standard numbers 27 luma + 15 chroma and 15 luma + 3 chroma contexts, so those are cut out of the header's rows.
INIT_VALUES = {
    "sao_merge": _init_slice("CTX_SAO_MERGE", 1), "sao_type": _init_slice("CTX_SAO_TYPE", 1),
    "split_cu": _init_slice("CTX_SPLIT", 3), "part_mode": _init_slice("CTX_PART_SIZE", 1),
    "prev_intra": _init_slice("CTX_INTRA_PRED", 1), "chroma_pred": _init_slice("CTX_CHROMA_PRED", 1),
    "split_transform": _init_slice("CTX_SUBDIV", 3),
    "cbf_luma": _init_slice("CTX_QT_CBF", 2), "cbf_chroma": _init_slice("CTX_QT_CBF", 5, 5),
    "tskip": _init_slice("CTX_TSKIP", 2),
    "last_x": _init_slice("CTX_LAST_X", 15) + _init_slice("CTX_LAST_X", 3, 15), "last_y": _init_slice("CTX_LAST_Y", 15) + _init_slice("CTX_LAST_Y", 3, 15),
    "csbf": _init_slice("CTX_SIG_CG", 4),
    "sig": _init_slice("CTX_SIG", 27) + _init_slice("CTX_SIG", 15, 28),
    "greater1": _init_slice("CTX_ONE", 24), "greater2": _init_slice("CTX_ABS", 6),
}
CTX_BASE = {}
_n = 0
for _k, _v in INIT_VALUES.items():
    CTX_BASE[_k] = _n
    _n += len(_v)
NUM_CTX = _n


# ---- 6.5.3 - 6.5.5: the scans, generated ------------------------------------------------------------------------------------------------------------
def _diag_scan(blk):
    out, x, y, stop = [], 0, 0, False
    while not stop:
        while y >= 0:
            if x < blk and y < blk:
                out.append((x, y))
            y -= 1
            x += 1
        y, x = x, 0
        if len(out) >= blk * blk:
            stop = True
    return out


def _hor_scan(blk):
    return [(x, y) for y in range(blk) for x in range(blk)]


def _ver_scan(blk):
    return [(x, y) for x in range(blk) for y in range(blk)]


# SCAN_ORDER[log2BlockSize][scanIdx] -> [(x, y)]; scanIdx 0 up-right diagonal, 1 horizontal, 2 vertical (7.4.9.11)
SCAN_ORDER = [[f(1 << l2) for f in (_diag_scan, _hor_scan, _ver_scan)] for l2 in range(4)]


def scan_idx_of(log2_size, c_idx, pred_mode):
    """7.4.9.11 (ChromaArrayType 1): the scan of a transform block of an intra CU."""
    if log2_size == 2 or (log2_size == 3 and c_idx == 0):
        if 6 <= pred_mode <= 14:
            return 2
        if 22 <= pred_mode <= 30:
            return 1
    return 0


def block_scan(log2_size, scan_idx):
    """The (x, y) positions of a transform block in coding order reversed (sub-block by sub-block, first position first), as residual_coding walks them."""
    sub = SCAN_ORDER[log2_size - 2][scan_idx]
    pos = SCAN_ORDER[2][scan_idx]
    return [[((xs << 2) + px, (ys << 2) + py) for px, py in pos] for xs, ys in sub]


# ---- 6.5.1, 6.5.2: tile scan and z-order -----------------------------------------------------------------------------------------------------------
class Geometry:
    """Picture geometry for CtbLog2SizeY 6, MinTbLog2SizeY 2: CtbAddrRsToTs, TileId (per raster address here), MinTbAddrZs."""

    def __init__(self, width, height, col_bd, row_bd, ctb_log2=6, min_tb_log2=2):
        self.w, self.h, self.ctb_log2, self.min_tb_log2 = width, height, ctb_log2, min_tb_log2
        ctb = 1 << ctb_log2
        self.wc, self.hc = (width + ctb - 1) >> ctb_log2, (height + ctb - 1) >> ctb_log2
        self.col_bd, self.row_bd = list(col_bd), list(row_bd)
        if self.col_bd[0] != 0 or self.col_bd[-1] != self.wc or self.row_bd[0] != 0 or self.row_bd[-1] != self.hc:
            raise SliceError("tile boundaries do not cover the picture")
        n = self.wc * self.hc
        self.rs2ts, self.ts2rs, self.tile_id_rs = [0] * n, [0] * n, [0] * n
        for rs in range(n):                                               # (6-4)
            tbx, tby = rs % self.wc, rs // self.wc
            tx = max(i for i in range(len(self.col_bd) - 1) if tbx >= self.col_bd[i])
            ty = max(j for j in range(len(self.row_bd) - 1) if tby >= self.row_bd[j])
            v = 0
            for i in range(tx):
                v += (self.row_bd[ty + 1] - self.row_bd[ty]) * (self.col_bd[i + 1] - self.col_bd[i])
            for j in range(ty):
                v += self.wc * (self.row_bd[j + 1] - self.row_bd[j])
            v += (tby - self.row_bd[ty]) * (self.col_bd[tx + 1] - self.col_bd[tx]) + tbx - self.col_bd[tx]
            self.rs2ts[rs] = v
            self.ts2rs[v] = rs
            self.tile_id_rs[rs] = ty * (len(self.col_bd) - 1) + tx
        self.slice_addr_rs = [0] * n                                      # SliceAddrRs of every CTB decoded so far (7.4.7.1); one slice: 0 everywhere
        self.slice_term = True                                            # False: a test's mutant of 6.4.1 that forgets the slice
        d = ctb_log2 - min_tb_log2
        self.w4, self.h4 = self.wc << d, self.hc << d
        self.zs = [[0] * self.w4 for _ in range(self.h4)]                 # MinTbAddrZs[y][x] (6-10)
        for y in range(self.h4):
            for x in range(self.w4):
                v = self.rs2ts[self.wc * (y >> d) + (x >> d)] << (2 * d)
                for i in range(d):
                    m = 1 << i
                    v += (m * m if m & x else 0) + (2 * m * m if m & y else 0)
                self.zs[y][x] = v

    def available(self, xc, yc, xn, yn):
        """6.4.1: 0 unavailable, 1 available; the reason of a refusal is in self.why ('picture', 'order', 'tile', 'slice'; a neighbour in another tile AND another
        slice says 'tile'), and self.other_slice says whether the neighbour's SliceAddrRs differs."""
        self.other_slice = False
        if xn < 0 or yn < 0 or xn >= self.w or yn >= self.h:
            self.why = "picture"
            return False
        s = self.min_tb_log2
        if self.zs[yn >> s][xn >> s] > self.zs[yc >> s][xc >> s]:
            self.why = "order"
            return False
        c = self.ctb_log2
        rn, rc = (yn >> c) * self.wc + (xn >> c), (yc >> c) * self.wc + (xc >> c)
        self.other_slice = self.slice_addr_rs[rn] != self.slice_addr_rs[rc]
        if self.tile_id_rs[rn] != self.tile_id_rs[rc]:
            self.why = "tile"
            return False
        if self.other_slice and self.slice_term:
            self.why = "slice"
            return False
        return True


def uniform_bounds(n_tiles, n_ctbs):
    """6.5.1 (uniform_spacing_flag 1): the tile boundaries in CTBs."""
    return [(i * n_ctbs) // n_tiles for i in range(n_tiles + 1)]


# ---- 9.3.4.3: the arithmetic decoding engine -----------------------------------------------------------------------------------------------------------
class Engine:
    def __init__(self, data):
        self.d, self.nbits, self.p = bytes(data), len(data) * 8, 0
        self.range = 510                                                  # 9.3.2.5
        self.offset = self.read(9)
        if self.offset >= 510:
            raise SliceError("ivlOffset 510 / 511 at initialisation")

    def read(self, n):
        p = self.p
        if p + n > self.nbits:
            raise SliceError("read past the end of the sub-stream (bit %d + %d of %d)" % (p, n, self.nbits))
        b0 = p >> 3
        nb = ((p + n + 7) >> 3) - b0
        self.p = p + n
        return (int.from_bytes(self.d[b0:b0 + nb], "big") >> (nb * 8 - (p & 7) - n)) & ((1 << n) - 1)

    def decision(self, st, mps, i):
        """9.3.4.3.2 DecodeDecision on context i of the state lists."""
        s = st[i]
        r = self.range
        lps = RANGE_TAB_LPS[s][(r >> 6) & 3]
        r -= lps
        if self.offset >= r:
            b = 1 - mps[i]
            self.offset -= r
            r = lps
            if s == 0:
                mps[i] = 1 - mps[i]
            st[i] = TRANS_IDX_LPS[s]
        else:
            b = mps[i]
            st[i] = TRANS_IDX_MPS[s]
        if r < 256:                                                       # 9.3.4.3.3 RenormD
            k = 9 - r.bit_length()
            r <<= k
            self.offset = (self.offset << k) | self.read(k)
        self.range = r
        return b

    def bypass(self):
        """9.3.4.3.4 DecodeBypass."""
        self.offset = (self.offset << 1) | self.read(1)
        if self.offset >= self.range:
            self.offset -= self.range
            return 1
        return 0

    def bypass_bits(self, n):
        """n bypass bins, first bin the most significant: n times 9.3.4.3.4 is one division (the offset stays below the range after every bin)."""
        if n == 0:
            return 0
        self.offset = (self.offset << n) | self.read(n)
        v, self.offset = divmod(self.offset, self.range)
        if v >> n:
            raise SliceError("arithmetic decoder out of step")
        return v

    def terminate(self):
        """9.3.4.3.5 DecodeTerminate."""
        self.range -= 2
        if self.offset >= self.range:
            return 1
        if self.range < 256:
            self.range <<= 1
            self.offset = (self.offset << 1) | self.read(1)
        return 0

    def finish(self):
        """After a terminating bin of 1 the engine does no renormalisation: the last bit it has read is the 1 of byte_alignment() /
        rbsp_slice_segment_trailing_bits() (the encoder's flush of 9.3.4.5 puts it there); zeros follow up to the byte boundary, and nothing after that."""
        p = self.p
        if not (self.d[(p - 1) >> 3] >> (7 - ((p - 1) & 7))) & 1:
            raise SliceError("the alignment bit behind the terminating bin is 0")
        while self.p & 7:
            if self.read(1):
                raise SliceError("a byte_alignment() zero bit is 1")
        if self.p != self.nbits:
            raise SliceError("%d bytes left behind byte_alignment()" % ((self.nbits - self.p) >> 3))


def init_contexts(qp):
    """9.3.2.2 for every context of an I slice -> (pStateIdx list, valMps list)."""
    st, mps = [0] * NUM_CTX, [0] * NUM_CTX
    q = min(51, max(0, qp))
    for name, vals in INIT_VALUES.items():
        for k, v in enumerate(vals):
            m, n = (v >> 4) * 5 - 45, ((v & 15) << 3) - 16
            pre = min(126, max(1, ((m * q) >> 4) + n))
            mps[CTX_BASE[name] + k] = 0 if pre <= 63 else 1
            st[CTX_BASE[name] + k] = pre - 64 if pre > 63 else 63 - pre
    return st, mps


def new_tally():
    t = {"rice": [0] * 5, "escape_prefix_max": 0, "escape_suffix_bins_max": 0, "escape_fixed_bits_max": 0, "num_sig_gt8": 0, "sign_hidden": 0, "scan": {},
         "mpm_idx": [0, 0, 0], "rem_mode": 0, "cand_left_other_ctu": 0, "cand_above_other_ctu_row": 0, "cand_tile_edge_left": 0, "cand_tile_edge_above": 0, "cand_picture_edge": 0,
         "chroma_mode": [0] * 5, "chroma_34": 0, "split_ctx_tile_edge": 0, "tskip_present": [0, 0], "tskip_set": [0, 0],
         "sao_merge_left": 0, "sao_merge_up": 0, "sao_merge_left_tile_edge": 0, "sao_merge_up_tile_edge": 0, "sao_band": 0, "sao_edge": 0,
         "sao_band_wrap": 0, "sao_band_position_max": -1, "sao_offset_abs_max": 0, "ctx_sync_from_above": 0, "ctx_init_at_row_start": 0,
         "chroma_4x4_behind_fourth": 0, "substreams": 0, "level_out_of_range": 0,
         # pictures of several slices / slice segments
         "slices": 0, "segments_dependent": 0, "segment_ends_mid_slice": 0, "split_ctx_slice_edge": 0, "sao_merge_up_slice_edge": 0, "sao_merge_left_slice_edge": 0,
         "cand_above_other_slice": 0, "cand_left_other_slice": 0, "ctx_restore_from_previous_segment": 0, "ctx_init_at_segment_start": 0,
         # counted by decode_access_unit (the picture entries leave them 0)
         "entry_points_in_dependent_header": 0, "emulation_bytes_in_multi_nal_picture": 0, "emulation_bytes_under_dependent_entry_points": 0}
    return t


def add_tally(a, b):
    """a += b, field by field (maxima for the *_max fields)."""
    for k, v in b.items():
        if k.endswith("_max"):
            a[k] = max(a[k], v)
        elif isinstance(v, list):
            a[k] = [x + y for x, y in zip(a[k], v)]
        elif isinstance(v, dict):
            for kk, vv in v.items():
                a[k][kk] = a[k].get(kk, 0) + vv
        else:
            a[k] += v
    return a


# ---- the slice data -------------------------------------------------------------------------------------------------------------------------------------
class _Picture:
    """One picture being decoded: sequence / picture parameters, the arrays the semantics keep (CtDepth, IntraPredModeY), the output."""

    def __init__(self, width, height, qp, tools, bit_depth, col_bd, row_bd, wavefront, sao, strict_levels=True, min_cb_log2=3, ctb_log2=6, min_tb_log2=2, max_tb_log2=5, max_th_depth_intra=2,
                 slice_term=True, sao_slice_rule=True, mid_slice_end=True):
        if ctb_log2 != 6 or min_tb_log2 != 2:
            raise SliceError("the record layout is that of 64x64 CTBs and 4x4 minimum transform blocks")
        self.g = Geometry(width, height, col_bd, row_bd, ctb_log2, min_tb_log2)
        self.g.slice_term, self.sao_slice_rule, self.mid_slice_end = bool(slice_term), bool(sao_slice_rule), bool(mid_slice_end)      # False: a test's mutants
        self.w, self.h, self.qp, self.bit_depth = width, height, qp, bit_depth
        self.tskip_enabled, self.sign_hiding = bool(tools & TOOL_TSKIP), bool(tools & TOOL_SIGN_HIDE)
        self.wavefront, self.sao_on, self.strict_levels = bool(wavefront), bool(sao), bool(strict_levels)
        self.min_cb_log2, self.ctb_log2, self.min_tb_log2, self.max_tb_log2, self.max_th_depth_intra = min_cb_log2, ctb_log2, min_tb_log2, max_tb_log2, max_th_depth_intra
        g = self.g
        self.ct_depth = [[-1] * g.w4 for _ in range(g.h4)]
        self.pred_y = [[-1] * g.w4 for _ in range(g.h4)]
        n = g.wc * g.hc
        self.f = {k: np.zeros((n,) + REC_DTYPE[k].shape, np.int64) for k in ("depth", "part_size", "luma_dir", "chroma_dir", "tr_idx", "cbf", "tskip")}
        self.coeff = [[[0] * 4096, [0] * 1024, [0] * 1024] for _ in range(n)]
        self.mask = np.zeros((n, 3, 256), bool)
        self.sao = np.zeros((n, 3), SAO_DTYPE)
        self.tally = new_tally()
        self.e = None
        self.st = self.mps = None

    # -- helpers
    def z_of(self, x, y):
        """(CTB raster address, z-scan index of the 4x4 block inside its CTB) of a luma location: the low bits of MinTbAddrZs (6.5.2)."""
        return (y >> 6) * self.g.wc + (x >> 6), self.g.zs[y >> 2][x >> 2] & 255

    def bin(self, name, inc=0):
        return self.e.decision(self.st, self.mps, CTX_BASE[name] + inc)

    # -- 7.3.8.3
    def sao_syntax(self, rx, ry, rs):
        g, t, p = self.g, self.tally, self.sao[rs]
        merge_left = merge_up = 0
        sl = g.slice_addr_rs
        if rx > 0:                                                        # 7.3.8.3: leftCtbInSliceSeg (SliceAddrRs) and leftCtbInTile
            other = sl[rs] != sl[rs - 1]
            t["sao_merge_left_slice_edge"] += other
            if g.tile_id_rs[rs] != g.tile_id_rs[rs - 1]:
                t["sao_merge_left_tile_edge"] += 1
            elif not (other and self.sao_slice_rule):
                merge_left = self.bin("sao_merge")
        if ry > 0 and not merge_left:
            other = sl[rs] != sl[rs - g.wc]
            t["sao_merge_up_slice_edge"] += other
            if g.tile_id_rs[rs] != g.tile_id_rs[rs - g.wc]:
                t["sao_merge_up_tile_edge"] += 1
            elif not (other and self.sao_slice_rule):
                merge_up = self.bin("sao_merge")
        if merge_left or merge_up:
            t["sao_merge_left" if merge_left else "sao_merge_up"] += 1
            p[0]["mode"], p[0]["type"] = 2, 0 if merge_left else 1
            return
        c_max = (1 << (min(self.bit_depth, 10) - 5)) - 1
        type_idx = eo_class = 0
        for c in range(3):
            if c < 2:                                                     # sao_type_idx_luma / _chroma: TR cMax 2, first bin context coded
                type_idx = 0
                if self.bin("sao_type"):
                    type_idx = 2 if self.e.bypass() else 1
            if type_idx == 0:
                continue
            absv = []
            for _ in range(4):                                            # sao_offset_abs: TR, bypass
                a = 0
                while a < c_max and self.e.bypass():
                    a += 1
                absv.append(a)
            t["sao_offset_abs_max"] = max(t["sao_offset_abs_max"], max(absv))
            p[c]["mode"] = 1
            if type_idx == 1:
                signs = [self.e.bypass() if a else 0 for a in absv]
                band = self.e.bypass_bits(5)
                p[c]["type"], p[c]["aux"] = 4, band
                for k in range(4):                                        # 7.4.9.3.2: bandTable[(k + sao_band_position) & 31] = k + 1
                    p[c]["offset"][(band + k) & 31] = -absv[k] if signs[k] else absv[k]
                t["sao_band"] += 1
                t["sao_band_wrap"] += band + 3 > 31
                t["sao_band_position_max"] = max(t["sao_band_position_max"], band)
            else:
                if c < 2:
                    eo_class = self.e.bypass_bits(2)
                p[c]["type"] = eo_class
                for k, cls in enumerate((0, 1, 3, 4)):                    # edge offsets: the first two are positive, the last two negative (7.4.9.3.2)
                    p[c]["offset"][cls] = absv[k] if k < 2 else -absv[k]
                t["sao_edge"] += 1

    # -- 7.3.8.4
    def coding_quadtree(self, x0, y0, log2, depth):
        size = 1 << log2
        if x0 + size <= self.w and y0 + size <= self.h and log2 > self.min_cb_log2:
            inc = 0
            for xn, yn in ((x0 - 1, y0), (x0, y0 - 1)):                   # 9.3.4.2.2
                if self.g.available(x0, y0, xn, yn):
                    inc += self.ct_depth[yn >> 2][xn >> 2] > depth
                else:
                    if self.g.why == "tile":
                        self.tally["split_ctx_tile_edge"] += 1
                    if self.g.other_slice:
                        self.tally["split_ctx_slice_edge"] += 1
            split = self.bin("split_cu", inc)
        else:
            split = 1 if log2 > self.min_cb_log2 else 0
        if split:
            half = size >> 1
            for k in range(4):
                x1, y1 = x0 + (k & 1) * half, y0 + (k >> 1) * half
                if x1 < self.w and y1 < self.h:
                    self.coding_quadtree(x1, y1, log2 - 1, depth + 1)
        else:
            self.coding_unit(x0, y0, log2, depth)

    # -- 7.3.8.5, 8.4.2, 8.4.3
    def coding_unit(self, x0, y0, log2, depth):
        t = self.tally
        size = 1 << log2
        nxn = 0
        if log2 == self.min_cb_log2 and log2 > self.min_tb_log2:
            nxn = 1 - self.bin("part_mode")
        rs, z0 = self.z_of(x0, y0)
        np_cu = (size >> 2) ** 2
        for y in range(y0 >> 2, (y0 + size) >> 2):
            row = self.ct_depth[y]
            for x in range(x0 >> 2, (x0 + size) >> 2):
                row[x] = depth
        self.f["depth"][rs, z0:z0 + np_cu] = depth
        self.f["part_size"][rs, z0:z0 + np_cu] = 3 if nxn else 0
        pb = size >> 1 if nxn else size
        parts = [(x0 + i, y0 + j) for j in range(0, size, pb) for i in range(0, size, pb)]
        prev = [self.bin("prev_intra") for _ in parts]
        coded = []
        for flag in prev:
            if flag:                                                      # mpm_idx: TR cMax 2, bypass ("0", "10", "11")
                coded.append((1 + self.e.bypass()) if self.e.bypass() else 0)
            else:                                                         # rem_intra_luma_pred_mode: FL 5 bits, bypass
                coded.append(self.e.bypass_bits(5))
        for k, (xp, yp) in enumerate(parts):                              # 8.4.2, in decoding order: a partition's neighbours may be its CU's earlier partitions
            cand_nb = []
            for which, (xn, yn) in enumerate(((xp - 1, yp), (xp, yp - 1))):
                if not self.g.available(xp, yp, xn, yn):
                    cand_nb.append(1)
                    if self.g.why != "slice":
                        t[("cand_tile_edge_above" if which else "cand_tile_edge_left") if self.g.why == "tile" else "cand_picture_edge"] += 1
                    if self.g.other_slice:
                        t["cand_above_other_slice" if which else "cand_left_other_slice"] += 1
                elif which == 1 and yp - 1 < ((yp >> self.ctb_log2) << self.ctb_log2):
                    cand_nb.append(1)
                    t["cand_above_other_ctu_row"] += 1
                else:
                    cand_nb.append(self.pred_y[yn >> 2][xn >> 2])
                    if which == 0 and (xn >> self.ctb_log2) != (xp >> self.ctb_log2):
                        t["cand_left_other_ctu"] += 1
            a, b = cand_nb
            if a == b:
                cand = [0, 1, 26] if a < 2 else [a, 2 + ((a + 29) % 32), 2 + ((a - 2 + 1) % 32)]
            else:
                cand = [a, b, 0 if (a != 0 and b != 0) else (1 if (a != 1 and b != 1) else 26)]
            if prev[k]:
                mode = cand[coded[k]]
                t["mpm_idx"][coded[k]] += 1
            else:
                mode = coded[k]
                for c in sorted(cand):
                    if mode >= c:
                        mode += 1
                t["rem_mode"] += 1
            if mode > 34:
                raise SliceError("IntraPredModeY %d" % mode)
            for y in range(yp >> 2, (yp + pb) >> 2):
                row = self.pred_y[y]
                for x in range(xp >> 2, (xp + pb) >> 2):
                    row[x] = mode
            _, zp = self.z_of(xp, yp)
            self.f["luma_dir"][rs, zp:zp + (pb >> 2) ** 2] = mode
        # intra_chroma_pred_mode: one context-coded bin, then FL 2 bits bypass; 8.4.3 with the mode of the CU's first partition
        icpm = 4
        if self.bin("chroma_pred"):
            icpm = self.e.bypass_bits(2)
        t["chroma_mode"][icpm] += 1
        luma0 = self.pred_y[y0 >> 2][x0 >> 2]
        if icpm == 4:
            mode_c, rec_c = luma0, DM_CHROMA
        else:
            mode_c = (0, 26, 10, 1)[icpm]
            if mode_c == luma0:
                mode_c = 34
                t["chroma_34"] += 1
            rec_c = mode_c
        self.f["chroma_dir"][rs, z0:z0 + np_cu] = rec_c
        self.cu_org, self.cu_parts = (x0, y0), np_cu
        self.cu = {"nxn": nxn, "mode_c": mode_c, "rs": rs, "max_depth": self.max_th_depth_intra + nxn}
        self.cbf_c = {}
        self.transform_tree(x0, y0, x0, y0, log2, 0, 0)

    # -- 7.3.8.8
    def transform_tree(self, x0, y0, xb, yb, log2, depth, blk):
        cu = self.cu
        if log2 <= self.max_tb_log2 and log2 > self.min_tb_log2 and depth < cu["max_depth"] and not (cu["nxn"] and depth == 0):
            split = self.bin("split_transform", 5 - log2)
        else:
            split = 1 if (log2 > self.max_tb_log2 or (cu["nxn"] and depth == 0)) else 0
        rs, z = self.z_of(x0, y0)
        npart = 1 << (2 * (log2 - 2))
        for c in (1, 2):
            if log2 > 2:
                flag = 0
                if depth == 0 or self.cbf_c[(c, xb, yb, depth - 1)]:
                    flag = self.bin("cbf_chroma", depth)
                self.cbf_c[(c, x0, y0, depth)] = flag
                if flag:
                    self.f["cbf"][rs, c, z:z + npart] |= 1 << depth
                    if log2 == 3 and split:                                # the record repeats a 4x4 chroma block's flag at the depth of its four luma blocks
                        self.f["cbf"][rs, c, z:z + npart] |= 1 << (depth + 1)
        if split:
            half = 1 << (log2 - 1)
            for k in range(4):
                self.transform_tree(x0 + (k & 1) * half, y0 + (k >> 1) * half, x0, y0, log2 - 1, depth + 1, k)
            return
        cbf_luma = self.bin("cbf_luma", 1 if depth == 0 else 0)          # an intra CU always carries it
        self.f["tr_idx"][rs, z:z + npart] = depth
        if cbf_luma:                                                      # the record keeps a luma flag at every depth down to the leaf's, over the ancestor's area
            _, zcu = self.z_of(*self.cu_org)
            ncu = self.cu_parts
            for d in range(depth + 1):
                nd = ncu >> (2 * d)
                org = zcu + ((z - zcu) & ~(nd - 1))
                self.f["cbf"][rs, 0, org:org + nd] |= 1 << d
        # 7.3.8.10 (cu_qp_delta_enabled_flag 0, cu_chroma_qp_offset_enabled_flag 0)
        if cbf_luma:
            self.residual_coding(x0, y0, log2, 0, rs, z)
        if log2 > 2:
            for c in (1, 2):
                if self.cbf_c[(c, x0, y0, depth)]:
                    self.residual_coding(x0, y0, log2 - 1, c, rs, z)
        elif blk == 3:
            rs_b, z_b = self.z_of(xb, yb)
            for c in (1, 2):
                if self.cbf_c[(c, xb, yb, depth - 1)]:
                    self.tally["chroma_4x4_behind_fourth"] += 1
                    self.residual_coding(xb, yb, 2, c, rs_b, z_b)

    # -- 7.3.8.11
    def residual_coding(self, x0, y0, log2, c_idx, rs, z):
        e, t, st, mps = self.e, self.tally, self.st, self.mps
        ch = 1 if c_idx else 0
        if self.tskip_enabled and log2 <= 2:
            flag = self.bin("tskip", ch)
            self.f["tskip"][rs, c_idx, z] = flag
            self.mask[rs, c_idx, z] = True
            t["tskip_present"][ch] += 1
            t["tskip_set"][ch] += flag
        # last_sig_coeff_{x,y}_prefix: TR cMax (log2 << 1) - 1, 9.3.4.2.3; suffix FL, bypass
        if ch:
            off, shift = 15, log2 - 2
        else:
            off, shift = 3 * (log2 - 2) + ((log2 - 1) >> 2), (log2 + 1) >> 2
        c_max = (log2 << 1) - 1
        pre = []
        for name in ("last_x", "last_y"):
            v = 0
            while v < c_max and e.decision(st, mps, CTX_BASE[name] + off + (v >> shift)):
                v += 1
            pre.append(v)
        last = []
        for v in pre:
            if v > 3:
                nb = (v >> 1) - 1
                v = (1 << nb) * (2 + (v & 1)) + e.bypass_bits(nb)
            last.append(v)
        pred = self.pred_y[y0 >> 2][x0 >> 2] if c_idx == 0 else self.cu["mode_c"]
        scan_idx = scan_idx_of(log2, c_idx, pred)
        key = ("chroma" if ch else "luma", 1 << log2, ("diag", "hor", "ver")[scan_idx])
        t["scan"][key] = t["scan"].get(key, 0) + 1
        lx, ly = (last[1], last[0]) if scan_idx == 2 else (last[0], last[1])
        size = 1 << log2
        if lx >= size or ly >= size:
            raise SliceError("last significant position outside the block")
        sub_scan = SCAN_ORDER[log2 - 2][scan_idx]
        pos_scan = SCAN_ORDER[2][scan_idx]
        last_sub = last_pos = None
        for i, (xs, ys) in enumerate(sub_scan):
            if xs == lx >> 2 and ys == ly >> 2:
                last_sub = i
        for n, (px, py) in enumerate(pos_scan):
            if px == lx & 3 and py == ly & 3:
                last_pos = n
        wsb = size >> 2
        csbf = [[0] * (wsb + 1) for _ in range(wsb + 1)]
        plane = self.coeff[rs][c_idx]
        base = z * (4 if ch else 16)
        sig_base, g1_base, g2_base = CTX_BASE["sig"] + (27 if ch else 0), CTX_BASE["greater1"] + (16 if ch else 0), CTX_BASE["greater2"] + (4 if ch else 0)
        prev_g1ctx = 1                                                    # lastGreater1Ctx of 9.3.4.2.6 for the first sub-block
        for i in range(last_sub, -1, -1):
            xs, ys = sub_scan[i]
            infer_dc = 0
            right, below = csbf[ys][xs + 1], csbf[ys + 1][xs]
            if i < last_sub and i > 0:
                coded_sb = e.decision(st, mps, CTX_BASE["csbf"] + min(right + below, 1) + (2 if ch else 0))
                infer_dc = 1
            else:
                coded_sb = 1
            csbf[ys][xs] = coded_sb
            sig = [0] * 16
            start = 15
            if i == last_sub:
                sig[last_pos] = 1
                start = last_pos - 1
            if coded_sb:
                prev_csbf = right + (below << 1)
                for n in range(start, -1, -1):
                    if n > 0 or not infer_dc:
                        px, py = pos_scan[n]
                        xc, yc = (xs << 2) + px, (ys << 2) + py
                        if log2 == 2:                                     # 9.3.4.2.5
                            sc = CTX_IDX_MAP[(yc << 2) + xc]
                        elif xc + yc == 0:
                            sc = 0
                        else:
                            if prev_csbf == 0:
                                sc = 2 if px + py == 0 else (1 if px + py < 3 else 0)
                            elif prev_csbf == 1:
                                sc = 2 if py == 0 else (1 if py == 1 else 0)
                            elif prev_csbf == 2:
                                sc = 2 if px == 0 else (1 if px == 1 else 0)
                            else:
                                sc = 2
                            if not ch:
                                if xs > 0 or ys > 0:
                                    sc += 3
                                sc += (9 if scan_idx == 0 else 15) if log2 == 3 else 21
                            else:
                                sc += 9 if log2 == 3 else 12
                        sig[n] = e.decision(st, mps, sig_base + sc)
                        if sig[n]:
                            infer_dc = 0
                    else:
                        sig[n] = 1                                        # the sub-block's only possible coefficient: inferred
            positions = [n for n in range(15, -1, -1) if sig[n]]
            if not positions:
                continue
            # coeff_abs_level_greater1_flag (at most 8), 9.3.4.2.6
            ctx_set = 0 if (i == 0 or ch) else 2
            if prev_g1ctx == 0:
                ctx_set += 1
            g1ctx = 1
            g1, g2 = {}, {}
            last_g1_pos = -1
            for n in positions[:8]:
                flag = e.decision(st, mps, g1_base + ctx_set * 4 + min(3, g1ctx))
                g1[n] = flag
                if g1ctx > 0:
                    g1ctx = 0 if flag else g1ctx + 1
                if flag and last_g1_pos == -1:
                    last_g1_pos = n
            prev_g1ctx = g1ctx
            if last_g1_pos != -1:
                g2[last_g1_pos] = e.decision(st, mps, g2_base + ctx_set)
            first_sig, last_sig = positions[-1], positions[0]
            hidden = self.sign_hiding and last_sig - first_sig > 3
            n_signs = len(positions) - (1 if hidden else 0)
            sign_bits = e.bypass_bits(n_signs)
            if len(positions) > 8:
                t["num_sig_gt8"] += 1
            if hidden:
                t["sign_hidden"] += 1
            rice = 0
            sum_abs = 0
            for k, n in enumerate(positions):
                base_level = 1 + g1.get(n, 0) + g2.get(n, 0)
                level = base_level
                if base_level == ((3 if n == last_g1_pos else 2) if k < 8 else 1):
                    t["rice"][rice] += 1                                  # coeff_abs_level_remaining, 9.3.3.11: TR prefix (cMax 4 << rice), EG(rice + 1) suffix
                    q = 0
                    while q < 4 and e.bypass():
                        q += 1
                    if q < 4:
                        rem = (q << rice) + e.bypass_bits(rice)
                        t["escape_prefix_max"] = max(t["escape_prefix_max"], q)
                    else:
                        kk = rice + 1
                        extra = 0
                        ones = 0
                        while e.bypass():
                            extra += 1 << kk
                            kk += 1
                            ones += 1
                            if ones > 28:
                                raise SliceError("coeff_abs_level_remaining prefix longer than 32 bins")
                        rem = (4 << rice) + extra + e.bypass_bits(kk)
                        t["escape_prefix_max"] = max(t["escape_prefix_max"], 4 + ones)
                        t["escape_suffix_bins_max"] = max(t["escape_suffix_bins_max"], ones + 1 + kk)      # the EGk bin string of 9.3.3.11
                        t["escape_fixed_bits_max"] = max(t["escape_fixed_bits_max"], kk)                    # its fixed-length tail
                    level = base_level + rem
                    if level > 3 * (1 << rice):
                        rice = min(rice + 1, 4)
                if k < n_signs:
                    neg = (sign_bits >> (n_signs - 1 - k)) & 1
                else:
                    neg = 0
                value = -level if neg else level
                if hidden:
                    sum_abs += level
                    if n == first_sig and sum_abs & 1:
                        value = -value
                if not -32768 <= value <= 32767:                          # 7.4.9.11: a conforming stream keeps TransCoeffLevel within 16 bits
                    if self.strict_levels:
                        raise SliceError("TransCoeffLevel %d outside 16 bits" % value)
                    t["level_out_of_range"] += 1
                    value = ((value + 32768) & 0xffff) - 32768
                px, py = pos_scan[n]
                plane[base + ((ys << 2) + py) * size + (xs << 2) + px] = value

    # -- 7.3.8.1, 7.3.8.2, 9.3.1, 9.3.2
    def slice_segment_data(self, segments):
        """segments: [(slice_segment_address, dependent_slice_segment_flag, [sub-streams])] in the order of their NAL units.  A segment runs from its address, in tile
        scan, up to the CTB whose end_of_slice_segment_flag is 1; the next segment's address must be the CTB behind that one, and the last one must end the picture."""
        g, t = self.g, self.tally
        n_ctb = g.wc * g.hc
        stored_wpp = stored_ds = None
        ts = 0
        slice_addr = None
        for si, (address, dependent, substreams) in enumerate(segments):
            if not 0 <= address < n_ctb:
                raise SliceError("slice_segment_address %d in a picture of %d CTBs" % (address, n_ctb))
            if ts >= n_ctb:
                raise SliceError("a slice segment behind the picture's last CTB")
            if address != g.ts2rs[ts]:
                raise SliceError("slice_segment_address %d, the CTB behind the segment before it is %d" % (address, g.ts2rs[ts]))
            if dependent:
                if slice_addr is None:
                    raise SliceError("a dependent slice segment opens the picture")
                t["segments_dependent"] += 1
            else:
                slice_addr = address                                      # SliceAddrRs (7.4.7.1)
                t["slices"] += 1
            if not substreams:
                raise SliceError("a slice segment without data")
            # the segment's last CTB, as its neighbours say: the CTB before the next segment's address, or the picture's last
            if si + 1 < len(segments):
                nxt_addr = segments[si + 1][0]
                if not 0 <= nxt_addr < n_ctb:
                    raise SliceError("slice_segment_address %d in a picture of %d CTBs" % (nxt_addr, n_ctb))
                last_ts = g.rs2ts[nxt_addr] - 1
                ends_mid_slice = bool(segments[si + 1][1])
            else:
                last_ts, ends_mid_slice = n_ctb - 1, False
            if last_ts < ts:
                raise SliceError("slice_segment_address %d does not lie behind segment %d" % (segments[si + 1][0], si))
            k = 0
            first_ts = ts
            while True:
                rs = g.ts2rs[ts]
                rx, ry = rs % g.wc, rs // g.wc
                x0, y0 = rx << 6, ry << 6
                g.slice_addr_rs[rs] = slice_addr
                new_tile = ts == 0 or g.tile_id_rs[rs] != g.tile_id_rs[g.ts2rs[ts - 1]]
                new_row = self.wavefront and rs % g.wc == 0
                if ts == first_ts or new_tile or new_row:                 # 9.3.1: the arithmetic decoder starts at the segment's data and behind every byte_alignment()
                    if ts != first_ts:
                        k += 1
                    if k >= len(substreams):
                        raise SliceError("segment %d: %d sub-streams, more are needed" % (si, len(substreams)))
                    self.e = Engine(substreams[k])
                    t["substreams"] += 1
                # 9.3.1, the context variables at the start of a CTU, in the order of the text
                if new_tile:
                    self.st, self.mps = init_contexts(self.qp)
                elif new_row:                                             # the spatial neighbour T (x0 + CtbSizeY, y0 - CtbSizeY) decides
                    if g.available(x0, y0, x0 + 64, y0 - 64):
                        self.st, self.mps = list(stored_wpp[0]), list(stored_wpp[1])
                        t["ctx_sync_from_above"] += 1
                    else:
                        self.st, self.mps = init_contexts(self.qp)
                        t["ctx_init_at_row_start"] += 1
                elif ts == first_ts and dependent:                        # TableStateIdxDs, stored at the end of the segment before (9.3.2.2)
                    self.st, self.mps = list(stored_ds[0]), list(stored_ds[1])
                    t["ctx_restore_from_previous_segment"] += 1
                elif ts == first_ts:
                    self.st, self.mps = init_contexts(self.qp)
                    t["ctx_init_at_segment_start"] += 1
                if self.sao_on:
                    self.sao_syntax(rx, ry, rs)
                self.coding_quadtree(x0, y0, 6, 0)
                end = self.e.terminate()                                  # end_of_slice_segment_flag
                want_end = ts == last_ts
                if want_end and ends_mid_slice and not self.mid_slice_end:
                    want_end = False                                      # a test's mutant: a border between two segments of a slice is taken for no border
                if end != (1 if want_end else 0):
                    raise SliceError("end_of_slice_segment_flag %d behind CTU %d of %d (segment %d ends behind CTU %d)" % (end, ts + 1, n_ctb, si, last_ts + 1))
                if self.wavefront and rs % g.wc == 1:                     # 9.3.2.2 storage: behind the second CTB of a row (one tile with wavefront here)
                    stored_wpp = (list(self.st), list(self.mps))
                ts += 1
                if end:
                    stored_ds = (list(self.st), list(self.mps))           # 9.3.2.2: at the end of the slice segment data (dependent_slice_segments_enabled_flag)
                    self.e.finish()                                       # rbsp_slice_segment_trailing_bits()
                    t["segment_ends_mid_slice"] += ends_mid_slice
                    break
                if ts >= n_ctb:
                    raise SliceError("no end_of_slice_segment_flag behind the picture's last CTU")
                nxt = g.ts2rs[ts]
                if g.tile_id_rs[nxt] != g.tile_id_rs[rs] or (self.wavefront and nxt % g.wc == 0):
                    if self.e.terminate() != 1:                           # end_of_subset_one_bit
                        raise SliceError("end_of_subset_one_bit is 0")
                    self.e.finish()                                       # byte_alignment()
                if ts - 1 == last_ts:                                     # (the mutant only) go on in the next segment's data
                    break
            if k + 1 != len(substreams):
                raise SliceError("segment %d: %d sub-streams, %d were used" % (si, len(substreams), k + 1))
        if ts != n_ctb:
            raise SliceError("the last slice segment ends behind CTU %d of %d" % (ts, n_ctb))

    def records(self):
        n = self.g.wc * self.g.hc
        recs = np.zeros(n, REC_DTYPE)
        for k, v in self.f.items():
            recs[k] = v
        for a in range(n):
            recs["coeff_y"][a], recs["coeff_cb"][a], recs["coeff_cr"][a] = self.coeff[a]
        return recs


def decode_picture(substreams, width, height, qp, tools, bit_depth=8, col_bd=None, row_bd=None, wavefront=False, sao=False, strict_levels=True, **sps):
    """The slice data of one picture of ONE slice segment from its sub-streams (one per tile in raster order of the tile grid, or one per CTU row with wavefront,
    otherwise one).  col_bd / row_bd: tile boundaries in CTUs including 0 and the picture's size (None: one tile).  tools: HEVCDL_TOOL_* bits (transform skip, sign
    hiding).  -> (records [ctus] in REC_DTYPE layout, SAO parameters [ctus, 3] in SAO_DTYPE layout or None, mask [ctus, 3, 256] of the tskip entries whose flag was in
    the stream, tally).  strict_levels False: a level outside 16 bits (a stream no conforming encoder writes) is counted in the tally and kept modulo 2^16."""
    return decode_picture_segments([(0, 0, substreams)], width, height, qp, tools, bit_depth, col_bd, row_bd, wavefront, sao, strict_levels, **sps)


def decode_picture_segments(segments, width, height, qp, tools, bit_depth=8, col_bd=None, row_bd=None, wavefront=False, sao=False, strict_levels=True,
                            slice_term=True, sao_slice_rule=True, mid_slice_end=True, **sps):
    """The slice data of one picture of several slices and slice segments.  segments: [(slice_segment_address, dependent_slice_segment_flag, [sub-streams])] in
    decoding order -- what the headers of the picture's slice NAL units say and what their entry points cut, or the same said about a coder's buffer.  col_bd /
    row_bd are the PPS's tiles: a picture cut into slices of CTU rows has one tile.  QP, SAO and the tool bits are the picture's (every independent header repeats them).
    slice_term / sao_slice_rule / mid_slice_end False: TEST-ONLY mutants (the slice term of 6.4.1 forgotten; SAO merge candidates taken across a slice border; a
    border between two segments of one slice taken for none) that a corpus must catch.  -> what decode_picture returns."""
    wc, hc = (width + 63) >> 6, (height + 63) >> 6
    pic = _Picture(width, height, qp, tools, bit_depth, col_bd or [0, wc], row_bd or [0, hc], wavefront, sao, strict_levels,
                   slice_term=slice_term, sao_slice_rule=sao_slice_rule, mid_slice_end=mid_slice_end, **sps)
    if wavefront and (len(pic.g.col_bd) > 2 or len(pic.g.row_bd) > 2):
        raise SliceError("wavefront together with tiles is outside this decoder")
    try:
        pic.slice_segment_data([(int(a), int(d), [bytes(b) for b in subs]) for a, d, subs in segments])
    except (IndexError, KeyError, TypeError) as e:                        # a damaged stream may lead outside the picture's arrays: the same refusal
        raise SliceError("syntax leads outside the picture: %r" % (e,))
    return pic.records(), (pic.sao if sao else None), pic.mask, pic.tally


# ---- a whole access unit ------------------------------------------------------------------------------------------------------------------------------
def unescape_with_positions(nal):
    """7.4.2 / 7.3.1.1: drop every emulation_prevention_three_byte -> (RBSP-side bytes incl. the NAL header, position of each kept byte in the NAL)."""
    out, pos, zeros = bytearray(), [], 0
    for i, b in enumerate(nal):
        if zeros >= 2 and b == 3:
            zeros = 0
            continue
        out.append(b)
        pos.append(i)
        zeros = zeros + 1 if b == 0 else 0
    return bytes(out), pos


def cut_substreams(nal, hdr):
    """One slice NAL unit and its parsed header -> (sub-streams without their emulation prevention bytes, payload bytes, emulation prevention bytes per sub-stream).
    The entry points count the bytes of the slice segment data WITH its emulation prevention bytes (7.4.7.1): sub-stream k is the bytes [sum of the offsets before
    k, + offset k) of the NAL's payload behind the header, the last one takes the rest, and no offset may reach past it."""
    rbsp, pos = unescape_with_positions(nal)
    if hdr["data_byte_pos"] >= len(pos):
        raise SliceError("a slice NAL unit without slice segment data")
    first = pos[hdr["data_byte_pos"]]                                     # the first byte of slice_segment_data() in the NAL
    payload = len(nal) - first
    offs = hdr["entry_points"]
    if sum(offs) >= payload:
        raise SliceError("entry points add up to %d bytes, the slice data has %d" % (sum(offs), payload))
    cuts = [first]
    for o in offs:
        cuts.append(cuts[-1] + o)
    cuts.append(len(nal))
    at = [bisect.bisect_left(pos, c) for c in cuts]                       # an emulation prevention byte belongs to the sub-stream it lies in and is dropped there
    subs = [rbsp[at[k]:at[k + 1]] for k in range(len(cuts) - 1)]
    emu = [(cuts[k + 1] - cuts[k]) - len(subs[k]) for k in range(len(subs))]
    return subs, payload, emu


def decode_access_unit(au, strict_levels=True, picture_decoder=None, segments_decoder=None, **mutants):
    """One access unit (Annex B: VPS, SPS, PPS, the picture's slice NAL units in order) -> what decode_picture returns, plus a dict of what the headers said.  Every
    NAL unit's sub-streams are cut at its own header's entry points against its own payload (cut_substreams).  Demanded of the headers, by SliceError: the first has
    first_slice_segment_in_pic_flag 1 and the others 0; every independent header of the picture carries the same QP, SAO flags and deblocking fields; and, by
    slice_segment_data, that every slice_segment_address is the CTB behind the last CTB of the segment before it and the last segment ends the picture.
    picture_decoder: a stand-in for decode_picture with its signature, used for a picture of one segment; segments_decoder: one for decode_picture_segments (a test's
    cache around each).  mutants: decode_picture_segments' test-only switches."""
    import hevc_parse as hp
    nals = [n for _, n in hp.split_annexb(au)]
    ps = {}
    for n in nals:
        ps.setdefault((n[0] >> 1) & 63, n)
    if 33 not in ps or 34 not in ps:
        raise SliceError("no SPS / PPS in the access unit")
    sps, pps = hp.parse_sps(ps[33]), hp.parse_pps(ps[34])
    slices = [n for n in nals if ((n[0] >> 1) & 63) < 32]
    if not slices:
        raise SliceError("no slice NAL unit in the access unit")
    if pps["cu_qp_delta"] or pps["tq_bypass"] or sps["pcm"] or sps["scaling_list"] or pps["scaling_list"] or sps["chroma_format"] != 1:
        raise SliceError("a syntax switch outside this decoder is on")
    w, h = sps["width"], sps["height"]
    ctb_log2 = sps["log2_min_cb_m3"] + 3 + sps["log2_diff_cb"]
    wc, hc = (w + (1 << ctb_log2) - 1) >> ctb_log2, (h + (1 << ctb_log2) - 1) >> ctb_log2
    col_bd, row_bd = [0, wc], [0, hc]
    if pps["tiles_enabled"]:
        if pps["uniform_spacing"]:
            col_bd, row_bd = uniform_bounds(pps["tile_columns"], wc), uniform_bounds(pps["tile_rows"], hc)
        else:
            col_bd = [sum(pps["column_widths"][:i]) for i in range(pps["tile_columns"])] + [wc]
            row_bd = [sum(pps["row_heights"][:i]) for i in range(pps["tile_rows"])] + [hc]
    segs, segments, first_hdr = [], [], None
    for i, nal in enumerate(slices):
        try:
            hdr, _ = hp.parse_slice_header(nal, sps, pps)
        except (AssertionError, IndexError) as e:
            raise SliceError("slice segment header %d: %r" % (i, e))
        if hdr["first_slice"] != (1 if i == 0 else 0):
            raise SliceError("first_slice_segment_in_pic_flag %d in slice NAL unit %d of the access unit" % (hdr["first_slice"], i))
        if not hdr["dependent"]:
            if sps["sao"] and hdr["sao_luma"] != hdr["sao_chroma"]:
                raise SliceError("SAO for one of luma / chroma only is outside this decoder")
            same = ("qp_delta", "sao_luma", "sao_chroma", "dbk_override_flag", "dbk_disabled", "beta_div2", "tc_div2", "slice_lf_across_slices")
            if first_hdr is None:
                first_hdr = hdr
            elif any(hdr.get(k) != first_hdr.get(k) for k in same):
                raise SliceError("the independent slice segment headers of the picture differ in %s" % [k for k in same if hdr.get(k) != first_hdr.get(k)])
        subs, payload, emu = cut_substreams(nal, hdr)
        segs.append({"first_slice": hdr["first_slice"], "dependent": hdr["dependent"], "address": hdr["address"], "entry_points": list(hdr["entry_points"]),
                     "offset_len_minus1": hdr.get("offset_len_minus1"), "substreams": subs, "payload_bytes": payload, "nal_bytes": len(nal), "emulation": emu, "header": hdr})
        segments.append((hdr["address"], hdr["dependent"], subs))
    qp = 26 + pps["init_qp_m26"] + first_hdr["qp_delta"]
    tools = (TOOL_TSKIP if pps["tskip"] else 0) | (TOOL_SIGN_HIDE if pps["sign_hiding"] else 0)
    bd = 8 + sps["bd_luma_m8"]
    sao = bool(sps["sao"] and first_hdr.get("sao_luma"))
    kw = dict(strict_levels=strict_levels, min_cb_log2=sps["log2_min_cb_m3"] + 3, ctb_log2=ctb_log2, min_tb_log2=sps["log2_min_tb_m2"] + 2,
              max_tb_log2=sps["log2_min_tb_m2"] + 2 + sps["log2_diff_tb"], max_th_depth_intra=sps["tu_depth_intra"])
    if len(segments) == 1 and not mutants:
        out = (picture_decoder or decode_picture)(segments[0][2], w, h, qp, tools, bd, col_bd, row_bd, bool(pps["wpp"]), sao, **kw)
    else:
        kw.update(mutants)
        out = (segments_decoder or decode_picture_segments)(segments, w, h, qp, tools, bd, col_bd, row_bd, bool(pps["wpp"]), sao, **kw)
    tally = dict(out[3])                                                  # (a cached result stays as it is)
    tally["entry_points_in_dependent_header"] = sum(len(g["entry_points"]) for g in segs if g["dependent"])
    tally["emulation_bytes_in_multi_nal_picture"] = sum(sum(g["emulation"]) for g in segs) if len(segs) > 1 else 0
    tally["emulation_bytes_under_dependent_entry_points"] = sum(sum(g["emulation"][:len(g["entry_points"])]) for g in segs if g["dependent"])
    info = {"width": w, "height": h, "qp": qp, "tools": tools, "bit_depth": bd, "col_bd": col_bd, "row_bd": row_bd, "wavefront": bool(pps["wpp"]), "sao": sao,
            "entry_points": list(segs[0]["entry_points"]), "substreams": [b for g in segs for b in g["substreams"]], "payload_bytes": segs[0]["payload_bytes"],
            "segments": segs, "dep_slices": bool(pps["dep_slices"]), "lf_across_slices": bool(pps["lf_across_slices"]),
            "dbk": (first_hdr.get("dbk_override_flag", 0), first_hdr["dbk_disabled"], first_hdr["beta_div2"], first_hdr["tc_div2"])}
    return out[:3] + (tally, info)
