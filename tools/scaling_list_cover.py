"""tools/scaling_list_cover.py -- TEST INFRASTRUCTURE.  What a parsed stream (hevcdl_amd.parse_stream(scaling_lists=True)) reaches of the scaling-list dequantisation,
computed from the parser's records, QP map and factor block alone: the table of tools/gen_scaling_list_fixtures.py and of tests/test_scaling_lists.py.

Per plane kind (Y4 Y8 Y16 Y32 C4 C8 C16; C counts Cb and Cr):
  nz_*     non-zero levels at positions whose factor is not 16
  dc_*     non-zero DC levels of 16x16 / 32x32 blocks whose DC factor differs from its list's first entry (the factor at (1, 0): the list's first entry repeated)
  ts_luma / ts_chroma   transform-skipped 4x4 blocks with a non-zero level at a non-16 factor
  clip     dequantised values that reach the 16-bit clip (8.6.4.2: level * factor * levelScale[qP % 6] << (qP / 6), rounded, >> bdShift)

with_scaling_lists(): test-side SPS syntax -- a stream of this library's writer (scaling_list_enabled_flag 0) with its SPS rewritten to carry scaling_list_data(), for
tools/time_decode.py; the slice data stays what it was, so the pictures such a stream decodes to are not the encoder's."""
import numpy as np

KINDS = ["Y4", "Y8", "Y16", "Y32", "C4", "C8", "C16"]
FIELDS = ["nz_" + k for k in KINDS] + ["dc_Y16", "dc_Y32", "dc_C16", "ts_luma", "ts_chroma", "clip"]
PLANE_OFFSET = {(0, 2): 0, (0, 3): 16, (0, 4): 80, (0, 5): 336, (1, 2): 1360, (1, 3): 1376, (1, 4): 1440, (2, 2): 1696, (2, 3): 1712, (2, 4): 1776}
LEVEL_SCALE = (40, 45, 51, 57, 64, 72)
CHROMA_QP = (29, 30, 31, 32, 33, 33, 34, 34, 35, 35, 36, 36, 37, 37)


def chroma_qp(qpi):
    return qpi if qpi < 30 else (qpi - 6 if qpi >= 43 else CHROMA_QP[qpi - 30])


def _z_xy(z):
    x = y = 0
    for b in range(4):
        x |= ((z >> (2 * b)) & 1) << b
        y |= ((z >> (2 * b + 1)) & 1) << b
    return x, y


def blocks_of(rec, w, h, x0, y0):
    """The transform blocks of one CTU record in coding order -> (comp, z, log2n, tskip, levels [n * n] raster)."""
    z = 0
    while z < 256:
        zx, zy = _z_xy(z)
        if x0 + 4 * zx >= w or y0 + 4 * zy >= h:
            z += 1
            continue
        trd = int(rec["tr_idx"][z])
        log2n = min(max(6 - int(rec["depth"][z]) - trd, 2), 5)
        np_ = 1 << (2 * (log2n - 2))
        if (rec["cbf"][0][z] >> trd) & 1:
            yield 0, z, log2n, int(rec["tskip"][0][z]), rec["coeff_y"][16 * z:16 * z + (1 << (2 * log2n))]
        zc = z if log2n > 2 else ((z & ~3) if (z & 3) == 3 else -1)
        if zc >= 0:
            l2c = log2n - 1 if log2n > 2 else 2
            for c in (1, 2):
                if (rec["cbf"][c][zc] >> trd) & 1:
                    yield c, zc, l2c, int(rec["tskip"][c][zc]), rec["coeff_cb" if c == 1 else "coeff_cr"][4 * zc:4 * zc + (1 << (2 * l2c))]
        z += np_


def coverage(p):
    """p: a ParsedStream with records, qp_map, qp_info and scaling_factors -> {field: count}."""
    out = dict.fromkeys(FIELDS, 0)
    w, h, bd = p.cfg.width, p.cfg.height, p.cfg.bit_depth
    cx = (w + 63) // 64
    f = p.scaling_factors.astype(np.int64)
    off = 6 * (bd - 8)
    for pic in range(p.records.shape[0]):
        for a in range(p.records.shape[1]):
            rec = p.records[pic, a]
            for comp, z, log2n, tskip, lvl in blocks_of(rec, w, h, (a % cx) * 64, (a // cx) * 64):
                n = 1 << log2n
                m = f[PLANE_OFFSET[(comp, log2n)]:PLANE_OFFSET[(comp, log2n)] + n * n]
                lv = lvl.astype(np.int64)
                kind = ("C" if comp else "Y") + str(n)
                hit = int(((lv != 0) & (m != 16)).sum())
                out["nz_" + kind] += hit
                if n >= 16 and lv[0] != 0 and m[0] != m[1]:
                    out["dc_" + kind] += 1
                if tskip and n == 4 and hit:
                    out["ts_chroma" if comp else "ts_luma"] += 1
                qpy = int(p.qp_map[pic, a, z])
                qp = qpy + off if comp == 0 else chroma_qp(min(max(qpy + (p.qp_info.cb_qp_offset if comp == 1 else p.qp_info.cr_qp_offset), -off), 57)) + off
                bds = bd + log2n - 5
                d = (lv * m * (LEVEL_SCALE[qp % 6] << (qp // 6)) + (1 << (bds - 1))) >> bds
                out["clip"] += int(((d <= -32768) | (d >= 32767)).sum())
    return out


def _diag(n):
    out, x, y = [], 0, 0
    while len(out) < n * n:
        while y >= 0:
            if x < n and y < n:
                out.append(y * n + x)
            y -= 1
            x += 1
        y, x = x, 0
    return out


def _ue(v):
    return "0" * ((v + 1).bit_length() - 1) + "{:b}".format(v + 1)


def _se(v):
    return _ue(2 * v - 1 if v > 0 else -2 * v)


def scaling_list_data_bits(L):
    """scaling_list_data() of 7.3.4 for the list arrays of a sclist_* fixture (raster order; lists32 [2, 64]: matrixId 0 and 3), every list coded with
    scaling_list_pred_mode_flag 1."""
    out = []
    for size_id, key, n in ((0, "lists4", 4), (1, "lists8", 8), (2, "lists16", 8), (3, "lists32", 8)):
        for m in range(0, 6, 3 if size_id == 3 else 1):
            vals = [int(v) for v in L[key][m // 3 if size_id == 3 else m]]
            out.append("1")
            nxt = 8
            if size_id > 1:
                nxt = int(L["dc32"][m // 3] if size_id == 3 else L["dc16"][m])
                out.append(_se(nxt - 8))
            for i in _diag(n):
                out.append(_se((vals[i] - nxt + 128) % 256 - 128))
                nxt = vals[i]
    return "".join(out)


def with_scaling_lists(stream, L):
    """stream: one of this library's writer (its SPS has scaling_list_enabled_flag 0) -> the stream with scaling_list_enabled_flag 1, sps_scaling_list_data_present_flag 1 and
    the lists of L in every SPS NAL unit."""
    out, at = bytearray(), 0
    while True:
        i = stream.find(b"\x00\x00\x01\x42\x01", at)
        if i < 0:
            return bytes(out) + stream[at:]
        i += 5
        j = stream.index(b"\x00\x00\x01", i)
        while stream[j - 1] == 0:
            j -= 1
        rbsp, zeros = bytearray(), 0
        for x in stream[i:j]:
            if zeros >= 2 and x == 3:
                zeros = 0
                continue
            rbsp.append(x)
            zeros = zeros + 1 if x == 0 else 0
        bits = "".join("{:08b}".format(x) for x in rbsp)
        pos = [104]

        def u(n):
            v = int(bits[pos[0]:pos[0] + n], 2)
            pos[0] += n
            return v

        def ue():
            z = 0
            while u(1) == 0:
                z += 1
            return (1 << z) - 1 + (u(z) if z else 0)
        ue(); ue(); ue(); ue()
        if u(1):
            ue(); ue(); ue(); ue()
        ue(); ue(); ue(); u(1); ue(); ue(); ue()
        for _ in range(6):
            ue()
        assert bits[pos[0]] == "0", "the SPS has scaling lists already"
        end = bits.rindex("1")                                    # rbsp_stop_one_bit
        new = bits[:pos[0]] + "11" + scaling_list_data_bits(L) + bits[pos[0] + 1:end] + "1"
        new += "0" * (-len(new) % 8)
        esc, zeros = bytearray(), 0
        for x in bytes(int(new[k:k + 8], 2) for k in range(0, len(new), 8)):
            if zeros >= 2 and x <= 3:
                esc.append(3)
                zeros = 0
            esc.append(x)
            zeros = zeros + 1 if x == 0 else 0
        out += stream[at:i] + esc
        at = j
