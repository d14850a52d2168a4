"""Source files in 4:0:0, 4:2:2 and 4:4:4, swapped chroma planes, an explicit window, a temporally subsampled read (csrc/source_core.h, the host side).  No GPU needed:
the host functions against a numpy restatement of the reference's file reader in the reference's own order, the argument checks, the frame sizes, and -- for every run
of the reference encoder under tests/golden/srcfmt_*.npz (tools/gen_source_format_fixtures.py) -- the stream, the reconstruction file and the PSNR columns of the log."""
import ctypes
import glob
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import GOLD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = sorted(glob.glob(os.path.join(GOLD, "srcfmt_*.npz")))
OLD_CASES = sorted(glob.glob(os.path.join(GOLD, "source_*.npz")))
FORMATS = (400, 420, 422, 444)
SHIFTS = {400: None, 420: (1, 1), 422: (1, 0), 444: (0, 0)}      # log2 of luma : chroma, horizontally and vertically


def dt(bd):
    return np.uint8 if bd <= 8 else np.dtype("<u2")


def np_scale(v, src_bd, dst_bd):
    """scalePlane (TVideoIOYuv.cpp:70-95) without the Rec.709 clip."""
    v = v.astype(np.int64)
    shift = dst_bd - src_bd
    if shift > 0:
        return v << shift
    if shift < 0:
        return np.clip((v + (1 << (-shift - 1))) >> -shift, 0, (1 << dst_bd) - 1)
    return v


def file_planes(frame, sw, sh, cf):
    """The planes of one source-format frame: Y, then both chroma planes at the file's own chroma size (4:0:0: none)."""
    ps = [frame[:sw * sh].reshape(sh, sw)]
    if cf != 400:
        csx, csy = SHIFTS[cf]
        fw, fh = sw >> csx, sh >> csy
        ps += [frame[sw * sh + k * fw * fh:sw * sh + (k + 1) * fw * fh].reshape(fh, fw) for k in range(2)]
    return ps


def source_samples(sw, sh, cf):
    return sw * sh + (0 if cf == 400 else 2 * (sw >> SHIFTS[cf][0]) * (sh >> SHIFTS[cf][1]))


def read_plane_in_order(plane, dw, dh, lim_w, lim_h, sx, sy):
    """readPlane (TVideoIOYuv.cpp:249-384) in the reference's ORDER: for every destination row inside the source read ONE file row (the odd rows of a vertically
    subsampled plane are skipped), keep every (1 << sx)-th sample of it, replicate the last kept sample into the padding columns; then replicate the last row down."""
    out = np.zeros((dh, dw), np.int64)
    for y in range(lim_h):
        row = plane[y << sy]                         # the file row
        out[y, :lim_w] = row[:lim_w << sx:1 << sx]   # pick
        out[y, lim_w:] = out[y, lim_w - 1]           # replicate columns
    for y in range(lim_h, dh):
        out[y] = out[lim_h - 1]                      # replicate rows (of replicated columns)
    return out


def np_load_in_order(src, sw, sh, cw, ch, cf, swap, in_bd, bd):
    out = []
    for frame in src:
        fp = file_planes(frame, sw, sh, cf)
        ps = [read_plane_in_order(fp[0], cw, ch, sw, sh, 0, 0)]
        for c in (1, 2):
            if cf == 400:
                ps.append(np.full((ch // 2, cw // 2), 1 << (in_bd - 1), np.int64))      # :280-293: the fill value at the file's depth, scaled like any sample
            else:
                csx, csy = SHIFTS[cf]
                ps.append(read_plane_in_order(fp[3 - c if swap else c], cw // 2, ch // 2, sw // 2, sh // 2, 1 - csx, 1 - csy))
        out.append(np.concatenate([np_scale(p, in_bd, bd).ravel() for p in ps]))
    return np.stack(out).astype(dt(bd))


def np_load_per_sample(src, sw, sh, cw, ch, cf, swap, in_bd, bd):
    """coded_c(x, y) = file_c(min(x, sw/2 - 1) << (1 - csx), min(y, sh/2 - 1) << (1 - csy)): the clamp in DESTINATION coordinates."""
    out = []
    for frame in src:
        fp = file_planes(frame, sw, sh, cf)
        ys, xs = np.minimum(np.arange(ch), sh - 1), np.minimum(np.arange(cw), sw - 1)
        ps = [fp[0][np.ix_(ys, xs)]]
        for c in (1, 2):
            if cf == 400:
                ps.append(np.full((ch // 2, cw // 2), 1 << (in_bd - 1)))
            else:
                csx, csy = SHIFTS[cf]
                ys, xs = np.minimum(np.arange(ch // 2), sh // 2 - 1) << (1 - csy), np.minimum(np.arange(cw // 2), sw // 2 - 1) << (1 - csx)
                ps.append(fp[3 - c if swap else c][np.ix_(ys, xs)])
        out.append(np.concatenate([np_scale(p, in_bd, bd).ravel() for p in ps]))
    return np.stack(out).astype(dt(bd))


def coded_planes(frame, w, h):
    return [frame[:w * h].reshape(h, w), frame[w * h:w * h * 5 // 4].reshape(h // 2, w // 2), frame[w * h * 5 // 4:].reshape(h // 2, w // 2)]


def np_store(pics, cw, ch, win, swap, bd, out_bd, sw, sh):
    """write (TVideoIOYuv.cpp:755-830): the window -- the coded picture minus the padding, or the explicit offsets (plane offset (left >> cs) + (top >> cs) * stride,
    :811-826) -- scaled to the output depth; the chroma planes back in the file's order when `swap`."""
    left, right, top, bottom = win
    ww, wh = sw - left - right, sh - top - bottom
    out = []
    for frame in pics:
        ps = coded_planes(frame, cw, ch)
        order = [0, 2, 1] if swap else [0, 1, 2]
        out.append(np.concatenate([np_scale(ps[o][(top >> (c > 0)):(top >> (c > 0)) + (wh >> (c > 0)), (left >> (c > 0)):(left >> (c > 0)) + (ww >> (c > 0))], bd, out_bd).ravel()
                                   for c, o in enumerate(order)]))
    return np.stack(out).astype(dt(out_bd))


def samples(n, bd, seed):
    rng = np.random.default_rng(seed)
    top = (1 << bd) - 1
    v = rng.integers(0, top + 1, n)
    pos = rng.integers(0, n, min(n, 24))
    v[pos] = np.resize(np.array([0, 1, 2, top, top - 1, top - 2, 1 << (bd - 1)]), pos.size)
    return v.astype(dt(bd))


SWEEP = [(w, 48 - w) for w in range(8, 42, 2)]      # 8 x 40 .. 40 x 8


@pytest.mark.parametrize("cf", FORMATS)
def test_host_load_equals_the_reader_in_its_own_order_and_the_per_sample_rule(cf):
    """Sizes 8 .. 40 in steps of 2, depths 8 / 10 / 12 / 16, paddings 0 .. 14 (every value occurs over the sweep, horizontally and vertically), with and without the swap."""
    import hevcdl_amd
    seen_px, seen_py = set(), set()
    for k, (sw, sh) in enumerate(SWEEP):
        for j, in_bd in enumerate((8, 10, 12, 16)):
            bd = (8, 10)[(k + j) & 1]
            px, py = 2 * ((k + 3 * j) % 8), 2 * ((5 * k + j + 1) % 8)
            seen_px.add(px); seen_py.add(py)
            swap = int(cf != 400 and (k + j) % 3 == 0)
            cw, ch = sw + px, sh + py
            src = samples(2 * source_samples(sw, sh, cf), in_bd, 31 * sw + 7 * sh + in_bd + cf).reshape(2, -1)
            a, b = np_load_in_order(src, sw, sh, cw, ch, cf, swap, in_bd, bd), np_load_per_sample(src, sw, sh, cw, ch, cf, swap, in_bd, bd)
            assert np.array_equal(a, b), (sw, sh, cw, ch, in_bd, bd, swap)
            fmt = hevcdl_amd.source_format(sw, sh, in_bd, bd, chroma_format=cf, colour_space=swap)
            got = hevcdl_amd.load_source_host(fmt, cw, ch, bd, src)
            assert got.dtype == dt(bd) and np.array_equal(got, a), (sw, sh, cw, ch, in_bd, bd, swap)
    assert seen_px == seen_py == set(range(0, 16, 2))


def test_padded_444_replicates_file_column_and_row_minus_two():
    """The place that is easiest to get wrong: the clamp acts on the coded coordinate, so the padding of a 4:4:4 file repeats file column sw - 2 and row sh - 2."""
    import hevcdl_amd
    sw, sh, cw, ch = 10, 8, 16, 16
    src = np.zeros(3 * sw * sh, np.uint8)
    cb = src[sw * sh:2 * sw * sh].reshape(sh, sw)
    cb[:] = np.arange(sw)[None, :] + 16 * np.arange(sh)[:, None]
    coded = hevcdl_amd.load_source_host(hevcdl_amd.source_format(sw, sh, 8, 8, chroma_format=444), cw, ch, 8, src[None])[0]
    u = coded[cw * ch:cw * ch * 5 // 4].reshape(ch // 2, cw // 2)
    assert u[0].tolist() == [0, 2, 4, 6, 8, 8, 8, 8] and u[:, 0].tolist() == [0, 32, 64, 96, 96, 96, 96, 96] and u[7, 7] == 96 + 8


@pytest.mark.parametrize("out_bd", (8, 10))
@pytest.mark.parametrize("bd", (8, 10))
def test_host_store_window_and_plane_order(bd, out_bd):
    import hevcdl_amd
    cw, ch = 72, 40
    pics = samples(2 * cw * ch * 3 // 2, bd, 5 * bd + out_bd).reshape(2, -1)
    for win in ((0, 0, 0, 0), (2, 0, 0, 2), (4, 2, 6, 8), (62, 0, 0, 38), (0, 70, 38, 0)):
        for cs, internal in ((0, 0), (1, 0), (1, 1)):
            fmt = hevcdl_amd.source_format(cw, ch, 8, out_bd, colour_space=cs, output_internal_colour_space=internal, conf_win=win)
            out = hevcdl_amd.store_output_host(fmt, cw, ch, bd, pics)
            assert out.dtype == dt(out_bd) and np.array_equal(out, np_store(pics, cw, ch, win, cs and not internal, bd, out_bd, cw, ch)), (win, cs, internal)
    # with padding (modes 1 / 2) the window is the source size, and the planes still change places
    fmt = hevcdl_amd.source_format(66, 34, 8, out_bd, colour_space=1)
    assert np.array_equal(hevcdl_amd.store_output_host(fmt, cw, ch, bd, pics), np_store(pics, cw, ch, (0, 0, 0, 0), True, bd, out_bd, 66, 34))


def test_invalid_combinations_are_invalid_arg():
    import hevcdl_amd
    lib = hevcdl_amd.load_library()
    buf = np.zeros(72 * 48 * 6, np.uint16)
    enc_cases = [
        dict(conf_win=(3, 0, 0, 0)), dict(conf_win=(0, 1, 0, 0)), dict(conf_win=(0, 0, 5, 0)), dict(conf_win=(0, 0, 0, 7)),      # odd offsets
        dict(conf_win=(-2, 0, 0, 0)),
        dict(conf_win=(36, 36, 0, 0)), dict(conf_win=(0, 0, 24, 24)), dict(conf_win=(72, 0, 0, 0)), dict(conf_win=(0, 0, 0, 48)),      # a window of no samples
        dict(colour_space=1, chroma_format=400),                                                                               # nothing to swap
        dict(colour_space=2), dict(colour_space=-1),
        dict(chroma_format=411), dict(chroma_format=1), dict(chroma_format=-420),                                              # an unknown format
    ]
    for kw in enc_cases:
        g = hevcdl_amd.source_format(72, 48, 8, 8, **kw)
        assert lib.hevcdl_load_source_host(ctypes.byref(g), 72, 48, 8, buf.ctypes.data, 1, buf.ctypes.data) == 1, kw
        assert lib.hevcdl_store_output_host(ctypes.byref(g), 72, 48, 8, buf.ctypes.data, 1, buf.ctypes.data) == 1, kw
        assert lib.hevcdl_source_frame_bytes(ctypes.byref(g)) == 0 and lib.hevcdl_output_frame_bytes(ctypes.byref(g)) == 0, kw
    # window offsets together with padding: fine against the source size itself, refused against a larger coded size
    g = hevcdl_amd.source_format(64, 40, 8, 8, conf_win=(2, 0, 0, 2))
    assert lib.hevcdl_source_frame_bytes(ctypes.byref(g)) == 64 * 40 * 3 // 2 and lib.hevcdl_output_frame_bytes(ctypes.byref(g)) == 62 * 38 * 3 // 2
    assert lib.hevcdl_load_source_host(ctypes.byref(g), 64, 40, 8, buf.ctypes.data, 1, buf.ctypes.data) == 0
    for cw, ch in ((72, 40), (64, 48), (72, 48)):
        assert lib.hevcdl_load_source_host(ctypes.byref(g), cw, ch, 8, buf.ctypes.data, 1, buf.ctypes.data) == 1
        assert lib.hevcdl_store_output_host(ctypes.byref(g), cw, ch, 8, buf.ctypes.data, 1, buf.ctypes.data) == 1
    # the stream configuration's window: the same rules
    recs = np.zeros(2, hevcdl_amd.REC_DTYPE)
    recs["luma_dir"][:] = 1; recs["chroma_dir"][:] = 36; recs["tr_idx"][:] = 1
    for cw in ((1, 0, 0, 0), (0, 0, 3, 0), (-2, 0, 0, 0), (36, 36, 0, 0), (0, 0, 40, 8)):
        with pytest.raises(hevcdl_amd.HevcdlError):
            hevcdl_amd.write_access_unit(72, 48, 32, 0, recs, conf_win=cw)


def test_sps_carries_all_four_offsets():
    import hevcdl_amd
    import hevc_parse as hp
    recs = np.zeros(2, hevcdl_amd.REC_DTYPE)
    recs["luma_dir"][:] = 1; recs["chroma_dir"][:] = 36; recs["tr_idx"][:] = 1
    au = hevcdl_amd.write_access_unit(72, 48, 32, 0, recs, conf_win=(4, 2, 6, 8))
    sps = hp.parse_sps(hp.split_annexb(au)[1][1])
    assert (sps["width"], sps["height"], sps["conf_win"], sps["conf"]) == (72, 48, 1, [2, 1, 3, 4])      # left, right, top, bottom in chroma units
    cfg = hevcdl_amd.stream_config(72, 48, 32)
    assert ctypes.sizeof(hevcdl_amd.StreamConfig) == cfg.struct_size and (cfg.conf_win_left, cfg.conf_win_top) == (0, 0)


def test_zero_fields_give_the_bytes_of_before():
    """A format whose new fields are all zero (and one that names 420 / UNCHANGED) is the format of before: the existing fixtures' bytes by the existing rule."""
    import hevcdl_amd
    lib = hevcdl_amd.load_library()
    assert OLD_CASES
    for p in OLD_CASES:
        f = np.load(p)
        sw, sh, w, h, bd = (int(f[k]) for k in ("source_width", "source_height", "width", "height", "bit_depth"))
        ib, ob = int(f["input_bit_depth"]), int(f["output_bit_depth"])
        zero = hevcdl_amd.SourceFormat()
        zero.struct_size, zero.source_width, zero.source_height, zero.input_bit_depth, zero.output_bit_depth = ctypes.sizeof(hevcdl_amd.SourceFormat), sw, sh, ib, ob
        named = hevcdl_amd.source_format(sw, sh, ib, ob, chroma_format=420, colour_space="UNCHANGED")
        src = f["yuv"]
        want = np_load_per_sample(src, sw, sh, w, h, 420, 0, ib, bd)
        pics = samples(src.shape[0] * w * h * 3 // 2, bd, 3).reshape(src.shape[0], -1)
        for fmt in (zero, named):
            assert np.array_equal(hevcdl_amd.load_source_host(fmt, w, h, bd, src), want)
            assert np.array_equal(hevcdl_amd.store_output_host(fmt, w, h, bd, pics), np_store(pics, w, h, (0, 0, 0, 0), False, bd, ob, sw, sh))
            assert lib.hevcdl_source_frame_bytes(ctypes.byref(fmt)) == (sw * sh * 3 // 2) * (2 if ib > 8 else 1)


def test_default_format_and_frame_bytes_per_format():
    import hevcdl_amd
    lib = hevcdl_amd.load_library()
    cfg = hevcdl_amd.default_config(72, 48, 32, bit_depth=10)
    fmt = hevcdl_amd.SourceFormat()
    assert lib.hevcdl_source_format_default(ctypes.byref(fmt), ctypes.byref(cfg)) == 0
    assert (fmt.struct_size, fmt.chroma_format, fmt.colour_space, fmt.output_internal_colour_space, fmt.snr_internal_colour_space) == (ctypes.sizeof(hevcdl_amd.SourceFormat), 0, 0, 0, 0)
    assert (fmt.conf_win_left, fmt.conf_win_right, fmt.conf_win_top, fmt.conf_win_bottom) == (0, 0, 0, 0)
    for cf, samples_ in ((400, 66 * 42), (420, 66 * 42 + 2 * 33 * 21), (422, 66 * 42 + 2 * 33 * 42), (444, 3 * 66 * 42), (0, 66 * 42 + 2 * 33 * 21)):
        for ib, ob in ((8, 8), (8, 10), (10, 8), (16, 12)):
            f = hevcdl_amd.source_format(66, 42, ib, ob, chroma_format=cf)
            assert lib.hevcdl_source_frame_bytes(ctypes.byref(f)) == samples_ * (2 if ib > 8 else 1), (cf, ib)
            assert lib.hevcdl_output_frame_bytes(ctypes.byref(f)) == (66 * 42 + 2 * 33 * 21) * (2 if ob > 8 else 1), (cf, ob)      # output frames are 4:2:0, never converted back
            assert f.source_samples == samples_ and f.output_samples == 66 * 42 + 2 * 33 * 21
    f = hevcdl_amd.source_format(72, 40, 8, 10, chroma_format=444, conf_win=(4, 2, 6, 8))
    assert lib.hevcdl_output_frame_bytes(ctypes.byref(f)) == 2 * (66 * 26 * 3 // 2) and f.window_size == (66, 26)


def test_padded_size_mode_3_derives_nothing():
    """ConformanceWindowMode 3 pads nothing: hevcdl_padded_size keeps answering HEVCDL_ERR_UNSUPPORTED for it (tests/test_source.py pins that), the coded size is the source
    size, which must be a multiple of 8, and the window goes into the format."""
    import hevcdl_amd
    with pytest.raises(hevcdl_amd.HevcdlError) as e:
        hevcdl_amd.padded_size(72, 40, 3)
    assert e.value.status == 2
    assert hevcdl_amd.padded_size(72, 40, 0) == (72, 40)


# ---- the reference's runs ------------------------------------------------------------------------------------------------------------------------------------------
def case_format(f):
    import hevcdl_amd
    return hevcdl_amd.source_format(int(f["source_width"]), int(f["source_height"]), int(f["input_bit_depth"]), int(f["output_bit_depth"]), chroma_format=int(f["chroma_format"]),
                                    colour_space=int(f["colour_space"]), output_internal_colour_space=int(f["output_internal_colour_space"]),
                                    snr_internal_colour_space=int(f["snr_internal_colour_space"]), conf_win=tuple(int(v) for v in f["conf_win"]))


def case_conf_win(f):
    win = tuple(int(v) for v in f["conf_win"])
    return win if int(f["mode"]) == 3 else (int(f["width"]) - int(f["source_width"]), int(f["height"]) - int(f["source_height"]))


def coded_source(f):
    """The pictures the reference coded: every ratio-th source frame."""
    return f["yuv"][::int(f["temporal_subsample_ratio"])][:int(f["pictures"])]


def log_psnr(line):
    m = re.search(r"\[Y ([0-9.]+) dB +U ([0-9.]+) dB +V ([0-9.]+) dB\]", line)
    return [float(m.group(k)) for k in (1, 2, 3)]


def psnr_columns(f, coded, final):
    """PSNR as the log prints it: over the coded picture minus the padding (mode 3: the whole picture), U and V in the file's order unless SNRInternalColourSpace."""
    sw, sh, w, h, bd = (int(f[k]) for k in ("source_width", "source_height", "width", "height", "bit_depth"))
    cols = []
    for c, (o, r) in enumerate(zip(coded_planes(coded, w, h), coded_planes(final, w, h))):
        d = o[:sh >> (c > 0), :sw >> (c > 0)].astype(np.int64) - r[:sh >> (c > 0), :sw >> (c > 0)].astype(np.int64)
        sse, n, mx = int((d * d).sum()), d.size, 255 << (bd - 8)
        cols.append(999.99 if sse == 0 else 10.0 * math.log10(mx * mx * n / sse))
    if int(f["colour_space"]) and not int(f["snr_internal_colour_space"]):
        cols = [cols[0], cols[2], cols[1]]
    return cols


@pytest.mark.parametrize("path", CASES, ids=lambda p: os.path.basename(p)[7:-4])
def test_stream_output_file_and_log_equal_the_reference(path, oracle_built):
    """hevcdl_load_source_host on the stored source, the oracle's decisions, deblocking and SAO on the coded picture, the host writer with the window in the SPS and the
    hash SEI over the whole coded picture: the reference's stream byte for byte.  hevcdl_store_output_host of the final pictures: its reconstruction file."""
    import hevcdl_amd
    import ref_tools
    f = np.load(path)
    fmt = case_format(f)
    w, h, qp, bd = (int(f[k]) for k in ("width", "height", "qp", "bit_depth"))
    coded = hevcdl_amd.load_source_host(fmt, w, h, bd, coded_source(f))
    recs, recon, _ = ref_tools.run_oracle(coded, w, h, qp, f["labels"], bit_depth=bd)
    dbk = ref_tools.run_deblock(recon, w, h, qp, recs, bit_depth=bd)
    params, final = ref_tools.run_sao(coded, dbk, w, h, qp, bit_depth=bd)
    stream = b"".join(hevcdl_amd.write_access_unit(w, h, qp, poc, recs[poc], sao=params[poc].view(hevcdl_amd.SAO_DTYPE), bit_depth=bd, conf_win=case_conf_win(f))
                      + hevcdl_amd.picture_hash_sei(w, h, final[poc], bd) for poc in range(coded.shape[0]))
    assert stream == f["bitstream"].tobytes()
    assert hevcdl_amd.store_output_host(fmt, w, h, bd, final).tobytes() == f["recon_file"].tobytes()
    ww, wh = fmt.window_size
    assert (int(f["decoded_width"]), int(f["decoded_height"])) == (ww, wh) and int(f["decoded_bytes"]) == coded.shape[0] * (ww * wh * 3 // 2) * (2 if bd > 8 else 1)
    lines = [l for l in f["stdout"].tolist() if l.startswith("POC")]
    assert len(lines) == coded.shape[0] == int(f["pictures"])
    for poc, line in enumerate(lines):
        assert line.startswith("POC %4d " % poc)      # consecutive POCs, also behind a temporally subsampled read
        assert ["%.4f" % v for v in psnr_columns(f, coded[poc], final[poc])] == ["%.4f" % v for v in log_psnr(line)], line
    if int(f["chroma_format"]) == 400:
        assert "U 999.9900 dB    V 999.9900 dB" in lines[0]


def test_fixtures_cover_the_cases_of_the_issue():
    names = {os.path.basename(p)[7:-4] for p in CASES}
    assert names == {"444_72x40", "444_66x42_m1_8to10", "422_68x44_m1", "422_64_10to8", "400_72x40", "400_60_m2_8to10", "400_64_10to8", "swap_72x40", "swap_72x40_internal",
                     "win3_72x40", "win3_80x48_8to10_o8", "444_swap_m1_68x44", "ts3_72x40"}
    f = np.load(os.path.join(GOLD, "srcfmt_422_64_10to8.npz"))
    cb = f["yuv"][0][64 * 64:64 * 64 + 32 * 64].reshape(64, 32)
    assert {1022, 1023} <= set(cb[0, 2:6].tolist()) and {1022, 1023} <= set(cb[1, 2:6].tolist())      # on a kept and on a dropped chroma row
    f = np.load(os.path.join(GOLD, "srcfmt_ts3_72x40.npz"))
    assert (int(f["source_frames"]), int(f["pictures"]), int(f["temporal_subsample_ratio"])) == (7, 3, 3)


# ---- the CLI's keys (no GPU: --PrintConfig) --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def app():
    import hevcdl_amd
    return hevcdl_amd.build_app()


def print_config(app, args, cwd):
    import json
    r = subprocess.run([app] + args + ["--PrintConfig"], cwd=cwd, capture_output=True, text=True, timeout=600)
    return r.returncode, json.loads(r.stdout)


BASE = ["-i", "in.yuv", "-wdt", "72", "-hgt", "40", "-q", "32"]


def test_cli_accepts_the_file_layout_keys(app, tmp_path):
    rc, c = print_config(app, BASE + ["--InputChromaFormat=444", "--ChromaFormatIDC=420"], tmp_path)
    assert rc == 0 and c["errors"] == [] and (c["InputChromaFormat"], c["ChromaFormatIDC"], c["Input ChromaFormatIDC"], c["Output (internal) ChromaFormatIDC"]) == (444, 420, "4:4:4", "4:2:0")
    rc, c = print_config(app, BASE + ["--InputChromaFormat=400", "-cf", "420", "-ts", "3", "-f", "7"], tmp_path)
    assert rc == 0 and (c["Input ChromaFormatIDC"], c["TemporalSubsampleRatio"]) == ("4:0:0", 3)
    rc, c = print_config(app, BASE + ["--InputChromaFormat=422", "-cf", "420"], tmp_path)
    assert rc == 0 and c["Input ChromaFormatIDC"] == "4:2:2"
    rc, c = print_config(app, BASE + ["--ConformanceWindowMode=3", "--ConfWinLeft=4", "--ConfWinRight=2", "--ConfWinTop=6", "--ConfWinBottom=8", "-pdx", "4"], tmp_path)
    assert rc == 0 and c["ConfWin"] == [4, 2, 6, 8] and c["coded_size"] == [72, 40]      # the padding keys are ignored, as in the reference
    rc, c = print_config(app, BASE + ["--InputColourSpaceConvert=YCbCrtoYCrCb", "--OutputInternalColourSpace=1", "--SNRInternalColourSpace=1"], tmp_path)
    assert rc == 0 and (c["InputColourSpaceConvert"], c["OutputInternalColourSpace"], c["SNRInternalColourSpace"]) == ("YCbCrtoYCrCb", 1, 1)
    rc, c = print_config(app, BASE + ["--InputColourSpaceConvert=UNCHANGED"], tmp_path)
    assert rc == 0 and c["InputColourSpaceConvert"] == "UNCHANGED"


def test_cli_rejects_what_stays_out(app, tmp_path):
    for extra, needle in ((["--InputChromaFormat=444"], "ChromaFormatConstraint must be 420 for non main-RExt profiles."),
                          (["--InputChromaFormat=444", "--ChromaFormatIDC=444"], "ChromaFormatConstraint must be 420"),
                          (["--ChromaFormatIDC=422"], "ChromaFormatConstraint must be 420"),
                          (["--InputChromaFormat=411", "--ChromaFormatIDC=420"], "InputChromaFormatIDC must be either 400, 420, 422 or 444"),
                          (["--InputColourSpaceConvert=RGBtoGBR"], "InputColourSpaceConvert"), (["--InputColourSpaceConvert=YCbCrtoYYY"], "InputColourSpaceConvert"),
                          (["--InputChromaFormat=400", "-cf", "420", "--InputColourSpaceConvert=YCbCrtoYCrCb"], "InputColourSpaceConvert"),
                          (["--ConformanceWindowMode=3", "--ConfWinLeft=3"], "ConfWinLeft"), (["--ConformanceWindowMode=3", "--ConfWinLeft=36", "--ConfWinRight=36"], "leave nothing"),
                          (["--ConfWinLeft=2"], "ConfWinLeft"), (["-ts", "0"], "Temporal subsample rate must be no less than 1"),
                          (["--MSBExtendedBitDepth=10"], "MSBExtendedBitDepth"), (["--InputBitDepthC=10"], "InputBitDepthC")):
        rc, c = print_config(app, BASE + extra, tmp_path)
        assert rc == 2 and needle in " ".join(c["errors"]), (extra, c["errors"])
    rc, c = print_config(app, ["-i", "in.yuv", "-wdt", "68", "-hgt", "44", "--ConformanceWindowMode=3", "--ConfWinRight=4"], tmp_path)      # mode 3 pads nothing
    assert rc == 2 and "ConformanceWindowMode = 3" in " ".join(c["errors"])


def test_cli_refusal_carries_the_reference_message(app, tmp_path):
    """Without --PrintConfig: exit code 2 and the line the reference itself prints (stored with the fixtures)."""
    f = np.load(CASES[0])
    want = f["refusal_444"].tolist()
    assert "Error: ChromaFormatConstraint must be 420 for non main-RExt profiles." in want and int(f["refusal_444_exit"]) != 0
    r = subprocess.run([app] + BASE + ["--InputChromaFormat=444"], cwd=tmp_path, capture_output=True, text=True, timeout=600)
    assert r.returncode == 2 and "Error: ChromaFormatConstraint must be 420 for non main-RExt profiles." in (r.stdout + r.stderr).splitlines()


def test_sanitizer_harness(tmp_path):
    """tests/source_format_harness.cpp + csrc/source_core.h built with the host compiler and -fsanitize=address,undefined -static-libasan and run as a program."""
    import hevcdl_amd
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no host g++")
    exe = str(tmp_path / "source_format_harness")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
           "-I" + os.path.join(hevcdl_amd.PKG_DIR, "csrc"), os.path.join(ROOT, "tests", "source_format_harness.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and "asan" in r.stderr.lower() and "cannot find" in r.stderr.lower():
        pytest.skip("the host compiler has no static AddressSanitizer runtime: " + r.stderr.strip().splitlines()[-1])
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True)
    startup = ("ASan runtime does not come first", "Shadow memory range interleaves", "ReserveShadowMemoryRange failed", "error while loading shared libraries")
    if r.returncode != 0 and "source format harness:" not in r.stdout and "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr and any(m in r.stderr for m in startup):
        pytest.skip("the sanitizer build cannot start here: " + (r.stderr.strip().splitlines() or ["exit %d" % r.returncode])[-1][:200])
    assert r.returncode == 0 and "runtime error" not in r.stderr, (r.stdout[-1500:], r.stderr[-3000:])
    assert "cases, 0 failed" in r.stdout
