"""The stream parser (csrc/hevcdl_parse.cpp, host only): hevcdl_parse_stream against every reference-encoder stream under tests/golden, against the shared coder's
output on the synthetic corpora (with the spec-level decoder oracle/slice_spec.py beside it), and against streams it must refuse.  No GPU."""
import ctypes
import glob
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import entropy_cases as ec
from conftest import GOLD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

# every fixture that holds a stream, by family: (files, the stream keys of a file -> the key of the records each was coded from, or None where the fixture stores none)
FAMILIES = {"rd": 56, "fqp": 10, "dqr": 8, "dbksel": 8, "lfoff": 1, "stream": 1, "slices": 12, "segments": 6, "source": 8, "srcfmt": 13, "full": 1}


def family_files(fam):
    return sorted(glob.glob(os.path.join(GOLD, fam + "_*.npz")))


def streams_of(f):
    """-> [(stream key, records key or None)] of a fixture.  bitstream_one_slice (slices_*) is the run without the slice keys: other decisions than the stored records."""
    out = []
    for k in f.files:
        if not k.startswith("bitstream"):
            continue
        rk = "records10" if k.endswith("10") and "records10" in f.files else ("records" if "records" in f.files else None)
        out.append((k, None if k == "bitstream_one_slice" else rk))
    return out


ALL_STREAMS = [(fam, os.path.basename(p)[:-4], k, rk) for fam in FAMILIES for p in family_files(fam) for k, rk in streams_of(np.load(p))]


def test_the_fixture_list_is_the_whole_of_tests_golden():
    """The count per family is pinned, so a fixture that appears or goes is seen here; every .npz under tests/golden with a stream in it belongs to a family."""
    assert {fam: len(family_files(fam)) for fam in FAMILIES} == FAMILIES
    with_stream = {os.path.basename(p) for p in glob.glob(os.path.join(GOLD, "*.npz")) if any(k.startswith("bitstream") for k in np.load(p).files)}
    listed = {os.path.basename(p) for fam in FAMILIES for p in family_files(fam)}
    assert with_stream <= listed and listed - with_stream == {"full_f1080_q32.npz"}      # (that one stores records alone: its stream is written here)
    assert len(ALL_STREAMS) == 215


def inside_mask(w, h):
    cx, cy = (w + 63) // 64, (h + 63) // 64
    m = np.zeros((cx * cy, 256), bool)
    for y in range(h // 4):
        for x in range(w // 4):
            m[(y >> 4) * cx + (x >> 4), ec._z_of(x & 15, y & 15)] = True
    return m


def tskip_mask(w, h, tools, recs):
    """[ctus, 3, 256]: the tskip entries whose flag is in the stream -- the first partition of every 4x4 block with a set cbf, under transform_skip_enabled_flag."""
    cx = (w + 63) // 64
    m = np.zeros((len(recs), 3, 256), bool)
    if tools & 0x04:
        for a in range(len(recs)):
            for comp, base, log2, _ in ec._walk_blocks(recs[a], (a % cx) * 64, (a // cx) * 64, w, h):
                if log2 == 2:
                    m[a, comp, base // (4 if comp else 16)] = True
    return m


def assert_stream_fields(got, want, w, h, tools, name):
    """Records of one picture, field by field in what a stream determines: inside the picture; tskip where the flag is coded, 0 elsewhere; every level."""
    ins = inside_mask(w, h)
    for k in ("depth", "part_size", "luma_dir", "chroma_dir", "tr_idx"):
        assert np.array_equal(got[k][ins], want[k][ins]), (name, k)
        assert not got[k][~ins].any(), (name, k, "outside the picture")
    for c in range(3):
        assert np.array_equal(got["cbf"][:, c][ins], want["cbf"][:, c][ins]), (name, "cbf", c)
    mask = tskip_mask(w, h, tools, want)
    assert np.array_equal(got["tskip"][mask], want["tskip"][mask]) and not got["tskip"][~mask].any(), (name, "tskip")
    for k in ("coeff_y", "coeff_cb", "coeff_cr"):
        assert np.array_equal(got[k], want[k]), (name, k)
    assert not got["bits"].any() and not got["dist"].any() and not got["cost"].any()


def rewrite(parsed):
    """A parsed stream written again by the host writer from nothing but the parser's output: configuration, layouts, per picture the QP, the deblocking choice, the
    records, the SAO parameters and the hash SEI."""
    import hevcdl_amd
    lib = hevcdl_amd.load_library()
    cfg = parsed.cfg
    out = []
    cap = cfg.width * cfg.height * 12 + (1 << 16)
    buf = np.zeros(cap, np.uint8)
    for i, pic in enumerate(parsed.pictures):
        c = hevcdl_amd.StreamConfig.from_buffer_copy(bytes(cfg))
        c.qp = pic.qp
        choice = pic.dbk if pic.dbk.override_enabled else None
        n = ctypes.c_size_t(0)
        r = np.ascontiguousarray(parsed.records[i])
        s = np.ascontiguousarray(parsed.sao[i]) if pic.sao else None
        assert bool(pic.sao) == bool(cfg.sao_enabled)
        st = lib.hevcdl_write_access_unit_segments(ctypes.byref(c), hevcdl_amd._layout_ptr(parsed.slices), hevcdl_amd._layout_ptr(parsed.segments), 0 if pic.nal_type != 21 else pic.poc,
                                                   r.ctypes.data, None if s is None else s.ctypes.data, None if choice is None else ctypes.addressof(choice), buf.ctypes.data, cap, ctypes.byref(n))
        assert st == 0, st
        out.append(buf[:n.value].tobytes())
        if pic.hash_method:
            out.append(hevcdl_amd.hash_sei(*parsed.digest(i)))
    return b"".join(out)


@pytest.mark.parametrize("fam,name,key,rec_key", ALL_STREAMS, ids=["%s:%s" % (n, k) for _, n, k, _ in ALL_STREAMS])
def test_parser_on_every_reference_stream(fam, name, key, rec_key):
    """Every stream the reference encoder wrote for a fixture -- the SAO and the no-SAO run where both are stored, every switch of stream_c192_q32, the slice and segment
    layouts, the source-format runs with their conformance windows:
      * the records equal the fixture's in the stream-determined fields (where the fixture stores the records of that run);
      * QP per picture, deblocking parameters, SAO parameters, layouts, parameter sets and the hash SEI equal the stored ones: the host writer, given nothing but the
        parser's output, writes the fixture's stream again byte for byte (whatever differed would be coded differently; the writer itself is pinned to the streams
        by tests/test_bitstream.py, test_slices.py, test_segments.py, test_frame_qp.py, test_deltaqprd.py, test_dbk_select.py);
      * the QPs equal the ones the fixture records (chosen_qp of dqr_*, qps of fqp_*, qp elsewhere)."""
    import hevcdl_amd
    f = np.load(os.path.join(GOLD, name + ".npz"))
    stream = f[key].tobytes()
    p = hevcdl_amd.parse_stream(stream)
    cfg = p.cfg
    if "width" in f.files and fam not in ("source", "srcfmt"):
        assert (cfg.width, cfg.height) == (int(f["width"]), int(f["height"]))
    if "bit_depth" in f.files and fam not in ("source", "srcfmt", "stream"):
        assert cfg.bit_depth == int(f["bit_depth"])
    if rec_key:
        want = np.frombuffer(f[rec_key].tobytes(), hevcdl_amd.REC_DTYPE).reshape(f[rec_key].shape[0], -1)
        assert p.records.shape == want.shape
        assert hevcdl_amd.validate_records(cfg, want) is None                  # (the reference's own records pass the check that callers' records get)
        for poc in range(want.shape[0]):
            assert_stream_fields(p.records[poc], want[poc], cfg.width, cfg.height, cfg.tools, (name, key, poc))
    want_qp = [int(v) for v in f["chosen_qp"]] if "chosen_qp" in f.files else ([int(v) for v in f["qps"]] if "qps" in f.files else ([int(f["qp"])] * len(p.pictures) if "qp" in f.files else None))
    if want_qp is not None:
        assert p.qps == want_qp[:len(p.qps)] and len(p.qps) <= len(want_qp)
    if "tools" in f.files:
        assert cfg.tools & 0x34 == int(f["tools"]) & 0x34
    for k, layout in (("slice", p.slices), ("segment", p.segments)):
        if k + "_mode" in f.files and key != "bitstream_one_slice":
            assert (layout.mode, layout.argument) == (int(f[k + "_mode"]), int(f[k + "_argument"]))
    assert hevcdl_amd.validate_records(cfg, p.records) is None
    assert rewrite(p) == stream


def test_parser_on_the_1080p_fixture():
    """full_f1080_q32 stores records and no stream: the host writer's stream of them, with wavefront rows and without, parses back to them (510 CTUs, a partial last row)."""
    import hevcdl_amd
    f = np.load(os.path.join(GOLD, "full_f1080_q32.npz"))
    w, h, qp = int(f["width"]), int(f["height"]), int(f["qp"])
    recs = np.frombuffer(f["records"].tobytes(), hevcdl_amd.REC_DTYPE).reshape(f["records"].shape[0], -1)
    au = hevcdl_amd.write_access_unit(w, h, qp, 0, recs[0])
    p = hevcdl_amd.parse_stream(au)
    assert (p.cfg.width, p.cfg.height, p.qps) == (w, h, [qp])
    assert_stream_fields(p.records[0], recs[0], w, h, p.cfg.tools, "full")
    assert rewrite(p) == au


# ---- the coder's own output ------------------------------------------------------------------------------------------------------------------------------
def _parsed_as_decoded(p, cfg, recs):
    """A ParsedStream of one picture in the shape ec.assert_round_trip takes a decoder's result."""
    return p.records[0], (p.sao[0] if p.pictures[0].sao else None), tskip_mask(cfg.width, cfg.height, cfg.tools, recs), None


def test_round_trip_of_the_shared_coder_on_the_synthetic_corpus():
    """records -> shared coder (hevcdl_write_access_unit) -> bytes -> parser: the canonical form of the input, for the 204 corpus pictures and the directed ones --
    levels up to +-32768, every scan, hidden signs that differ from the input's, SAO merges at tile edges, wavefront rows, tiles."""
    import hevcdl_amd
    refused = 0
    for name, cfg, recs, sao in ec.fuzz_corpus() + ec.directed_pictures():
        try:
            p = hevcdl_amd.parse_stream(ec.host_writer_stream(cfg, recs, sao))
        except hevcdl_amd.HevcdlError as e:
            recs = _refused_for_its_levels(e, name, recs, lambda: ec.decode_substreams(cfg, ec.substreams_of(hevcdl_amd.code_slice_data(cfg, recs, sao)))[3])
            refused += 1
            p = hevcdl_amd.parse_stream(ec.host_writer_stream(cfg, recs, sao))
        assert (p.cfg.width, p.cfg.height, p.qps, p.cfg.bit_depth, bool(p.cfg.wavefront), p.cfg.tools & 0x14) == (cfg.width, cfg.height, [cfg.qp], cfg.bit_depth, bool(cfg.wavefront), cfg.tools & 0x14), name
        back, want = hevcdl_amd.StreamConfig.from_buffer_copy(bytes(p.cfg)), hevcdl_amd.StreamConfig.from_buffer_copy(bytes(cfg))
        back.tools = (back.tools & 0x34) | (cfg.tools & ~0x34)                    # four tool bits leave no trace in a stream,
        if want.tile_uniform_spacing:                                             # and neither do the sizes of uniformly spaced tiles
            for i in range(19):
                want.tile_column_width[i] = 0
            for i in range(21):
                want.tile_row_height[i] = 0
        assert bytes(back) == bytes(want), name                                   # tiles, spacing, offsets, level, SAO, bit depth: the configuration comes back
        ec.assert_round_trip(name, cfg, recs[0], None if sao is None else sao[0], _parsed_as_decoded(p, cfg, recs[0]))
    assert 0 < refused < 150


def test_round_trip_on_the_layout_corpus_agrees_with_the_spec_decoder():
    """The same under every slice and segment layout the writer accepts (entropy_cases.layout_corpus), and on the same bytes the parser and oracle/slice_spec.py read the
    same records and SAO parameters; the parser names the layout the stream was written with."""
    import hevcdl_amd
    import slice_spec as ss
    refused = 0
    for name, cfg, recs, sao, lay in ec.layout_corpus():
        au, _ = ec.write_layout_access_units(cfg, recs, sao, lay)
        try:
            p = hevcdl_amd.parse_stream(au)
        except hevcdl_amd.HevcdlError as e:
            bad = au
            recs = _refused_for_its_levels(e, name, recs, lambda: ss.decode_access_unit(bad, strict_levels=False, picture_decoder=ec.cached_decode_picture, segments_decoder=ec.cached_decode_picture_segments)[3])
            refused += 1
            au, _ = ec.write_layout_access_units(cfg, recs, sao, lay)
            p = hevcdl_amd.parse_stream(au)
        slices, segs = lay["slices"], lay["segments"]
        assert ((p.slices.mode, p.slices.argument) if p.slices else (0, 0)) == (tuple(slices) if slices and _several(cfg, lay, "slices") else (0, 0)), name
        assert ((p.segments.mode, p.segments.argument) if p.segments else (0, 0)) == (tuple(segs) if segs and _several(cfg, lay, "segments") else (0, 0)), name
        decoded = _parsed_as_decoded(p, cfg, recs[0])
        ec.assert_layout_round_trip(name, cfg, recs[0], None if sao is None else sao[0], lay, decoded)
        spec = ss.decode_access_unit(au, strict_levels=False, picture_decoder=ec.cached_decode_picture, segments_decoder=ec.cached_decode_picture_segments)
        for k in ec.RT_FIELDS:
            assert np.array_equal(spec[0][k], p.records[0][k]), (name, k)
        assert (spec[1] is None) == (sao is None) and (sao is None or np.array_equal(spec[1], p.sao[0])), name
        if lay["choice"]:
            d = p.pictures[0].dbk
            assert (d.override_enabled, d.override_flag, d.disabled, d.beta_offset_div2, d.tc_offset_div2) == tuple(lay["choice"]), name
    assert 0 < refused < 100


def _refused_for_its_levels(e, name, recs, spec_tally):
    """The coder codes any records, and the corpora hold levels of -32768 at positions whose sign is hidden: where the parity of the group turns such a level positive the
    stream says +32768, which is no TransCoeffLevel (7.4.9.11).  The parser refuses that stream as damaged -- the spec-level decoder, in its lenient mode, counts the level
    and wraps it -- and the picture is then round-tripped with -32767 in place of -32768, which conforms.  -> those records."""
    assert e.status == 1 and "a level outside 16 bits" in str(e), name
    assert spec_tally()["level_out_of_range"] > 0, name
    out = recs.copy()
    for k in ("coeff_y", "coeff_cb", "coeff_cr"):
        out[k][out[k] == -32768] = -32767
    return out


def _several(cfg, lay, what):
    """Does the layout key cut this picture at all?  (A slice or segment argument that covers the whole picture leaves one NAL unit: the stream does not say the key.)"""
    borders, _, _ = ec.segment_borders(cfg, lay)
    return sum(1 for _, dep, _, _ in borders if bool(dep) == (what == "segments")) > (1 if what == "slices" else 0)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------------------------
def _nals(stream):
    import hevc_parse as hp
    return [(sc, bytes(n)) for sc, n in hp.split_annexb(stream)]


def _join(nals):
    return b"".join(b"\0" * (sc - 3) + b"\0\0\1" + n for sc, n in nals)


def _escape(rbsp):
    out, zeros = bytearray(), 0
    for v in rbsp:
        if zeros >= 2 and v <= 3:
            out.append(3)
            zeros = 0
        out.append(v)
        zeros = zeros + 1 if v == 0 else 0
    return bytes(out)


def _flip(nal, bit):
    """One bit of a NAL unit's RBSP (counted behind the two header bytes, emulation prevention aside) flipped."""
    import hevc_parse as hp
    raw = bytearray(hp.unescape(nal))
    raw[2 + (bit >> 3)] ^= 0x80 >> (bit & 7)
    return bytes(raw[:2]) + _escape(raw[2:])


def _sps_positions(nal):
    import hevc_parse as hp
    r = hp.Bits(hp.unescape(nal)[2:])
    pos = {}
    r.u(8); r.u(96); r.ue()
    pos["chroma_format_idc"] = r.p; r.ue(); r.ue(); r.ue()
    if r.u(1):
        [r.ue() for _ in range(4)]
    pos["bit_depth"] = r.p; r.ue(); r.ue(); r.ue(); r.u(1); r.ue(); r.ue(); r.ue(); r.ue()
    pos["log2_diff_cb"] = r.p; r.ue(); r.ue(); r.ue(); r.ue(); r.ue()
    pos["scaling_list"] = r.p; r.u(1); r.u(1); r.u(1)
    pos["pcm"] = r.p
    return pos


def _pps_positions(nal):
    import hevc_parse as hp
    r = hp.Bits(hp.unescape(nal)[2:])
    pos = {}
    r.ue(); r.ue(); r.u(7); r.ue(); r.ue(); r.se(); r.u(1); r.u(1)
    pos["cu_qp_delta"] = r.p; r.u(1); r.se(); r.se(); r.u(3)
    pos["tq_bypass"] = r.p
    return pos


REFUSALS = [("chroma_format_idc", 33, 2, "4:2:0"), ("bit_depth", 33, 0, "bit depth"), ("log2_diff_cb", 33, 4, "CTU 64"), ("scaling_list", 33, 0, "scaling lists"), ("pcm", 33, 0, "PCM"),
            ("cu_qp_delta", 34, 0, "cu_qp_delta_enabled_flag"), ("tq_bypass", 34, 0, "transquant bypass"), ("slice_type", 19, 3, "P and B slices")]


@pytest.mark.parametrize("field,nal_type,bit,sentence", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_unsupported_features_are_refused_with_their_sentence(field, nal_type, bit, sentence):
    """One bit of a parameter set (or of the first slice header) of a fixture stream turned: 4:2:2, another bit depth, 32x32 CTUs, scaling lists, PCM, cu_qp_delta,
    transquant bypass, a B slice.  HEVCDL_ERR_UNSUPPORTED, and hevcdl_parse_error names the feature."""
    import hevcdl_amd
    stream = np.load(os.path.join(GOLD, "rd_e64x8_q20.npz"))["bitstream"].tobytes()
    nals = _nals(stream)
    k = next(i for i, (_, n) in enumerate(nals) if (n[0] >> 1) & 63 == nal_type)
    at = 0 if nal_type == 19 else (_sps_positions if nal_type == 33 else _pps_positions)(nals[k][1])[field]
    nals[k] = (nals[k][0], _flip(nals[k][1], at + bit))
    with pytest.raises(hevcdl_amd.HevcdlError) as e:
        hevcdl_amd.parse_stream(_join(nals))
    assert e.value.status == 2 and sentence in str(e.value), str(e.value)
    assert hevcdl_amd.parse_stream(stream).qps == [20] and hevcdl_amd.load_library().hevcdl_parse_error() == b""


def test_layouts_outside_the_writer_are_refused():
    """A slice that starts in the middle of a CTU row: slice_segment_address of the second slice of a row-slice stream moved by one CTU."""
    import hevc_parse as hp
    import hevcdl_amd
    stream = np.load(os.path.join(GOLD, "slices_r128_a2.npz"))["bitstream"].tobytes()
    nals = _nals(stream)
    sps, pps = hp.parse_sps(nals[1][1]), hp.parse_pps(nals[2][1])
    hdr, _ = hp.parse_slice_header(nals[4][1], sps, pps)
    assert hdr["address"] == 2 and hdr["address_bits"] == 2
    nals[4] = (nals[4][0], _flip(nals[4][1], hdr["address_bit_pos"] - 16 + 1))      # 2 -> 3
    with pytest.raises(hevcdl_amd.HevcdlError) as e:
        hevcdl_amd.parse_stream(_join(nals))
    assert e.value.status == 2 and "does not start at a CTU row or a tile" in str(e.value)


def _status(stream):
    import hevcdl_amd
    try:
        return 0, hevcdl_amd.parse_stream(stream)
    except hevcdl_amd.HevcdlError as e:
        return e.status, None


@pytest.mark.parametrize("name,key", [("rd_w200_q27_r2", "bitstream"), ("slices_r128_a2", "bitstream"), ("segments_t512x128_s2_a1", "bitstream"), ("stream_c192_q32", "bitstream_ps0")])
def test_truncated_streams_return_an_error_status(name, key):
    """The stream cut at every NAL boundary, and every slice NAL unit cut one byte short and in its middle.  A cut that leaves nothing but whole pictures (in front of a
    picture's parameter sets or first slice, or between a picture and its hash SEI) is a shorter stream, and must parse to exactly the pictures in front of the cut;
    every other cut is an error status.  (The issue's wording is "truncation at every NAL boundary returns an error status"; a prefix of whole access units is itself a
    conforming stream, so for those cuts the test demands the stronger thing: status OK and exactly the pictures in front of the cut, records included.)"""
    import hevc_parse as hp
    stream = np.load(os.path.join(GOLD, name + ".npz"))[key].tobytes()
    whole = _status(stream)[1]
    nals = _nals(stream)
    segs_seen, pictures_before, errors = 0, [], 0
    seg_total = [p.n_segments for p in whole.pictures]
    done = 0                                                              # pictures complete in front of NAL unit k
    for k, (sc, n) in enumerate(nals):
        t = (n[0] >> 1) & 63
        pictures_before.append((done, segs_seen == 0))
        if t < 32:
            segs_seen += 1
            if segs_seen == seg_total[done]:
                done, segs_seen = done + 1, 0
    for k in range(1, len(nals)):
        st, p = _status(_join(nals[:k]))
        n_done, at_picture_end = pictures_before[k]
        if at_picture_end and n_done > 0:
            assert st == 0 and len(p.pictures) == n_done and np.array_equal(p.records, whole.records[:n_done]), (k, st)
        else:
            assert st != 0, k
            errors += 1
        if (nals[k][1][0] >> 1) & 63 < 32:
            for cut in (len(nals[k][1]) - 1, len(nals[k][1]) // 2):
                assert _status(_join(nals[:k]) + b"\0\0\1" + nals[k][1][:cut])[0] != 0, (k, cut)
    assert errors >= 3


FLIP_STREAMS = [("rd_e8x8_q32", "bitstream"), ("dbksel_inpps0_72x72_q32_dis", "bitstream"), ("slices_c64x192_a1", "bitstream")]


@pytest.mark.parametrize("name,key", FLIP_STREAMS)
def test_single_bit_flips_never_give_out_of_range_records(name, key):
    """Every single bit of three small fixture streams flipped, one at a time: the parser returns a status, and whatever it returns HEVCDL_OK for passes
    hevcdl_validate_records and keeps its SAO parameters in range -- nothing a later stage would index memory with is out of range.  (A flip in the VPS, in the profile
    fields or in the hash SEI's digest changes nothing the parser hands on, or only the digest: those parse.)"""
    import hevcdl_amd
    stream = np.load(os.path.join(GOLD, name + ".npz"))[key].tobytes()
    ok = refused = 0
    data = bytearray(stream)
    for bit in range(len(stream) * 8):
        data[bit >> 3] ^= 0x80 >> (bit & 7)
        st, p = _status(bytes(data))
        data[bit >> 3] ^= 0x80 >> (bit & 7)
        assert st in (0, 1, 2)
        if st:
            refused += 1
            continue
        ok += 1
        assert hevcdl_amd.validate_records(p.cfg, p.records) is None, bit
        mx = (1 << (min(p.cfg.bit_depth, 10) - 5)) - 1
        assert p.sao["mode"].min() >= 0 and p.sao["mode"].max() <= 2 and p.sao["type"].min() >= 0 and p.sao["type"].max() <= 4 and 0 <= p.sao["aux"].min() and p.sao["aux"].max() <= 31
        assert np.abs(p.sao["offset"]).max() <= mx and all(0 <= q <= 51 for q in p.qps)
    print("%s: %d flips, %d refused, %d parsed" % (name, len(stream) * 8, refused, ok))
    assert refused > 0 and ok > 0


def test_validate_records_names_what_is_wrong():
    import hevcdl_amd
    cfg = hevcdl_amd.stream_config(72, 72, 30)
    good = ec.synth_records(np.random.default_rng(5), 72, 72)[None]
    assert hevcdl_amd.validate_records(cfg, good) is None
    for field, z, value, sentence in (("depth", 0, 4, "depth above 3"), ("luma_dir", 0, 35, "luma prediction mode above 34"), ("chroma_dir", 0, 7, "chroma prediction mode"),
                                      ("part_size", 0, 1, "part size"), ("tr_idx", 0, 9, "transform tree"), ("cbf", 0, 0x80, "cbf bit")):
        bad = good.copy()
        if field == "tr_idx":
            bad["depth"][0, 0, :] = 0
            bad["part_size"][0, 0, :] = 0
            bad["luma_dir"][0, 0, :] = 1
            bad["chroma_dir"][0, 0, :] = 36
            bad["tr_idx"][0, 0, :] = value
        elif field == "cbf":
            bad["cbf"][0, 0, 1, z] = value
        else:
            bad[field][0, 0, z] = value
        why = hevcdl_amd.validate_records(cfg, bad)
        assert why is not None and sentence in why, (field, why)
    assert hevcdl_amd.validate_records(cfg, ec.garbage_records(3, 4)[None]) is not None


def test_sanitizer_harness(tmp_path):
    """tests/decode_harness.cpp + csrc/hevcdl_parse.cpp + csrc/hevcdl_bitstream.cpp built with the host compiler and -fsanitize=address,undefined -static-libasan and run
    as a program: every fixture stream parsed from an exact-size heap block (a read one byte past the stream is caught), the records compared with the fixture's
    where the dump carries them, and the flip corpus of the test above with hevcdl_validate_records behind every flip that parses."""
    import hevcdl_amd
    cxx = shutil.which("g++")
    if not cxx:
        pytest.skip("no host g++")
    csrc = os.path.join(hevcdl_amd.PKG_DIR, "csrc")
    exe = str(tmp_path / "decode_harness")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
           "-I" + os.path.join(ROOT, "include"), "-I" + csrc, os.path.join(ROOT, "tests", "decode_harness.cpp"), os.path.join(csrc, "hevcdl_parse.cpp"),
           os.path.join(csrc, "hevcdl_bitstream.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and "asan" in r.stderr.lower() and "cannot find" in r.stderr.lower():
        pytest.skip("the host compiler has no static AddressSanitizer runtime: " + r.stderr.strip().splitlines()[-1])
    assert r.returncode == 0, r.stderr[-2000:]
    dumps = []
    for i, (fam, name, key, rec_key) in enumerate(ALL_STREAMS):
        f = np.load(os.path.join(GOLD, name + ".npz"))
        path = str(tmp_path / ("s%03d.bin" % i))
        flips = 1 if (name, key) in FLIP_STREAMS else 0
        recs = f[rec_key].tobytes() if rec_key else b""
        with open(path, "wb") as out:
            out.write(np.array([len(f[key]), len(recs), flips], np.int64).tobytes() + f[key].tobytes() + recs)
        dumps.append(path)
    r = subprocess.run([exe] + dumps, capture_output=True, text=True)
    startup = ("ASan runtime does not come first", "Shadow memory range interleaves", "ReserveShadowMemoryRange failed", "error while loading shared libraries")
    if r.returncode != 0 and "decode harness:" not in r.stdout and "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr and any(m in r.stderr for m in startup):
        pytest.skip("the sanitizer build cannot start here: " + (r.stderr.strip().splitlines() or ["exit %d" % r.returncode])[-1][:200])
    assert r.returncode == 0 and "runtime error" not in r.stderr, (r.stdout[-1500:], r.stderr[-3000:])
    assert "%d dumps, 0 failed" % len(dumps) in r.stdout


def test_pipeline_parse_sequence_reads_a_stream_file(tmp_path):
    """pipeline.parse_sequence: the front end over a file; headers_only leaves the records out."""
    import hevcdl_amd
    from hevcdl_amd import pipeline
    f = np.load(os.path.join(GOLD, "rd_w200_q27_r2.npz"))
    (tmp_path / "s.bin").write_bytes(f["bitstream"].tobytes())
    p = pipeline.parse_sequence(str(tmp_path / "s.bin"))
    want = np.frombuffer(f["records"].tobytes(), hevcdl_amd.REC_DTYPE).reshape(f["records"].shape[0], -1)
    assert p.qps == [27, 27] and bool(p.cfg.wavefront) and p.records.shape == want.shape and np.array_equal(p.records["coeff_y"], want["coeff_y"])
    assert [p.digest(i)[0] for i in range(2)] == [1, 1] and len(p.digest(0)[1]) == 48
    h = pipeline.parse_sequence(str(tmp_path / "s.bin"), headers_only=True)
    assert h.records is None and h.qps == p.qps and [q.n_segments for q in h.pictures] == [1, 1]
