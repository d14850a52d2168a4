"""The entropy coder against a DECODER (oracle/slice_spec.py, an I-slice slice-data decoder restated from H.265): records -> coder -> bytes -> decoder -> records.
The decoder is first pinned to the 56 reference-encoder streams, then applied to the synthetic corpus, whose streams nothing else ever decodes; a tally of the
branches the decoder took holds the corpus to the paths it is there for.  No GPU (the device coder's round trip is in tests/test_entropy_gpu.py)."""
import os
import subprocess

import numpy as np
import pytest

import entropy_cases as ec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_DEC = os.path.join(ROOT, "oracle", "_ref", "TAppDecoder_ref")


def access_units(stream):
    """A stream of several pictures -> its access units (each opens with its VPS, or is a lone slice NAL)."""
    import hevc_parse as hp
    out, cur = [], b""
    for sc, n in hp.split_annexb(stream):
        if (n[0] >> 1) & 63 == 32 and cur:
            out.append(cur)
            cur = b""
        cur += b"\0" * (sc - 3) + b"\0\0\1" + n
    return out + [cur]


def inside_mask(w, h):
    """[ctus, 256]: the 4x4 partitions of every CTU that lie inside the picture -- a record says nothing the stream carries about the others."""
    cx, cy = (w + 63) // 64, (h + 63) // 64
    m = np.zeros((cx * cy, 256), bool)
    for y in range(h // 4):
        for x in range(w // 4):
            m[(y >> 4) * cx + (x >> 4), ec._z_of(x & 15, y & 15)] = True
    return m


def test_tables_typed_from_the_standard_equal_the_products():
    """transIdxLps, transIdxMps and the 4x4 ctxIdxMap as typed into slice_spec == csrc/entropy_tables.h (which packs (state << 1) | mps); the record layouts agree."""
    import hevcdl_amd
    import slice_spec as ss
    _, arrays = ss._parse_tables_header()
    for s in range(64):
        for m in (0, 1):
            lps = (ss.TRANS_IDX_LPS[s] << 1) | ((1 - m) if s == 0 else m)
            assert arrays["NEXT_LPS"][(s << 1) | m] == lps and arrays["NEXT_MPS"][(s << 1) | m] == (ss.TRANS_IDX_MPS[s] << 1) | m
    assert arrays["CTX_IND_MAP_4x4"] == ss.CTX_IDX_MAP
    assert ss.REC_DTYPE == hevcdl_amd.REC_DTYPE and ss.SAO_DTYPE == hevcdl_amd.SAO_DTYPE
    for l2 in range(4):                                                   # every generated scan visits every position once
        for scan in ss.SCAN_ORDER[l2]:
            assert sorted(scan) == sorted((x, y) for x in range(1 << l2) for y in range(1 << l2))


@pytest.mark.parametrize("path", ec.CASES, ids=lambda p: os.path.basename(p)[3:-4])
def test_decoder_reproduces_the_reference_encoders_records(path):
    """56 reference-encoder runs: every access unit of bitstream_nosao, decoded through the access-unit entry, gives the fixture's records in every field the stream
    carries (partitions outside the picture are not carried; tskip only where the flag was coded)."""
    import slice_spec as ss
    cfg, recs, stream = ec.fixture_case(path)
    aus = access_units(stream)
    assert len(aus) == recs.shape[0]
    ins = inside_mask(cfg.width, cfg.height)
    for poc, au in enumerate(aus):
        got, sao, mask, tally, info = ss.decode_access_unit(au)
        assert sao is None and (info["width"], info["height"], info["qp"], info["bit_depth"], info["wavefront"]) == (cfg.width, cfg.height, cfg.qp, cfg.bit_depth, bool(cfg.wavefront))
        assert tally["level_out_of_range"] == 0
        for k in ("depth", "part_size", "luma_dir", "chroma_dir", "tr_idx"):
            assert np.array_equal(got[k][ins], recs[poc][k][ins]), k
        for c in range(3):
            assert np.array_equal(got["cbf"][:, c][ins], recs[poc]["cbf"][:, c][ins])
        assert np.array_equal(got["tskip"][mask], recs[poc]["tskip"][mask]) and not got["tskip"][~mask].any()
        for k in ("coeff_y", "coeff_cb", "coeff_cr"):
            assert np.array_equal(got[k], recs[poc][k]), k


@pytest.mark.parametrize("name", ec.SAO_CASES)
def test_decoder_gives_back_the_sao_parameters(name, oracle_built):
    import slice_spec as ss
    cfg, recs, sao = ec.sao_case(name)
    aus = access_units(ec.host_writer_stream(cfg, recs, sao))
    assert len(aus) == recs.shape[0]
    for poc, au in enumerate(aus):
        decoded = ss.decode_access_unit(au)
        assert decoded[4]["sao"] and decoded[3]["level_out_of_range"] == 0
        got, want = decoded[0].copy(), recs[poc].copy()
        ins = inside_mask(cfg.width, cfg.height)
        for k in ("depth", "part_size", "luma_dir", "chroma_dir", "tr_idx"):      # outside the picture the fixture keeps what the reference left there
            got[k][~ins], want[k][~ins] = 0, 0
        for c in range(3):
            got["cbf"][:, c][~ins], want["cbf"][:, c][~ins] = 0, 0
        ec.assert_round_trip(name, cfg, want, sao[poc], (got,) + decoded[1:4])


_TALLY = {}


def corpus_round_trip():
    """Every picture of the corpus and the directed pictures through the shared coder on the host and the decoder, once per session -> (summed tally, counts)."""
    import hevcdl_amd
    import slice_spec as ss
    if not _TALLY:
        tally, counts = ss.new_tally(), {}
        for name, cfg, recs, sao in ec.fuzz_corpus() + ec.directed_pictures():
            coded = hevcdl_amd.code_slice_data(cfg, recs, sao)
            decoded = ec.decode_substreams(cfg, ec.substreams_of(coded))
            ec.assert_round_trip(name, cfg, recs[0], None if sao is None else sao[0], decoded, counts)
            ss.add_tally(tally, decoded[3])
        _TALLY["tally"], _TALLY["counts"] = tally, counts
    return _TALLY["tally"], _TALLY["counts"]


def test_round_trip_of_the_shared_coder():
    """204 corpus pictures + the directed ones: what the decoder reads out of code_slice_data's sub-streams is the canonical form of the input."""
    corpus_round_trip()


def test_round_trip_of_the_host_writer_through_the_access_unit_entry():
    """The same through hevcdl_write_access_unit and the access-unit entry: parameter sets, slice header, entry points and emulation prevention around synthetic
    payloads.  (The entry cuts the sub-streams itself; sub-streams whose bytes and parameters the picture entry has decoded already are looked up, not decoded again.)"""
    import hevc_parse as hp
    import slice_spec as ss
    escaped = 0
    for name, cfg, recs, sao in ec.fuzz_corpus() + ec.directed_pictures():
        au = ec.host_writer_stream(cfg, recs, sao)
        out = ss.decode_access_unit(au, strict_levels=False, picture_decoder=ec.cached_decode_picture)
        info = out[4]
        assert (info["width"], info["height"], info["qp"], info["bit_depth"], info["sao"], info["wavefront"]) == (cfg.width, cfg.height, cfg.qp, cfg.bit_depth, sao is not None, bool(cfg.wavefront))
        assert sum(info["entry_points"]) + len(info["substreams"][-1]) <= info["payload_bytes"]
        slice_nal = hp.split_annexb(au)[-1][1]
        escaped += len(slice_nal) - len(hp.unescape(slice_nal))
        ec.assert_round_trip(name, cfg, recs[0], None if sao is None else sao[0], out[:4])
    assert escaped > 0      # emulation prevention bytes did occur inside the payloads


def test_access_unit_entry_on_synthetic_pictures():
    """The access-unit entry itself, end to end, on one picture per layout (plain, wavefront, tile rows, tile columns): header values, cut sub-streams, records."""
    import hevcdl_amd
    import slice_spec as ss
    corpus = ec.fuzz_corpus()
    picks = [corpus[15], next(c for c in corpus if c[1].wavefront and c[2].shape[1] >= 4), next(c for c in corpus if c[1].tile_rows > 1 and c[3] is not None)] + ec.directed_pictures()
    for name, cfg, recs, sao in picks:
        coded = hevcdl_amd.code_slice_data(cfg, recs, sao)
        out = ss.decode_access_unit(ec.assemble(cfg, coded), strict_levels=False)
        assert out[4]["substreams"] == ec.substreams_of(coded) and (out[4]["qp"], out[4]["tools"] & cfg.tools, out[4]["bit_depth"]) == (cfg.qp, cfg.tools & 0x14, cfg.bit_depth)
        assert sum(out[4]["entry_points"]) + len(out[4]["substreams"][-1]) <= out[4]["payload_bytes"]
        ec.assert_round_trip(name, cfg, recs[0], None if sao is None else sao[0], out[:4])


def test_the_corpus_reaches_the_paths_it_is_there_for():
    """Conditions on the decoder's tally over the corpus and the directed pictures; each is a path no reference stream is known to take."""
    t, counts = corpus_round_trip()
    print(t, counts)
    assert t["rice"][4] > 0 and all(v > 0 for v in t["rice"])
    # coeff_abs_level_remaining of |level| 32768: a prefix of 4 + 13 ones; the suffix bin string of 9.3.3.11 (the EGk code) is 13 + 1 + 14 = 28 bins, of which the
    # 14 behind the unary part are fixed-length -- 14 is the most that 16-bit levels reach (EG1 of 32765 - 4: 2^14 - 2 <= 32761 < 2^15 - 2)
    assert t["escape_suffix_bins_max"] >= 15 and t["escape_fixed_bits_max"] == 14 and t["escape_prefix_max"] == 17
    assert t["num_sig_gt8"] > 0 and t["sign_hidden"] > 0 and counts["hidden_sign_differed"] > 0
    for comp, n in (("luma", 4), ("luma", 8), ("chroma", 4)):
        for scan in ("diag", "hor", "ver"):
            assert t["scan"].get((comp, n, scan), 0) > 0, (comp, n, scan)
    assert all(v > 0 for v in t["mpm_idx"]) and t["rem_mode"] > 0
    assert t["cand_left_other_ctu"] > 0 and t["cand_above_other_ctu_row"] > 0 and t["cand_tile_edge_left"] > 0 and t["cand_tile_edge_above"] > 0
    assert t["chroma_34"] > 0 and all(v > 0 for v in t["chroma_mode"])
    assert t["split_ctx_tile_edge"] > 0
    assert t["sao_merge_left"] > 0 and t["sao_merge_up"] > 0 and t["sao_merge_left_tile_edge"] > 0 and t["sao_merge_up_tile_edge"] > 0
    assert t["sao_band_position_max"] > 28 and t["sao_band_wrap"] > 0 and t["sao_offset_abs_max"] == 31
    assert t["ctx_sync_from_above"] > 0 and t["ctx_init_at_row_start"] > 0
    assert t["tskip_set"][1] > 0 and t["chroma_4x4_behind_fourth"] > 0


def test_a_flipped_bit_never_decodes_to_the_same_records():
    """200 seeded bit positions over three pictures (plain with SAO, wavefront, tile rows): the decoder raises or returns other records, never the same -- a decoder
    that accepts anything would prove nothing.  A flip among the zeros of byte_alignment() raises."""
    import hevcdl_amd
    import slice_spec as ss
    corpus = ec.fuzz_corpus()
    picks = [corpus[19], corpus[39], corpus[44]]
    assert picks[0][3] is not None and picks[1][1].wavefront and picks[2][1].tile_rows == 2
    rng = np.random.default_rng(4711)
    raised = changed = same = 0
    for name, cfg, recs, sao in picks:
        subs = ec.substreams_of(hevcdl_amd.code_slice_data(cfg, recs, sao))
        base = ec.decode_substreams(cfg, subs)
        total = sum(len(s) for s in subs) * 8
        for bit in rng.choice(total, size=67 if name != picks[0][0] else 66, replace=False):
            k, b = 0, int(bit)
            while b >= len(subs[k]) * 8:
                b -= len(subs[k]) * 8
                k += 1
            bad = bytearray(subs[k])
            bad[b >> 3] ^= 0x80 >> (b & 7)
            try:
                got = ss.decode_picture(subs[:k] + [bytes(bad)] + subs[k + 1:], cfg.width, cfg.height, cfg.qp, cfg.tools, cfg.bit_depth, wavefront=bool(cfg.wavefront),
                                        sao=sao is not None, strict_levels=False, row_bd=[0, 1, 2] if cfg.tile_rows == 2 else None)
            except ss.SliceError:
                raised += 1
                continue
            if all(np.array_equal(got[0][f], base[0][f]) for f in ec.RT_FIELDS) and np.array_equal(got[2], base[2]) and (sao is None or np.array_equal(got[1], base[1])):
                same += 1
            else:
                changed += 1
    print("flips: %d raised, %d other records, %d unchanged" % (raised, changed, same))
    assert raised + changed == 200 and same == 0 and raised > 0
    zeros = 0
    for name, cfg, recs, sao in corpus[12:40]:                            # a sub-stream whose byte_alignment() has zeros: its last byte ends in 1 0 ... 0
        subs = ec.substreams_of(hevcdl_amd.code_slice_data(cfg, recs, sao))
        last = subs[-1][-1]
        if last & 1:
            continue
        bad = subs[:-1] + [subs[-1][:-1] + bytes([last | 1])]
        with pytest.raises(ss.SliceError):
            ec.decode_substreams(cfg, bad)
        zeros += 1
        if zeros == 3:
            break
    assert zeros == 3


@pytest.mark.skipif(not os.path.exists(REF_DEC), reason="reference decoder build (oracle/_ref) only exists in the survey container")
def test_reference_decoder_accepts_synthetic_streams(tmp_path):
    """The first 12 corpus pictures, a corpus picture with two tile rows, the directed picture with two tile columns and the directed wavefront picture: the reference
    decoder returns 0 without an ERROR.  (The tiles pictures are four CTUs wide or more: the reference decoder asserts that width for every tile of a profile's
    stream -- a limit on the picture format, not on slice data -- so the corpus pictures of one or two CTU columns with tile rows cannot be offered to it.)"""
    corpus, directed = ec.fuzz_corpus(), ec.directed_pictures()
    assert corpus[17][1].tile_rows == 2 and corpus[17][1].width == 200
    for name, cfg, recs, sao in corpus[:12] + [corpus[17]] + directed[:2]:
        (tmp_path / "s.bin").write_bytes(ec.host_writer_stream(cfg, recs, sao))
        r = subprocess.run([REF_DEC, "-b", "s.bin", "-o", "dec.yuv"], cwd=tmp_path, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "ERROR" not in r.stdout, (name, r.stdout[-400:], r.stderr[-400:])
