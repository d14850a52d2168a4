"""Pictures of several slices and dependent slice segments against the DECODER (oracle/slice_spec.py): the decoder is first pinned to the reference encoder's
multi-NAL streams (tests/golden/slices_*.npz, segments_*.npz), then the synthetic layout corpus (entropy_cases.layout_corpus) goes records -> coder / writer -> bytes ->
decoder -> records under every layout hevcdl_write_access_unit_segments accepts.  A tally holds the corpus to the paths it is there for, damaged streams and three
mutants of the decoder show that the check can fail.  No GPU (the device coder on the same corpus: tests/test_entropy_slices_gpu.py)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import entropy_cases as ec
import segments_cases as gc
import slices_cases as sc
from test_entropy_roundtrip import REF_DEC, access_units, inside_mask

NEW_TALLY = ("slices", "segments_dependent", "segment_ends_mid_slice", "split_ctx_slice_edge", "sao_merge_up_slice_edge", "sao_merge_left_slice_edge", "cand_above_other_slice",
             "entry_points_in_dependent_header", "emulation_bytes_in_multi_nal_picture")


# ---- the extended decoder against the reference encoder ------------------------------------------------------------------------------------------------------
def _fixture(kind, path):
    """-> (name, case, layout, [(stream, with SAO)], SAO parameters [frames, ctus, 3] by the oracle or None)."""
    import hevcdl_amd
    if kind == "slices":
        import test_slices
        c = sc.Case(path)
        lay = ec._lay(tiles=c.tiles, slices=c.slices, lf_across_slices=c.lf_slices, choice=c.choice(), lf_offsets=c.offsets)
        params = test_slices.filtered(c)[0] if c.sao else None
        streams = [(c.stream, c.sao)]
        cfg = test_slices.stream_cfg(c, c.sao)
    else:
        import test_segments
        c = gc.Case(path)
        lay = ec._lay(tiles=c.tiles, wavefront=c.wavefront, slices=c.slices, segments=c.segments)
        params = test_segments.filtered(c)[1]
        streams = [(c.stream, True), (c.stream_nosao, False)]
        cfg = test_segments.stream_cfg(c, True)
    if params is not None:
        params = np.ascontiguousarray(params).view(hevcdl_amd.SAO_DTYPE).reshape(c.nf, -1, 3)
    return c, cfg, lay, streams, params


@pytest.mark.parametrize("kind,path", [("slices", p) for p in sc.CASES] + [("segments", p) for p in gc.CASES], ids=lambda v: os.path.basename(v)[:-4] if v.endswith(".npz") else None)
def test_decoder_reproduces_the_reference_encoders_slices_and_segments(kind, path, oracle_built):
    """Every access unit of every slice and segment fixture (with SAO, and the run without it where the fixture has one): the headers say the fixture's layout -- the
    number of NAL units, which are dependent, the addresses --, the records are the fixture's in every field the stream carries (the masks of
    test_decoder_reproduces_the_reference_encoders_records), and with SAO the parameters are the ones the oracle computes on the fixture.  w64x192_a1, one CTU wide,
    decides the rule at a wavefront row start whose neighbour T does not exist: initialise (ctx_init_at_row_start)."""
    import hevcdl_amd
    import slice_spec as ss
    c, cfg, lay, streams, params = _fixture(kind, path)
    recs = c.records(hevcdl_amd.REC_DTYPE)
    borders, (cb, rb), wpp = ec.segment_borders(cfg, lay)
    if kind == "slices":
        assert len(borders) == c.n_slices
    else:
        assert [d for _, d, _, _ in borders] == c.dependent
    ins = inside_mask(c.w, c.h)
    for stream, with_sao in streams:
        aus = access_units(sc.strip_sei(stream))
        assert len(aus) == c.nf
        for poc, au in enumerate(aus):
            got, sao, mask, tally, info = ss.decode_access_unit(au)
            assert (info["width"], info["height"], info["qp"], info["bit_depth"], info["wavefront"], info["sao"]) == (c.w, c.h, c.qp, c.bd, wpp, with_sao)
            assert (info["col_bd"], info["row_bd"]) == (list(cb), list(rb))
            assert [(g["address"], g["dependent"], len(g["substreams"])) for g in info["segments"]] == [(a, d, n) for a, d, _, n in borders]
            assert [g["first_slice"] for g in info["segments"]] == [1] + [0] * (len(borders) - 1)
            assert tally["level_out_of_range"] == 0 and tally["slices"] == sum(1 - d for _, d, _, _ in borders) and tally["segments_dependent"] == sum(d for _, d, _, _ in borders)
            assert tally["ctx_restore_from_previous_segment"] == 0
            if c.name == "w64x192_a1":
                assert tally["ctx_init_at_row_start"] == 2 and tally["ctx_sync_from_above"] == 0
            if lay["choice"] is not None:
                assert info["dbk"] == tuple(lay["choice"][1:])
            for k in ("depth", "part_size", "luma_dir", "chroma_dir", "tr_idx"):
                assert np.array_equal(got[k][ins], recs[poc][k][ins]), k
            for comp in range(3):
                assert np.array_equal(got["cbf"][:, comp][ins], recs[poc]["cbf"][:, comp][ins])
            assert np.array_equal(got["tskip"][mask], recs[poc]["tskip"][mask]) and not got["tskip"][~mask].any()
            for k in ("coeff_y", "coeff_cb", "coeff_cr"):
                assert np.array_equal(got[k], recs[poc][k]), k
            if with_sao:
                scfg = hevcdl_amd.stream_config(c.w, c.h, c.qp, sao=True, tiles=lay["tiles"], bit_depth=c.bd, tools=c.tools, wavefront=lay["wavefront"])
                _, want = ec.canonical_layout(scfg, recs[poc], params[poc], mask, lay)
                assert np.array_equal(sao, want), [a for a in range(len(want)) if not np.array_equal(sao[a], want[a])][:4]
            else:
                assert sao is None


# ---- the layout corpus ----------------------------------------------------------------------------------------------------------------------------------
_RUN = {}


def corpus_run():
    """Every layout picture through the shared coder on the host, both writers and both decoder entries, once per session -> {name: (coded, access unit, decoded from the
    buffer, decoded from the access unit)}."""
    import slice_spec as ss
    if not _RUN:
        for name, cfg, recs, sao, lay in ec.layout_corpus():
            coded = ec.code_layout(cfg, recs, sao, lay)
            from_buffer = ec.decode_layout_substreams(cfg, lay, ec.substreams_of(coded))
            a, b = ec.write_layout_access_units(cfg, recs, sao, lay, coded)
            assert a == b, "%s: the two writers differ" % name
            from_au = ss.decode_access_unit(a, strict_levels=False, picture_decoder=ec.cached_decode_picture, segments_decoder=ec.cached_decode_picture_segments)
            _RUN[name] = (coded, a, from_buffer, from_au)
    return _RUN


def test_the_corpus_is_what_the_issue_asks_for():
    corpus = ec.layout_corpus()
    assert 60 <= len(corpus) <= 100 and all(c[2].shape[1] <= 12 for c in corpus) and len({c[0] for c in corpus}) == len(corpus)
    kinds = {c[0].split("_")[-1] for c in corpus}
    assert kinds >= {"rs1", "rs1lf0", "rs2", "ts1", "ts2", "ws1", "ws2", "tg1", "tg2", "ts2g1", "ts3g2", "rs1dbk", "t12s5g2", "w1x3"}
    assert {c[1].bit_depth for c in corpus} == {8, 10} and {c[3] is None for c in corpus} == {False, True}
    twelve = next(c for c in corpus if c[0].endswith("t12s5g2"))
    assert [n for _, _, _, n in ec.segment_borders(twelve[1], twelve[4])[0]] == [2, 2, 1, 2, 2, 1, 2] and [d for _, d, _, _ in ec.segment_borders(twelve[1], twelve[4])[0]] == [0, 1, 1, 0, 1, 1, 0]


def test_round_trip_of_the_shared_coder_under_every_layout():
    """code_slice_data(layout=, segments=) -> decode_picture_segments on the buffer's sub-streams and the layout's borders -> the canonical records and SAO parameters."""
    run = corpus_run()
    for name, cfg, recs, sao, lay in ec.layout_corpus():
        ec.assert_layout_round_trip(name, cfg, recs[0], None if sao is None else sao[0], lay, run[name][2])


def test_round_trip_through_the_writers_and_the_access_unit_entry():
    """hevcdl_write_access_unit_segments and the shared coder + hevcdl_write_access_unit_from_slice_data_segments give the same bytes (corpus_run), and through
    decode_access_unit the canonical records, the headers the layout implies, and every NAL unit within hevcdl_access_unit_bound_segments."""
    import hevc_parse as hp
    import hevcdl_amd
    run = corpus_run()
    lib = hevcdl_amd.load_library()
    beyond = []
    for name, cfg, recs, sao, lay in ec.layout_corpus():
        coded, au, _, out = run[name]
        info = out[4]
        borders, (cb, rb), wpp = ec.segment_borders(cfg, lay)
        assert (info["width"], info["height"], info["qp"], info["bit_depth"], info["sao"], info["wavefront"]) == (cfg.width, cfg.height, cfg.qp, cfg.bit_depth, sao is not None, wpp), name
        assert (info["col_bd"], info["row_bd"]) == (list(cb), list(rb)) and info["dep_slices"] == (lay["segments"] is not None), name
        assert [(g["first_slice"], g["address"], g["dependent"], len(g["substreams"])) for g in info["segments"]] == [(int(i == 0), a, d, n) for i, (a, d, _, n) in enumerate(borders)], name
        assert info["substreams"] == ec.substreams_of(coded), name
        assert info["lf_across_slices"] == bool(lay["slices"] is None or lay["lf_across_slices"]), name
        if lay["choice"] is not None:
            assert info["dbk"] == tuple(lay["choice"][1:]), name
        for g in info["segments"]:
            assert sum(g["entry_points"]) + len(g["substreams"][-1]) <= g["payload_bytes"]
            assert len(g["entry_points"]) == (len(g["substreams"]) - 1 if (cfg.tile_columns * cfg.tile_rows > 1 or wpp) else 0)
        layout, segments = ec.layout_keys(lay)
        bound = lib.hevcdl_access_unit_bound_segments(cfg.width, cfg.height, hevcdl_amd._layout_ptr(layout), hevcdl_amd._layout_ptr(hevcdl_amd.segment_layout(segments)))
        # hevcdl_access_unit_bound is 3 bytes per luma sample: DESIGN.md (capacity and fallback) records that a picture of +-32767 levels, 3.7 bytes per coefficient, does
        # not fit it and that the writer then answers INVALID_ARG with the length it needs.  Those pictures (M...) are held to that statement, every other one to the bound.
        if name.startswith("M") and len(au) > bound:
            beyond.append(name)
            small, n = np.zeros(bound, np.uint8), ctypes.c_size_t(0)
            cp, _keep = hevcdl_amd._choice_ptr(lay["choice"])
            r, p = np.ascontiguousarray(recs[0]), None if sao is None else np.ascontiguousarray(sao[0])
            st = lib.hevcdl_write_access_unit_segments(ctypes.byref(cfg), hevcdl_amd._layout_ptr(layout), hevcdl_amd._layout_ptr(hevcdl_amd.segment_layout(segments)), 0, r.ctypes.data,
                                                       None if p is None else p.ctypes.data, cp, small.ctypes.data, bound, ctypes.byref(n))
            assert st == 1 and n.value == len(au), name
        else:
            assert len(au) <= bound and all(len(n) <= bound for _, n in hp.split_annexb(au)), name
        ec.assert_layout_round_trip(name, cfg, recs[0], None if sao is None else sao[0], lay, out[:4])
    print("pictures of maximal levels beyond hevcdl_access_unit_bound_segments:", beyond)


def test_the_layout_corpus_reaches_the_paths_it_is_there_for():
    """Conditions on the tally over the layout corpus, decoded from its access units."""
    import slice_spec as ss
    run = corpus_run()
    t = ss.new_tally()
    mixed_len = []
    for name, cfg, recs, sao, lay in ec.layout_corpus():
        out = run[name][3]
        ss.add_tally(t, out[3])
        lens = {(g["dependent"], g["offset_len_minus1"]) for g in out[4]["segments"] if g["entry_points"]}
        if any(d0 != d1 and l0 != l1 for d0, l0 in lens for d1, l1 in lens):
            mixed_len.append(name)
    print({k: t[k] for k in NEW_TALLY + ("ctx_restore_from_previous_segment", "emulation_bytes_under_dependent_entry_points", "ctx_init_at_segment_start", "ctx_init_at_row_start")}, mixed_len)
    for k in NEW_TALLY:
        assert t[k] > 0, k
    # 9.3.1 restores the contexts of the previous segment's end only at a dependent segment that starts neither a tile nor a wavefront row.  The product's segments are
    # whole tiles or whole wavefront rows (csrc/slice_grid.h refuses SliceSegmentMode 1 without WaveFrontSynchro), so the two earlier branches of 9.3.1 always win.
    assert t["ctx_restore_from_previous_segment"] == 0
    assert t["emulation_bytes_under_dependent_entry_points"] > 0          # an emulation prevention byte inside a sub-stream that a dependent header's entry point measures
    assert mixed_len                                                      # an access unit whose independent and dependent headers use different offset_len_minus1
    assert t["ctx_init_at_row_start"] > 0 and t["ctx_sync_from_above"] > 0 and t["ctx_init_at_segment_start"] > 0


# ---- the decoder is strict ------------------------------------------------------------------------------------------------------------------------------
def _join(nals):
    return b"".join(b"\0\0\1" + n for n in nals)


def _flip(nal, bit_in_unescaped):
    """One bit of a NAL unit, addressed in its unescaped form (where the header parser counts)."""
    import slice_spec as ss
    _, pos = ss.unescape_with_positions(nal)
    out = bytearray(nal)
    out[pos[bit_in_unescaped >> 3]] ^= 0x80 >> (bit_in_unescaped & 7)
    return bytes(out)


@pytest.mark.parametrize("kind", ["136x200_rs2", "136x200_ws2", "64x768_t12s5g2"])
def test_a_damaged_multi_nal_picture_never_decodes_to_the_same_records(kind):
    """Row slices, wavefront segments and tile segments in slices (the first corpus picture of each layout, 12 CTUs; the third is the twelve-tile picture, whose slices
    hold dependent segments of two tiles, so that a dependent header has an entry point): a flipped
    dependent_slice_segment_flag, every bit of every slice_segment_address flipped, every bit of the first entry point of a dependent header, every bit of the last
    byte of every segment's last sub-stream, two NAL units swapped, one dropped -- the decoder raises SliceError or returns other records, never the same.  The
    picture of row slices has no dependent header (its PPS has dependent_slice_segments_enabled_flag 0): the two damages of one apply to the other two pictures."""
    import hevc_parse as hp
    import slice_spec as ss
    name, cfg, recs, sao, lay = next(c for c in ec.layout_corpus() if c[0].endswith("_" + kind))
    au = corpus_run()[name][1]
    base = ss.decode_access_unit(au, strict_levels=False)
    nals = [n for _, n in hp.split_annexb(au)]
    first = next(i for i, n in enumerate(nals) if ((n[0] >> 1) & 63) < 32)
    segs = base[4]["segments"]
    assert len(nals) - first == len(segs) >= 2
    damaged = []
    for i, g in enumerate(segs):
        h = g["header"]
        if i > 0:
            if base[4]["dep_slices"]:
                damaged.append(("dependent flag of NAL %d" % i, nals[:first + i] + [_flip(nals[first + i], h["address_bit_pos"] - 1)] + nals[first + i + 1:]))
            for b in range(h["address_bits"]):
                damaged.append(("address bit %d of NAL %d" % (b, i), nals[:first + i] + [_flip(nals[first + i], h["address_bit_pos"] + b)] + nals[first + i + 1:]))
        if g["dependent"] and g["entry_points"]:
            for b in range(h["offset_len_minus1"] + 1):
                damaged.append(("entry point bit %d of NAL %d" % (b, i), nals[:first + i] + [_flip(nals[first + i], h["entry_point_bit_pos"] + b)] + nals[first + i + 1:]))
        for b in range(8):
            n = bytearray(nals[first + i])
            n[-1] ^= 1 << b
            damaged.append(("last byte bit %d of NAL %d" % (b, i), nals[:first + i] + [bytes(n)] + nals[first + i + 1:]))
    for i in range(len(segs) - 1):
        damaged.append(("NAL %d and %d swapped" % (i, i + 1), nals[:first + i] + [nals[first + i + 1], nals[first + i]] + nals[first + i + 2:]))
    for i in range(len(segs)):
        damaged.append(("NAL %d dropped" % i, nals[:first + i] + nals[first + i + 1:]))
    kinds = {k for k in ("dependent flag", "address bit", "entry point bit", "last byte bit", "swapped", "dropped") if any(k in d[0] for d in damaged)}
    assert kinds == {"address bit", "last byte bit", "swapped", "dropped"} | ({"dependent flag", "entry point bit"} if not kind.endswith("rs2") else set()), kinds
    raised = changed = 0
    for what, bad in damaged:
        try:
            got = ss.decode_access_unit(_join(bad), strict_levels=False)
        except ss.SliceError:
            raised += 1
            continue
        same = all(np.array_equal(got[0][f], base[0][f]) for f in ec.RT_FIELDS) and np.array_equal(got[2], base[2]) and (sao is None or np.array_equal(got[1], base[1]))
        assert not same, "%s: %s decodes to the same records" % (name, what)
        changed += 1
    print("%s: %d damages, %d raised, %d other records" % (name, len(damaged), raised, changed))
    assert raised > 0


# ---- mutants of the decoder -------------------------------------------------------------------------------------------------------------------------------
# the first corpus picture that catches each mutant (recorded from a run; the test asserts them, so a corpus that drifts says so)
MUTANTS = {"slice_term": "L14_136x200_rs1", "sao_slice_rule": "L00_8x72_rs1", "mid_slice_end": "M03_8x72_ws1"}


@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_a_mutant_of_the_decoder_fails_the_round_trip(mutant):
    """As tests/test_filters_adversarial.py does for filter_spec: the decoder with the slice term of 6.4.1 switched off, with SAO merge candidates taken across a slice
    border, and with a border between two segments of a slice taken for none must each fail the corpus' round trip -- or the corpus would not notice a coder with the
    same mistake."""
    import slice_spec as ss
    run = corpus_run()
    caught = None
    for name, cfg, recs, sao, lay in ec.layout_corpus():
        try:
            decoded = ec.decode_layout_substreams(cfg, lay, ec.substreams_of(run[name][0]), **{mutant: False})
            ec.assert_layout_round_trip(name, cfg, recs[0], None if sao is None else sao[0], lay, decoded)
        except (ss.SliceError, AssertionError):
            caught = name
            break
    print("mutant %s: first caught by %s" % (mutant, caught))
    assert caught == MUTANTS[mutant]


# ---- the reference decoder ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists(REF_DEC), reason="reference decoder build (oracle/_ref) only exists in the survey container")
def test_reference_decoder_accepts_layout_streams(tmp_path):
    """Row slices, wavefront segments, and -- on the pictures four CTUs wide or more, the width the reference decoder demands of every tile -- tile slices and tile
    segments: the reference decoder returns 0 without an ERROR (no picture hash SEI in the stream)."""
    picks = [c for c in ec.layout_corpus() if c[0].split("_", 1)[1] in ("72x72_rs1", "136x200_rs2", "72x72_ws1", "136x200_ws2", "64x192_w1x3", "200x136_ts2", "200x136_ts2g1", "200x136_ts3g2",
                                                                        "456x64_c2s1", "520x64_c2g1")]
    names = {c[0].split("_", 1)[1] for c in picks}
    assert len(names) == 10
    seen = set()
    for name, cfg, recs, sao, lay in picks:
        if name.split("_", 1)[1] in seen:
            continue
        seen.add(name.split("_", 1)[1])
        (tmp_path / "s.bin").write_bytes(corpus_run()[name][1])
        r = subprocess.run([REF_DEC, "-b", "s.bin", "-o", "dec.yuv"], cwd=tmp_path, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "ERROR" not in r.stdout, (name, r.stdout[-400:], r.stderr[-400:])
