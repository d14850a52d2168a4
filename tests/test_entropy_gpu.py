"""The device entropy coder (csrc/entropy_kernel.hip) on the MI355X: byte for byte the reference's streams, the host instantiation of the same source and the
streams recorded from the former host writer (tests/golden/entropy_host_writer_digests.json); batches, the two-phase wavefront path, the capacity guard, the picture
pipeline.  Inputs: tests/entropy_cases.py."""
import os

import numpy as np
import pytest

import entropy_cases as ec

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("path", ec.CASES, ids=lambda p: os.path.basename(p)[3:-4])
def test_fixture_streams_without_sao(path):
    import hevcdl_amd
    cfg, recs, want = ec.fixture_case(path)
    coded = hevcdl_amd.code_slice_data(cfg, recs, device=0)
    ec.check_guard(coded)
    assert ec.assemble(cfg, coded) == want


@pytest.mark.parametrize("name", ec.SAO_CASES)
def test_fixture_streams_with_sao(name, oracle_built):
    import hevcdl_amd
    cfg, recs, sao = ec.sao_case(name)
    dev = hevcdl_amd.code_slice_data(cfg, recs, sao, device=0)
    assert same_coded(dev, hevcdl_amd.code_slice_data(cfg, recs, sao))
    ec.assert_recorded_stream("sao_" + name, cfg, recs, sao, ec.assemble(cfg, dev))


def same_coded(a, b):
    """Two code_slice_data results: lengths, overflow words and the stored bytes of every sub-stream."""
    if not (np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])):
        return False
    for f in range(a[0].shape[0]):
        for k in range(len(a[3])):
            n = min(int(a[1][f, k]), int(a[4][k]))
            if not np.array_equal(a[0][f, a[3][k]:a[3][k] + n], b[0][f, b[3][k]:b[3][k] + n]):
                return False
    return True


def test_fuzz_corpus_equals_the_host_instantiation():
    """... and, assembled, the stream recorded from the former host writer."""
    import hevcdl_amd
    for name, cfg, recs, sao in ec.fuzz_corpus():
        dev = hevcdl_amd.code_slice_data(cfg, recs, sao, device=0)
        ec.check_guard(dev)
        assert same_coded(dev, hevcdl_amd.code_slice_data(cfg, recs, sao)), name
        ec.assert_recorded_stream(name, cfg, recs, sao, ec.assemble(cfg, dev))


def test_batches():
    """Frames of three fixtures of one size and QP in one launch: every sub-stream is what its own launch gives, whatever its position; two runs agree.  The
    launches of 3 and 5 single-sub-stream pictures, and the phase-1 launch of the 7 wavefront pictures (one wave per picture), are no multiple of the four waves of a
    workgroup; the 28 rows of those 7 pictures are one."""
    import hevcdl_amd
    parts = [ec.fixture_case(os.path.join(ec.GOLD, "rd_c128_q32_d%d.npz" % d)) for d in (0, 1, 2)]
    cfg = parts[0][0]
    solo = [hevcdl_amd.code_slice_data(cfg, p[1], device=0) for p in parts]
    for order in ([0, 1, 2], [2, 0, 1, 0], [1, 1, 2, 0, 2]):
        recs = np.concatenate([parts[i][1] for i in order])
        batch = hevcdl_amd.code_slice_data(cfg, recs, device=0)
        assert same_coded(batch, hevcdl_amd.code_slice_data(cfg, recs, device=0))
        at = 0
        for i in order:
            n = parts[i][1].shape[0]
            assert same_coded(tuple(x[at:at + n] for x in batch[:3]) + batch[3:], solo[i])
            at += n
    wcfg, wrecs, _ = ec.fixture_case(os.path.join(ec.GOLD, "rd_w200_q27_r2.npz"))      # 2 pictures x 4 rows, and once more with 7 pictures x 4 rows
    many = np.concatenate([wrecs, wrecs, wrecs, wrecs[:1]])
    assert same_coded(hevcdl_amd.code_slice_data(wcfg, many, device=0), hevcdl_amd.code_slice_data(wcfg, many))
    assert same_coded(hevcdl_amd.code_slice_data(cfg, np.concatenate([p[1] for p in parts])[:5], device=0), hevcdl_amd.code_slice_data(cfg, np.concatenate([p[1] for p in parts])[:5]))


@pytest.mark.parametrize("name", ["w64_q32_r", "w128_q22_r", "w200_q27_r2", "w200_q30_b10"])
def test_wavefront_two_phase_path(name):
    import hevcdl_amd
    cfg, recs, want = ec.fixture_case(os.path.join(ec.GOLD, "rd_%s.npz" % name))
    assert cfg.wavefront == 1
    assert ec.assemble(cfg, hevcdl_amd.code_slice_data(cfg, recs, device=0)) == want


def test_wavefront_synthetic_13x7_ctus():
    import hevcdl_amd
    w, h = 13 * 64 - 8, 7 * 64 - 24
    rng = np.random.default_rng(99)
    recs = ec.synth_records(rng, w, h)[None]
    sao = ec.synth_sao(rng, recs.shape[1], 8)[None]
    cfg = hevcdl_amd.stream_config(w, h, 29, sao=True, wavefront=True)
    dev = hevcdl_amd.code_slice_data(cfg, recs, sao, device=0)
    assert dev[1].shape == (1, 7) and same_coded(dev, hevcdl_amd.code_slice_data(cfg, recs, sao))
    assert ec.assemble(cfg, dev) == ec.host_writer_stream(cfg, recs, sao)


@pytest.mark.parametrize("name", ["c192_q32_r2", "t576_q27_2x3", "w200_q27_r2"])
def test_overflow_is_flagged_and_nothing_is_written_past_the_region(name):
    """The canaries lie inside the device allocation (the whole buffer is uploaded and downloaded): nothing here reads or writes outside allocated memory."""
    import hevcdl_amd
    cfg, recs, _ = ec.fixture_case(os.path.join(ec.GOLD, "rd_%s.npz" % name))
    small = hevcdl_amd.code_slice_data(cfg, recs, capacity_per_ctu=16, device=0)
    ec.check_guard(small)
    assert small[2].any() and same_coded(small, hevcdl_amd.code_slice_data(cfg, recs, capacity_per_ctu=16))


@pytest.mark.parametrize("layout", ["plain", "wavefront", "tiles", "sao10"])
def test_garbage_records_stay_inside_the_guard(layout):
    import hevcdl_amd
    cfg = hevcdl_amd.stream_config(640, 1280, 30, sao=layout == "sao10", tiles=(2, 3) if layout == "tiles" else (1, 1), bit_depth=10 if layout == "sao10" else 8, wavefront=layout == "wavefront")
    recs = ec.garbage_records(7, 200)[None]
    sao = ec.garbage_sao(8, 200)[None] if layout == "sao10" else None
    for cpc in (0, 64):
        dev = hevcdl_amd.code_slice_data(cfg, recs, sao, capacity_per_ctu=cpc, device=0)
        ec.check_guard(dev)
        assert same_coded(dev, hevcdl_amd.code_slice_data(cfg, recs, sao, capacity_per_ctu=cpc))


@pytest.mark.parametrize("w,h,n,bd", [(416, 240, 3, 8), (200, 136, 2, 10)])
def test_pipeline_stream_equals_chunked_plus_host_writer(w, h, n, bd):
    import hevcdl_amd
    import ref_tools
    yuv = ref_tools.synth_yuv(w, h, n, seed=11)
    if bd == 10:
        yuv = yuv.astype(np.uint16) << 2
    enc = hevcdl_amd.Encoder(w, h, 32, max_frames=n, bit_depth=bd)
    try:
        with pytest.raises(hevcdl_amd.HevcdlError) as err:
            enc.get_slice_data(0, 1)
        assert err.value.status == 1                                   # switch off: HEVCDL_ERR_INVALID_ARG
        plain = enc.encode_pictures_chunked(yuv, chunk_frames=2)
        want = []
        for first, recs, pics, sao, stats in plain:
            want += [hevcdl_amd.write_access_unit(w, h, 32, first + i, recs[i], sao=sao[i], bit_depth=bd) for i in range(recs.shape[0])]
        enc.enable_device_entropy(True)
        cfg = hevcdl_amd.stream_config(w, h, 32, sao=True, bit_depth=bd)
        got = []
        for first, data, sizes, stats, pics, recs in enc.encode_pictures_stream(yuv, chunk_frames=2):
            assert pics is None and recs is None
            got += [hevcdl_amd.write_access_unit_from_slice_data(cfg, first + i, data[i], sizes[i]) for i in range(len(data))]
        assert got == want
        chunks = enc.encode_pictures_stream(yuv, want_pictures=True, want_records=True)
        assert np.array_equal(chunks[0][4], np.concatenate([c[2] for c in plain])) and np.array_equal(chunks[0][5], np.concatenate([c[1] for c in plain]))
        inside = []                                                       # the old callback, switch on: hevcdl_get_slice_data INSIDE it gives the chunk's payload

        def hook(first, count):
            data, sizes = enc.get_slice_data(first, count)
            inside.extend((first + i, hevcdl_amd.write_access_unit_from_slice_data(cfg, first + i, data[i], sizes[i])) for i in range(count))
        again = enc.encode_pictures_chunked(yuv, chunk_frames=2, on_chunk_hook=hook)
        assert [poc for poc, _ in inside] == list(range(n)) and [au for _, au in inside] == want
        assert enc.entropy_info()[0] == 0                                 # no picture went to the host
        data, sizes = enc.get_slice_data(0, n)                            # and it stays valid until the next call
        assert [hevcdl_amd.write_access_unit_from_slice_data(cfg, i, data[i], sizes[i]) for i in range(n)] == want
        assert all(np.array_equal(a[1], b[1]) for a, b in zip(again, plain))
        enc.enable_device_entropy(False)
        with pytest.raises(hevcdl_amd.HevcdlError):
            enc.get_slice_data(0, 1)
    finally:
        enc.close()


def test_pipeline_overflow_falls_back_to_the_host_writer():
    """A capacity of 16 bytes per CTU (hevcdl_set_entropy_capacity, a test entry point) makes sub-streams overflow: those pictures are coded on the host from
    their records (hevcdl_host_writer_slice_data: the same coder with the room it asks for), the batch is put together in picture order, and the access units are the same bytes.  Picture 1 is flat and fits even 16 bytes per CTU (12 CTUs:
    256 bytes), the others do not fit 64 (832 bytes), so kernel-coded and host-coded pictures meet in one batch; a second batch follows one with fallbacks."""
    import hevcdl_amd
    import ref_tools
    w, h, n = 200, 136, 4
    yuv = ref_tools.synth_yuv(w, h, n, seed=13)
    yuv[1] = 128                                                          # a flat picture codes to a few bytes: it fits where the others overflow
    enc = hevcdl_amd.Encoder(w, h, 27, max_frames=n)
    try:
        plain = enc.encode_pictures_chunked(yuv)
        want = [hevcdl_amd.write_access_unit(w, h, 27, c[0] + i, c[1][i], sao=c[3][i]) for c in plain for i in range(c[1].shape[0])]
        cfg = hevcdl_amd.stream_config(w, h, 27, sao=True)
        seen = []
        for cpc in (16, 64):
            enc.set_entropy_capacity(cpc)
            enc.enable_device_entropy(True)
            with pytest.raises(hevcdl_amd.HevcdlError):
                enc.set_entropy_capacity(0)                               # only while the switch is off
            for _ in range(2):                                            # a second batch after one with fallbacks
                got = [hevcdl_amd.write_access_unit_from_slice_data(cfg, c[0] + i, c[1][i], c[2][i]) for c in enc.encode_pictures_stream(yuv, chunk_frames=3) for i in range(len(c[1]))]
                assert got == want
            seen.append(enc.entropy_info()[0])
            enc.enable_device_entropy(False)
        print("pictures coded on the host at 16 and 64 bytes per CTU:", seen)
        assert seen[0] >= n - 1 and 0 < seen[1] < n
    finally:
        enc.close()


def test_encode_sequence_with_device_entropy(tmp_path):
    """pipeline.encode_sequence(device_entropy=True) writes the stream and the reconstruction of the run without it."""
    import ref_tools
    from hevcdl_amd import pipeline
    w, h, n = 200, 136, 3
    ref_tools.synth_yuv(w, h, n, seed=17).tofile(tmp_path / "in.yuv")
    outs = []
    for key in (False, True):
        b, r = str(tmp_path / ("s%d.bin" % key)), str(tmp_path / ("s%d.yuv" % key))
        pipeline.encode_sequence(str(tmp_path / "in.yuv"), w, h, 32, n, b, r, wavefront=True, device_entropy=key, log=lambda *a: None)
        outs.append((open(b, "rb").read(), open(r, "rb").read()))
    assert outs[0] == outs[1] and len(outs[0][0]) > 500


@pytest.mark.parametrize("extra", [[], ["--WaveFrontSynchro=1"], ["--NumTileColumnsMinus1=1", "--NumTileRowsMinus1=1", "--TileUniformSpacing=1"], ["--SEIDecodedPictureHash=1"], ["--Devices=0,0"], ["--LoopFilterDisable=1", "nofiles"]],
                         ids=["default", "wavefront", "tiles2x2", "md5", "devices", "no_records_no_pictures"])
def test_cli_device_entropy_changes_no_output(extra, tmp_path):
    """--DeviceEntropy 1: stream, reconstruction file, record file and the log's picture lines and summary are those of the same command without the key.  The last case
    names no record file and no reconstruction file and disables the loop filter, so the run fetches neither records nor pictures from the device."""
    import re
    import subprocess
    import hevcdl_amd
    import ref_tools
    from test_app_cli import CFG_MAIN
    app = hevcdl_amd.build_app()
    w, h, n = 576, 192, 3
    ref_tools.synth_yuv(w, h, n, seed=21).tofile(tmp_path / "in.yuv")
    (tmp_path / "main.cfg").write_text(CFG_MAIN)
    nofiles = "nofiles" in extra
    extra = [e for e in extra if e != "nofiles"]
    outs = []
    for key in (0, 1):
        tag = "e%d" % key
        (tmp_path / (tag + ".cfg")).write_text("InputFile : in.yuv\nInputBitDepth : 8\nInputChromaFormat : 420\nFrameRate : 30\nFrameSkip : 0\nSourceWidth : %d\nSourceHeight : %d\n"
                                               "FramesToBeEncoded : %d\nLevel : 3.1\nBitstreamFile : %s.bin\n%s" % (w, h, n, tag, "" if nofiles else "ReconFile : %s.yuv\n" % tag))
        args = ["-c", "main.cfg", "-c", tag + ".cfg", "-q", "32", "--DeviceEntropy=%d" % key] + ([] if nofiles else ["--RecordFile=" + tag + ".rec"]) + extra
        r = subprocess.run([app] + args, cwd=tmp_path, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
        lines = r.stdout.splitlines()
        at = [i for i, ln in enumerate(lines) if ln.startswith("SUMMARY")]
        log = [re.sub(r"\[ET[^\]]*\]", "", ln) for ln in lines if ln.startswith("POC")] + (lines[at[0]:at[0] + 4] if at else [])
        assert sum(ln.startswith("POC") for ln in log) == n and at
        assert nofiles == (not (tmp_path / (tag + ".yuv")).exists()) and nofiles == (not (tmp_path / (tag + ".rec")).exists())
        outs.append(((tmp_path / (tag + ".bin")).read_bytes(), b"" if nofiles else (tmp_path / (tag + ".yuv")).read_bytes(), b"" if nofiles else (tmp_path / (tag + ".rec")).read_bytes(), log))
    assert outs[0][0] == outs[1][0] and len(outs[0][0]) > 1000
    assert outs[0][1] == outs[1][1] and outs[0][2] == outs[1][2] and outs[0][3] == outs[1][3]


# ---- the device coder's bytes through the decoder (oracle/slice_spec.py), and the edges of its output staging ----------------------------------------------
def _device_round_trip(name, cfg, recs, sao):
    import hevcdl_amd
    dev = hevcdl_amd.code_slice_data(cfg, recs, sao, device=0)
    ec.check_guard(dev)
    decoded = ec.decode_substreams(cfg, ec.substreams_of(dev))            # straight from the device's buffer: the host instantiation is not in between
    ec.assert_round_trip(name, cfg, recs[0], None if sao is None else sao[0], decoded)


@pytest.mark.parametrize("size", ["8x8", "64x8", "8x72", "72x72"])
def test_device_round_trip_of_the_small_corpus_pictures(size):
    """Every corpus picture of at most 4 CTUs (34 per size): what the decoder reads out of the device coder's sub-streams is the canonical form of the input."""
    picks = [c for c in ec.fuzz_corpus() if c[0].endswith("_" + size)]
    assert len(picks) == 34
    for name, cfg, recs, sao in picks:
        _device_round_trip(name, cfg, recs, sao)


@pytest.mark.parametrize("which", [1, 2], ids=["wavefront_3x3_sao", "two_tile_rows_10bit_sao"])
def test_device_round_trip_of_the_two_launch_path_and_a_tile_origin(which):
    name, cfg, recs, sao = ec.directed_pictures()[which]
    assert (cfg.wavefront == 1 and recs.shape[1] == 9) if which == 1 else (cfg.tile_rows == 2 and (cfg.width, cfg.height) == (136, 200))
    _device_round_trip(name, cfg, recs, sao)


@pytest.mark.parametrize("kind", sorted(ec.STAGE_SEEDS))
def test_stage_edges(kind):
    """One sub-stream that ends on, one byte behind and one byte before a 256-byte stage boundary, and with 1, 2, 3 bytes in its last dword: first the host
    instantiation confirms the residue the committed seed is there for, then the device gives the same bytes and length inside intact canaries."""
    import hevcdl_amd
    cfg, recs, length = ec.stage_picture(kind)
    host = hevcdl_amd.code_slice_data(cfg, recs)
    assert host[1].shape == (1, 1) and int(host[1][0, 0]) == length > 256
    want = {"on_boundary": length % 256 == 0, "one_past": length % 256 == 1, "one_before": length % 256 == 255, "tail_1": length % 4 == 1, "tail_2": length % 4 == 2, "tail_3": length % 4 == 3}
    assert want[kind]
    dev = hevcdl_amd.code_slice_data(cfg, recs, device=0)
    ec.check_guard(dev)
    assert int(dev[1][0, 0]) == length and not dev[2].any() and ec.substreams_of(dev) == ec.substreams_of(host)


def test_stage_edges_short_substream_and_a_later_wave():
    """A sub-stream shorter than one dword (a flat 8x8 picture: 3 bytes), and five stage-edge pictures in one launch: waves 1, 2 and 3 of the first workgroup and
    wave 0 of a second one code an edge case too, not only the launch's first wave."""
    import hevcdl_amd
    cfg, recs = ec.flat_picture()
    host, dev = hevcdl_amd.code_slice_data(cfg, recs), hevcdl_amd.code_slice_data(cfg, recs, device=0)
    ec.check_guard(dev)
    assert 2 <= int(host[1][0, 0]) < 4 and same_coded(dev, host) and ec.substreams_of(dev) == ec.substreams_of(host)
    cfg, last, length = ec.stage_picture("on_boundary")
    batch = np.concatenate([ec.stage_picture(k)[1] for k in ("tail_1", "tail_2", "tail_3", "one_before")] + [last])
    host, dev = hevcdl_amd.code_slice_data(cfg, batch), hevcdl_amd.code_slice_data(cfg, batch, device=0)
    ec.check_guard(dev)
    assert int(dev[1][4, 0]) == length and same_coded(dev, host)
    assert [ec.substreams_of(dev, f) for f in range(5)] == [ec.substreams_of(host, f) for f in range(5)]


@pytest.mark.parametrize("kind", ["tail_3", "one_past", "on_boundary"])
def test_capacity_edges(kind):
    """The region's capacity c on and beside the true length L rounded down to a dword (L4) and the last stage boundary below L (B): the reported size is L, the overflow
    word is set exactly when L > c, the stored bytes are the head of the full stream, the canaries (inside the allocation, as in the tests above) are intact, and the
    device result is the host's."""
    import hevcdl_amd
    cfg, recs, length = ec.stage_picture(kind)
    full = ec.substreams_of(hevcdl_amd.code_slice_data(cfg, recs))[0]
    assert len(full) == length
    l4, b = length & ~3, ((length - 1) // 256) * 256
    seen = set()
    for c in sorted({l4 - 4, l4, l4 + 4, b - 4, b, b + 4}):
        cpc = c - 64                                                      # one CTU: its region holds capacity_per_ctu + 64 bytes
        assert cpc > 0 and cpc % 4 == 0 and int(hevcdl_amd.slice_data_layout(cfg, cpc)[3][0]) == c
        host, dev = hevcdl_amd.code_slice_data(cfg, recs, capacity_per_ctu=cpc), hevcdl_amd.code_slice_data(cfg, recs, capacity_per_ctu=cpc, device=0)
        for coded in (host, dev):
            ec.check_guard(coded)
            buf, sizes, ovf, off, cap = coded
            assert int(cap[0]) == c and int(sizes[0, 0]) == length and bool(ovf[0, 0]) == (length > c)
            n = min(length, c)
            assert buf[0, int(off[0]):int(off[0]) + n].tobytes() == full[:n]
        assert same_coded(dev, host)
        seen.add(length > c)
    assert seen == {False, True}
