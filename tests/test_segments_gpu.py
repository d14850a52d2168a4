"""Dependent slice segments on the device: a context created with SliceSegmentMode / SliceSegmentArgument decides, filters, plans and launches as the context without the
keys; only the entropy kernel's sub-streams that end a segment, and the NAL units round them, change.  Every picture here is a few CTUs."""
import os
import re
import subprocess

import numpy as np
import pytest

import quality_ref as qr
import segments_cases as sg

pytestmark = pytest.mark.gpu
IDS = dict(ids=sg.case_id)
FIELDS = ["depth", "part_size", "luma_dir", "chroma_dir", "tr_idx", "cbf", "tskip", "bits", "dist", "cost", "coeff_y", "coeff_cb", "coeff_cr"]
WAVEFRONT = [p for p in sg.CASES if sg.case_id(p).startswith("w")]


def encoder(c, segments=True):
    import hevcdl_amd
    kw = c.kw()
    if not segments:
        del kw["segments"]
    return hevcdl_amd.Encoder(c.w, c.h, c.qp, max_frames=c.nf, **kw)


def same_records(got, want):
    return [k for k in FIELDS if not np.array_equal(got[k], want[k])]


def stream_cfg(c, sao):
    import hevcdl_amd
    return hevcdl_amd.stream_config(c.w, c.h, c.qp, sao=sao, tiles=c.tiles, bit_depth=c.bd, tools=c.tools, wavefront=c.wavefront)


@pytest.mark.parametrize("path", sg.CASES, **IDS)
def test_decisions_and_launch_are_those_of_the_context_without_the_keys(path):
    """hevcdl_compress_frames on the segment context: the reference's records and unfiltered reconstruction behind every compressCtu, exactly, by the launch the context
    without the keys makes."""
    import hevcdl_amd
    c = sg.Case(path)
    launches = []
    for segments in (True, False):
        e = encoder(c, segments)
        try:
            recs, recon, _ = e.compress_frames(c.yuv, c.labels)
            launches.append((e.lib.hevcdl_last_rd_launch(e._h) or b"").decode())
            lay = hevcdl_amd.SegmentLayout()
            assert e.lib.hevcdl_get_segment_layout(e._h, lay) == 0 and (lay.mode, lay.argument) == (c.segments if segments else (0, 0))
        finally:
            e.close()
        assert same_records(recs, c.records(hevcdl_amd.REC_DTYPE)) == []
        assert np.array_equal(recon, c.prefilter())
    assert launches[0] == launches[1] and launches[0]


@pytest.mark.parametrize("path", sg.CASES, **IDS)
def test_picture_pipeline_gives_the_pictures_and_both_streams(path):
    """hevcdl_encode_pictures with device entropy, with SAO and without: the reference's final (deblocked) picture; its stream through the writer from the records; the
    same stream from the device's slice data, whose sub-streams are the host coder's byte for byte."""
    import hevcdl_amd
    c = sg.Case(path)
    layout = hevcdl_amd.slice_layout(c.slices)
    e = encoder(c)
    try:
        e.enable_device_entropy(True)
        for sao, picture, want in ((True, c.final, c.stream), (False, c.deblocked, c.stream_nosao)):
            recs, final, params, _ = e.encode_pictures(c.yuv, c.labels, deblock=True, sao=sao)
            data, sizes = e.get_slice_data(0, c.nf)
            assert e.entropy_info()[0] == 0
            assert same_records(recs, c.records(hevcdl_amd.REC_DTYPE)) == [] and np.array_equal(final, picture)
            want = sg.strip_sei(want)
            written = b"".join(hevcdl_amd.write_access_unit(c.w, c.h, c.qp, poc, recs[poc], sao=params[poc] if sao else None, tiles=c.tiles, bit_depth=c.bd, tools=c.tools,
                                                            wavefront=c.wavefront, slices=c.slices, segments=c.segments) for poc in range(c.nf))
            assert written == want
            scfg = stream_cfg(c, sao)
            host = hevcdl_amd.code_slice_data(scfg, recs, params if sao else None, layout=layout, segments=c.segments)
            assert sizes.shape == host[1].shape and np.array_equal(sizes, host[1])
            assert [bytes(data[poc]) for poc in range(c.nf)] == [hevcdl_amd.pack_slice_data(host[0][poc], host[1][poc], host[3]) for poc in range(c.nf)]
            got = b"".join(hevcdl_amd.write_access_unit_from_slice_data(scfg, poc, data[poc], sizes[poc], layout=e.slice_layout, segments=e.segment_layout) for poc in range(c.nf))
            assert got == want
    finally:
        e.close()


@pytest.mark.parametrize("name", ["w264x264_a10", "t512x128_s2_a1"])
def test_host_fallback_codes_a_segment_picture(name):
    """A capacity below a sub-stream's length: the sub-streams overflow their regions and the host codes those pictures with the same coder and the context's segment
    layout; the stream is the same."""
    import hevcdl_amd
    c = sg.Case(sg.path_of(name))
    e = encoder(c)
    try:
        e.set_entropy_capacity(8)
        e.enable_device_entropy(True)
        chunks = e.encode_pictures_stream(c.yuv, c.labels, deblock=True, sao=True)
        fallbacks = e.entropy_info()[0]
        layout, segments = e.slice_layout, e.segment_layout
    finally:
        e.close()
    assert fallbacks >= 1
    scfg = stream_cfg(c, True)
    got = b""
    for first, data, sizes, _, _, _ in chunks:
        got += b"".join(hevcdl_amd.write_access_unit_from_slice_data(scfg, first + i, data[i], sizes[i], None, layout=layout, segments=segments) for i in range(len(data)))
    assert got == sg.strip_sei(c.stream)


def test_device_coder_entry_point_with_segments():
    """hevcdl_code_slice_data_segments (the kernels on uploaded records) against hevcdl_code_slice_data_host_segments: the same bytes, lengths and untouched gaps, for rows
    (two a segment, and a picture one CTU wide), tiles, and tiles in slices."""
    import hevcdl_amd
    for name in ("w264x264_a10", "w64x192_a1", "t512x128_a3", "t512x128_s2_a1"):
        c = sg.Case(sg.path_of(name))
        scfg = stream_cfg(c, False)
        layout = hevcdl_amd.slice_layout(c.slices)
        recs = c.records(hevcdl_amd.REC_DTYPE)
        host = hevcdl_amd.code_slice_data(scfg, recs, layout=layout, segments=c.segments)
        dev = hevcdl_amd.code_slice_data(scfg, recs, layout=layout, segments=c.segments, device=0)
        assert np.array_equal(host[1], dev[1]) and not dev[2].any(), name
        off, cap = dev[3], dev[4]
        for poc in range(c.nf):      # the used bytes (the device rounds a sub-stream's last store up to a dword of zeros: inside its region) and the gaps no coder writes
            assert hevcdl_amd.pack_slice_data(host[0][poc], host[1][poc], off) == hevcdl_amd.pack_slice_data(dev[0][poc], dev[1][poc], off), name
            for k in range(len(off)):
                assert (dev[0][poc, int(off[k]) + int(cap[k]):int(off[k]) + int(cap[k]) + 64] == hevcdl_amd.CANARY).all(), name
        aus = b"".join(hevcdl_amd.write_access_unit_from_slice_data(scfg, poc, hevcdl_amd.pack_slice_data(dev[0][poc], dev[1][poc], off), dev[1][poc], layout=layout, segments=c.segments)
                       for poc in range(c.nf))
        assert aus == sg.strip_sei(c.stream_nosao), name


@pytest.mark.parametrize("path", WAVEFRONT, ids=[sg.case_id(p) for p in WAVEFRONT])
def test_per_ctu_session_on_a_segment_context(path):
    """The decisions are unchanged, so the per-CTU session keeps working: every CTU's record is the batched path's, which is the reference's."""
    import hevcdl_amd
    c = sg.Case(path)
    e = encoder(c)
    try:
        recs, recon, _ = e.compress_frames(c.yuv, c.labels)
        e.begin_frames(c.yuv, c.labels)
        for f in range(c.nf):
            for a in range(e.ctus):
                rec, _ = e.compress_ctu(f, a)
                for name in hevcdl_amd.REC_DTYPE.names:
                    assert np.array_equal(rec[0][name], recs[f, a][name]), (f, a, name)
            assert np.array_equal(e.get_recon(f), recon[f].reshape(-1))
    finally:
        e.close()
    assert same_records(recs, c.records(hevcdl_amd.REC_DTYPE)) == []


@pytest.mark.parametrize("name", ["w264x136_a5", "t512x128_s2_a1"])
def test_encode_sequence_takes_the_keys(name, tmp_path):
    """pipeline.encode_sequence with segments=: the reference's stream (hash SEI included) and reconstruction file, host-coded, with device entropy, and with nothing but
    slice data and reports leaving the device."""
    import hevcdl_amd.pipeline as pipeline
    c = sg.Case(sg.path_of(name))
    c.yuv.astype(np.uint8).tofile(tmp_path / "in.yuv")
    for tag, kw in (("host", {}), ("device", dict(device_entropy=True)), ("stream", dict(device_entropy=True, device_report=True))):
        recon = None if tag == "stream" else str(tmp_path / (tag + ".yuv"))
        pipeline.encode_sequence(str(tmp_path / "in.yuv"), c.w, c.h, c.qp, c.nf, bitstream_path=str(tmp_path / (tag + ".bin")), recon_path=recon, batch=c.nf, tiles=c.tiles,
                                 hash_sei=True, labels_fn=lambda b0, nb: c.labels[b0:b0 + nb], log=lambda *a: None, tools=c.tools, wavefront=c.wavefront, slices=c.slices,
                                 segments=c.segments, **kw)
        assert (tmp_path / (tag + ".bin")).read_bytes() == c.stream, tag
        assert recon is None or (tmp_path / (tag + ".yuv")).read_bytes() == c.final.tobytes(), tag


def log_of(lines):
    """Picture lines without [ET ...] and the reference build's "nQP <n> ", with their hash text, and the two lines of the summary block."""
    poc = [re.sub(r"nQP -?\d+ ", "", qr.strip_et(l)) + " " + l[l.index("[MD5:"):].strip() for l in lines if l.startswith("POC")]
    i = next(k for k, l in enumerate(lines) if l.startswith("SUMMARY"))
    return poc, [l.rstrip() for l in lines[i + 1:i + 3]]


@pytest.mark.parametrize("name", ["w264x264_a10", "w64x192_a1", "t512x128_a3", "t512x128_s2_a1"])
def test_cli_reproduces_the_reference_run(name, tmp_path):
    """The reference's own keys on the reference's own input: stream, reconstruction file and log lines (the picture's bit count is all its slice NAL units); with
    --DeviceEntropy=1 --DeviceReport=1 the same once more."""
    import hevcdl_amd
    app = hevcdl_amd.build_app()
    c = sg.Case(sg.path_of(name))
    c.yuv.astype(np.uint8).tofile(tmp_path / "in.yuv")
    for f in range(c.nf):
        os.makedirs(tmp_path / "pred" / str(f))
        for a in range(c.nctu):
            (tmp_path / "pred" / str(f) / ("ctu%d.txt" % a)).write_text(" ".join(str(int(v)) for v in c.labels[f, a]) + " ")
    base = [app, "-i", "in.yuv", "-wdt", str(c.w), "-hgt", str(c.h), "-q", str(c.qp), "-f", str(c.nf), "--LabelDir=pred", "--Level=6.2", "--SEIDecodedPictureHash=1",
            "--InputBitDepth=8", "--Profile=main"] + [str(k) for k in c.f["keys"]]
    want = log_of([str(l) for l in c.f["stdout"]])
    for tag, extra in (("plain", []), ("device", ["--DeviceEntropy=1", "--DeviceReport=1"])):
        r = subprocess.run(base + ["-b", tag + ".bin", "-o", tag + ".yuv"] + extra, cwd=tmp_path, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
        assert (tmp_path / (tag + ".bin")).read_bytes() == c.stream, tag
        assert (tmp_path / (tag + ".yuv")).read_bytes() == c.final.tobytes(), tag
        assert log_of(r.stdout.splitlines()) == want, tag
