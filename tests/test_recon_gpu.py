"""hevcdl_recon_kernel on the MI355X (csrc/recon_kernel.hip): the reference's unfiltered reconstruction from parsed streams, batches against single pictures, records that
do not validate, and whole decodes assembled from the stages -- parse, reconstruct, deblock, SAO with the stream's parameters -- against the reference's final picture
and the digests of its hash SEI.  Every picture is a few CTUs."""
import os

import numpy as np
import pytest

import entropy_cases as ec
from conftest import GOLD, fixture_tiles, fixture_lf, fixture_lf_offsets
from test_recon import parsed_and_expected, assert_unfiltered

pytestmark = pytest.mark.gpu

TIME_LIMIT = 60                                                           # seconds a test; each takes a second or two


@pytest.fixture(autouse=True)
def own_time_limit():
    """Every test here runs under its own time limit: faulthandler's watchdog thread ends the process when a launch does not return (no Python-level alarm is served
    while the interpreter sits in native code); a test that returns in time disarms it.  The limit ends the WHOLE pytest process, not the one test: the tests behind a
    hang get no verdict.  On a shared GPU that is meant -- nothing more is started on a device that a kernel has just hung."""
    import faulthandler
    faulthandler.dump_traceback_later(TIME_LIMIT, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


# the smallest fixtures that can still go wrong: one 8x8 CU, one row / one column of them, partial CTUs at both extremes of QP, 10 bits, every tool off, tiles, one CTU
# column of wavefront rows, several rows in flight, row slices, wavefront segments
RECON_CASES = ["rd_e8x8_q32", "rd_e64x8_q20", "rd_e8x72_q40", "rd_e136_q0", "rd_e136_q51", "rd_e72_q0_b10", "rd_k200_q27_all0", "rd_t512_q32_2x2", "rd_w64_q32_r", "rd_w200_q27_r2",
               "slices_r128_a2", "segments_w264x136_a5"]


@pytest.mark.parametrize("name", RECON_CASES)
def test_reconstruction_from_records_equals_the_stored_unfiltered_reconstruction(name):
    import hevcdl_amd
    p, f = parsed_and_expected(name)
    dev = hevcdl_amd.reconstruct_frames(p.cfg, p.records, slices=p.slices, qps=p.qps, device=0)
    assert_unfiltered(dev, f, name)
    assert np.array_equal(dev, hevcdl_amd.reconstruct_frames(p.cfg, p.records, slices=p.slices, qps=p.qps))      # ... and the same source on the CPU


def test_a_batch_of_40_pictures_equals_40_single_reconstructions():
    """40 pictures of 64x136 (three CTU rows each, 120 rows on one ticket, more rows than a picture has in flight at any time), synthetic records with levels up to
    +-32767 and every mode, a QP per picture: the batch == the pictures one at a time == the host."""
    import hevcdl_amd
    rng = np.random.default_rng(20250107)
    recs = np.stack([ec.synth_records(rng, 64, 136) for _ in range(40)])
    qps = [int(q) for q in rng.integers(0, 52, 40)]
    for bd in (8, 10):
        cfg = hevcdl_amd.stream_config(64, 136, 30, bit_depth=bd)
        batch = hevcdl_amd.reconstruct_frames(cfg, recs, qps=qps, device=0)
        assert np.array_equal(batch, hevcdl_amd.reconstruct_frames(cfg, recs, qps=qps))
        for i in (0, 1, 17, 39):
            assert np.array_equal(hevcdl_amd.reconstruct_frames(cfg, recs[i:i + 1], qps=qps[i:i + 1], device=0)[0], batch[i]), i
        assert int(batch.max()) <= (1 << bd) - 1 and len(np.unique(batch)) > 16


def test_records_that_fail_validation_launch_nothing():
    import hevcdl_amd
    lib = hevcdl_amd.load_library()
    cfg = hevcdl_amd.stream_config(72, 72, 30)
    good = ec.synth_records(np.random.default_rng(5), 72, 72)[None]
    before = lib.hevcdl_recon_launches()
    hevcdl_amd.reconstruct_frames(cfg, good, device=0)
    assert lib.hevcdl_recon_launches() == before + 1
    bad = good.copy()
    bad["luma_dir"][0, 0, 0] = 35
    for recs in (bad, ec.garbage_records(3, 4)[None]):
        with pytest.raises(hevcdl_amd.HevcdlError) as e:
            hevcdl_amd.reconstruct_frames(cfg, recs, device=0)
        assert e.value.status == 1
    assert lib.hevcdl_recon_launches() == before + 1


DECODES = ["rd_e8x8_q32", "rd_e72_q0_b10", "rd_k200_q27_all0", "rd_t512_q32_2x2", "rd_l576_q32_lf0", "rd_l520_q27_lf0_b10", "rd_o200_q27_bm3_t3", "rd_w200_q27_r2", "rd_x576_q30_2x3"]


@pytest.mark.parametrize("name", DECODES)
def test_whole_decode_from_the_stages_equals_the_reference_picture(name):
    """stream -> hevcdl_parse_stream -> hevcdl_recon_kernel -> deblocking from the parsed records -> SAO with the parsed parameters == the reference's final picture, and
    its MD5 digests are the ones of the stream's hash SEI: nothing of the fixture but the stream goes in."""
    import hevcdl_amd
    p, f = parsed_and_expected(name)
    w, h, bd, nf = p.cfg.width, p.cfg.height, p.cfg.bit_depth, len(p.pictures)
    final = np.frombuffer(f["recon_filtered"].tobytes(), np.uint8 if bd == 8 else np.dtype("<u2")).reshape(nf, -1)
    recon = hevcdl_amd.reconstruct_frames(p.cfg, p.records, slices=p.slices, qps=p.qps, device=0)
    tiles = (p.cfg.tile_columns, p.cfg.tile_rows) if p.cfg.tile_uniform_spacing else fixture_tiles(f)
    e = hevcdl_amd.Encoder(w, h, p.qps[0], max_frames=nf, tiles=tiles, bit_depth=bd, lf_across_tiles=bool(p.cfg.lf_across_tiles),
                           lf_offsets=(p.cfg.lf_beta_offset_div2, p.cfg.lf_tc_offset_div2))
    try:
        out = e.sao_apply_frames(e.deblock_frames(recon, p.records), p.sao)
    finally:
        e.close()
    assert np.array_equal(out, final)
    for i in range(nf):
        method, digest = p.digest(i)
        assert method == 1 and bytes(hevcdl_amd.picture_hash(w, h, out[i], bd, method)) == digest, i


# one or more streams of every family that stores the reference decoder's / encoder's final pictures: per-picture QPs (fqp, dqr), deblocking parameters chosen per picture
# and sent in the slice header, the filter off in the PPS with and without SAO, row and tile slices with the filters stopping at their borders, 10 bits, CRC and checksum
STREAM_DECODES = [("fqp_d192_q32", "bitstream", "recon_file"), ("fqp_t512_q32", "bitstream", "recon_file"), ("fqp_d192_q32_b10", "bitstream", "recon_file"),
                  ("dqr_c128_q30_n1_b10", "bitstream", "recon_file"), ("dqr_t512x128_q32_n1", "bitstream", "recon_file"),
                  ("dbksel_m1_104x72_q37_off", "bitstream", "recon_file"), ("dbksel_inpps0_72x72_q32_dis", "bitstream", "recon_file"), ("dbksel_m2_72x72_q27_b10_off", "bitstream", "recon_file"),
                  ("lfoff_c192_q32", "bitstream_sao", "recon_sao"), ("lfoff_c192_q32", "bitstream_nosao", "recon"),
                  ("slices_r192x200_a6_lf0", "bitstream", "recon_file"), ("slices_t512_a1_lf0", "bitstream", "recon_file"), ("slices_r128_a2_b10", "bitstream", "recon_file"),
                  ("stream_c192_q32", "bitstream_crc10", "recon_crc10"), ("stream_c192_q32", "bitstream_sum", "recon_sum"), ("stream_c192_q32", "bitstream_ps0", "recon_ps0"),
                  ("segments_t512x128_s2_a1", "bitstream", None), ("segments_w264x136_a5", "bitstream", None), ("segments_w64x192_a1", "bitstream", None)]


@pytest.mark.parametrize("name,key,pic_key", STREAM_DECODES, ids=["%s:%s" % (n, k) for n, k, _ in STREAM_DECODES])
def test_decode_stream_gives_the_reference_decoders_pictures(name, key, pic_key):
    """pipeline.decode_stream on a reference stream of every family == the picture file the reference wrote for it, and the digests computed from the decoded pictures
    equal the stream's hash SEI wherever it carries one (the segment fixtures store no final picture: their MD5 SEIs are the reference)."""
    from hevcdl_amd import pipeline
    f = np.load(os.path.join(GOLD, name + ".npz"))
    pictures, p, verdicts = pipeline.decode_stream(f[key].tobytes())
    assert all(v is True for v in verdicts if v is not None), verdicts
    assert pic_key is not None or all(v is True for v in verdicts)
    if pic_key is not None:
        want = np.frombuffer(f[pic_key].tobytes(), pictures.dtype).reshape(len(p.pictures), -1)
        assert np.array_equal(pictures, want)


def test_decode_sequence_writes_the_window_and_reports_every_picture(tmp_path):
    """The file front end on a stream with a conformance window (source_a68x44_m1: 72x48 coded, 68x44 shown): the file is the reference's, one line a picture."""
    from hevcdl_amd import pipeline
    f = np.load(os.path.join(GOLD, "source_a68x44_m1.npz"))
    (tmp_path / "s.bin").write_bytes(f["bitstream"].tobytes())
    lines = []
    pictures, p, verdicts = pipeline.decode_sequence(str(tmp_path / "s.bin"), str(tmp_path / "rec.yuv"), log=lines.append)
    assert (p.cfg.conf_win_right, p.cfg.conf_win_bottom) == (4, 4) and verdicts == [True, True] and len(lines) == 2 and "hash OK" in lines[0]
    assert (tmp_path / "rec.yuv").stat().st_size == 2 * 68 * 44 * 3 // 2
    if "recon_file" in f.files:
        assert (tmp_path / "rec.yuv").read_bytes() == f["recon_file"].tobytes()


@pytest.mark.parametrize("w,h,bd,tiles,kw", [(200, 136, 10, (1, 1), {}), (520, 136, 8, (2, 2), {}), (136, 200, 8, (1, 1), {"wavefront": True})], ids=["200x136_b10", "520x136_t2x2", "136x200_wpp"])
def test_self_round_trip_without_the_reference(tmp_path, w, h, bd, tiles, kw):
    """Random content, encoded by this pipeline (CNN labels, decisions, both filters, the stream with its MD5 SEI) and decoded again: the decoder's pictures are the
    encoder's final pictures, every hash verdict OK -- no reference file involved."""
    from hevcdl_amd import pipeline
    rng = np.random.default_rng(w * 7 + h)
    n = 2
    smooth = np.repeat(np.repeat(rng.integers(40, 200, (n, (h * 3 // 2 + 7) // 8, (w + 7) // 8)), 8, 1), 8, 2)[:, :h * 3 // 2, :w]
    yuv = np.clip(smooth + rng.integers(-12, 13, smooth.shape), 0, 255).astype(np.uint16 if bd > 8 else np.uint8)
    if bd > 8:
        yuv = yuv * 4 + rng.integers(0, 4, yuv.shape).astype(np.uint16)
    yuv.reshape(n, -1).astype("<u2" if bd > 8 else np.uint8).tofile(str(tmp_path / "in.yuv"))
    pipeline.encode_sequence(str(tmp_path / "in.yuv"), w, h, 30, n, bitstream_path=str(tmp_path / "s.bin"), recon_path=str(tmp_path / "enc.yuv"), tiles=tiles, bit_depth=bd,
                             hash_sei=True, log=lambda *a: None, **kw)
    pictures, p, verdicts = pipeline.decode_sequence(str(tmp_path / "s.bin"), str(tmp_path / "dec.yuv"))
    assert verdicts == [True] * n and (p.cfg.bit_depth, p.cfg.tile_columns * p.cfg.tile_rows) == (bd, tiles[0] * tiles[1])
    assert (tmp_path / "dec.yuv").read_bytes() == (tmp_path / "enc.yuv").read_bytes()
    assert len(np.unique(pictures)) > 16


def _cli(args, cwd):
    import subprocess
    import hevcdl_amd
    return subprocess.run([hevcdl_amd.build_decoder_app()] + args, cwd=cwd, capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("name,pic_key", [("rd_w200_q27_r2", "recon_filtered"), ("rd_x576_q30_2x3", "recon_filtered"), ("source_a68x44_m1", "recon_file")], ids=["8bit", "10bit_tiles", "window"])
def test_cli_writes_the_reference_decoders_file(tmp_path, name, pic_key):
    """bin/TAppDecoderHevcdl -b str.bin -o rec.yuv on an 8-bit stream, a 10-bit stream of 2x3 tiles and a stream with a conformance window: the file is the reference's,
    a line a picture with the hash verdict, exit status 0; with one digest byte of the last SEI changed: ***ERROR*** on that picture and exit status 1."""
    f = np.load(os.path.join(GOLD, name + ".npz"))
    stream = f["bitstream"].tobytes()
    (tmp_path / "s.bin").write_bytes(stream)
    r = _cli(["-b", "s.bin", "-o", "rec.yuv"], tmp_path)
    nf = len(f["yuv"]) if "yuv" in f.files else f["records"].shape[0]
    assert r.returncode == 0 and r.stdout.count("(OK)") == nf and "ERROR" not in r.stdout, (r.stdout[-600:], r.stderr[-600:])
    assert (tmp_path / "rec.yuv").read_bytes() == f[pic_key].tobytes()
    bad = bytearray(stream)
    bad[-3] ^= 0x55                                                       # inside the last picture's digest (rbsp_trailing_bits is the last byte)
    (tmp_path / "bad.bin").write_bytes(bytes(bad))
    r = _cli(["-b", "bad.bin"], tmp_path)
    assert r.returncode == 1 and r.stdout.count("***ERROR***") == 1 and r.stdout.count("(OK)") == nf - 1, r.stdout[-600:]
    r = _cli(["-b", "missing.bin"], tmp_path)
    assert r.returncode == 2


def test_cli_converts_the_files_bit_depth(tmp_path):
    """-d 8 on a 10-bit stream: every sample (v + 2) >> 2, clipped; -d 10 on an 8-bit stream: v << 2."""
    for name, d, conv in (("rd_x128_q32_r", 8, lambda a: np.minimum((a.astype(np.int32) + 2) >> 2, 255).astype(np.uint8)), ("rd_c128_q32_d1", 10, lambda a: (a.astype(np.uint16) << 2).astype("<u2"))):
        f = np.load(os.path.join(GOLD, name + ".npz"))
        (tmp_path / "s.bin").write_bytes(f["bitstream"].tobytes())
        r = _cli(["-b", "s.bin", "-o", "rec.yuv", "-d", str(d)], tmp_path)
        assert r.returncode == 0, (r.stdout[-400:], r.stderr[-400:])
        src = np.frombuffer(f["recon_filtered"].tobytes(), np.dtype("<u2") if d == 8 else np.uint8)
        assert (tmp_path / "rec.yuv").read_bytes() == conv(src).tobytes()


def test_decode_stream_verdicts_come_from_the_device_and_refusals_carry_their_sentence():
    """hevcdl_decode_stream: the digests are the report kernels' (a changed SEI digest turns exactly that picture's verdict, the pictures stay the same); a context that
    does not describe the stream and a stream the parser refuses both come back with status and sentence in hevcdl_last_error."""
    import ctypes
    import hevcdl_amd
    lib = hevcdl_amd.load_library()
    for name in ("stream_c192_q32:bitstream_crc", "stream_c192_q32:bitstream_sum10", "rd_w200_q27_r2:bitstream"):
        fix, key = name.split(":")
        stream = np.load(os.path.join(GOLD, fix + ".npz"))[key].tobytes()
        good, _, info, verdicts = hevcdl_amd.decode_stream(stream, batch=2)      # (three pictures in batches of two)
        assert all(v is True for v in verdicts) and len(verdicts) == len(info)
        bad = bytearray(stream)
        bad[-3] ^= 0x55
        pictures, _, _, v2 = hevcdl_amd.decode_stream(bytes(bad), batch=2)
        assert v2 == [True] * (len(v2) - 1) + [False] and np.array_equal(pictures, good)
    stream = np.load(os.path.join(GOLD, "rd_w200_q27_r2.npz"))["bitstream"].tobytes()
    e = hevcdl_amd.Encoder(192, 136, 27, max_frames=2)
    try:
        n = ctypes.c_int(0)
        buf = np.frombuffer(stream, np.uint8)
        st = lib.hevcdl_decode_stream(e._h, buf.ctypes.data, buf.size, None, 0, ctypes.byref(n), None, None)
        assert st == 1 and n.value == 2 and b"does not describe the stream" in lib.hevcdl_last_error(e._h)
        st = lib.hevcdl_decode_stream(e._h, buf.ctypes.data, 40, None, 0, ctypes.byref(n), None, None)
        assert st == 1 and n.value == 0 and lib.hevcdl_last_error(e._h) != b""
    finally:
        e.close()
