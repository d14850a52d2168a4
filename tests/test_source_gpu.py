"""Source pictures of any size and bit depth on the device (csrc/source_kernel.hip): the load and store kernels against the host functions byte for byte, the picture
pipeline with a source format against runs of the reference encoder (tests/golden/source_*.npz), window SSE and MS-SSIM, and the CLI end to end."""
import glob
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import GOLD
import quality_ref as qr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = sorted(glob.glob(os.path.join(GOLD, "source_*.npz")))
# (source size, coded size): ConformanceWindowMode 1 of the small sizes; 200 x 136 without padding and with 8 / 16 (more than one workgroup a plane)
SIZES = [((2, 2), (8, 8)), ((6, 10), (8, 16)), ((66, 42), (72, 48)), ((70, 2), (72, 8)), ((200, 136), (200, 136)), ((200, 136), (208, 152))]


def dt(bd):
    return np.uint8 if bd <= 8 else np.dtype("<u2")


def samples(shape, bd, other_bd, seed):
    """Random samples of depth bd with both rails and the midpoints of the rounding shift to other_bd among them."""
    rng = np.random.default_rng(seed)
    top = (1 << bd) - 1
    v = rng.integers(0, top + 1, int(np.prod(shape)))
    special = [0, 1, top, top - 1]
    if bd > other_bd:
        half = 1 << (bd - other_bd - 1)
        special += [half - 1, half, half + 1, top - half, top - half + 1, 3 * half]
    pos = rng.integers(0, v.size, min(v.size, 8 * len(special)))
    v[pos] = np.resize(np.array(special), pos.size)
    return v.astype(dt(bd)).reshape(shape)


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d_in_%dx%d" % (s[0] + s[1]))
def test_kernels_equal_the_host_functions(size, bd):
    """hevcdl_load_source / hevcdl_store_output (host buffers) and the device entry points with pointers that are only sample aligned, for input and output depths 8, 10
    and 12 and batches of 1 and 3 pictures: the bytes of hevcdl_load_source_host / hevcdl_store_output_host.  What lies around the device buffers is left alone."""
    import torch
    import hevcdl_amd
    (sw, sh), (cw, ch) = size
    ss, cs = sw * sh * 3 // 2, cw * ch * 3 // 2
    enc = hevcdl_amd.Encoder(cw, ch, 32, max_frames=3, bit_depth=bd)
    try:
        with pytest.raises(hevcdl_amd.HevcdlError) as err:      # no format set
            enc.load_source_dev(1, 1, 1)
        assert err.value.status == 1
        for io_bd in (8, 10, 12):
            fmt = hevcdl_amd.source_format(sw, sh, io_bd, io_bd)
            enc.set_source_format(fmt)
            for n in (1, 3):
                src = samples((n, ss), io_bd, bd, 3 * sw + io_bd + n)
                pics = samples((n, cs), bd, io_bd, 5 * cw + io_bd + n)
                want_coded = hevcdl_amd.load_source_host(fmt, cw, ch, bd, src)
                want_out = hevcdl_amd.store_output_host(fmt, cw, ch, bd, pics)
                assert enc.load_source(src).tobytes() == want_coded.tobytes(), (io_bd, n)
                assert enc.store_output(pics).tobytes() == want_out.tobytes(), (io_bd, n)
                # device buffers that start one sample behind a 64-byte boundary (the unaligned path of both sides), canaries around them
                for a, b, fn in ((src, want_coded, enc.load_source_dev), (pics, want_out, enc.store_output_dev)):
                    sa, sb = a.dtype.itemsize, b.dtype.itemsize
                    d_a = torch.full((a.nbytes + 128,), 0x5A, dtype=torch.uint8, device="cuda")
                    d_b = torch.full((b.nbytes + 128,), 0xA5, dtype=torch.uint8, device="cuda")
                    d_a[64 + sa:64 + sa + a.nbytes] = torch.from_numpy(a.view(np.uint8).reshape(-1)).cuda()
                    fn(d_a.data_ptr() + 64 + sa, n, d_b.data_ptr() + 64 + sb)
                    torch.cuda.synchronize()
                    got = d_b.cpu().numpy()
                    assert got[64 + sb:64 + sb + b.nbytes].tobytes() == b.tobytes(), (io_bd, n, fn.__name__)
                    assert (got[:64 + sb] == 0xA5).all() and (got[64 + sb + b.nbytes:] == 0xA5).all()
            if io_bd > 8 or bd > 8:      # a pointer that is not sample aligned is refused, not run
                d = torch.zeros(4 * max(ss, cs) * 3 + 64, dtype=torch.uint8, device="cuda")
                with pytest.raises(hevcdl_amd.HevcdlError) as err:
                    enc.load_source_dev(d.data_ptr() + (1 if io_bd > 8 else 0), 1, d.data_ptr() + (1 if bd > 8 else 0))
                assert err.value.status == 1
        with pytest.raises(hevcdl_amd.HevcdlError):      # a source larger than the context's picture
            enc.set_source_format(hevcdl_amd.source_format(cw + 2, ch, 8, 8))
        enc.set_source_format(None)
        assert enc.source_format is None
    finally:
        enc.close()


def window(pics, cw, ch, sw, sh):
    """[n, coded samples] -> [n, window samples] at the same depth"""
    out = []
    for fr in pics:
        ps = [fr[:cw * ch].reshape(ch, cw), fr[cw * ch:cw * ch * 5 // 4].reshape(ch // 2, cw // 2), fr[cw * ch * 5 // 4:].reshape(ch // 2, cw // 2)]
        out.append(np.concatenate([p[:sh >> (c > 0), :sw >> (c > 0)].ravel() for c, p in enumerate(ps)]))
    return np.stack(out)


def plane_sse(a, b, sw, sh):
    d = (a.astype(np.int64) - b.astype(np.int64)) ** 2
    y = sw * sh
    return [[int(r[:y].sum()), int(r[y:y + y // 4].sum()), int(r[y + y // 4:].sum())] for r in d]


@pytest.mark.parametrize("path", CASES, ids=lambda p: os.path.basename(p)[7:-4])
def test_pipeline_with_a_source_format_reproduces_the_reference_run(path, oracle_built):
    """hevcdl_encode_pictures on the SOURCE frames of every fixture: records, filtered picture and SAO parameters are the oracle's on the host-converted picture, the stream
    (window in the SPS, hash SEI over the coded picture) is the reference's; the statistics' SSE, the quality's SSE and MS-SSIM and the report's SSE are the window's.
    Then with device entropy and the picture report on: the same stream from slice data and report digests."""
    import hevcdl_amd
    from test_source import oracle_run
    f = np.load(path)
    sw, sh, w, h, qp = (int(f[k]) for k in ("source_width", "source_height", "width", "height", "qp"))
    bd, obd = int(f["bit_depth"]), int(f["output_bit_depth"])
    fmt, coded, o_recs, o_final, o_params, o_stream = oracle_run(f)
    assert o_stream == f["bitstream"].tobytes()
    n = coded.shape[0]
    src = f["yuv"].astype(dt(int(f["input_bit_depth"])))
    win_org = window(coded, w, h, sw, sh)
    enc = hevcdl_amd.Encoder(w, h, qp, max_frames=n, bit_depth=bd)
    try:
        enc.set_source_format(fmt)
        enc.enable_quality(True)
        recs, pics, sao, stats = enc.encode_pictures(src, f["labels"])
        for k in hevcdl_amd.REC_DTYPE.names:
            assert np.array_equal(recs[k], o_recs[k]), k
        assert pics.tobytes() == o_final.tobytes() and sao.tobytes() == o_params.tobytes()
        stream = b"".join(hevcdl_amd.write_access_unit(w, h, qp, poc, recs[poc], sao=sao[poc], bit_depth=bd, conf_win=(w - sw, h - sh)) + hevcdl_amd.picture_hash_sei(w, h, pics[poc], bd)
                          for poc in range(n))
        assert stream == f["bitstream"].tobytes()
        assert enc.store_output(pics).tobytes() == f["recon_file"].tobytes()      # the device's crop and scaling of its own pictures: the reference's reconstruction file
        q = enc.get_quality(0, n)
        want_sse = plane_sse(win_org, window(pics, w, h, sw, sh), sw, sh)
        assert q["sse"].tolist() == want_sse
        if obd == bd and int(f["input_bit_depth"]) == bd:      # the file's own samples are the window's at the internal depth: the SSE recomputed from the reference's files
            assert q["sse"].tolist() == plane_sse(src, np.frombuffer(f["recon_file"].tobytes(), dt(obd)).reshape(n, -1), sw, sh)
        for i in range(n):      # MS-SSIM of the window's planes: the same kernels on a plane of that size
            for c, (o, r) in enumerate(zip(qr.planes(win_org[i], sw, sh), qr.planes(window(pics, w, h, sw, sh)[i], sw, sh))):
                _, ms = hevcdl_amd.plane_quality(o, r, bd)
                assert q["msssim"][i][c] == ms or (np.isnan(ms) and np.isnan(q["msssim"][i][c])), (i, c)
        # the statistics: SSE of the reconstruction before the in-loop filters, over the window
        _, recon, _, stats0 = enc.encode_pictures(src, f["labels"], deblock=False, sao=False)
        assert stats0["sse"].tolist() == plane_sse(win_org, window(recon, w, h, sw, sh), sw, sh) and stats["sse"].tolist() == stats0["sse"].tolist()
        enc.enable_quality(False)
        # slice data and report from the device: nothing but them leaves HBM
        enc.enable_device_entropy(True)
        enc.enable_picture_report(True, 1)
        chunks = enc.encode_pictures_stream(src, f["labels"], want_pictures=False)
        rep = enc.get_picture_report(0, n)
        scfg = hevcdl_amd.stream_config(w, h, qp, sao=True, bit_depth=bd, conf_win=(w - sw, h - sh))
        slices = [s for c in chunks for s in c[1]]
        sizes = np.concatenate([c[2] for c in chunks])
        stream2 = b"".join(hevcdl_amd.write_access_unit_from_slice_data(scfg, poc, slices[poc], sizes[poc]) + hevcdl_amd.hash_sei(1, hevcdl_amd.report_digest(rep[poc])) for poc in range(n))
        assert stream2 == f["bitstream"].tobytes()
        assert rep["sse"].tolist() == want_sse
        assert all(c[4] is None for c in chunks) and enc.get_output_frames(0, n).tobytes() == f["recon_file"].tobytes()      # the reconstruction file's frames without the coded pictures leaving HBM
        assert enc.get_output_frames(n - 1, 1).tobytes() == f["recon_file"].tobytes()[-len(f["recon_file"]) // n:]
        with pytest.raises(hevcdl_amd.HevcdlError):
            enc.get_output_frames(n, 1)
    finally:
        enc.close()


def test_without_a_source_format_nothing_changes():
    """A small existing fixture through the picture pipeline with no format set, and again after a format was set and cleared: the reference's pictures and stream as before."""
    import hevcdl_amd
    f = np.load(os.path.join(GOLD, "rd_c192_q32_r2.npz"))
    w, h, qp, n = int(f["width"]), int(f["height"]), int(f["qp"]), f["yuv"].shape[0]
    enc = hevcdl_amd.Encoder(w, h, qp, max_frames=n)
    try:
        outs = []
        for step in range(2):
            recs, pics, sao, stats = enc.encode_pictures(f["yuv"], f["labels"])
            assert pics.tobytes() == f["recon_filtered"].tobytes()
            stream = b"".join(hevcdl_amd.write_access_unit(w, h, qp, poc, recs[poc], sao=sao[poc]) + hevcdl_amd.picture_hash_sei(w, h, pics[poc]) for poc in range(n))
            assert stream == f["bitstream"].tobytes()
            outs.append((recs.tobytes(), sao.tobytes(), stats.tobytes()))
            enc.set_source_format(hevcdl_amd.source_format(w - 4, h - 2, 8, 8))
            enc.set_source_format(None)
        assert outs[0] == outs[1]
    finally:
        enc.close()


@pytest.mark.parametrize("entropy,report", [(False, False), (True, True)])
def test_encode_sequence_with_a_source_format(tmp_path, entropy, report):
    """pipeline.encode_sequence(source_format=...) on the reference's own input file (8-bit, 66 x 42, coded at 10 bits): the reference's stream and reconstruction file,
    rows with the window's squared errors -- on the host path and with slice data and reports from the device."""
    import hevcdl_amd
    from hevcdl_amd import pipeline
    f = np.load(os.path.join(GOLD, "source_b66x42_8to10_m1.npz"))
    sw, sh, w, h, qp, bd = (int(f[k]) for k in ("source_width", "source_height", "width", "height", "qp", "bit_depth"))
    f["yuv"].astype(np.uint8).tofile(tmp_path / "in.yuv")
    fmt = hevcdl_amd.source_format(sw, sh, 8, int(f["output_bit_depth"]))
    assert hevcdl_amd.padded_size(sw, sh, 1) == (w, h)
    n = f["yuv"].shape[0]
    summ, rows = pipeline.encode_sequence(str(tmp_path / "in.yuv"), w, h, qp, n, str(tmp_path / "s.bin"), str(tmp_path / "s.yuv"), bit_depth=bd, hash_sei=True, source_format=fmt,
                                          labels_fn=lambda first, count: f["labels"][first:first + count], device_entropy=entropy, device_report=report, log=lambda *a: None)
    assert (tmp_path / "s.bin").read_bytes() == f["bitstream"].tobytes() and (tmp_path / "s.yuv").read_bytes() == f["recon_file"].tobytes()
    coded = hevcdl_amd.load_source_host(fmt, w, h, bd, f["yuv"])
    final = np.frombuffer(f["recon_file"].tobytes(), "<u2").reshape(n, -1)      # the output depth is the internal one here: the file is the window of the final picture
    assert [list(map(int, r[2:5])) for r in np.asarray(rows)] == plane_sse(window(coded, w, h, sw, sh), final, sw, sh)


def cli_inputs(tmp_path, f):
    f["yuv"].astype(dt(int(f["input_bit_depth"]))).tofile(tmp_path / "in.yuv")
    labels = f["labels"]
    for fr in range(labels.shape[0]):
        os.makedirs(tmp_path / "pred" / str(fr))
        for a in range(labels.shape[1]):
            (tmp_path / "pred" / str(fr) / ("ctu%d.txt" % a)).write_text(" ".join(str(int(v)) for v in labels[fr, a]))


def log_of(lines):
    """Picture lines without [ET ...] and the reference build's "nQP <n> ", with their hash text, and the two lines of the summary block."""
    poc = [re.sub(r"nQP -?\d+ ", "", qr.strip_et(l)) + " " + l[l.index("[MD5:"):].strip() for l in lines if l.startswith("POC")]
    i = next(k for k, l in enumerate(lines) if l.startswith("SUMMARY"))
    return poc, [l.rstrip() for l in lines[i + 1:i + 3]]


@pytest.mark.parametrize("case", ["a68x44_m1", "b66x42_8to10_m1", "e64_10to8_o10", "q100x76_m1_quality"])
def test_cli_reproduces_the_reference_run(case, tmp_path):
    """The reference's own keys on the reference's own input file: stream and reconstruction file byte for byte, picture lines (PSNR, MSE and MS-SSIM over the window) and
    summary as the reference printed them; with --DeviceEntropy=1 --DeviceReport=1 the same once more."""
    import hevcdl_amd
    app = hevcdl_amd.build_app()
    f = np.load(os.path.join(GOLD, "source_%s.npz" % case))
    cli_inputs(tmp_path, f)
    bd, obd = int(f["bit_depth"]), int(f["output_bit_depth"])
    keys = ["--InputBitDepth=%d" % int(f["input_bit_depth"]), "--InternalBitDepth=%d" % bd, "--Profile=%s" % ("main" if bd == 8 else "main10"), "--ConformanceWindowMode=%d" % int(f["mode"])]
    keys += ["--OutputBitDepth=%d" % obd, "--OutputBitDepthC=%d" % obd] if obd != bd else []
    keys += [str(k) for k in f["keys"]]
    base = [app, "-i", "in.yuv", "-wdt", str(int(f["source_width"])), "-hgt", str(int(f["source_height"])), "-q", str(int(f["qp"])), "--LabelDir=pred", "--Level=6.2", "--SEIDecodedPictureHash=1"] + keys
    want = log_of([str(l) for l in f["stdout"]])
    for tag, extra in (("plain", []), ("device", ["--DeviceEntropy=1", "--DeviceReport=1"])):
        r = subprocess.run(base + ["-b", tag + ".bin", "-o", tag + ".yuv"] + extra, cwd=tmp_path, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
        assert (tmp_path / (tag + ".bin")).read_bytes() == f["bitstream"].tobytes(), tag
        assert (tmp_path / (tag + ".yuv")).read_bytes() == f["recon_file"].tobytes(), tag
        assert log_of(r.stdout.splitlines()) == want, tag
