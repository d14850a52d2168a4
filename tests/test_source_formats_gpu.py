"""Source files in 4:0:0, 4:2:2 and 4:4:4, swapped chroma planes and an explicit window on the device (csrc/source_kernel.hip, the *_fmt kernels): the kernels against
the host functions byte for byte, the picture pipeline with such a format against runs of the reference encoder (tests/golden/srcfmt_*.npz), and the CLI end to end."""
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
CASES = sorted(glob.glob(os.path.join(GOLD, "srcfmt_*.npz")))
# Source sizes: rows shorter than one 16-sample piece (8 x 8, 10 x 8: coded chroma 4 and 8 wide), a piece hanging over both row ends, an odd chroma width (34 x 18: 17,
# 66 x 42: 33, 130 x 74: 65), more than one workgroup a plane and the batch stride (130 x 74 with 3 pictures).  The coded size is ConformanceWindowMode 1's; none of
# these sizes reaches a multiple of 8 with 12 more rows, so the mode-2 padding of 12 rows rides on a sixth source, 34 x 20 -> 40 x 32 (padding 6 / 12).
SIZES = [((8, 8), 1, 0, 0), ((10, 8), 1, 0, 0), ((34, 18), 1, 0, 0), ((66, 42), 1, 0, 0), ((130, 74), 1, 0, 0), ((34, 20), 2, 6, 12)]
DEPTHS = [(8, 8), (8, 10), (10, 8), (16, 10)]      # file depth -> internal depth
OFFSETS = (0, 1, 3)                                # samples between a 16-byte boundary and the first sample of a device buffer
GUARD = 64


def dt(bd):
    return np.uint8 if bd <= 8 else np.dtype("<u2")


def samples(shape, bd, other_bd, seed):
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


def run_dev(fn, a, want, n, off_a, off_b):
    """fn(d_a, n, d_b) on device copies of `a` that start off_a / off_b samples behind a 16-byte boundary -> asserts the bytes of `want` and untouched guards."""
    import torch
    sa, sb = a.dtype.itemsize, want.dtype.itemsize
    pa, pb = GUARD + off_a * sa, GUARD + off_b * sb
    d_a = torch.full((a.nbytes + 2 * GUARD + 8,), 0x5A, dtype=torch.uint8, device="cuda")
    d_b = torch.full((want.nbytes + 2 * GUARD + 8,), 0xA5, dtype=torch.uint8, device="cuda")
    assert d_a.data_ptr() % 16 == 0 and d_b.data_ptr() % 16 == 0
    if a.nbytes:
        d_a[pa:pa + a.nbytes] = torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).cuda()
    fn(d_a.data_ptr() + pa, n, d_b.data_ptr() + pb)
    torch.cuda.synchronize()
    got = d_b.cpu().numpy()
    assert got[pb:pb + want.nbytes].tobytes() == want.tobytes()
    assert (got[:pb] == 0xA5).all() and (got[pb + want.nbytes:] == 0xA5).all()      # the guard words around the output


@pytest.mark.parametrize("cf", [400, 422, 444])
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d_m%d" % (s[0] + (s[1],)))
def test_load_kernel_equals_the_host_function(size, cf):
    import hevcdl_amd
    (sw, sh), mode, px, py = size
    cw, ch = hevcdl_amd.padded_size(sw, sh, mode, px, py)
    for bd in (8, 10):
        enc = hevcdl_amd.Encoder(cw, ch, 32, max_frames=3, bit_depth=bd)
        try:
            for in_bd in [i for i, b in DEPTHS if b == bd]:
                for swap in ((0,) if cf == 400 else (0, 1)):
                    fmt = hevcdl_amd.source_format(sw, sh, in_bd, bd, chroma_format=cf, colour_space=swap)
                    enc.set_source_format(fmt)
                    for n in (1, 3):
                        src = samples((n, fmt.source_samples), in_bd, bd, 3 * sw + in_bd + n + cf)
                        want = hevcdl_amd.load_source_host(fmt, cw, ch, bd, src)
                        if swap == 0:
                            assert enc.load_source(src).tobytes() == want.tobytes(), (in_bd, bd, n)      # host buffers: only the file's bytes go up
                        for off_a in OFFSETS:
                            for off_b in OFFSETS:
                                if swap and off_a != off_b:
                                    continue
                                run_dev(enc.load_source_dev, src, want, n, off_a, off_b)
        finally:
            enc.close()


WINDOWS = [(2, 0, 0, 2), (4, 2, 6, 8), (62, 0, 0, 38)]      # the last one is two samples wide and two high (chroma: one sample)


@pytest.mark.parametrize("bd", [8, 10])
@pytest.mark.parametrize("win", WINDOWS, ids=lambda w: "%d_%d_%d_%d" % w)
def test_windowed_store_kernel_equals_the_host_function(win, bd):
    import hevcdl_amd
    cw, ch = 72, 40
    enc = hevcdl_amd.Encoder(cw, ch, 32, max_frames=3, bit_depth=bd)
    try:
        for out_bd in (8, 10):
            for cs, internal in ((0, 0), (1, 0), (1, 1)):
                fmt = hevcdl_amd.source_format(cw, ch, 8, out_bd, colour_space=cs, output_internal_colour_space=internal, conf_win=win)
                enc.set_source_format(fmt)
                for n in (1, 3):
                    pics = samples((n, cw * ch * 3 // 2), bd, out_bd, 5 * out_bd + n + win[0])
                    want = hevcdl_amd.store_output_host(fmt, cw, ch, bd, pics)
                    assert want.shape == (n, fmt.output_samples)
                    if cs == 0:
                        assert enc.store_output(pics).tobytes() == want.tobytes()
                    for off_a in OFFSETS:
                        for off_b in (OFFSETS if cs == 0 else (off_a,)):
                            run_dev(enc.store_output_dev, pics, want, n, off_a, off_b)
        with pytest.raises(hevcdl_amd.HevcdlError) as err:      # a window together with padding
            enc.set_source_format(hevcdl_amd.source_format(cw - 8, ch, 8, 8, conf_win=(2, 0, 0, 0)))
        assert err.value.status == 1
    finally:
        enc.close()


def test_swapped_store_of_a_padded_picture_and_plain_formats_unchanged():
    """YCbCrtoYCrCb with padding (the window is the source size, the planes change places on the way out), and a format whose new fields are zero next to it."""
    import hevcdl_amd
    sw, sh, cw, ch = 66, 42, 72, 48
    enc = hevcdl_amd.Encoder(cw, ch, 32, max_frames=2)
    try:
        pics = samples((2, cw * ch * 3 // 2), 8, 8, 9)
        src = samples((2, sw * sh * 3 // 2), 8, 8, 10)
        for kw in (dict(colour_space=1), dict(colour_space=1, output_internal_colour_space=1), dict()):
            fmt = hevcdl_amd.source_format(sw, sh, 8, 8, **kw)
            enc.set_source_format(fmt)
            assert enc.store_output(pics).tobytes() == hevcdl_amd.store_output_host(fmt, cw, ch, 8, pics).tobytes(), kw
            assert enc.load_source(src).tobytes() == hevcdl_amd.load_source_host(fmt, cw, ch, 8, src).tobytes(), kw
    finally:
        enc.close()


# ---- the reference's runs ------------------------------------------------------------------------------------------------------------------------------------------
def coded_planes(frame, w, h):
    return [frame[:w * h].reshape(h, w), frame[w * h:w * h * 5 // 4].reshape(h // 2, w // 2), frame[w * h * 5 // 4:].reshape(h // 2, w // 2)]


def measured_sse(f, coded, final):
    """Per picture [Y, U, V]: over the coded picture minus the padding (mode 3: the whole picture), U and V in the file's order unless SNRInternalColourSpace."""
    sw, sh, w, h = (int(f[k]) for k in ("source_width", "source_height", "width", "height"))
    out = []
    for o_, r_ in zip(coded, final):
        row = []
        for c, (o, r) in enumerate(zip(coded_planes(o_, w, h), coded_planes(r_, w, h))):
            d = o[:sh >> (c > 0), :sw >> (c > 0)].astype(np.int64) - r[:sh >> (c > 0), :sw >> (c > 0)].astype(np.int64)
            row.append(int((d * d).sum()))
        out.append([row[0], row[2], row[1]] if int(f["colour_space"]) and not int(f["snr_internal_colour_space"]) else row)
    return out


@pytest.mark.parametrize("path", CASES, ids=lambda p: os.path.basename(p)[7:-4])
def test_pipeline_with_a_file_layout_reproduces_the_reference_run(path):
    """Encoder.set_source_format + encode_pictures / _chunked / _stream on the SOURCE frames of every fixture: the reference's stream (all four window offsets in the SPS,
    hash SEI over the coded picture), its reconstruction file from the device's window store, and the squared errors behind its PSNR columns in its column order."""
    import hevcdl_amd
    from test_source_formats import case_format, case_conf_win, coded_source, log_psnr, psnr_columns
    f = np.load(path)
    fmt = case_format(f)
    w, h, qp, bd = (int(f[k]) for k in ("width", "height", "qp", "bit_depth"))
    src = coded_source(f)
    n = src.shape[0]
    coded = hevcdl_amd.load_source_host(fmt, w, h, bd, src)
    conf_win = case_conf_win(f)
    lines = [l for l in f["stdout"].tolist() if l.startswith("POC")]
    enc = hevcdl_amd.Encoder(w, h, qp, max_frames=n, bit_depth=bd)
    try:
        enc.set_source_format(fmt)
        enc.enable_quality(True)
        recs, pics, sao, stats = enc.encode_pictures(src, f["labels"])
        stream = b"".join(hevcdl_amd.write_access_unit(w, h, qp, poc, recs[poc], sao=sao[poc], bit_depth=bd, conf_win=conf_win) + hevcdl_amd.picture_hash_sei(w, h, pics[poc], bd) for poc in range(n))
        assert stream == f["bitstream"].tobytes()
        assert enc.store_output(pics).tobytes() == f["recon_file"].tobytes()
        assert enc.get_output_frames(0, n).tobytes() == f["recon_file"].tobytes()
        want_sse = measured_sse(f, coded, pics)
        q = enc.get_quality(0, n)
        assert q["sse"].tolist() == want_sse
        for poc in range(n):      # the log's own columns from those numbers
            assert ["%.4f" % v for v in psnr_columns(f, coded[poc], pics[poc])] == ["%.4f" % v for v in log_psnr(lines[poc])]
        if int(f["colour_space"]):      # MS-SSIM follows the same column order: U is the quality of one coded chroma plane, V of the other
            internal = enc_quality_internal(hevcdl_amd, f, src, w, h, qp, bd, n)
            order = [0, 1, 2] if int(f["snr_internal_colour_space"]) else [0, 2, 1]
            assert [[row[k] for k in order] for row in internal["msssim"].tolist()] == q["msssim"].tolist()
        enc.enable_quality(False)
        chunks = enc.encode_pictures_chunked(src, f["labels"], chunk_frames=2)
        assert np.concatenate([c[2] for c in chunks]).tobytes() == pics.tobytes() and np.concatenate([c[1] for c in chunks]).tobytes() == recs.tobytes()
        enc.enable_device_entropy(True)
        enc.enable_picture_report(True, 1)
        chunks = enc.encode_pictures_stream(src, f["labels"], want_pictures=False)
        rep = enc.get_picture_report(0, n)
        scfg = hevcdl_amd.stream_config(w, h, qp, sao=True, bit_depth=bd, conf_win=conf_win)
        slices = [s for c in chunks for s in c[1]]
        sizes = np.concatenate([c[2] for c in chunks])
        stream2 = b"".join(hevcdl_amd.write_access_unit_from_slice_data(scfg, poc, slices[poc], sizes[poc]) + hevcdl_amd.hash_sei(1, hevcdl_amd.report_digest(rep[poc])) for poc in range(n))
        assert stream2 == f["bitstream"].tobytes()
        assert rep["sse"].tolist() == want_sse
        assert all(c[4] is None for c in chunks) and enc.get_output_frames(0, n).tobytes() == f["recon_file"].tobytes()
    finally:
        enc.close()


def enc_quality_internal(hevcdl_amd, f, src, w, h, qp, bd, n):
    """The same run with SNRInternalColourSpace 1: the quality in the coded plane order."""
    fmt = hevcdl_amd.source_format(int(f["source_width"]), int(f["source_height"]), int(f["input_bit_depth"]), int(f["output_bit_depth"]), chroma_format=int(f["chroma_format"]),
                                   colour_space=1, snr_internal_colour_space=1)
    enc = hevcdl_amd.Encoder(w, h, qp, max_frames=n, bit_depth=bd)
    try:
        enc.set_source_format(fmt)
        enc.enable_quality(True)
        enc.encode_pictures(src, f["labels"])
        return enc.get_quality(0, n)
    finally:
        enc.close()


@pytest.mark.parametrize("case,entropy,report", [("444_swap_m1_68x44", False, False), ("win3_80x48_8to10_o8", True, True), ("400_60_m2_8to10", False, False)])
def test_encode_sequence_with_a_file_layout(tmp_path, case, entropy, report):
    import hevcdl_amd
    from hevcdl_amd import pipeline
    from test_source_formats import case_format, log_psnr
    f = np.load(os.path.join(GOLD, "srcfmt_%s.npz" % case))
    w, h, qp, bd = (int(f[k]) for k in ("width", "height", "qp", "bit_depth"))
    f["yuv"].tofile(tmp_path / "in.yuv")
    fmt = case_format(f)
    n = f["yuv"].shape[0]
    summ, rows = pipeline.encode_sequence(str(tmp_path / "in.yuv"), w, h, qp, n, str(tmp_path / "s.bin"), str(tmp_path / "s.yuv"), bit_depth=bd, hash_sei=True, source_format=fmt,
                                          labels_fn=lambda first, count: f["labels"][first:first + count], device_entropy=entropy, device_report=report, log=lambda *a: None)
    assert (tmp_path / "s.bin").read_bytes() == f["bitstream"].tobytes() and (tmp_path / "s.yuv").read_bytes() == f["recon_file"].tobytes()
    # the rows' squared errors give the PSNR columns of the reference's log, in its column order
    sw, sh = int(f["source_width"]), int(f["source_height"])
    lines = [l for l in f["stdout"].tolist() if l.startswith("POC")]
    for row, line in zip(np.asarray(rows), lines):
        cols = [999.99 if int(s) == 0 else 10.0 * np.log10(float(255 << (bd - 8)) ** 2 * (sw * sh / (4 if c else 1)) / int(s)) for c, s in enumerate(row[2:5])]
        assert ["%.4f" % v for v in cols] == ["%.4f" % v for v in log_psnr(line)]


def cli_inputs(tmp_path, f):
    f["yuv"].tofile(tmp_path / "in.yuv")
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


@pytest.mark.parametrize("path", CASES, ids=lambda p: os.path.basename(p)[7:-4])
def test_cli_reproduces_the_reference_run(path, tmp_path):
    """The reference's own keys on the reference's own input file (the temporally subsampled read among them): stream and reconstruction file byte for byte, picture lines
    and summary as the reference printed them; with --DeviceEntropy=1 --DeviceReport=1 the same once more."""
    import hevcdl_amd
    app = hevcdl_amd.build_app()
    f = np.load(path)
    cli_inputs(tmp_path, f)
    keys = ["--InputBitDepth=%d" % int(f["input_bit_depth"]), "--InputChromaFormat=%d" % int(f["chroma_format"]), "-f", str(int(f["source_frames"]))] + [str(k) for k in f["keys"]]
    base = [app, "-i", "in.yuv", "-wdt", str(int(f["source_width"])), "-hgt", str(int(f["source_height"])), "-q", str(int(f["qp"])), "--LabelDir=pred", "--Level=6.2", "--SEIDecodedPictureHash=1"] + keys
    want = log_of([str(l) for l in f["stdout"]])
    for tag, extra in (("plain", []), ("device", ["--DeviceEntropy=1", "--DeviceReport=1"])):
        r = subprocess.run(base + ["-b", tag + ".bin", "-o", tag + ".yuv"] + extra, cwd=tmp_path, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
        assert (tmp_path / (tag + ".bin")).read_bytes() == f["bitstream"].tobytes(), tag
        assert (tmp_path / (tag + ".yuv")).read_bytes() == f["recon_file"].tobytes(), tag
        assert log_of(r.stdout.splitlines()) == want, tag
    if int(f["temporal_subsample_ratio"]) > 1:      # the same over two device entries: the blocks read their own source frames
        r = subprocess.run(base + ["-b", "multi.bin", "-o", "multi.yuv", "--Devices=0,0"], cwd=tmp_path, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
        assert (tmp_path / "multi.bin").read_bytes() == f["bitstream"].tobytes() and (tmp_path / "multi.yuv").read_bytes() == f["recon_file"].tobytes()


def test_cli_refuses_444_without_chroma_format_idc(tmp_path):
    import hevcdl_amd
    app = hevcdl_amd.build_app()
    f = np.load(os.path.join(GOLD, "srcfmt_444_72x40.npz"))
    cli_inputs(tmp_path, f)
    r = subprocess.run([app, "-i", "in.yuv", "-wdt", "72", "-hgt", "40", "-q", "32", "--LabelDir=pred", "--InputChromaFormat=444", "-b", "x.bin"], cwd=tmp_path, capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and [l for l in f["refusal_444"].tolist() if "ChromaFormatConstraint" in l][0] in (r.stdout + r.stderr).splitlines()
    assert not (tmp_path / "x.bin").exists()
