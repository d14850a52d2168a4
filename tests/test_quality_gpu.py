"""Row f-3, quality report on the device: csrc/quality_kernel.hip against the f64 restatement of TEncGOP::xCalculateMSSSIM (tests/quality_ref.py), the
pipeline's switch, and the CLI with PrintMSSSIM / PrintFrameMSE / PrintSequenceMSE against the reference encoder's own stdout (tests/golden/quality_*.npz).

Tolerance of msssim: quality_ref.msssim_tolerance -- derived there from the one freedom the kernel has (the order in which a scale's blocks are added), not
measured.  sse is exact."""
import math
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import quality_ref as qr

pytestmark = pytest.mark.gpu


def bits(v):
    return struct.pack("<d", float(v))


def check_plane(o, r, bit_depth, got_sse, got_ms, what):
    want, info = qr.msssim(o, r, bit_depth, details=True)
    tol = qr.msssim_tolerance(want, info)
    print("%s: msssim %.17g (restatement %.17g, |diff| %.3g, tolerance %.3g)  sse %d" % (what, got_ms, want, abs(got_ms - want) if math.isfinite(want) else 0.0, tol, got_sse))
    assert got_sse == qr.sse(o, r), what
    if math.isnan(want):
        assert math.isnan(got_ms), what
    elif tol == 0.0:
        assert got_ms == want and math.copysign(1.0, got_ms) == math.copysign(1.0, want), what      # no freedom: 0 / totalBlocks, exactly
    else:
        assert abs(got_ms - want) <= tol, what


@pytest.mark.parametrize("case", qr.CASES)
def test_kernel_matches_the_restatement_on_the_fixture_pictures(case):
    import hevcdl_amd
    fx = qr.Fixture(case)
    enc = hevcdl_amd.Encoder(fx.width, fx.height, fx.qp, max_frames=fx.n, bit_depth=fx.bit_depth)
    try:
        q = enc.picture_quality(fx.yuv, fx.recon)
        again = enc.picture_quality(fx.yuv, fx.recon)
        assert q.tobytes() == again.tobytes()                         # the same bits on a second run
        for f in range(fx.n):
            for c, (o, r) in enumerate(zip(qr.planes(fx.yuv[f], fx.width, fx.height), qr.planes(fx.recon[f], fx.width, fx.height))):
                check_plane(o, r, fx.bit_depth, int(q["sse"][f][c]), float(q["msssim"][f][c]), "%s picture %d plane %d" % (case, f, c))
                assert "%1.6f" % q["msssim"][f][c] == fx.printed_msssim()[f][c]
    finally:
        enc.close()


# plane sizes on both sides of every cut-off of the number of scales (22 / 44 / 88 / 176), in either dimension, with odd sizes at the lower scales, and planes
# smaller than the window in one or both dimensions (0 / totalBlocks with totalBlocks negative, positive and zero)
SIZES = [(21, 50), (22, 50), (50, 21), (50, 22), (43, 60), (44, 60), (60, 43), (60, 44), (87, 100), (88, 100), (100, 87), (100, 88),
         (175, 190), (176, 190), (190, 175), (190, 176), (45, 47), (91, 93), (183, 181), (365, 183), (8, 8), (8, 30), (10, 10), (11, 11), (300, 20)]


@pytest.mark.parametrize("bit_depth", [8, 10])
def test_kernel_matches_the_restatement_on_random_planes(bit_depth):
    import hevcdl_amd
    rng = np.random.default_rng(20 + bit_depth)
    dt = np.uint8 if bit_depth == 8 else np.uint16
    top = (1 << bit_depth) - 1
    for i, (w, h) in enumerate(SIZES):
        yy, xx = np.mgrid[0:h, 0:w]
        base = (0.5 + 0.35 * np.sin(xx / 9.0 + i) * np.cos(yy / 7.0)) * top
        o = np.clip(base + rng.normal(0, top / 40.0, (h, w)), 0, top).astype(dt)
        kind = i % 3      # noisy copy, smoothed copy, unrelated noise (negative covariances)
        r = np.clip(o.astype(np.float64) + rng.normal(0, top / 30.0, (h, w)), 0, top).astype(dt) if kind == 0 else \
            ((o.astype(np.uint32) + np.roll(o, 1, 1) + np.roll(o, 1, 0) + np.roll(o, 2, 1)) // 4).astype(dt) if kind == 1 else rng.integers(0, top + 1, (h, w)).astype(dt)
        s, ms = hevcdl_amd.plane_quality(o, r, bit_depth)
        check_plane(o, r, bit_depth, s, ms, "%d-bit %dx%d kind %d" % (bit_depth, w, h, kind))
        s2, ms2 = hevcdl_amd.plane_quality(o, r, bit_depth)
        assert (s2, bits(ms2)) == (s, bits(ms))


@pytest.mark.parametrize("bit_depth,w,h", [(8, 352, 176), (10, 176, 88), (8, 88, 48)])
def test_whole_pictures_and_the_position_in_the_batch(bit_depth, w, h):
    """Random 4:2:0 pictures through a context (chroma planes of 176 x 88 / 88 x 44 / 44 x 24: on the cut-offs); the same picture as picture 0 of a batch of one
    and as picture 2 of a batch of three gives the same bits."""
    import hevcdl_amd
    rng = np.random.default_rng(w + bit_depth)
    dt = np.uint8 if bit_depth == 8 else np.uint16
    top = (1 << bit_depth) - 1
    n = w * h * 3 // 2
    org = rng.integers(0, top + 1, (3, n)).astype(dt)
    pic = np.clip(org.astype(np.int64) + rng.integers(-6, 7, (3, n)), 0, top).astype(dt)
    enc = hevcdl_amd.Encoder(w, h, 32, max_frames=3, bit_depth=bit_depth)
    try:
        q3 = enc.picture_quality(org, pic)
        q1 = enc.picture_quality(org[2:3], pic[2:3])
        assert q1[0].tobytes() == q3[2].tobytes()
        assert enc.picture_quality(org[1:3], pic[1:3]).tobytes() == q3[1:3].tobytes()
        for f in range(3):
            for c, (o, r) in enumerate(zip(qr.planes(org[f], w, h), qr.planes(pic[f], w, h))):
                check_plane(o, r, bit_depth, int(q3["sse"][f][c]), float(q3["msssim"][f][c]), "%d-bit %dx%d picture %d plane %d" % (bit_depth, w, h, f, c))
        same = enc.picture_quality(org, org)                          # a picture against itself
        assert (same["sse"] == 0).all() and (same["msssim"] == 1.0).all()
    finally:
        enc.close()


def test_bad_arguments_return_a_status():
    """Results inside the pictures they are computed from are rejected (in == out aliasing is not supported); so are null pointers and too many frames."""
    import torch
    import hevcdl_amd
    w, h = 64, 64
    enc = hevcdl_amd.Encoder(w, h, 32, max_frames=2)
    try:
        n = w * h * 3 // 2
        d_org = torch.zeros(2 * n, dtype=torch.uint8, device="cuda")
        d_pic = torch.ones(2 * n, dtype=torch.uint8, device="cuda")
        d_out = torch.zeros(2 * 6, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        for args in ((d_org.data_ptr(), d_pic.data_ptr(), 2, d_org.data_ptr()), (d_org.data_ptr(), d_pic.data_ptr(), 2, d_pic.data_ptr() + 96),
                     (None, d_pic.data_ptr(), 1, d_out.data_ptr()), (d_org.data_ptr(), d_pic.data_ptr(), 1, None), (d_org.data_ptr(), d_pic.data_ptr(), 3, d_out.data_ptr())):
            with pytest.raises(hevcdl_amd.HevcdlError) as e:
                enc.picture_quality_dev(*args)
            assert e.value.status == 1
        enc.picture_quality_dev(d_org.data_ptr(), d_pic.data_ptr(), 2, d_out.data_ptr())
        torch.cuda.synchronize()
        got = np.frombuffer(d_out.cpu().numpy().tobytes(), hevcdl_amd.QUALITY_DTYPE)
        assert got["sse"].tolist() == [[w * h, w * h // 4, w * h // 4]] * 2
        assert torch.count_nonzero(d_org).item() == 0                # the inputs are only read
        with pytest.raises(hevcdl_amd.HevcdlError):
            enc.get_quality(0, 1)                                     # the switch is off
        with pytest.raises(hevcdl_amd.HevcdlError):
            hevcdl_amd.plane_quality(np.zeros((4, 4), np.uint8), np.zeros((4, 4), np.uint8), bit_depth=7)
    finally:
        enc.close()


def test_pipeline_switch_measures_the_output_pictures():
    import hevcdl_amd
    fx = qr.Fixture("r200_q27_f2")
    enc = hevcdl_amd.Encoder(fx.width, fx.height, fx.qp, max_frames=fx.n)
    try:
        recs0, out0, sao0, _ = enc.encode_pictures(fx.yuv, labels=fx.labels)
        enc.enable_quality(True)
        recs, out, sao, _ = enc.encode_pictures(fx.yuv, labels=fx.labels)
        assert np.array_equal(out, out0) and recs.tobytes() == recs0.tobytes() and np.array_equal(out, fx.recon)      # the switch changes nothing else
        q = enc.get_quality(0, fx.n)
        assert q.tobytes() == enc.picture_quality(fx.yuv, out).tobytes()
        assert enc.get_quality(1, 1).tobytes() == q[1:2].tobytes()
        with pytest.raises(hevcdl_amd.HevcdlError):
            enc.get_quality(1, fx.n)
        chunks = enc.encode_pictures_chunked(fx.yuv, labels=fx.labels, chunk_frames=1)
        assert len(chunks) == fx.n and enc.get_quality(0, fx.n).tobytes() == q.tobytes()
        enc.enable_quality(False)
        enc.encode_pictures(fx.yuv, labels=fx.labels)
        with pytest.raises(hevcdl_amd.HevcdlError):
            enc.get_quality(0, 1)
        # switching off gives the workspace back; the entry points and a second switch-on allocate it again and compute the same bits
        assert enc.picture_quality(fx.yuv, out).tobytes() == q.tobytes()
        enc.enable_quality(True)
        enc.encode_pictures(fx.yuv, labels=fx.labels)
        assert enc.get_quality(0, fx.n).tobytes() == q.tobytes()
    finally:
        enc.close()


@pytest.fixture(scope="module")
def app():
    import hevcdl_amd
    return hevcdl_amd.build_app()


def run(app, args, cwd):
    return subprocess.run([app] + args, cwd=cwd, capture_output=True, text=True, timeout=600)


def cli_inputs(tmp_path, yuv, labels, bit_depth):
    yuv.astype(np.uint8 if bit_depth == 8 else "<u2").tofile(tmp_path / "in.yuv")
    for fr in range(labels.shape[0]):
        os.makedirs(tmp_path / "pred" / str(fr))
        for a in range(labels.shape[1]):
            (tmp_path / "pred" / str(fr) / ("ctu%d.txt" % a)).write_text(" ".join(str(int(v)) for v in labels[fr, a]))


def log_of(stdout):
    """Picture lines without [ET ...] but with their hash text, and the two lines of the summary block."""
    lines = stdout.splitlines()
    poc = [qr.strip_et(l) + " " + l[l.index("[MD5:"):].strip() for l in lines if l.startswith("POC")]
    i = next(k for k, l in enumerate(lines) if l.startswith("SUMMARY"))
    return poc, lines[i + 1:i + 3]


KEYS = ["--PrintMSSSIM=1", "--PrintFrameMSE=1", "--PrintSequenceMSE=1"]


@pytest.mark.parametrize("case", qr.CASES)
def test_cli_prints_the_references_report(app, tmp_path, case):
    """("nQP <n> " of the reference build's line aside: see tests/test_quality.py.)"""
    fx = qr.Fixture(case)
    cli_inputs(tmp_path, fx.yuv, fx.labels, fx.bit_depth)
    base = ["-i", "in.yuv", "-wdt", str(fx.width), "-hgt", str(fx.height), "-q", str(fx.qp), "--LabelDir=pred", "--Level=6.2", "--SEIDecodedPictureHash=1"] + \
           ([] if fx.bit_depth == 8 else ["--InputBitDepth=10", "--InternalBitDepth=10", "--Profile=main10"])
    r0 = run(app, base + ["-b", "plain.bin", "-o", "plain.yuv"], tmp_path)
    assert r0.returncode == 0, r0.stdout + r0.stderr
    r = run(app, base + ["-b", "str.bin", "-o", "rec.yuv"] + KEYS, tmp_path)
    assert r.returncode == 0, r.stdout + r.stderr
    poc, summary = log_of(r.stdout)
    want = [re.sub(r"nQP -?\d+ ", "", qr.strip_et(l)) + " " + l[l.index("[MD5:"):].strip() for l in fx.poc_lines]
    assert poc == want
    assert summary == fx.summary
    # the stream and the reconstruction are those of a run without the keys (and the reference's pictures)
    assert (tmp_path / "str.bin").read_bytes() == (tmp_path / "plain.bin").read_bytes() and (tmp_path / "rec.yuv").read_bytes() == (tmp_path / "plain.yuv").read_bytes()
    assert np.array_equal(np.fromfile(tmp_path / "rec.yuv", fx.recon.dtype).reshape(fx.n, -1), fx.recon)
    # two contexts on one device, rows gathered (three more words a row): the same log
    r2 = run(app, base + ["-b", "two.bin", "-o", "two.yuv", "--Devices", "0,0"] + KEYS, tmp_path)
    assert r2.returncode == 0, r2.stdout + r2.stderr
    assert log_of(r2.stdout) == (poc, summary) and (tmp_path / "two.bin").read_bytes() == (tmp_path / "str.bin").read_bytes()
    assert "Picture rows gathered" in r2.stderr
    # one key at a time: the groups stand alone
    r3 = run(app, base + ["--PrintFrameMSE=1"], tmp_path)
    assert r3.returncode == 0 and "[MS-SSIM" not in r3.stdout and "[Y MSE" in r3.stdout and "Y-MSE" not in r3.stdout


def test_cli_with_the_keys_off_writes_what_it_always_wrote(app, tmp_path):
    from conftest import GOLD
    f = np.load(os.path.join(GOLD, "rd_b416_q32_r.npz"))
    w, h, qp = int(f["width"]), int(f["height"]), int(f["qp"])
    cli_inputs(tmp_path, f["yuv"], f["labels"], 8)
    base = ["-i", "in.yuv", "-wdt", str(w), "-hgt", str(h), "-q", str(qp), "--LabelDir=pred", "--Level=6.2", "--SEIDecodedPictureHash=1"]
    a = run(app, base + ["-b", "a.bin", "-o", "a.yuv"], tmp_path)
    b = run(app, base + ["-b", "b.bin", "-o", "b.yuv", "--PrintMSSSIM=0"], tmp_path)
    assert a.returncode == 0 and b.returncode == 0, a.stderr + b.stderr
    et = lambda t: re.sub(r"\[ET +\d+ \]", "[ET]", t)                  # (the one number of the log that is a measured time)
    assert et(a.stdout) == et(b.stdout) and "MS-SSIM" not in a.stdout and "MSE" not in a.stdout
    assert (tmp_path / "a.bin").read_bytes() == (tmp_path / "b.bin").read_bytes() == f["bitstream"].tobytes()
    assert (tmp_path / "a.yuv").read_bytes() == (tmp_path / "b.yuv").read_bytes()
