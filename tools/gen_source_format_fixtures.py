#!/usr/bin/env python3
"""Writes tests/golden/srcfmt_*.npz: runs of the reference encoder (oracle/_ref, built by build()) on source FILES that are not planar 4:2:0 with Cb before Cr --
4:0:0, 4:2:2 and 4:4:4 files coded as 4:2:0 (InputChromaFormat with ChromaFormatIDC 420), files with Cr before Cb (InputColourSpaceConvert YCbCrtoYCrCb), an explicit
window (ConformanceWindowMode 3 with ConfWin*) and a temporally subsampled read (TemporalSubsampleRatio).  Each file holds the source frames as the reference read
them, the labels (through label files: the CNN plays no part), the reference's stream, the bytes of its reconstruction file, the picture and summary lines of its
log, and the size of what the reference decoder wrote for the stream.

The chroma planes of the 4:2:2 / 4:4:4 sources carry independent noise per sample, so a wrong phase (the odd instead of the even sample or row) changes the stream.
The script starts the binaries itself, as tools/gen_source_fixtures.py does (same cfg files, same label files)."""
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import ref_tools              # noqa: E402


def case(sw, sh, n, qp, in_bd=8, bd=8, out_bd=0, mode=0, pad=(0, 0), cf=420, csc="", out_internal=0, snr_internal=0, win=(0, 0, 0, 0), ts=1, rails=False):
    return dict(sw=sw, sh=sh, n=n, qp=qp, in_bd=in_bd, bd=bd, out_bd=out_bd, mode=mode, pad=pad, cf=cf, csc=csc, out_internal=out_internal, snr_internal=snr_internal,
                win=win, ts=ts, rails=rails)


CASES = {
    "444_72x40": case(72, 40, 2, 32, cf=444),                                             # plain 2:1 subsampling both ways
    "444_66x42_m1_8to10": case(66, 42, 1, 30, bd=10, mode=1, cf=444),                     # padding 6 / 6, odd chroma width 33: the replicated sample is file column 64 / row 40
    "422_68x44_m1": case(68, 44, 1, 32, mode=1, cf=422),                                  # vertical subsampling only, padding 4 / 4
    "422_64_10to8": case(64, 64, 1, 32, in_bd=10, cf=422, rails=True),                    # 2-byte file samples, the rounding down-shift with the clip on kept and dropped positions
    "400_72x40": case(72, 40, 1, 32, cf=400),                                             # constant 128, the 999.9900 PSNR columns
    "400_60_m2_8to10": case(60, 60, 1, 30, bd=10, mode=2, pad=(4, 12), cf=400),           # constant 128 -> 512, a vertical padding of 12
    "400_64_10to8": case(64, 64, 1, 32, in_bd=10, cf=400),                                # constant 512 at the file depth -> 128
    "swap_72x40": case(72, 40, 1, 32, csc="YCbCrtoYCrCb"),
    "swap_72x40_internal": case(72, 40, 1, 32, csc="YCbCrtoYCrCb", out_internal=1, snr_internal=1),
    "win3_72x40": case(72, 40, 1, 32, mode=3, win=(4, 2, 6, 8)),                          # the SPS window, the cropped file, PSNR over the whole picture
    "win3_80x48_8to10_o8": case(80, 48, 1, 30, bd=10, out_bd=8, mode=3, win=(2, 0, 0, 2)),
    "444_swap_m1_68x44": case(68, 44, 1, 32, mode=1, cf=444, csc="YCbCrtoYCrCb"),         # format, permutation and padding together
    "ts3_72x40": case(72, 40, 7, 32, ts=3),                                               # -f 7 -ts 3: three pictures, from source frames 0, 3, 6
}


def padded(sw, sh, mode, px, py):
    if mode == 1:
        return sw + (8 - sw % 8) % 8, sh + (8 - sh % 8) % 8
    if mode == 2:
        return sw + px, sh + py
    return sw, sh


def chroma_size(sw, sh, cf):
    return {400: (0, 0), 420: (sw // 2, sh // 2), 422: (sw // 2, sh), 444: (sw, sh)}[cf]


def source_frames(c, seed):
    """[n, source samples]: the luma (and, for a 4:2:0 file, the chroma) of ref_tools.synth_yuv; the chroma planes of a 4:2:2 / 4:4:4 file are a smooth ramp plus
    independent noise per sample."""
    sw, sh, n, in_bd, cf = c["sw"], c["sh"], c["n"], c["in_bd"], c["cf"]
    base = ref_tools.synth_yuv(sw, sh, n, seed)
    rng = np.random.default_rng(seed + 2000)
    cw, chh = chroma_size(sw, sh, cf)
    if cf == 420:
        yuv = base.astype(np.uint16)
    else:
        planes = [base[:, :sw * sh].astype(np.uint16)]
        for k in range(2 if cf != 400 else 0):
            ramp = 96 + 24 * k + (np.arange(cw)[None, :] * 40 // max(cw, 1) + np.arange(chh)[:, None] * 30 // max(chh, 1))
            planes.append(np.clip(ramp[None] + rng.integers(-24, 25, (n, chh, cw)), 0, 255).astype(np.uint16).reshape(n, -1))
        yuv = np.concatenate(planes, axis=1)
    if in_bd > 8:
        yuv = (yuv << (in_bd - 8)) | rng.integers(0, 1 << (in_bd - 8), yuv.shape).astype(np.uint16)
        top = (1 << in_bd) - 1
        yuv[:, 5:9] = [top, top - 1, top, top - 1]                    # both rails and the values that round up into the clip
        yuv[:, 40:44] = [0, 1, 2, 3]
        if c["rails"] and cw:                                         # the same on chroma rows and columns the subsampling keeps AND on ones it drops
            for k in range(2):
                p = yuv[:, sw * sh + k * cw * chh:sw * sh + (k + 1) * cw * chh].reshape(n, chh, cw)
                p[:, 0, 2:6] = [top - 1, top, top, top - 1]           # a kept row (even)
                p[:, 1, 2:6] = [top, top - 1, top - 1, top]           # a dropped row (odd) of a vertically subsampled file
                p[:, 6, 9:13] = [top, top - 1, 0, 1]
                p[:, 7, 9:13] = [top - 1, top, 1, 0]
    return yuv.astype(np.uint8 if in_bd == 8 else "<u2")


def ref_args(c):
    """The keys of the case, as the reference's command line (the CLI of this project takes the same)."""
    a = ["--InternalBitDepth=%d" % c["bd"], "--Profile=%s" % ("main" if c["bd"] == 8 else "main10"), "--ConformanceWindowMode=%d" % c["mode"]]
    if c["mode"] == 2:
        a += ["--HorizontalPadding=%d" % c["pad"][0], "--VerticalPadding=%d" % c["pad"][1]]
    if c["mode"] == 3:
        a += ["--ConfWinLeft=%d" % c["win"][0], "--ConfWinRight=%d" % c["win"][1], "--ConfWinTop=%d" % c["win"][2], "--ConfWinBottom=%d" % c["win"][3]]
    if c["out_bd"]:
        a += ["--OutputBitDepth=%d" % c["out_bd"], "--OutputBitDepthC=%d" % c["out_bd"]]
    if c["cf"] != 420:
        a += ["--ChromaFormatIDC=420"]
    if c["csc"]:
        a += ["--InputColourSpaceConvert=%s" % c["csc"], "--OutputInternalColourSpace=%d" % c["out_internal"], "--SNRInternalColourSpace=%d" % c["snr_internal"]]
    if c["ts"] != 1:
        a += ["--TemporalSubsampleRatio=%d" % c["ts"]]
    return a


def run(c, yuv, labels):
    """-> (stdout, stream bytes, reconstruction file bytes, decoder output bytes)."""
    d = tempfile.mkdtemp(prefix="hmfmt_")
    os.makedirs(os.path.join(d, "rec"))
    yuv.tofile(os.path.join(d, "in.yuv"))
    for f in range(labels.shape[0]):
        os.makedirs(os.path.join(d, "pred", str(f)))
        for a in range(labels.shape[1]):
            with open(os.path.join(d, "pred", str(f), "ctu%d.txt" % a), "w") as fh:
                fh.write(" ".join(str(int(v)) for v in labels[f, a]) + " ")
    open(os.path.join(d, "enc.cfg"), "w").write(open(ref_tools.REF_CFG).read().replace(".\\rec\\", "rec/"))
    open(os.path.join(d, "bs.cfg"), "w").write(
        "InputFile : in.yuv\nInputBitDepth : %d\nInputChromaFormat : %d\nFrameRate : 30\nFrameSkip : 0\n"
        "SourceWidth : %d\nSourceHeight : %d\nFramesToBeEncoded : %d\nLevel : 6.2\n" % (c["in_bd"], c["cf"], c["sw"], c["sh"], c["n"]))
    cmd = [ref_tools.REF_ENC, "-c", "enc.cfg", "-c", "bs.cfg", "-q", str(c["qp"]), "--SEIDecodedPictureHash=1"] + ref_args(c)
    p = subprocess.run(cmd, cwd=d, capture_output=True, text=True)
    if p.returncode != 0:
        raise RuntimeError("reference encoder failed: " + p.stdout[-2000:] + p.stderr[-2000:])
    stream = open(os.path.join(d, "rec", "str.bin"), "rb").read()
    recon = open(os.path.join(d, "rec", "rec.yuv"), "rb").read()
    q = subprocess.run([ref_tools.REF_DEC, "-b", os.path.join("rec", "str.bin"), "-o", "dec.yuv"], cwd=d, capture_output=True, text=True)
    if q.returncode != 0 or "ERROR" in q.stdout:
        raise RuntimeError("reference decoder failed: " + q.stdout[-2000:] + q.stderr[-2000:])
    decoded = open(os.path.join(d, "dec.yuv"), "rb").read()
    shutil.rmtree(d)
    return p.stdout, stream, recon, decoded


def refusal():
    """What the reference says to a 4:4:4 file without ChromaFormatIDC -> (exit code, the error lines)."""
    d = tempfile.mkdtemp(prefix="hmfmt_")
    os.makedirs(os.path.join(d, "rec"))
    np.zeros(72 * 40 * 3, np.uint8).tofile(os.path.join(d, "in.yuv"))
    open(os.path.join(d, "enc.cfg"), "w").write(open(ref_tools.REF_CFG).read().replace(".\\rec\\", "rec/"))
    open(os.path.join(d, "bs.cfg"), "w").write("InputFile : in.yuv\nInputBitDepth : 8\nInputChromaFormat : 444\nFrameRate : 30\nFrameSkip : 0\nSourceWidth : 72\nSourceHeight : 40\nFramesToBeEncoded : 1\nLevel : 6.2\n")
    p = subprocess.run([ref_tools.REF_ENC, "-c", "enc.cfg", "-c", "bs.cfg", "-q", "32"], cwd=d, capture_output=True, text=True)
    shutil.rmtree(d)
    return p.returncode, [l for l in (p.stdout + p.stderr).splitlines() if l.startswith("Error")]


def main():
    if not os.path.exists(ref_tools.REF_ENC) or not os.path.exists(ref_tools.REF_DEC):
        sys.exit("oracle/_ref/TAppEncoder_ref / TAppDecoder_ref are missing: run build() first")
    rc, lines = refusal()
    assert rc != 0 and lines, (rc, lines)
    for name, c in CASES.items():
        seed = 700 + sorted(CASES).index(name)
        sw, sh = c["sw"], c["sh"]
        cw, ch = padded(sw, sh, c["mode"], *c["pad"])
        pics = (c["n"] + c["ts"] - 1) // c["ts"]
        yuv = source_frames(c, seed)
        labels = ref_tools.make_labels(cw, ch, pics, "rand", seed=seed)
        stdout, stream, recon, decoded = run(c, yuv, labels)
        ww, wh = (sw - c["win"][0] - c["win"][1], sh - c["win"][2] - c["win"][3])
        out_bd = c["out_bd"] or c["bd"]
        # the decoder crops to the window: its output holds window-sized 4:2:0 frames at the internal depth; the reconstruction file the same at the output depth
        assert len(decoded) == pics * (ww * wh * 3 // 2) * (2 if c["bd"] > 8 else 1), (name, len(decoded))
        assert len(recon) == pics * (ww * wh * 3 // 2) * (2 if out_bd > 8 else 1), (name, len(recon))
        out = os.path.join(ROOT, "tests", "golden", "srcfmt_%s.npz" % name)
        np.savez_compressed(out, source_width=sw, source_height=sh, width=cw, height=ch, qp=c["qp"], input_bit_depth=c["in_bd"], bit_depth=c["bd"], output_bit_depth=out_bd,
                            mode=c["mode"], pad_x=c["pad"][0], pad_y=c["pad"][1], chroma_format=c["cf"], colour_space=1 if c["csc"] else 0,
                            output_internal_colour_space=c["out_internal"], snr_internal_colour_space=c["snr_internal"], conf_win=np.array(c["win"], np.int32),
                            temporal_subsample_ratio=c["ts"], source_frames=c["n"], pictures=pics, seed=seed, yuv=yuv, labels=labels,
                            bitstream=np.frombuffer(stream, np.uint8), recon_file=np.frombuffer(recon, np.uint8), decoded_bytes=len(decoded), decoded_width=ww, decoded_height=wh,
                            keys=np.array(ref_args(c), dtype=str), refusal_444=np.array(lines, dtype=str), refusal_444_exit=rc,
                            stdout=np.array([l for l in stdout.splitlines() if l.startswith("POC") or "SUMMARY" in l or "Total Frames" in l or l.startswith("\t ")]))
        print("%s: seed %d, coded %dx%d, %d pictures, %d bytes" % (name, seed, cw, ch, pics, os.path.getsize(out)))
        for l in stdout.splitlines():
            if l.startswith("POC"):
                print("   ", l)


if __name__ == "__main__":
    main()
