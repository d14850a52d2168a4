#!/usr/bin/env python3
"""Writes tests/golden/source_*.npz: runs of the reference encoder (oracle/_ref, built by build()) on source pictures that are NOT in the codec's own format --
sizes that are no multiple of the minimum CU (ConformanceWindowMode 1 / 2) and files whose bit depth differs from the internal one (InputBitDepth / InternalBitDepth /
OutputBitDepth).  Each file holds the source frames as the reference read them, the labels, the reference's stream, the bytes of its reconstruction file (the window,
at the output depth) and the picture and summary lines of its log; and what the reference decoder wrote for the stream (its size: the window's).

oracle/ref_tools.run_reference writes its input file with the sample type of its bit_depth argument, which is also the internal depth there; here the two differ, so
this script starts the binary itself (same cfg files, same label files).  The reference's OutputBitDepthC defaults to the INTERNAL chroma depth, not to OutputBitDepth, so a run
with an output depth names both keys (chroma-specific depths are outside this project's path).

The case with --PrintMSSSIM=1 --PrintFrameMSE=1 is chosen by the rule of tools/gen_quality_fixtures.py: a seed is only kept when every MS-SSIM the reference prints
lies further from a rounding boundary of the sixth decimal than 100 times the derived bound on what another order of the block sum may change."""
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import quality_ref as qr      # noqa: E402
import ref_tools              # noqa: E402
from gen_quality_fixtures import boundary_distance      # noqa: E402

# case -> (source width, source height, frames, qp, input depth, internal depth, output depth (0: the internal one), ConformanceWindowMode, pad x, pad y, extra keys)
CASES = {
    "a68x44_m1": (68, 44, 2, 32, 8, 8, 0, 1, 0, 0, []),                 # padding 4 and 4
    "b66x42_8to10_m1": (66, 42, 1, 30, 8, 10, 0, 1, 0, 0, []),          # padding 6 and 6; the chroma width of 33 is odd
    "c64_8to10_o8": (64, 64, 1, 32, 8, 10, 8, 0, 0, 0, []),
    "d64_10to8": (64, 64, 1, 32, 10, 8, 0, 0, 0, 0, []),                # the rounding down-shift with the clip at 255: the source holds 1022 and 1023
    "e64_10to8_o10": (64, 64, 1, 27, 10, 8, 10, 0, 0, 0, []),
    "f60_m2": (60, 60, 1, 32, 8, 8, 0, 2, 4, 12, []),                   # a vertical padding above 8: replicated rows of replicated rows
    "g72x40_m1": (72, 40, 1, 32, 8, 8, 0, 1, 0, 0, []),                 # already a multiple of 8: no padding, the stream of the mode-0 run
    "q100x76_m1_quality": (100, 76, 2, 27, 8, 8, 0, 1, 0, 0, ["--PrintMSSSIM=1", "--PrintFrameMSE=1", "--PrintSequenceMSE=1"]),
}


def padded(sw, sh, mode, px, py):
    if mode == 1:
        return sw + (8 - sw % 8) % 8, sh + (8 - sh % 8) % 8
    if mode == 2:
        return sw + px, sh + py
    return sw, sh


def source_frames(sw, sh, n, in_bd, seed):
    yuv = ref_tools.synth_yuv(sw, sh, n, seed)
    if in_bd > 8:
        rng = np.random.default_rng(seed + 1000)
        yuv = (yuv.astype(np.uint16) << (in_bd - 8)) | rng.integers(0, 1 << (in_bd - 8), yuv.shape).astype(np.uint16)
        top = (1 << in_bd) - 1
        yuv[:, 5:9] = [top, top - 1, top, top - 1]                    # both rails and the values that round up into the clip
        yuv[:, sw * sh + 3:sw * sh + 7] = [top - 1, top, 0, 1]
        yuv[:, 40:44] = [0, 1, 2, 3]
    return yuv


def run(yuv, sw, sh, cw, ch, qp, labels, in_bd, bd, out_bd, mode, px, py, extra):
    """-> (stdout, stream bytes, reconstruction file bytes, decoder output bytes)."""
    n = yuv.shape[0]
    d = tempfile.mkdtemp(prefix="hmsrc_")
    os.makedirs(os.path.join(d, "rec"))
    yuv.astype(np.uint8 if in_bd == 8 else "<u2").tofile(os.path.join(d, "in.yuv"))
    for f in range(n):
        os.makedirs(os.path.join(d, "pred", str(f)))
        for a in range(labels.shape[1]):
            with open(os.path.join(d, "pred", str(f), "ctu%d.txt" % a), "w") as fh:
                fh.write(" ".join(str(int(v)) for v in labels[f, a]) + " ")
    open(os.path.join(d, "enc.cfg"), "w").write(open(ref_tools.REF_CFG).read().replace(".\\rec\\", "rec/"))
    open(os.path.join(d, "bs.cfg"), "w").write(
        "InputFile : in.yuv\nInputBitDepth : %d\nInputChromaFormat : 420\nFrameRate : 30\nFrameSkip : 0\n"
        "SourceWidth : %d\nSourceHeight : %d\nFramesToBeEncoded : %d\nLevel : 6.2\n" % (in_bd, sw, sh, n))
    env = dict(os.environ, HEVCDL_DUMP=os.path.join(d, "dump.bin"))
    if bd > 8:
        env["HEVCDL_DUMP16"] = "1"
    cmd = [ref_tools.REF_ENC, "-c", "enc.cfg", "-c", "bs.cfg", "-q", str(qp), "--SEIDecodedPictureHash=1", "--InternalBitDepth=%d" % bd, "--Profile=%s" % ("main" if bd == 8 else "main10"),
           "--ConformanceWindowMode=%d" % mode] + (["--HorizontalPadding=%d" % px, "--VerticalPadding=%d" % py] if mode == 2 else []) + (["--OutputBitDepth=%d" % out_bd, "--OutputBitDepthC=%d" % out_bd] if out_bd else []) + list(extra)
    p = subprocess.run(cmd, cwd=d, env=env, capture_output=True, text=True)
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


def msssim_safe(yuv, recon, sw, sh, bd):
    """The rule of tools/gen_quality_fixtures.safe, over the window (8-bit source and output: the source frames and the reconstruction file are the window's planes)."""
    sums = [0.0, 0.0, 0.0]
    for f in range(yuv.shape[0]):
        for c, (o, r) in enumerate(zip(qr.planes(yuv[f], sw, sh), qr.planes(recon[f], sw, sh))):
            v, info = qr.msssim(o, r, bd, details=True)
            sums[c] += v
            if np.isfinite(v) and boundary_distance(v) <= 100.0 * qr.msssim_tolerance(v, info) + 1e-12:
                return False
    return all(not np.isfinite(s) or boundary_distance(s / yuv.shape[0]) > 1e-9 for s in sums)


def main():
    if not os.path.exists(ref_tools.REF_ENC) or not os.path.exists(ref_tools.REF_DEC):
        sys.exit("oracle/_ref/TAppEncoder_ref / TAppDecoder_ref are missing: run build() first")
    for case, (sw, sh, n, qp, in_bd, bd, out_bd, mode, px, py, extra) in CASES.items():
        cw, ch = padded(sw, sh, mode, px, py)
        for seed in range(500, 540):
            yuv = source_frames(sw, sh, n, in_bd, seed)
            labels = ref_tools.make_labels(cw, ch, n, "rand", seed=seed)
            stdout, stream, recon, decoded = run(yuv, sw, sh, cw, ch, qp, labels, in_bd, bd, out_bd, mode, px, py, extra)
            if not extra or msssim_safe(yuv, np.frombuffer(recon, np.uint8).reshape(n, -1), sw, sh, bd):
                break
            print("%s: seed %d dropped (a printed MS-SSIM too close to a rounding boundary)" % (case, seed))
        else:
            sys.exit("%s: no seed gave a usable picture" % case)
        # the decoder crops to the window: its output holds window-sized frames at the internal depth
        assert len(decoded) == n * (sw * sh * 3 // 2) * (2 if bd > 8 else 1), (case, len(decoded))
        assert len(recon) == n * (sw * sh * 3 // 2) * (2 if (out_bd or bd) > 8 else 1), (case, len(recon))
        more = {}
        if case.startswith("g"):      # the same source without the key: the reference's mode-0 stream
            more["bitstream_mode0"] = np.frombuffer(run(yuv, sw, sh, cw, ch, qp, labels, in_bd, bd, out_bd, 0, 0, 0, extra)[1], np.uint8)
        out = os.path.join(ROOT, "tests", "golden", "source_%s.npz" % case)
        np.savez_compressed(out, source_width=sw, source_height=sh, width=cw, height=ch, qp=qp, input_bit_depth=in_bd, bit_depth=bd, output_bit_depth=out_bd or bd,
                            mode=mode, pad_x=px, pad_y=py, seed=seed, yuv=yuv, labels=labels, bitstream=np.frombuffer(stream, np.uint8), recon_file=np.frombuffer(recon, np.uint8),
                            decoded_bytes=len(decoded), keys=np.array(extra, dtype=str),
                            stdout=np.array([l for l in stdout.splitlines() if l.startswith("POC") or "SUMMARY" in l or "Total Frames" in l or l.startswith("\t ")]), **more)
        print("%s: seed %d, coded %dx%d, %d bytes" % (case, seed, cw, ch, os.path.getsize(out)))
        for l in stdout.splitlines():
            if l.startswith("POC"):
                print("   ", l)


if __name__ == "__main__":
    main()
