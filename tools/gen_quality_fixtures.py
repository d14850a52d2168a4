#!/usr/bin/env python3
"""Writes tests/golden/quality_*.npz: runs of the reference encoder with --PrintMSSSIM=1 --PrintFrameMSE=1 --PrintSequenceMSE=1 (oracle/_ref, built by
build()).  Each file holds the input frames, the labels, the reference's final pictures and its stdout lines.

A picture is only kept when every MS-SSIM the reference prints for it lies further from a rounding boundary of the sixth decimal than 100 times the
derived bound on what another order of the block sum may change (tests/quality_ref.msssim_tolerance); otherwise the next seed is tried.  The same is asked
of the averaged columns of the summary."""
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import quality_ref as qr      # noqa: E402
import ref_tools              # noqa: E402

KEYS = ["--PrintMSSSIM=1", "--PrintFrameMSE=1", "--PrintSequenceMSE=1"]
# case -> (width, height, frames, qp, bit depth, kind)
CASES = {"c416_q32": (416, 240, 1, 32, 8, "synth"), "r200_q27_f2": (200, 136, 2, 27, 8, "synth"), "b192_q30_b10": (192, 128, 1, 30, 10, "synth"),
         "s64_q32": (64, 64, 1, 32, 8, "synth"),            # chroma planes of 32 x 32: two scales; luma three
         "k64_q32_const": (64, 64, 1, 32, 8, "const"),      # SSE 0 -> 999.99 dB, MS-SSIM 1
         "t16_q32": (16, 16, 1, 32, 8, "synth")}            # 8 x 8 chroma planes: smaller than the window, the reference prints 0 / totalBlocks


def boundary_distance(v):
    """Distance of v from the nearest value at which its sixth decimal rounds the other way."""
    t = v * 1e6
    return abs(t - math.floor(t) - 0.5) * 1e-6


def frames(width, height, n, bit_depth, kind, seed):
    if kind == "const":
        return np.full((n, width * height * 3 // 2), 128, np.uint8)
    yuv = ref_tools.synth_yuv(width, height, n, seed)
    if bit_depth > 8:
        rng = np.random.default_rng(seed + 1000)
        yuv = (yuv.astype(np.uint16) << (bit_depth - 8)) | rng.integers(0, 1 << (bit_depth - 8), yuv.shape).astype(np.uint16)
    return yuv


def safe(yuv, recon, width, height, bit_depth):
    sums = [0.0, 0.0, 0.0]
    for f in range(yuv.shape[0]):
        for c, (o, r) in enumerate(zip(qr.planes(yuv[f], width, height), qr.planes(recon[f], width, height))):
            v, info = qr.msssim(o, r, bit_depth, details=True)
            sums[c] += v
            if math.isfinite(v) and boundary_distance(v) <= 100.0 * qr.msssim_tolerance(v, info) + 1e-12:
                return False
    return all(not math.isfinite(s) or boundary_distance(s / yuv.shape[0]) > 1e-9 for s in sums)


def main():
    if not os.path.exists(ref_tools.REF_ENC):
        sys.exit("oracle/_ref/TAppEncoder_ref is missing: run build() first")
    for case, (w, h, n, qp, bd, kind) in CASES.items():
        for seed in range(300, 340):
            yuv = frames(w, h, n, bd, kind, seed)
            labels = ref_tools.make_labels(w, h, n, "rand", seed=seed)
            _, stdout, _, recon = ref_tools.run_reference(yuv, w, h, qp, labels, extra_args=KEYS, bit_depth=bd)
            recon = np.frombuffer(recon, np.uint8 if bd == 8 else "<u2").reshape(n, -1)
            if safe(yuv, recon, w, h, bd):
                break
            print("%s: seed %d dropped (a printed MS-SSIM too close to a rounding boundary)" % (case, seed))
        else:
            sys.exit("%s: no seed gave a usable picture" % case)
        out = os.path.join(ROOT, "tests", "golden", "quality_%s.npz" % case)
        np.savez_compressed(out, width=w, height=h, qp=qp, bit_depth=bd, seed=seed, yuv=yuv, labels=labels, recon_filtered=recon,
                            stdout=np.array([l for l in stdout.splitlines() if l.startswith("POC") or "SUMMARY" in l or "Total Frames" in l or l.startswith("\t ")]))
        print("%s: seed %d, %d bytes" % (case, seed, os.path.getsize(out)))
        for l in stdout.splitlines():
            if l.startswith("POC"):
                print("   ", l)


if __name__ == "__main__":
    main()
