#!/usr/bin/env python3
"""Writes tests/golden/dbksel_*.npz: runs of the reference encoder (oracle/_ref, built by build()) with the two deblocking keys this project rejected until now --
DeblockingFilterMetric 1 (one deblocking offset per picture from the blockiness of its reconstruction, signalled in the slice header) and LoopFilterOffsetInPPS 0 (the
slice header repeats the cfg's offsets), the latter also with LoopFilterDisable 1.  Each file holds the frames, the labels (through label files: the CNN plays no
part), the reference's stream, the bytes of its reconstruction file and the picture and summary lines of its log.  Only data goes into the files.

The metric looks at the 32-sample grid only, so its pictures are coded with depth-0 labels (64x64 CUs, 32x32 transform blocks) at QP 37 .. 45 over smooth waves whose
amplitude differs from frame to frame: a flat frame stays under the threshold (no override), steeper ones reach different offsets.  tests/test_dbk_select.py asserts on
the committed files what this script asserts when it writes them: both branches and at least two different offsets occur.

The pictures of DeblockingFilterMetric 2 (the search over filter trials) are ref_tools.synth_yuv with random quadtrees at QP 27 and 32, where the 49 pairs give different
distortions, the walk leaves early and the window round the previous picture's best changes a choice against the full search (tests/test_dbk_select.py asserts it).  A stream
fixture with tiles is not possible inside the size limit: the reference refuses tile columns under four CTUs (TComPicSym.cpp:388), 256 samples; tiles with
LFCrossTileBoundaryFlag 0 are covered by the trial-table test against the restatement (tests/test_dbk_select_gpu.py)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import ref_tools              # noqa: E402
import dbk_select_ref as ref  # noqa: E402


def waves(w, h, amps, noises, seed, bd=8):
    """Frames [n, samples]: a luma wave of amplitude amps[f] on a ramp plus noise of sigma noises[f]; smooth chroma."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    out = []
    for f, (a, s) in enumerate(zip(amps, noises)):
        Y = np.clip(128 + a * np.sin(x / 23.0 + f) * np.cos(y / 17.0) + (x + 2 * y) * 0.3 + rng.normal(0, s, (h, w)), 0, 255)
        U = np.clip(128 + 20 * np.sin(x[::2, ::2] / 31.0) + rng.normal(0, 1, (h // 2, w // 2)), 0, 255)
        V = np.clip(128 + 20 * np.cos(y[::2, ::2] / 27.0) + rng.normal(0, 1, (h // 2, w // 2)), 0, 255)
        fr = np.concatenate([Y.ravel(), U.ravel(), V.ravel()])
        if bd > 8:
            fr = fr * (1 << (bd - 8)) + rng.integers(0, 1 << (bd - 8), fr.shape)
        out.append(np.round(fr))
    return np.stack(out).astype(np.uint8 if bd == 8 else np.uint16)


def case(w, h, qp, metric=0, in_pps=1, offsets=(0, 0), disable=0, bd=8, amps=None, noises=None, n=2, synth_seed=None):
    return dict(w=w, h=h, qp=qp, metric=metric, in_pps=in_pps, offsets=offsets, disable=disable, bd=bd, amps=amps, noises=noises, n=len(amps) if amps else n, synth_seed=synth_seed)


CASES = {
    "m1_128x64_q45": case(128, 64, 45, metric=1, in_pps=0, amps=(40, 10, 45, 30), noises=(0, 0, 0, 0)),                  # offsets 5, none, 6, 4
    "m1_128x64_q41_b10": case(128, 64, 41, metric=1, in_pps=0, bd=10, amps=(10, 45, 50), noises=(0, 0, 0)),
    "m1_104x72_q37_off": case(104, 72, 37, metric=1, in_pps=0, offsets=(1, -1), amps=(50, 30, 35), noises=(0, 0, 0)),    # width no multiple of 32: the edge at 96 is dropped; a picture without override runs with the PPS's (1, -1)
    "m1_64x64_q12": case(64, 64, 12, metric=1, in_pps=0, amps=(60, 30), noises=(2, 0)),                                   # beta(12) = 0: thr2 = 0, nothing can qualify
    # DeblockingFilterMetric 2: a chain of four pictures (the search window of every picture lies round the best of the one before), and one at 10 bits (the distortion is
    # shifted per sample)
    "m2_128x64_q32": case(128, 64, 32, metric=2, in_pps=0, n=4, synth_seed=2),
    "m2_72x72_q27_b10_off": case(72, 72, 27, metric=2, in_pps=0, offsets=(1, -2), bd=10, n=3, synth_seed=1),
    "inpps0_72x72_q32_off": case(72, 72, 32, in_pps=0, offsets=(2, -1)),
    "inpps0_72x72_q32_dis": case(72, 72, 32, in_pps=0, offsets=(2, -1), disable=1),
}


def ref_args(c):
    a = ["--DeblockingFilterMetric=%d" % c["metric"], "--LoopFilterOffsetInPPS=%d" % c["in_pps"], "--LoopFilterDisable=%d" % c["disable"],
         "--LoopFilterBetaOffset_div2=%d" % c["offsets"][0], "--LoopFilterTcOffset_div2=%d" % c["offsets"][1]]
    return a


def main():
    if not os.path.exists(ref_tools.REF_ENC):
        sys.exit("oracle/_ref/TAppEncoder_ref is missing: run build() first")
    seen, seen2 = [], []
    for name, c in CASES.items():
        seed = 900 + sorted(CASES).index(name)
        w, h, n, bd = c["w"], c["h"], c["n"], c["bd"]
        if c["metric"] == 1:
            yuv = waves(w, h, c["amps"], c["noises"], seed, bd)
            labels = ref_tools.make_labels(w, h, n, 0)
        elif c["metric"] == 2:
            yuv = ref_tools.synth_yuv(w, h, n, c["synth_seed"])
            if bd > 8:
                yuv = (yuv.astype(np.uint16) << (bd - 8)) | np.random.default_rng(seed).integers(0, 1 << (bd - 8), yuv.shape).astype(np.uint16)
            labels = ref_tools.make_labels(w, h, n, "rand", seed=c["synth_seed"])
        else:
            yuv = ref_tools.synth_yuv(w, h, n, seed)
            labels = ref_tools.make_labels(w, h, n, "rand", seed=seed)
        _, stdout, stream, recon = ref_tools.run_reference(yuv, w, h, c["qp"], labels, extra_args=ref_args(c), bit_depth=bd)
        out = os.path.join(ROOT, "tests", "golden", "dbksel_%s.npz" % name)
        np.savez_compressed(out, width=w, height=h, qp=c["qp"], bit_depth=bd, metric=c["metric"], lf_offset_in_pps=c["in_pps"], lf_disable=c["disable"],
                            lf_offsets=np.array(c["offsets"], np.int32), tiles=np.array((1, 1), np.int32), lf_across_tiles=1, seed=seed, yuv=yuv, labels=labels,
                            bitstream=np.frombuffer(stream, np.uint8), recon_file=np.frombuffer(recon, np.uint8), keys=np.array(ref_args(c), dtype=str),
                            stdout=np.array([l for l in stdout.splitlines() if l.startswith("POC") or "SUMMARY" in l or "Total Frames" in l or l.startswith("\t ")]))
        ch = ref.pictures(ref.load(name))[2]
        print("%s: seed %d, %d pictures, %d bytes, choices %s" % (name, seed, n, os.path.getsize(out), [tuple(int(v) for v in x) for x in ch]))
        if c["metric"] == 2:
            seen2 += [int(x["override_flag"]) for x in ch]
        if c["metric"] == 1:
            seen += [(int(x["override_flag"]), int(x["beta_offset_div2"])) for x in ch]
    assert any(o for o, _ in seen) and any(not o for o, _ in seen), "both branches of the metric must occur"
    assert len({v for o, v in seen if o}) >= 2, "at least two different offsets"
    assert any(o for o in seen2), "at least one picture of DeblockingFilterMetric 2 must choose something other than the PPS values"


if __name__ == "__main__":
    main()
