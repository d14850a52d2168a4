"""Slices as units of the decision launch, as a record -> profiles/slices_time.txt (needs an MI355X).

3840 x 2160 at QP 32 (60 x 34 CTUs), SliceMode 1 with 1, 2, 6 and 17 slices a picture (34, 17, 6 and 2 CTU rows a slice), one picture and a launch of 75: the decision
kernel alone (HIP events of hevcdl_compress_frames, and its wall time) and the whole picture pipeline (hevcdl_encode_pictures: decisions, deblocking, SAO, with the
copies).  Labels are random valid quadtrees of one picture, the same for every picture and every run, so the CNN plays no part.  Each figure is the median of
--rounds timed calls behind one warm-up call (which also grows the workspace).  This is a record, not a bar."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
W, H, QP = 3840, 2160, 32
CX, CY = 60, 34
SLICES = ((1, CY), (2, 17), (6, 6), (17, 2))      # (slices a picture, CTU rows a slice)


def median(v):
    return sorted(v)[len(v) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--frames", type=int, default=75)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "slices_time.txt"))
    a = ap.parse_args()
    import hevcdl_amd
    import ref_tools
    one = ref_tools.synth_yuv(W, H, 1, seed=9)
    lab = ref_tools.make_labels(W, H, 1, "rand", seed=9)
    out = ["== %dx%d QP %d, SliceMode 1; labels: random quadtrees (no CNN); median of %d calls behind a warm-up ==" % (W, H, QP, a.rounds),
           "pictures  slices  rows/slice  decisions kernel ms  decisions wall s  pipeline wall s  launch"]
    for n in (1, a.frames):
        yuv, labels = np.repeat(one, n, axis=0), np.repeat(lab, n, axis=0)
        base = None
        for slices, rows in SLICES:
            e = hevcdl_amd.Encoder(W, H, QP, max_frames=n, slices=(1, rows * CX) if slices > 1 else None)
            try:
                e.profile_enable(True)
                e.compress_frames(yuv, labels)
                e.profile_get()
                k_ms, d_s, p_s = [], [], []
                for _ in range(a.rounds):
                    t0 = time.perf_counter(); e.compress_frames(yuv, labels); d_s.append(time.perf_counter() - t0)
                    k_ms.append(e.profile_get()["rd_ms"])
                launch = e.last_rd_launch()
                e.encode_pictures(yuv, labels)
                for _ in range(a.rounds):
                    t0 = time.perf_counter(); e.encode_pictures(yuv, labels); p_s.append(time.perf_counter() - t0)
            finally:
                e.close()
            k = median(k_ms)
            base = base or k
            out.append("%8d  %6d  %10d  %19.1f  %16.3f  %15.3f  %s   (kernel x %.2f of one slice)" % (n, slices, rows, k, median(d_s), median(p_s), launch, k / base))
            print(out[-1], flush=True)
    with open(a.out, "w") as f:
        f.write("\n".join(out) + "\n")


if __name__ == "__main__":
    main()
