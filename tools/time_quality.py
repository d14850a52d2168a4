#!/usr/bin/env python3
"""Time of the quality pass (csrc/quality_kernel.hip) per 2160p picture -> stdout (committed as profiles/quality_time.txt).

  --device      the pass alone on a batch of 64 pictures in device buffers, timed with HIP events; beside it the f64 operation count per picture and the rate
  --cli         the CLI on 16 pictures of 2160p with and without --PrintMSSSIM=1 (wall time, and the e2e per-picture time the pass must stay under)
  --reference   the yardstick: wall time of the reference encoder (oracle/_ref/TAppEncoder_ref, where it exists) on one 2160p frame with and without the key
No threshold: a record."""
import argparse
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
W, H = 3840, 2160


def scales(w, h):
    return 1 if (w < 22 or h < 22) else 2 if (w < 44 or h < 44) else 3 if (w < 88 or h < 88) else 4 if (w < 176 or h < 176) else 5


def windows_per_picture(w, h):
    n = 0
    for pw, ph in ((w, h), (w // 2, h // 2), (w // 2, h // 2)):
        for s in range(scales(pw, ph)):
            n += max(0, (pw >> s) - 10) * max(0, (ph >> s) - 10)
    return n


OPS_PER_WINDOW = 121 * 10 + 16      # five (a * w) products and five additions per tap; variances, the two quotients


def device_pass(batch, reps):
    import torch
    import hevcdl_amd
    n = W * H * 3 // 2
    g = torch.Generator(device="cuda").manual_seed(1)
    org = torch.randint(0, 256, (batch, n), dtype=torch.uint8, device="cuda", generator=g)
    pic = (org.to(torch.int16) + torch.randint(-4, 5, (batch, n), dtype=torch.int16, device="cuda", generator=g)).clamp(0, 255).to(torch.uint8)
    out = torch.zeros(batch * 6, dtype=torch.int64, device="cuda")
    enc = hevcdl_amd.Encoder(W, H, 32, max_frames=batch)
    enc.picture_quality_dev(org.data_ptr(), pic.data_ptr(), batch, out.data_ptr())      # allocates the workspace
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        enc.picture_quality_dev(org.data_ptr(), pic.data_ptr(), batch, out.data_ptr())
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b) / batch)
    # the yardstick on the device side: the whole picture pipeline (upload, CNN, decisions, deblocking, SAO, download) per picture, without and with the switch
    import ref_tools
    nf = batch
    yuv = np.concatenate([ref_tools.synth_yuv(W, H, 2, seed=3)] * (nf // 2))
    e2e = {}
    for tag, on in (("warm-up", False), ("switch off", False), ("switch on", True)):
        enc.enable_quality(on)
        t0 = time.time()
        enc.encode_pictures(yuv)
        e2e[tag] = (time.time() - t0) * 1e3 / nf
    enc.close()
    win = windows_per_picture(W, H)
    ops = win * OPS_PER_WINDOW
    best = min(ms)
    print("device pass alone, %dx%d, batch of %d from device buffers, HIP events, %d repetitions:" % (W, H, batch, reps))
    print("  ms per picture: min %.3f  median %.3f  max %.3f" % (best, sorted(ms)[len(ms) // 2], max(ms)))
    print("  windows per picture: %d   f64 operations per window: %d   per picture: %.3e" % (win, OPS_PER_WINDOW, ops))
    print("  implied rate at the min: %.2f T f64 operations / s (multiplies and additions counted singly; nothing is fused)" % (ops / (best * 1e-3) / 1e12))
    print("whole picture pipeline (hevcdl_encode_pictures, host buffers, %d pictures of %dx%d, labels from the CNN), wall ms per picture:" % (nf, W, H))
    print("  switch off %.2f   switch on (hevcdl_enable_quality) %.2f" % (e2e["switch off"], e2e["switch on"]))
    print("  the pass alone is %.1f %% of the pipeline's per-picture time: %s" % (100.0 * best / e2e["switch off"], "cheaper" if best < e2e["switch off"] else "NOT cheaper"))
    # the benchmark's e2e leg (600 pictures in flight, entropy coding included) is the steadier figure; its last committed record
    rec = os.path.join(ROOT, "profiles", "r06r_bench_c4_f600.json")
    if os.path.exists(rec):
        import json
        pps = json.load(open(rec))["e2e"]["pictures_per_s"]
        print("  benchmark's e2e leg (profiles/r06r_bench_c4_f600.json, 600 pictures): %.2f ms per picture; the pass alone is %.1f %% of it: %s"
              % (1e3 / pps, 100.0 * best * pps / 1e3, "cheaper" if best < 1e3 / pps else "NOT cheaper"))


def cli(frames):
    import hevcdl_amd
    import ref_tools
    app = hevcdl_amd.build_app()
    d = tempfile.mkdtemp(prefix="qtime_")
    one = ref_tools.synth_yuv(W, H, 2, seed=3)
    np.concatenate([one] * ((frames + 1) // 2))[:frames].tofile(os.path.join(d, "in.yuv"))
    res = {}
    for tag, extra in (("warm-up", []), ("without", []), ("with PrintMSSSIM", ["--PrintMSSSIM=1"])):
        t0 = time.time()
        r = subprocess.run([app, "-i", "in.yuv", "-wdt", str(W), "-hgt", str(H), "-q", "32", "-b", "s.bin"] + extra, cwd=d, capture_output=True, text=True, timeout=900)
        res[tag] = (time.time() - t0, r.returncode, [l for l in r.stderr.splitlines() if l.startswith("stage seconds")])
    print("CLI, %d pictures of %dx%d, labels from the on-device CNN (wall seconds of the whole process; its own stage line):" % (frames, W, H))
    for tag in ("without", "with PrintMSSSIM"):
        print("  %-18s %.2f s  = %.1f ms per picture  (exit %d)  %s" % (tag, res[tag][0], res[tag][0] * 1e3 / frames, res[tag][1], " ".join(res[tag][2])))
    print("  difference: %.1f ms per picture" % ((res["with PrintMSSSIM"][0] - res["without"][0]) * 1e3 / frames))
    for f in os.listdir(d):
        os.remove(os.path.join(d, f))
    os.rmdir(d)


def reference():
    import ref_tools
    if not os.path.exists(ref_tools.REF_ENC):
        print("reference: oracle/_ref/TAppEncoder_ref is not here; not timed")
        return
    yuv = ref_tools.synth_yuv(W, H, 1, seed=3)
    labels = ref_tools.make_labels(W, H, 1, 1)
    t = {}
    for tag, extra in (("without", []), ("with --PrintMSSSIM=1", ["--PrintMSSSIM=1"])):
        t0 = time.time()
        ref_tools.run_reference(yuv, W, H, 32, labels, extra_args=extra)
        t[tag] = time.time() - t0
        print("reference encoder, one %dx%d frame, %s: %.2f s wall" % (W, H, tag, t[tag]))
    print("reference's cost of the key: %.2f s per picture (one host core)" % (t["with --PrintMSSSIM=1"] - t["without"]))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", action="store_true")
    ap.add_argument("--cli", action="store_true")
    ap.add_argument("--reference", action="store_true")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--frames", type=int, default=16)
    a = ap.parse_args()
    if a.device:
        device_pass(a.batch, a.reps)
    if a.cli:
        cli(a.frames)
    if a.reference:
        reference()
