#!/usr/bin/env python3
"""Time of the per-picture deblocking parameters (DeblockingFilterMetric 1 and 2) per 2160p picture -> stdout (committed as profiles/dbk_select_time.txt).

  the metric launch alone (csrc/dbk_select_kernel.hip) on a batch of pictures in device buffers, HIP events, beside the bytes it must read and the rate;
  the deblocking launches with a row of parameters per picture against the launches without, alternating, on the same buffers;
  the whole picture pipeline (hevcdl_encode_pictures, host buffers) of a context with the metric against one without, alternating, on the same build.
  the trial launch of DeblockingFilterMetric 2 (one launch, 49 pairs) against the composition the library offered before it: 49 x (hevcdl_deblock_frames_dev into a trial
  picture + the SSE of that picture against the original, hevcdl_picture_report_dev with method 0: hevcdl_launch_quality_sse and a small finish launch), alternating; the ratio.
The pipeline's pictures are smooth waves coded with depth-0 labels at QP 37, content the metric switches on.  No threshold: a record.  Needs a GPU."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
W, H, QP = 3840, 2160, 37


def events_ms(fn, reps):
    import torch
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return out


def stat(ms, per):
    ms = sorted(v / per for v in ms)
    return "min %.4f  median %.4f  max %.4f" % (ms[0], ms[len(ms) // 2], ms[-1])


def main(batch, reps, pipe_frames):
    import torch
    import hevcdl_amd
    import ref_tools
    if not torch.cuda.is_available():
        sys.exit("no GPU: nothing is measured")
    n = W * H * 3 // 2
    g = torch.Generator(device="cuda").manual_seed(1)
    # smooth content with a little noise: lines on both sides of the metric's thresholds (pure noise never qualifies and would time the cheap path only)
    x = torch.arange(W, device="cuda").view(1, 1, W); y = torch.arange(H, device="cuda").view(1, H, 1)
    luma = (128 + 60 * torch.sin(x / 23.0) * torch.cos(y / 17.0) + ((x // 32) * 5 + (y // 32) * 3) % 17).expand(batch, H, W) + torch.randint(-1, 2, (batch, H, W), dtype=torch.int16, device="cuda", generator=g)
    pics = torch.cat([luma.clamp(0, 255).to(torch.uint8).view(batch, -1), torch.randint(0, 256, (batch, n - W * H), dtype=torch.uint8, device="cuda", generator=g)], dim=1).contiguous()
    sums = torch.zeros((batch, 2), dtype=torch.int64, device="cuda")
    enc = hevcdl_amd.Encoder(W, H, QP, max_frames=batch)
    ctus = enc.ctus
    recs = torch.zeros((batch, ctus * hevcdl_amd.REC_DTYPE.itemsize), dtype=torch.uint8, device="cuda")      # all-zero records: one 64x64 CU per CTU, 32x32 transform blocks
    recs.view(batch, ctus, -1)[:, :, 4 * 256:5 * 256] = 1      # tr_idx 1
    out = torch.zeros_like(pics)
    metric = lambda: enc.dbk_metric_frames_dev(pics.data_ptr(), batch, sums.data_ptr())
    metric(); torch.cuda.synchronize()
    host = pics[:1, :W * H].cpu().numpy().reshape(H, W)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import dbk_select_ref
    want = dbk_select_ref.metric_sums(host, QP, 8)
    assert tuple(int(v) for v in sums[0].cpu()) == want, (sums[0], want)
    print("picture %dx%d, 8 bits, QP %d, batch of %d in device buffers, HIP events, %d repetitions after a warm-up; picture 0's sums %s equal the CPU restatement" % (W, H, QP, batch, reps, want))
    ms = events_ms(metric, reps)
    # what the launch must move lies between the bytes it asks for (8 a line across a vertical edge, six rows a horizontal edge) and the whole 128-byte lines those sit in
    asked = ((W >> 5) - 1) * H * 8 + ((H >> 5) - 1) * 6 * W
    lines = ((W >> 5) - 1) * H * 128 + ((H >> 5) - 1) * 6 * W
    med = sorted(ms)[len(ms) // 2] / batch * 1e-3
    print("metric launch (memset + hevcdl_dbk_metric_kernel), ms per picture: %s" % stat(ms, batch))
    print("  bytes per picture of %.2f MB luma: %.2f MB asked for, %.2f MB if every 128-byte line they sit in is fetched whole; at the median %.0f .. %.0f GB/s (how much of a line the memory system really fetches was not measured)"
          % (W * H / 1e6, asked / 1e6, lines / 1e6, asked / 1e9 / med, lines / 1e9 / med))
    choices = np.zeros(batch, hevcdl_amd.DBK_CHOICE_DTYPE)
    choices["override_enabled"] = 1; choices["override_flag"] = np.arange(batch) % 2; choices["beta_offset_div2"] = choices["tc_offset_div2"] = (np.arange(batch) % 5 + 2) * (np.arange(batch) % 2)
    plain = lambda: enc.deblock_frames_dev(pics.data_ptr(), batch, recs.data_ptr(), out.data_ptr())
    rows = lambda: enc.deblock_frames_choice_dev(pics.data_ptr(), batch, recs.data_ptr(), choices, out.data_ptr())
    plain(); rows(); torch.cuda.synchronize()
    a, b = [], []
    for _ in range(reps):      # alternating, so that both see the same machine
        a += events_ms(plain, 1); b += events_ms(rows, 1)
    print("deblocking launches (luma + chroma), ms per picture:\n  one triple per launch:        %s\n  a row of parameters a picture: %s  (with the upload of the rows)" % (stat(a, batch), stat(b, batch)))
    # DeblockingFilterMetric 2: the fused trial launch against 49 x (deblock + SSE), on a smaller batch (the composition needs 49 passes over it)
    tb = min(batch, 32)
    org = (pics[:tb].to(torch.int16) + torch.randint(-3, 4, (tb, n), dtype=torch.int16, device="cuda", generator=g)).clamp(0, 255).to(torch.uint8)
    tables = torch.zeros((tb, 49), dtype=torch.int64, device="cuda")
    rep_out = torch.zeros((tb, hevcdl_amd.REPORT_DTYPE.itemsize), dtype=torch.uint8, device="cuda")
    fused = lambda: enc.dbk_trial_frames_dev(org.data_ptr(), pics.data_ptr(), tb, recs.data_ptr(), tables.data_ptr())

    def naive():
        for _ in range(49):
            enc.deblock_frames_dev(pics.data_ptr(), tb, recs.data_ptr(), out.data_ptr())
            enc.picture_report_dev(org.data_ptr(), out.data_ptr(), tb, 0, rep_out.data_ptr())
    fused(); naive(); torch.cuda.synchronize()
    # the centre entry (0, 0) of picture 0 is the composition's number for the context's own offsets
    sse = np.frombuffer(rep_out[0].cpu().numpy().tobytes(), hevcdl_amd.REPORT_DTYPE)[0]["sse"]
    assert int(tables[0, 24].cpu()) == int(sse.sum()), (int(tables[0, 24].cpu()), sse)
    a, b = [], []
    for _ in range(max(3, reps // 2)):
        a += events_ms(fused, 1); b += events_ms(naive, 1)
    ma, mb = sorted(a)[len(a) // 2] / tb, sorted(b)[len(b) // 2] / tb
    print("DeblockingFilterMetric 2, batch of %d, ms per picture (entry (0, 0) of picture 0 equals the composition's SSE):\n  trial launch (memset + luma + chroma kernels, 49 pairs): %s\n  49 x (deblock launches + SSE launches):              %s\n  ratio composition / trial launch at the medians: %.2f"
          % (tb, stat(a, tb), stat(b, tb), mb / ma))
    enc.close()
    del pics, out, recs, org
    torch.cuda.empty_cache()
    # the whole pipeline step: two contexts on the same build, alternating
    import gen_dbk_select_fixtures as fixtures
    two = fixtures.waves(W, H, (60, 25), (0, 0), 5)
    yuv = np.concatenate([two] * (pipe_frames // 2))
    labels = np.zeros((pipe_frames, ((W + 63) // 64) * ((H + 63) // 64), 16), np.uint8)      # depth 0 (the library clamps them to the picture): 32x32 transform blocks, the grid the metric looks at
    encs = {0: hevcdl_amd.Encoder(W, H, QP, max_frames=pipe_frames), 1: hevcdl_amd.Encoder(W, H, QP, max_frames=pipe_frames, deblocking_metric=1, lf_offset_in_pps=False),
            2: hevcdl_amd.Encoder(W, H, QP, max_frames=pipe_frames, deblocking_metric=2, lf_offset_in_pps=False)}
    t = {0: [], 1: [], 2: []}
    for rep in range(reps + 1):
        for k, e in encs.items():
            t0 = time.time(); e.encode_pictures(yuv, labels); dtm = (time.time() - t0) * 1e3
            if rep:
                t[k].append(dtm)
    over = int(encs[1].get_dbk_choice(0, pipe_frames)["override_flag"].sum())
    over2 = int(encs[2].get_dbk_choice(0, pipe_frames)["override_flag"].sum())
    for e in encs.values():
        e.close()
    print("whole picture pipeline (hevcdl_encode_pictures, host buffers, %d pictures, depth-0 labels, wall clock around the call), ms per picture, %d alternating repetitions after a warm-up:" % (pipe_frames, reps))
    print("  DeblockingFilterMetric 0: %s\n  DeblockingFilterMetric 1: %s  (%d of %d pictures override)\n  DeblockingFilterMetric 2: %s  (%d of %d pictures override)"
          % (stat(t[0], pipe_frames), stat(t[1], pipe_frames), over, pipe_frames, stat(t[2], pipe_frames), over2, pipe_frames))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=96)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--pipe-frames", type=int, default=16)
    a = ap.parse_args()
    main(a.batch, a.reps, a.pipe_frames)
