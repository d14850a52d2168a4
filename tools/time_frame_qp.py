"""A QP per picture (csrc/frame_permute_kernel.hip, hevcdl_api.hip frame_qp_decide): what the grouping costs, as a record -> profiles/frame_qp_time.txt.  Needs an MI355X.

64 pictures of 1920 x 1080, device buffers, labels of the on-device CNN, in one session; every step is a process of its own under its own time limit, and a step that
fails ends the session (the steps behind it are written as NOT TIMED):
  a  one call with two alternating QPs (32 37 32 37 ...): the permuted path -- gather, two decision launches, scatter;
  b  the same call with the list sorted (32 x 32, then 37 x 32): two decision launches on offsets into the caller's buffers, nothing copied;
  c  two calls of 32 pictures from two contexts at QP 32 and QP 37 -- with --parent LIB on the parent commit's library, which is what a sweep cost before; otherwise on
     this tree's library without a list (the same code path).
The permute kernel's time comes from HIP events round its two launches (hevcdl_get_frame_qp_info); bytes counts what a launch reads plus what it writes.
The file is a record: no test takes a threshold from it."""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
W, H, N, QPS, ROUNDS = 1920, 1080, 64, (32, 37), 5
LIMIT = {"a": 240, "b": 240, "c": 240}      # seconds a step may take, context creation and the first (paying) call included


def frames(n):
    import ref_tools
    base = ref_tools.synth_yuv(W, H, 4, seed=43)
    return base[np.arange(n) % 4]


def timed(torch, fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def step_list(kind):
    import torch
    import hevcdl_amd
    dev = torch.device("cuda", 0)
    enc = hevcdl_amd.Encoder(W, H, QPS[0], max_frames=N)
    try:
        qps = list(QPS) * (N // 2) if kind == "a" else [QPS[0]] * (N // 2) + [QPS[1]] * (N // 2)
        enc.set_frame_qps(qps)
        enc.reserve_workspace()
        d_yuv = torch.from_numpy(frames(N)).to(dev)
        d_lab = torch.zeros((N, enc.ctus, 16), dtype=torch.uint8, device=dev)
        d_rec = torch.zeros((N, enc.ctus * 15120), dtype=torch.uint8, device=dev)
        d_recon, d_stats = torch.zeros_like(d_yuv), torch.zeros((N, 40), dtype=torch.uint8, device=dev)
        enc.predict_depth_dev(d_yuv.data_ptr(), N, d_lab.data_ptr())
        call = lambda: enc.compress_frames_dev(d_yuv.data_ptr(), N, d_lab.data_ptr(), d_rec.data_ptr(), d_recon.data_ptr(), d_stats.data_ptr())
        timed(torch, call)                                   # the first call pays what is paid once
        enc.profile_enable(True)
        wall, rd, gather, scatter = [], [], [], []
        for _ in range(ROUNDS):
            wall.append(timed(torch, call))
            rd.append(enc.profile_get()["rd_ms"])
            info = enc.get_frame_qp_info(want_ms=True)
            gather.append(info[3][0]); scatter.append(info[3][1])
        per_gather, per_scatter = enc.frame_bytes + 16 * enc.ctus, enc.ctus * 15120 + enc.frame_bytes + 40
        return dict(step=kind, wall_ms=wall, rd_ms=rd, gather_ms=gather, scatter_ms=scatter, rd_launches=info[1], permute_launches=info[2], set_bytes=info[0],
                    gather_bytes=2 * N * per_gather, scatter_bytes=2 * N * per_scatter, launch=enc.last_rd_launch())
    finally:
        enc.close()


def step_two_contexts(parent):
    import torch
    import hevcdl_amd
    lib = ctypes.CDLL(os.path.abspath(parent)) if parent else hevcdl_amd.load_library()
    vp, ci = ctypes.c_void_p, ctypes.c_int
    lib.hevcdl_config_default_bd.argtypes = [vp, ci, ci, ci, ci]
    lib.hevcdl_create.argtypes = [vp, vp, ctypes.c_size_t, vp]
    lib.hevcdl_reserve_workspace.argtypes = [vp]
    lib.hevcdl_predict_depth_dev.argtypes = [vp, vp, ci, vp, vp, vp]
    lib.hevcdl_compress_frames_dev.argtypes = [vp, vp, ci, vp, vp, vp, vp, vp]
    lib.hevcdl_destroy.argtypes = [vp]
    dev = torch.device("cuda", 0)
    half, wts = N // 2, hevcdl_amd.load_weights()
    ctus = ((W + 63) // 64) * ((H + 63) // 64)
    ctxs = []
    for qp in QPS:      # the library fills its own configuration (the parent's struct may be shorter: struct_size says which)
        cfg = hevcdl_amd.Config()
        assert lib.hevcdl_config_default_bd(ctypes.byref(cfg), W, H, qp, 8) == 0
        cfg.max_frames = half
        h = vp()
        assert lib.hevcdl_create(ctypes.byref(cfg), wts.ctypes.data, wts.size, ctypes.byref(h)) == 0
        assert lib.hevcdl_reserve_workspace(h) == 0
        ctxs.append(h)
    try:
        d_yuv = torch.from_numpy(frames(N)[::2].copy()).to(dev)      # the 32 pictures a QP of steps a and b
        d_lab = torch.zeros((half, ctus, 16), dtype=torch.uint8, device=dev)
        d_rec = [torch.zeros((half, ctus * 15120), dtype=torch.uint8, device=dev) for _ in QPS]
        d_recon = [torch.zeros_like(d_yuv) for _ in QPS]
        d_stats = torch.zeros((half, 40), dtype=torch.uint8, device=dev)
        assert lib.hevcdl_predict_depth_dev(ctxs[0], d_yuv.data_ptr(), half, d_lab.data_ptr(), None, None) == 0

        def call():
            for k, h in enumerate(ctxs):
                assert lib.hevcdl_compress_frames_dev(h, d_yuv.data_ptr(), half, d_lab.data_ptr(), d_rec[k].data_ptr(), d_recon[k].data_ptr(), d_stats.data_ptr(), None) == 0
        timed(torch, call)
        wall = [timed(torch, call) for _ in range(ROUNDS)]
        return dict(step="c", wall_ms=wall, library="parent" if parent else "this tree, no list")
    finally:
        for h in ctxs:
            lib.hevcdl_destroy(h)


def med(v):
    return float(np.median(np.asarray(v, float)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", choices=["a", "b", "c"], default=None, help="run one step in this process and print its JSON line")
    ap.add_argument("--parent", default=None, metavar="LIB", help="the parent commit's libhevcdl_hip.so for step c")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "frame_qp_time.txt"))
    a = ap.parse_args()
    if a.step:
        res = step_two_contexts(a.parent) if a.step == "c" else step_list(a.step)
        print("RESULT " + json.dumps(res))
        return
    lines = ["A QP per picture (csrc/frame_permute_kernel.hip, hevcdl_api.hip frame_qp_decide): %d pictures of %dx%d, QPs %d and %d, device buffers, labels of the on-device CNN; medians of %d calls"
             % (N, W, H, QPS[0], QPS[1], ROUNDS), "behind one call that pays what is paid once.  Steps as tools/time_frame_qp.py runs them.  No threshold was fixed in advance.", ""]
    res, failed = {}, None
    for step in ("a", "b", "c"):
        if failed:
            lines.append("== %s ==\nNOT TIMED: step %s did not finish." % (step, failed))
            continue
        cmd = [sys.executable, os.path.abspath(__file__), "--step", step] + (["--parent", a.parent] if a.parent and step == "c" else [])
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=LIMIT[step])
            got = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
            if r.returncode != 0 or not got:
                failed = step
                lines.append("== %s ==\nFAILED with exit status %d: %s" % (step, r.returncode, (r.stderr.strip().splitlines() or [""])[-1][:300]))
                continue
            res[step] = json.loads(got[-1][len("RESULT "):])
        except subprocess.TimeoutExpired:
            failed = step
            lines.append("== %s ==\nNOT FINISHED within %d s." % (step, LIMIT[step]))
            continue
        d = res[step]
        if step in ("a", "b"):
            lines.append("== %s: one call, list %s ==" % (step, "32 37 32 37 ... (the permuted path)" if step == "a" else "32 x 32 then 37 x 32 (contiguous runs, no copy)"))
            lines.append("call %.2f ms; %d decision launches %.2f ms; %d permute launches; sorted sets %.1f MB; last launch: %s" % (med(d["wall_ms"]), d["rd_launches"], med(d["rd_ms"]), d["permute_launches"], d["set_bytes"] / 1e6, d["launch"]))
            if d["permute_launches"]:
                g, s = med(d["gather_ms"]), med(d["scatter_ms"])
                lines.append("    gather  (originals, labels): %.1f MB read and written in %.3f ms = %.0f GB/s" % (d["gather_bytes"] / 1e6, g, d["gather_bytes"] / 1e9 / (g / 1e3) if g > 0 else 0))
                lines.append("    scatter (records, reconstruction, statistics): %.1f MB read and written in %.3f ms = %.0f GB/s" % (d["scatter_bytes"] / 1e6, s, d["scatter_bytes"] / 1e9 / (s / 1e3) if s > 0 else 0))
            lines.append("    calls [ms]: " + " ".join("%.2f" % v for v in d["wall_ms"]))
        else:
            lines.append("== c: two calls of %d pictures from two contexts (%s) ==" % (N // 2, d["library"]))
            lines.append("both calls %.2f ms; calls [ms]: %s" % (med(d["wall_ms"]), " ".join("%.2f" % v for v in d["wall_ms"])))
        lines.append("")
    if "a" in res and "b" in res and "c" in res:
        lines.append("a / b = %.3f, a / c = %.3f, b / c = %.3f (medians)" % (med(res["a"]["wall_ms"]) / med(res["b"]["wall_ms"]), med(res["a"]["wall_ms"]) / med(res["c"]["wall_ms"]), med(res["b"]["wall_ms"]) / med(res["c"]["wall_ms"])))
    open(a.out, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))
    sys.exit(1 if failed else 0)


if __name__ == "__main__":
    main()
