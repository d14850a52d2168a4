"""DeltaQpRD (csrc/qp_rd_kernel.hip, hevcdl_api.hip qp_rd_search): what the key costs, as a record -> profiles/deltaqprd_time.txt.  Needs an MI355X.

  --device [--n N]   3840 x 2160 at QP 32, DeltaQpRD N (default 1), device buffers (hevcdl_compress_frames_dev on labels of the on-device CNN), batches of 1 and 75 pictures
                     and 600 pictures as 8 batches of 75 (the CLI's BatchFrames form): the 2N+1 decision launches (hevcdl_profile_get), the sum launches and the keep
                     launches from HIP events (hevcdl_get_qp_rd_info), the bytes the keep launches moved -- counted from the rows: a picture is copied behind every candidate
                     that beats the best before it, records + reconstruction + statistics read and written -- and the rate that gives; the wall time of the call against the
                     same call on a context with the key 0.
  --against LIB [--rounds R]   the key-0 path: hevcdl_compress_frames_dev of this tree's library and of LIB (the parent commit's build) in alternation, R rounds each
                     (default 7), 75 pictures of 3840 x 2160; medians, and the other library's interquartile spread as the margin the machine supports.
Sections that were not run are written as NOT TIMED YET."""
import argparse
import ctypes
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
W, H, QP = 3840, 2160, 32


def quartiles(v):
    q1, med, q3 = np.percentile(np.asarray(v, float), [25, 50, 75])
    return float(med), float(q3 - q1)


def frames(n):
    """n pictures: three distinct synthetic frames, repeated (a frame is a serial chain; what a launch costs depends on the number of frames, not on their being unlike)."""
    import ref_tools
    base = ref_tools.synth_yuv(W, H, 3, seed=41)
    return base[np.arange(n) % 3]


class DeviceBuffers:
    def __init__(self, torch, enc, yuv):
        n = yuv.shape[0]
        dev = torch.device("cuda", 0)
        self.n = n
        self.yuv = torch.from_numpy(yuv).to(dev)
        self.labels = torch.zeros((n, enc.ctus, 16), dtype=torch.uint8, device=dev)
        self.records = torch.zeros((n, enc.ctus * 15120), dtype=torch.uint8, device=dev)
        self.recon = torch.zeros_like(self.yuv)
        self.stats = torch.zeros((n, 40), dtype=torch.uint8, device=dev)


def timed_call(torch, fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def device_section(out, n_key):
    import torch
    import hevcdl_amd
    import deltaqprd_cases as dc
    out.append("== device: %dx%d, QP %d, DeltaQpRD %d (%d candidates), device buffers, labels of the on-device CNN ==" % (W, H, QP, n_key, 2 * n_key + 1))
    for batch, repeats in ((1, 1), (75, 1), (75, 8)):
        yuv = frames(batch)
        per_pic = None
        res = {}
        for key in (0, n_key):
            enc = hevcdl_amd.Encoder(W, H, QP, max_frames=batch, delta_qp_rd=key)
            try:
                enc.reserve_workspace()
                b = DeviceBuffers(torch, enc, yuv)
                enc.predict_depth_dev(b.yuv.data_ptr(), batch, b.labels.data_ptr())
                call = lambda: enc.compress_frames_dev(b.yuv.data_ptr(), batch, b.labels.data_ptr(), b.records.data_ptr(), b.recon.data_ptr(), b.stats.data_ptr())
                timed_call(torch, call)                                   # the first call pays what is paid once
                enc.profile_enable(True)
                wall = rd = s_ms = k_ms = 0.0
                moved = 0
                for _ in range(repeats):
                    wall += timed_call(torch, call)
                    rd += enc.profile_get()["rd_ms"]
                    if key:
                        ms = enc.get_qp_rd_kernel_ms()
                        s_ms, k_ms = s_ms + ms[0], k_ms + ms[1]
                        rows, _ = enc.get_qp_rd(0, batch)
                        per_pic = enc.ctus * 15120 + enc.frame_bytes + 40
                        lam = hevcdl_amd.qp_rd_candidates(enc.cfg)[1]
                        for r in rows:                                    # a candidate behind the first is copied when it beats every candidate before it
                            moved += sum(1 for i in range(1, 2 * key + 1) if dc.pick(r["bits"][:i + 1], r["dist"][:i + 1], lam) == i)
                res[key] = (wall, rd, s_ms, k_ms, moved)
            finally:
                enc.close()
        n = batch * repeats
        w0, rd0 = res[0][0], res[0][1]
        w1, rd1, s_ms, k_ms, moved = res[n_key]
        out.append("%d pictures%s: key 0: call %.3f s (decision launch %.1f ms); key %d: call %.3f s = %.2f x; %d decision launches %.1f ms; sum launches %.3f ms; keep launches %.3f ms"
                   % (n, " as %d calls of %d" % (repeats, batch) if repeats > 1 else "", w0, rd0, n_key, w1, w1 / w0, (2 * n_key + 1) * repeats, rd1, s_ms, k_ms))
        out.append("    keep: %d picture copies of %.1f MB, read and written: %.1f MB in %.3f ms = %s" % (moved, per_pic / 1e6, 2 * moved * per_pic / 1e6, k_ms,
                   ("%.0f GB/s" % (2 * moved * per_pic / 1e9 / (k_ms / 1e3))) if moved and k_ms > 0 else "no picture was copied"))


def against_section(out, other, rounds):
    import torch
    import hevcdl_amd
    batch = 75
    libs = (("base", ctypes.CDLL(os.path.abspath(other))), ("this", hevcdl_amd.load_library()))
    out.append("== the key-0 path: this library against base = %s: hevcdl_compress_frames_dev, %d pictures of %dx%d at QP %d; %d rounds each in alternation ==" % (other, batch, W, H, QP, rounds))
    yuv = frames(batch)
    wts = hevcdl_amd.load_weights()
    vp, ci = ctypes.c_void_p, ctypes.c_int
    ctxs = {}
    for name, lib in libs:      # every library fills its own configuration (the parent's struct is shorter: struct_size says which)
        cfg = hevcdl_amd.Config()
        lib.hevcdl_config_default_bd.argtypes = [vp, ci, ci, ci, ci]
        assert lib.hevcdl_config_default_bd(ctypes.byref(cfg), W, H, QP, 8) == 0
        cfg.max_frames = batch
        h = vp()
        lib.hevcdl_create.argtypes = [vp, vp, ctypes.c_size_t, vp]
        assert lib.hevcdl_create(ctypes.byref(cfg), wts.ctypes.data, wts.size, ctypes.byref(h)) == 0, name
        lib.hevcdl_reserve_workspace.argtypes = [vp]
        lib.hevcdl_predict_depth_dev.argtypes = [vp, vp, ci, vp, vp, vp]
        lib.hevcdl_compress_frames_dev.argtypes = [vp, vp, ci, vp, vp, vp, vp, vp]
        lib.hevcdl_destroy.argtypes = [vp]
        assert lib.hevcdl_reserve_workspace(h) == 0
        ctxs[name] = h
    dev = torch.device("cuda", 0)
    d_yuv = torch.from_numpy(yuv).to(dev)
    ctus = ((W + 63) // 64) * ((H + 63) // 64)
    d_lab = torch.zeros((batch, ctus, 16), dtype=torch.uint8, device=dev)
    d_stats = torch.zeros((batch, 40), dtype=torch.uint8, device=dev)
    outs = {name: (torch.zeros((batch, ctus * 15120), dtype=torch.uint8, device=dev), torch.zeros_like(d_yuv)) for name, _ in libs}
    assert libs[1][1].hevcdl_predict_depth_dev(ctxs["this"], d_yuv.data_ptr(), batch, d_lab.data_ptr(), None, None) == 0

    def call(name, lib):
        assert lib.hevcdl_compress_frames_dev(ctxs[name], d_yuv.data_ptr(), batch, d_lab.data_ptr(), outs[name][0].data_ptr(), outs[name][1].data_ptr(), d_stats.data_ptr(), None) == 0
    for name, lib in libs:
        timed_call(torch, lambda: call(name, lib))
    same = bool(torch.equal(outs["base"][0], outs["this"][0]) and torch.equal(outs["base"][1], outs["this"][1]))
    out.append("records and reconstruction of the two libraries: %s" % ("identical" if same else "DIFFERENT"))
    got = {"base": [], "this": []}
    for _ in range(rounds):
        for name, lib in libs:
            got[name].append(timed_call(torch, lambda: call(name, lib)) * 1e3)
    for name, lib in libs:
        lib.hevcdl_destroy(ctxs[name])
    (mb, iqr), (mt, _) = quartiles(got["base"]), quartiles(got["this"])
    for name in ("base", "this"):
        out.append("%s [ms]: %s" % (name, " ".join("%.1f" % v for v in got[name])))
    out.append("median base %.1f ms, this %.1f ms (%+.2f %%); interquartile spread of base %.1f ms: %s" % (mb, mt, 100 * (mt - mb) / mb, iqr, "within" if mt <= mb + iqr else "SLOWER THAN THE MARGIN"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", action="store_true")
    ap.add_argument("--n", type=int, default=1)
    ap.add_argument("--against", default=None, metavar="LIB")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "deltaqprd_time.txt"))
    a = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    lines = ["DeltaQpRD (csrc/qp_rd_kernel.hip, hevcdl_api.hip qp_rd_search).  Sections as tools/time_deltaqprd.py prints them (--device, --against).  No threshold was fixed in advance.", ""]
    if a.device:
        device_section(lines, a.n)
    else:
        lines.append("== device ==\nNOT TIMED YET.")
    lines.append("")
    if a.against:
        against_section(lines, a.against, a.rounds)
    else:
        lines.append("== the key-0 path against the parent commit's library ==\nNOT TIMED YET.")
    open(a.out, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
