"""Source format: the host's conversion functions against the device kernels (csrc/source_core.h, csrc/source_kernel.hip), as a record -> profiles/source_time.txt.

  --host     needs no GPU.  hevcdl_load_source_host / hevcdl_store_output_host on one 3840 x 2160 picture on one core (best of 3), 8 -> 8 and 8 -> 10 bits.
  --device   needs an MI355X.  HIP-event times of the load and the store launch for 1, 75 and 600 pictures of 3840 x 2160 already in HBM, 8 -> 8 and 8 -> 10 bits
             (second and third of three runs, the shorter), the bytes each launch moves and that as a fraction of the HBM peak (8.0 TB/s by the data sheet; a float4
             copy reaches about 6.3); and the bytes a picture pipeline call uploads per picture with and without a source format, 8 -> 10.
A half that is not run keeps what the file holds for it (or NOT TIMED YET)."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
W, H = 3840, 2160
HBM_PEAK = 8.0e12
PAIRS = ((8, 8), (8, 10))


def best_of(fn, reps=3):
    best = 1e9
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); best = min(best, time.perf_counter() - t0)
    return best


def host_section(out):
    import hevcdl_amd
    out.append("== host: one %dx%d picture on one core; %d CPUs here ==" % (W, H, os.cpu_count() or 1))
    rng = np.random.default_rng(1)
    for in_bd, bd in PAIRS:
        fmt = hevcdl_amd.source_format(W, H, in_bd, in_bd)
        src = rng.integers(0, 1 << in_bd, W * H * 3 // 2).astype(np.uint8 if in_bd == 8 else "<u2")[None]
        pic = rng.integers(0, 1 << bd, W * H * 3 // 2).astype(np.uint8 if bd == 8 else "<u2")[None]
        out.append("%d -> %d bits: hevcdl_load_source_host %.2f ms, hevcdl_store_output_host (back to %d bits) %.2f ms per picture (the Python wrapper's allocation of the result included)"
                   % (in_bd, bd, 1e3 * best_of(lambda: hevcdl_amd.load_source_host(fmt, W, H, bd, src)), in_bd, 1e3 * best_of(lambda: hevcdl_amd.store_output_host(fmt, W, H, bd, pic))))


def device_section(out):
    import torch
    import hevcdl_amd
    fs = W * H * 3 // 2
    out.append("== device: %dx%d, no padding; launches timed with HIP events on the launch stream, the shorter of the second and third run ==" % (W, H))
    stream = torch.cuda.current_stream().cuda_stream
    for in_bd, bd in PAIRS:
        sb, cb = (1 if in_bd == 8 else 2), (1 if bd == 8 else 2)
        for n in (1, 75, 600):
            enc = hevcdl_amd.Encoder(W, H, 32, max_frames=n, bit_depth=bd)
            enc.set_source_format(hevcdl_amd.source_format(W, H, in_bd, in_bd))
            d_src = torch.randint(0, 256, (n, fs * sb), dtype=torch.uint8, device="cuda")
            d_pic = torch.zeros((n, fs * cb), dtype=torch.uint8, device="cuda")
            d_out = torch.zeros((n, fs * sb), dtype=torch.uint8, device="cuda")
            ms = {}
            for name, fn in (("load", lambda: enc.load_source_dev(d_src.data_ptr(), n, d_pic.data_ptr(), stream)), ("store", lambda: enc.store_output_dev(d_pic.data_ptr(), n, d_out.data_ptr(), stream))):
                best = 1e9
                for rep in range(3):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record(); fn(); b.record()
                    torch.cuda.synchronize()
                    if rep:
                        best = min(best, a.elapsed_time(b))
                ms[name] = best
            moved = n * fs * (sb + cb)
            out.append("%d -> %d bits, %3d pictures: load launch %.3f ms (%.3f ms per picture, %.0f%% of the HBM peak), store launch %.3f ms (%.0f%%); %.1f MB moved by each"
                       % (in_bd, bd, n, ms["load"], ms["load"] / n, 100 * moved / (ms["load"] * 1e-3) / HBM_PEAK, ms["store"], 100 * moved / (ms["store"] * 1e-3) / HBM_PEAK, moved / 1e6))
            assert torch.equal(d_out, d_src) or bd < in_bd      # up and back down again gives the source
            del d_src, d_pic, d_out
            enc.close()
            torch.cuda.empty_cache()
    out.append("upload per picture of a picture pipeline call, 8-bit source coded at 10 bits: %d bytes with a source format (the file's own frame), %d without (the caller converts on the host and uploads the coded format)"
               % (fs, 2 * fs))


def halves(path):
    host, dev = ["== host ==", "NOT TIMED YET."], ["== device ==", "NOT TIMED YET."]
    if os.path.exists(path):
        lines = open(path).read().splitlines()
        at_h = [i for i, ln in enumerate(lines) if ln.startswith("== host")]
        at_d = [i for i, ln in enumerate(lines) if ln.startswith("== device")]
        if at_h and at_d:
            host = [ln for ln in lines[at_h[0]:at_d[0]] if ln.strip()]
            dev = [ln for ln in lines[at_d[0]:] if ln.strip()]
    return host, dev


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--device", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "source_time.txt"))
    a = ap.parse_args()
    host, dev = halves(a.out)
    if a.host:
        host = []
        host_section(host)
    if a.device:
        dev = []
        device_section(dev)
    lines = ["Source format (csrc/source_core.h, csrc/source_kernel.hip).  Halves as tools/time_source.py writes them (--host, --device).", ""] + host + [""] + dev
    open(a.out, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))
