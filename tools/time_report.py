"""Picture report: the host's hash and SSE loops against the device kernels (csrc/report_kernel.hip, the SSE kernel of csrc/quality_kernel.hip), as a record
-> profiles/report_time.txt.

  --host     needs no GPU.  hevcdl_picture_hash per 3840 x 2160 picture on one core for the three methods (best of 3), and the CLI's SSE loop (csrc/hevcdl_app.cpp, restated
             in a small C++ program compiled here with the host compiler at -O2, as the CLI is) on the same picture.
  --device   needs an MI355X.  HIP-event times of the SSE / partial or MD5 / finish launches (Encoder.report_info with profile_enable) for 1, 75 and 600 pictures of
             3840 x 2160 already in HBM, each method, second of two runs; then hevcdl_encode_pictures_stream with device entropy for 75 pictures: with the pictures handed
             to the callback (what a run that prints PSNR and writes a hash SEI needs without the report) and without them but with the report on: wall time and the bytes
             handed to the callback, counted from the arrays handed over.
A half that is not run keeps what the file holds for it (or NOT TIMED YET)."""
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
METHODS = ((1, "MD5"), (2, "CRC"), (3, "checksum"))

SSE_LOOP = r"""
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdint>
#include <vector>
int main() {
  const size_t n = (size_t)3840 * 2160 * 3 / 2;
  std::vector<uint8_t> o(n), r(n);
  uint32_t s = 12345;
  for (size_t i = 0; i < n; i++) { s = s * 1664525u + 1013904223u; o[i] = (uint8_t)(s >> 24); r[i] = (uint8_t)(o[i] + ((s >> 8) & 3)); }
  double best = 1e9; unsigned long long keep = 0;
  for (int rep = 0; rep < 3; rep++) {
    const auto t0 = std::chrono::steady_clock::now();
    unsigned long long sse = 0;
    for (size_t k0 = 0; k0 < n; k0 += 4096) { // 32-bit partial sums over short runs: the loop vectorises (hevcdl_app.cpp)
      unsigned part = 0; const size_t k1 = std::min(n, k0 + 4096);
      for (size_t k = k0; k < k1; k++) { const int d = (int)o[k] - (int)r[k]; part += (unsigned)(d * d); }
      sse += part;
    }
    keep += sse;
    best = std::min(best, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
  }
  printf("%.3f %llu\n", best * 1e3, keep);
  return 0;
}
"""


def best_of(fn, reps=3):
    best = 1e9
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); best = min(best, time.perf_counter() - t0)
    return best


def host_section(out):
    import hevcdl_amd
    out.append("== host: one %dx%d picture of 8-bit samples on one core; %d CPUs here ==" % (W, H, os.cpu_count() or 1))
    pic = np.random.default_rng(1).integers(0, 256, W * H * 3 // 2).astype(np.uint8)
    for m, name in METHODS:
        out.append("hevcdl_picture_hash, %s: %.2f ms per picture" % (name, 1e3 * best_of(lambda: hevcdl_amd.picture_hash(W, H, pic, 8, m))))
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "sse.cpp"), "w").write(SSE_LOOP)
        subprocess.run(["g++", "-O2", "-std=c++17", os.path.join(d, "sse.cpp"), "-o", os.path.join(d, "sse")], check=True)
        ms = subprocess.run([os.path.join(d, "sse")], check=True, capture_output=True, text=True).stdout.split()[0]
    out.append("the CLI's SSE loop (three planes): %s ms per picture" % ms)


def device_section(out):
    import torch
    import hevcdl_amd
    import ref_tools
    fb = W * H * 3 // 2
    out.append("== device: %dx%d, 8-bit samples; launches timed with HIP events, second of two runs ==" % (W, H))
    for n in (1, 75, 600):
        enc = hevcdl_amd.Encoder(W, H, 32, max_frames=n)
        enc.profile_enable(True)
        d_pic = torch.randint(0, 256, (n, fb), dtype=torch.uint8, device="cuda")
        d_org = torch.randint(0, 256, (n, fb), dtype=torch.uint8, device="cuda")
        d_out = torch.zeros(n * 80, dtype=torch.uint8, device="cuda")
        for m, name in METHODS:
            for _ in range(2):
                enc.picture_report_dev(d_org.data_ptr(), d_pic.data_ptr(), n, m, d_out.data_ptr())
                torch.cuda.synchronize()
            ms = enc.report_info()
            out.append("%3d pictures, %-8s: SSE launch %.3f ms, %s launch %.3f ms, finish launch %.3f ms; all three %.3f ms = %.3f ms per picture"
                       % (n, name, ms[0], "MD5" if m == 1 else "partial", ms[1], ms[2], sum(ms), sum(ms) / n))
        del d_pic, d_org, d_out
        enc.close()
        torch.cuda.empty_cache()
    n = 75
    out.append("== device: hevcdl_encode_pictures_stream with device entropy, %d pictures of %dx%d, QP 32; second of two calls ==" % (n, W, H))
    yuv = np.tile(ref_tools.synth_yuv(W, H, 1, seed=2), (n, 1))
    enc = hevcdl_amd.Encoder(W, H, 32, max_frames=n)
    enc.enable_device_entropy(True)

    def handed(chunks):
        return sum(sum(len(d) for d in c[1]) + c[2].nbytes + c[3].nbytes + (c[4].nbytes if c[4] is not None else 0) + (c[5].nbytes if c[5] is not None else 0) for c in chunks)
    for label, method, want in (("report off, pictures handed over (for the host's SSE and hash)", None, True), ("report on (MD5), no pictures", 1, False),
                                ("report on (CRC), no pictures", 2, False), ("report on (checksum), no pictures", 3, False)):
        enc.enable_picture_report(method is not None, method or 0)
        for _ in range(2):
            t0 = time.perf_counter()
            chunks = enc.encode_pictures_stream(yuv, want_pictures=want)
            t = time.perf_counter() - t0
        extra = 80 * n if method is not None else 0
        out.append("%s: wall %.3f s; bytes handed to the callback %d (+ %d of reports) = %.0f per picture" % (label, t, handed(chunks), extra, (handed(chunks) + extra) / n))
    enc.close()


def halves(path):
    """(host lines, device lines) the file holds, or the NOT TIMED YET text."""
    host, dev = ["== host ==", "NOT TIMED YET."], ["== device ==", "NOT TIMED YET.  The MD5 chain of a 2160p luma plane is 129 600 dependent blocks on one lane however many pictures are in the batch;",
                                                   "read from the code that is on the order of 0.1 s, against about 10 ms on a host core: an estimate, not a measurement."]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "report_time.txt"))
    a = ap.parse_args()
    host, dev = halves(a.out)
    if a.host:
        host = []
        host_section(host)
    if a.device:
        dev = []
        device_section(dev)
    lines = ["Picture report (csrc/picture_hash_core.h, csrc/report_kernel.hip).  Halves as tools/time_report.py writes them (--host, --device).", ""] + host + [""] + dev
    open(a.out, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))
