"""Entropy coding: the host writer against the device kernels (csrc/entropy_kernel.hip), as a record -> profiles/entropy_time.txt.

  --host     needs no GPU.  The host writer (hevcdl_write_access_unit) per access unit on one core (mean of 10), and the tail of 75 and
             600 access units on 16 threads.  Records: the QP 32 golden fixture rd_c192_q32_r2 (a reference encode) tiled over 1920 x 1088 and 3840 x 2176 -- whole CTUs,
             so that every depth map stays valid; the levels are those of QP 32 content, which is what the time depends on.
  --device   needs an MI355X.  3840 x 2160 at QP 32, default cfg and WaveFrontSynchro 1, batches of 1 and 75 pictures and 600 pictures as 8 batches of 75 (the CLI's
             BatchFrames form): the three kernels from HIP events (Encoder.entropy_info with profile_enable: wavefront phase 1, coding, pack), the host writer on the same
             pictures' records (one core and 16 threads), the wall time of the pipeline calls, and the bytes that reach the callback per picture with and without
             want_records / want_pictures (counted from the arrays handed over, not computed).
  --cli N    tools/bench_cli.py N with and without --DeviceEntropy=1 (an MI355X).
  --against LIB [--rounds N]   needs no GPU.  How a change of the coder is accepted: hevcdl_write_access_unit of this tree's library and of LIB (the parent commit's
             build) in alternation, N rounds each (default 7), 3840 x 2176 with wavefront 0 and 1 on the --host records: per round the one-core time per access unit
             (mean of 5) and the tail of 600 access units on 16 threads; medians, and the other library's interquartile spread as the margin the machine supports.
Sections that were not run are written as NOT TIMED YET."""
import argparse
import os
import subprocess
import sys
import threading
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
THREADS = 16


def tail(write_one, n, threads=THREADS):
    """Wall time of n access units on a pool of `threads` (ctypes drops the GIL)."""
    with ThreadPoolExecutor(threads) as pool:
        t0 = time.perf_counter()
        list(pool.map(write_one, range(n)))
        return time.perf_counter() - t0


def host_section(out):
    import hevcdl_amd
    import entropy_cases as ec
    _, fx, _ = ec.fixture_case(os.path.join(ec.GOLD, "rd_c192_q32_r2.npz"))      # 192 x 128: 3 x 2 CTUs, two pictures
    out.append("== host: records of the QP 32 fixture rd_c192_q32_r2 tiled over the picture (whole CTUs); %d CPUs here ==" % (os.cpu_count() or 1))
    for w, h in ((1920, 1088), (3840, 2176)):
        cx, cy = w // 64, h // 64
        grid = np.arange(cx * cy).reshape(cy, cx)
        recs = fx[0][((grid // cx) % 2) * 3 + (grid % cx) % 3].reshape(1, -1)
        for wpp in (False, True):
            cfg = hevcdl_amd.stream_config(w, h, 32, wavefront=wpp)
            write_one = lambda i: hevcdl_amd.write_access_unit(w, h, 32, 0, recs[0], sao=None, wavefront=wpp)
            au = write_one(0)
            assert ec.assemble(cfg, hevcdl_amd.code_slice_data(cfg, recs)) == au
            t0 = time.perf_counter()
            for i in range(10):
                write_one(i)
            t1 = time.perf_counter()
            line = "%dx%d wavefront %d: access unit %d bytes; host writer on one core %.2f ms" % (w, h, wpp, len(au), 1e2 * (t1 - t0))
            for n in (75, 600):
                line += "; %d access units on %d threads %.3f s" % (n, THREADS, tail(write_one, n))
            out.append(line)


def quartiles(v):
    v = sorted(v)
    q = lambda p: v[int(round(p * (len(v) - 1)))]
    return q(0.5), q(0.75) - q(0.25)


def against_section(out, other, rounds):
    import ctypes
    import hevcdl_amd
    import entropy_cases as ec
    libs = (("base", ctypes.CDLL(other)), ("this", hevcdl_amd.load_library()))
    _, fx, _ = ec.fixture_case(os.path.join(ec.GOLD, "rd_c192_q32_r2.npz"))
    w, h = 3840, 2176
    cx, cy = w // 64, h // 64
    grid = np.arange(cx * cy).reshape(cy, cx)
    recs = np.ascontiguousarray(fx[0][((grid // cx) % 2) * 3 + (grid % cx) % 3].reshape(-1))
    cap = w * h * 3 + 4096
    out.append("== this library against base = %s: hevcdl_write_access_unit, %dx%d, records as in --host; %d rounds each in alternation; %d CPUs here ==" % (other, w, h, rounds, os.cpu_count() or 1))
    local = threading.local()
    for wpp in (0, 1):
        cfg = hevcdl_amd.stream_config(w, h, 32, wavefront=bool(wpp))

        def one(lib):
            if not hasattr(local, "buf"):
                local.buf = np.empty(cap, np.uint8)
            n = ctypes.c_size_t(0)
            st = lib.hevcdl_write_access_unit(ctypes.byref(cfg), 0, ctypes.c_void_p(recs.ctypes.data), None, ctypes.c_void_p(local.buf.ctypes.data), ctypes.c_size_t(cap), ctypes.byref(n))
            assert st == 0, st
            return local.buf[:n.value].tobytes()
        assert one(libs[0][1]) == one(libs[1][1]), "the two libraries write different access units"
        core, tails = {"base": [], "this": []}, {"base": [], "this": []}
        for _ in range(rounds):
            for name, lib in libs:
                t0 = time.perf_counter()
                for _ in range(5):
                    one(lib)
                core[name].append((time.perf_counter() - t0) / 5 * 1e3)
                tails[name].append(tail(lambda i: one(lib), 600))
        for what, unit, got in (("one core, per access unit", "ms", core), ("600 access units on %d threads" % THREADS, "s", tails)):
            (mb, iqr), (mt, _) = quartiles(got["base"]), quartiles(got["this"])
            for name in ("base", "this"):
                out.append("wavefront %d, %s, %s [%s]: %s" % (wpp, what, name, unit, " ".join("%.3f" % v for v in got[name])))
            out.append("wavefront %d, %s: median base %.3f, this %.3f (%+.1f %%); interquartile spread of base %.3f: %s" %
                       (wpp, what, mb, mt, 100 * (mt - mb) / mb, iqr, "within" if mt <= mb + iqr else "SLOWER THAN THE MARGIN"))


def device_section(out, batch):
    import hevcdl_amd
    import ref_tools
    w, h = 3840, 2160
    out.append("== device: %dx%d, QP 32; kernel times from HIP events, summed over the batches ==" % (w, h))
    base = ref_tools.synth_yuv(w, h, 1, seed=2)
    for wpp in (False, True):
        enc = hevcdl_amd.Encoder(w, h, 32, max_frames=batch, wavefront=wpp)
        enc.encode_pictures_chunked(base)                                      # warm-up: workspaces, code objects
        c = enc.encode_pictures_chunked(base)[0]
        rec1, sao1 = c[1][0], c[3][0]
        old_bytes = c[1].nbytes + c[2].nbytes + c[3].nbytes + c[4].nbytes
        write_one = lambda i: hevcdl_amd.write_access_unit(w, h, 32, i, rec1, sao=sao1, wavefront=wpp)
        write_one(0)
        t0 = time.perf_counter(); au = write_one(0); t_one = time.perf_counter() - t0
        enc.enable_device_entropy(True)
        enc.profile_enable(True)
        copied = []
        for wp, wr in ((False, False), (True, False), (False, True), (True, True)):
            s = enc.encode_pictures_stream(base, want_pictures=wp, want_records=wr)[0]
            copied.append(sum(len(d) for d in s[1]) + s[2].nbytes + s[3].nbytes + (s[4].nbytes if s[4] is not None else 0) + (s[5].nbytes if s[5] is not None else 0))
        out.append("wavefront %d: access unit %d bytes, host writer %.2f ms on one core; bytes handed to the callback per picture: old callback %d; stream callback %d, "
                   "with pictures %d, with records %d, with both %d" % (wpp, len(au), 1e3 * t_one, old_bytes, copied[0], copied[1], copied[2], copied[3]))
        for n, reps in ((1, 1), (batch, 1), (batch, 600 // batch)):
            yuv = np.tile(base, (n, 1))
            enc.enable_device_entropy(False)
            t0 = time.perf_counter()
            for _ in range(reps):
                enc.encode_pictures_chunked(yuv)
            t_old = time.perf_counter() - t0
            t_tail = tail(write_one, n * reps)
            enc.enable_device_entropy(True)
            ms = [0.0, 0.0, 0.0]
            t0 = time.perf_counter()
            for _ in range(reps):
                enc.encode_pictures_stream(yuv)
                ms = [a + b for a, b in zip(ms, enc.entropy_info()[1])]
            t_new = time.perf_counter() - t0
            out.append("wavefront %d, %d pictures (%d x %d): kernels: phase 1 %.2f ms, coding %.2f ms, pack %.2f ms; host writer on %d threads %.3f s (one core: %.3f s by the single "
                       "figure); pipeline + old callback %.3f s (the host writer comes on top), pipeline with device entropy + stream callback %.3f s"
                       % (wpp, n * reps, reps, n, ms[0], ms[1], ms[2], THREADS, t_tail, t_one * n * reps, t_old, t_new))
        enc.close()


def cli_section(out, n):
    out.append("== CLI: tools/bench_cli.py %d, without and with --DeviceEntropy=1 ==" % n)
    for extra in ([], ["--DeviceEntropy=1"]):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "bench_cli.py"), str(n)] + extra, capture_output=True, text=True)
        out += [ln for ln in r.stdout.splitlines() if ln.startswith("cli")] or ["bench_cli.py failed: " + r.stderr.strip()[-300:]]


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--device", action="store_true")
    ap.add_argument("--cli", type=int, default=0)
    ap.add_argument("--batch", type=int, default=75)
    ap.add_argument("--against", default=None, metavar="LIB")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "entropy_time.txt"))
    a = ap.parse_args()
    lines = ["Entropy coding (csrc/entropy_coder.h, csrc/entropy_kernel.hip).  Sections as tools/time_entropy.py prints them (--host, --device, --cli).", ""]
    if a.host:
        host_section(lines)
    else:
        lines.append("== host ==\nNOT TIMED YET.")
    lines.append("")
    if a.against:
        against_section(lines, os.path.abspath(a.against), a.rounds)
        lines.append("")
    if a.device:
        device_section(lines, a.batch)
    else:
        lines.append("== device ==\nNOT TIMED YET.  No figure exists for the two entropy kernels and the pack kernel, for the bytes handed over per picture with and without\n"
                     "want_records / want_pictures, or for the pipeline with and without the switch.  The default cfg is one serial chain of ~2040 CTUs per 2160p frame on one\n"
                     "wave: it may well be slower than 16 host threads, which is why the feature is opt-in.")
    lines.append("")
    if a.cli:
        cli_section(lines, a.cli)
    else:
        lines.append("== CLI ==\nNOT TIMED YET.")
    open(a.out, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))
