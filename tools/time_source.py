"""Source format: the host's conversion functions against the device kernels (csrc/source_core.h, csrc/source_kernel.hip), as a record -> profiles/source_time.txt.

  --host     needs no GPU.  hevcdl_load_source_host / hevcdl_store_output_host on one 3840 x 2160 picture on one core (best of 3), 8 -> 8 and 8 -> 10 bits.
  --device   needs an MI355X.  HIP-event times of the load and the store launch for 1, 75 and 600 pictures of 3840 x 2160 already in HBM, 8 -> 8 and 8 -> 10 bits
             (second and third of three runs, the shorter), the bytes each launch moves and that as a fraction of the HBM peak (8.0 TB/s by the data sheet; a float4
             copy reaches about 6.3); and the bytes a picture pipeline call uploads per picture with and without a source format, 8 -> 10.
  --formats  needs an MI355X.  The file layouts: load from a 4:4:4 file at 8 -> 8 and 8 -> 10 bits, from a 4:2:2 and a 4:0:0 file at 8 -> 8, and the windowed store (offsets
             2, 0, 0, 2), for 75 and 600 pictures: ms, bytes read + written, the fraction of the HBM peak; and the upload bytes per picture and format.
  --compare PARENT_LIB   needs an MI355X.  The four 4:2:0 rows (8 -> 8 and 8 -> 10 bits, 75 and 600 pictures, load and store) by the parent commit's library and by this
             one, alternately, each run a process of its own that loads its library through HEVCDL_LIB: parent, parent, new, parent, new.  The parent's runs against each
             other give its own spread; the new rows are recorded next to it.  (--rows420 is the child's mode: it prints one JSON line.)
A section that is not run keeps what the file holds for it (or NOT TIMED YET / not measured)."""
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


def timed(fn):
    """HIP-event ms of fn() on the current stream: the shorter of the second and third of three runs."""
    import torch
    best = 1e9
    for rep in range(3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        torch.cuda.synchronize()
        if rep:
            best = min(best, a.elapsed_time(b))
    return best


def formats_section(out):
    import torch
    import hevcdl_amd
    out.append("== formats: %dx%d, no padding; HIP events on the launch stream, the shorter of the second and third run; bytes = read + written ==" % (W, H))
    stream = torch.cuda.current_stream().cuda_stream
    cs = W * H * 3 // 2
    rows = [("load from 4:4:4", 444, 8, 8), ("load from 4:4:4", 444, 8, 10), ("load from 4:2:2", 422, 8, 8), ("load from 4:0:0", 400, 8, 8)]
    for n in (75, 600):
        for name, cf, in_bd, bd in rows:
            fmt = hevcdl_amd.source_format(W, H, in_bd, in_bd, chroma_format=cf)
            enc = hevcdl_amd.Encoder(W, H, 32, max_frames=n, bit_depth=bd)
            enc.set_source_format(fmt)
            d_src = torch.randint(0, 256, (n, fmt.source_samples), dtype=torch.uint8, device="cuda")
            d_pic = torch.zeros((n, cs * (1 if bd == 8 else 2)), dtype=torch.uint8, device="cuda")
            ms = timed(lambda: enc.load_source_dev(d_src.data_ptr(), n, d_pic.data_ptr(), stream))
            # what the kernel touches: every second row of a vertically subsampled chroma plane, whole 32-sample reads of a horizontally subsampled one
            read = W * H + {444: 2 * W * (H // 2), 422: 2 * (W // 2) * (H // 2), 400: 0}[cf]
            moved = n * (read + cs * (1 if bd == 8 else 2))
            out.append("%s, %d -> %d bits, %3d pictures: %.3f ms, %.1f MB read + written, %.0f%% of 8.0 TB/s" % (name, in_bd, bd, n, ms, moved / 1e6, 100 * moved / (ms * 1e-3) / HBM_PEAK))
            del d_src, d_pic
            enc.close()
            torch.cuda.empty_cache()
        win = (2, 0, 0, 2)
        fmt = hevcdl_amd.source_format(W, H, 8, 8, conf_win=win)
        enc = hevcdl_amd.Encoder(W, H, 32, max_frames=n, bit_depth=8)
        enc.set_source_format(fmt)
        d_pic = torch.randint(0, 256, (n, cs), dtype=torch.uint8, device="cuda")
        d_out = torch.zeros((n, fmt.output_samples), dtype=torch.uint8, device="cuda")
        ms = timed(lambda: enc.store_output_dev(d_pic.data_ptr(), n, d_out.data_ptr(), stream))
        moved = 2 * n * fmt.output_samples
        out.append("windowed store (2, 0, 0, 2), 8 -> 8 bits, %3d pictures: %.3f ms, %.1f MB read + written, %.0f%% of 8.0 TB/s" % (n, ms, moved / 1e6, 100 * moved / (ms * 1e-3) / HBM_PEAK))
        del d_pic, d_out
        enc.close()
        torch.cuda.empty_cache()
    out.append("upload per picture of a picture pipeline call, 8-bit file: " + ", ".join("%s %d bytes" % (k, hevcdl_amd.source_format(W, H, 8, 8, chroma_format=c).source_samples)
                                                                                         for k, c in (("4:0:0", 400), ("4:2:0", 420), ("4:2:2", 422), ("4:4:4", 444))) + " (the coded picture is %d bytes at 8 bits)" % cs)


def rows420(old_abi):
    """The four 4:2:0 rows by whatever library HEVCDL_LIB names -> {row: ms}.  old_abi: the library is the parent commit's, whose hevcdl_source_format ends behind the two depths."""
    import torch
    import hevcdl_amd
    fs = W * H * 3 // 2
    stream = torch.cuda.current_stream().cuda_stream
    res = {}
    for in_bd, bd in PAIRS:
        cb = 1 if bd == 8 else 2
        for n in (75, 600):
            enc = hevcdl_amd.Encoder(W, H, 32, max_frames=n, bit_depth=bd)
            fmt = hevcdl_amd.source_format(W, H, in_bd, in_bd)
            if old_abi:
                fmt.struct_size = 20
            enc.set_source_format(fmt)
            d_src = torch.randint(0, 256, (n, fs), dtype=torch.uint8, device="cuda")
            d_pic = torch.zeros((n, fs * cb), dtype=torch.uint8, device="cuda")
            d_out = torch.zeros((n, fs), dtype=torch.uint8, device="cuda")
            res["%d -> %d bits, %3d pictures, load" % (in_bd, bd, n)] = timed(lambda: enc.load_source_dev(d_src.data_ptr(), n, d_pic.data_ptr(), stream))
            res["%d -> %d bits, %3d pictures, store" % (in_bd, bd, n)] = timed(lambda: enc.store_output_dev(d_pic.data_ptr(), n, d_out.data_ptr(), stream))
            assert torch.equal(d_out, d_src)
            del d_src, d_pic, d_out
            enc.close()
            torch.cuda.empty_cache()
    return res


def compare_section(out, parent_lib):
    """Alternates the two libraries, a process each (a library is chosen when the package is imported); a run that fails or runs out of its time ends the section."""
    new_lib = os.path.join(ROOT, "hevc-deep-learning-pipeline_amd", "lib", "libhevcdl_hip.so")
    runs = {"parent": [], "new": []}
    for who in ("parent", "parent", "new", "parent", "new"):
        cmd = [sys.executable, os.path.abspath(__file__), "--rows420"] + (["--old-abi"] if who == "parent" else [])
        r = subprocess.run(["timeout", "-k", "10", "240"] + cmd, env=dict(os.environ, HEVCDL_LIB=parent_lib if who == "parent" else new_lib), capture_output=True, text=True)
        if r.returncode != 0:
            out.append("== compare: the %s run ended with status %d; not measured ==" % (who, r.returncode))
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-2000:])
            return False
        runs[who].append(json.loads(r.stdout.strip().splitlines()[-1]))
    out.append("== compare: the 4:2:0 rows by the parent commit's library and by this one, alternately (parent, parent, new, parent, new), a process each; ms ==")
    inside = True
    for row in runs["parent"][0]:
        p, q = [x[row] for x in runs["parent"]], [x[row] for x in runs["new"]]
        ok = min(q) <= max(p)
        inside = inside and ok
        out.append("%s: parent %s (spread %.3f .. %.3f), new %s -> %s" % (row, " ".join("%.3f" % v for v in p), min(p), max(p), " ".join("%.3f" % v for v in q),
                                                                             "within the parent's spread" if min(p) <= min(q) <= max(p) else ("below the parent's spread" if ok else "ABOVE the parent's spread")))
    out.append("every new row %s" % ("lies within (or below) the spread of the parent's own runs" if inside else "does NOT lie within the parent's spread: see the rows marked ABOVE"))
    return True


def halves(path):
    host, dev = ["== host ==", "NOT TIMED YET."], ["== device ==", "NOT TIMED YET."]
    if os.path.exists(path):
        lines = open(path).read().splitlines()
        at_h = [i for i, ln in enumerate(lines) if ln.startswith("== host")]
        at_d = [i for i, ln in enumerate(lines) if ln.startswith("== device")]
        if at_h and at_d:
            end = min([i for i, ln in enumerate(lines) if ln.startswith("== formats") or ln.startswith("== compare")] + [len(lines)])
            host = [ln for ln in lines[at_h[0]:at_d[0]] if ln.strip()]
            dev = [ln for ln in lines[at_d[0]:end] if ln.strip()]
    return host, dev


def section(path, head, missing):
    """The lines of the section that starts with `head`, up to the next section."""
    if os.path.exists(path):
        lines = open(path).read().splitlines()
        at = [i for i, ln in enumerate(lines) if ln.startswith(head)]
        if at:
            nxt = [i for i, ln in enumerate(lines) if i > at[0] and ln.startswith("== ")]
            return [ln for ln in lines[at[0]:(nxt[0] if nxt else len(lines))] if ln.strip()]
    return [head + " ==", missing]


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--device", action="store_true")
    ap.add_argument("--formats", action="store_true")
    ap.add_argument("--compare", metavar="PARENT_LIB")
    ap.add_argument("--rows420", action="store_true")
    ap.add_argument("--old-abi", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "source_time.txt"))
    a = ap.parse_args()
    if a.rows420:
        print(json.dumps(rows420(a.old_abi)))
        sys.exit(0)
    host, dev = halves(a.out)
    fmts, comp = section(a.out, "== formats", "not measured"), section(a.out, "== compare", "not measured")
    if a.host:
        host = []
        host_section(host)
    if a.device:
        dev = []
        device_section(dev)
    if a.formats:
        fmts = []
        formats_section(fmts)
    if a.compare:
        comp = []
        compare_section(comp, os.path.abspath(a.compare))
    lines = ["Source format (csrc/source_core.h, csrc/source_kernel.hip).  Sections as tools/time_source.py writes them (--host, --device, --formats, --compare).", ""] + host + [""] + dev + [""] + fmts + [""] + comp
    open(a.out, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))
