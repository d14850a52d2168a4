"""Times of the decoder on one device, written to profiles/decode_time.txt: a record, not a bound.

One synthetic 2160p picture and a batch of them are encoded by this pipeline (so the run needs nothing but the repository), then decoded.  Measured, each as the best
of three runs with the device idle before and after (wall clock around a synchronous call, so a stage's time includes its host <-> device copies; the parser has none):
  parse           hevcdl_parse_stream on the host
  parse (device)  hevcdl_parse_stream_dev: headers on the host, the slice data by hevcdl_slice_decode_kernel (one wave a unit: a picture without tiles, slices or
                  wavefront rows is ONE unit), records and SAO blocks downloaded
  reconstruct     hevcdl_reconstruct_frames (hevcdl_recon_kernel)
  deblock         hevcdl_deblock_frames
  sao             hevcdl_sao_apply_frames
  decode_stream   hevcdl_decode_stream: everything, the pictures staying in HBM between the stages, digests by the report kernels; a second row with
                  hevcdl_enable_device_parse, where the records never leave HBM either
and, where oracle/_ref/TAppDecoder_ref is present, the reference decoder's wall time on the same stream.

    python tools/time_decode.py [--batch 8] [--width 3840 --height 2160] [--qp 32]
"""
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


def best(fn, runs=3):
    t = []
    for _ in range(runs):
        t0 = time.perf_counter()
        out = fn()
        t.append(time.perf_counter() - t0)
    return min(t) * 1000.0, out


def main():
    import hevcdl_amd
    from hevcdl_amd import pipeline
    import ref_tools
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--qp", type=int, default=32)
    a = ap.parse_args()
    w, h, qp = a.width, a.height, a.qp
    lines = ["decoder times, %dx%d 8-bit QP %d, ms (best of 3; wall clock around synchronous calls)" % (w, h, qp)]
    with tempfile.TemporaryDirectory() as d:
        for n in (1, a.batch):
            yuv = ref_tools.synth_yuv(w, h, n, seed=77)
            yuv.tofile(os.path.join(d, "in.yuv"))
            pipeline.encode_sequence(os.path.join(d, "in.yuv"), w, h, qp, n, bitstream_path=os.path.join(d, "s.bin"), hash_sei=True, log=lambda *x: None)
            stream = open(os.path.join(d, "s.bin"), "rb").read()
            t_parse, p = best(lambda: hevcdl_amd.parse_stream(stream))
            t_parse_dev, pd = best(lambda: hevcdl_amd.parse_stream(stream, engine="device"))
            assert pd.records.tobytes() == p.records.tobytes() and pd.sao.tobytes() == p.sao.tobytes()
            t_rec, recon = best(lambda: hevcdl_amd.reconstruct_frames(p.cfg, p.records, slices=p.slices, qps=p.qps, device=0))
            e = hevcdl_amd.Encoder(w, h, qp, max_frames=n)
            t_dbk, dbk = best(lambda: e.deblock_frames(recon, p.records))
            t_sao, _ = best(lambda: e.sao_apply_frames(dbk, p.sao))
            e.close()
            t_all, out = best(lambda: hevcdl_amd.decode_stream(stream, batch=n))
            assert all(v is True for v in out[3])
            lines.append("pictures %3d  stream %8d bytes  parse %8.1f  parse (device) %8.1f  reconstruct %8.1f  deblock %8.1f  sao %8.1f  decode_stream %8.1f  (%.1f a picture)" %
                         (n, len(stream), t_parse, t_parse_dev, t_rec, t_dbk, t_sao, t_all, t_all / n))
            t_dp, out_dp = best(lambda: hevcdl_amd.decode_stream(stream, batch=n, device_parse=True))
            assert all(v is True for v in out_dp[3]) and np.array_equal(out_dp[0], out[0])
            lines.append("pictures %3d  decode_stream with device parse %8.1f  (%.1f a picture)" % (n, t_dp, t_dp / n))
            ref = os.path.join(ROOT, "oracle", "_ref", "TAppDecoder_ref")
            if os.path.exists(ref):
                t0 = time.perf_counter()
                r = subprocess.run([ref, "-b", "s.bin", "-o", "ref.yuv"], cwd=d, capture_output=True, text=True)
                lines.append("pictures %3d  reference decoder %8.1f  (exit %d)" % (n, (time.perf_counter() - t0) * 1000.0, r.returncode))
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    lines.append("(tools/time_decode.py on one MI355X.  decode_stream is the Python entry hevcdl_amd.decode_stream: it creates and destroys a context per call, which is in its time; the\n"
                 "stage columns include their host <-> device copies.  One 2160p picture is a chain of 34 CTU rows two CTUs apart, so a single picture is bound by that chain's latency and a\n"
                 "batch amortises it.  A record, not a bound.)")
    with open(os.path.join(ROOT, "profiles", "decode_time.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
