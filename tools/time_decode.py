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
A second leg times a stream with a QP per CU: one picture of the same size coded by the reference encoder with AdaptiveQP 1, MaxCuDQPDepth 2
(--cu-qp-stream FILE: such a stream made beforehand; otherwise oracle/_ref/TAppEncoder_ref makes it, and without either the leg is written as "not measured") -- parse on
the host and on the device with the QP map, and reconstruction and deblocking of the SAME records with the map (the QP-map instantiations) and without it (the constant-QP
kernels at the slice QP: another picture, the same work), then hevcdl_decode_stream with the switch on.
A third leg times the scaling-list instantiation: the batch stream above with its SPS rewritten on the spot to carry the lists of
tests/golden/sclist_file_rand.npz (tools/scaling_list_cover.py: with_scaling_lists -- test-side SPS syntax; the slice data is untouched, so the records and the work are
the same and the pictures are not the encoder's: every digest verdict is False, and is not asserted) -- hevcdl_decode_stream with hevcdl_enable_scaling_lists against the
constant-QP decode of the stream as it was, five calls each in alternation, and the reconstruction stage alone with and without the factors.
--keep-lines N keeps the last N lines of the file that is there (results another tool appended, e.g. a comparison against the parent commit; 8 keeps those of sections 5m and 5o).

    python tools/time_decode.py [--batch 8] [--width 3840 --height 2160] [--qp 32] [--cu-qp-stream FILE]
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


def note(text):
    """Progress on stderr: the table itself is printed at the end."""
    print("[time_decode] " + text, file=sys.stderr, flush=True)


def best(fn, runs=3):
    t = []
    for _ in range(runs):
        t0 = time.perf_counter()
        out = fn()
        t.append(time.perf_counter() - t0)
    return min(t) * 1000.0, out


def cu_qp_leg(hevcdl_amd, ref_tools, a, d):
    """The lines of the QP-map leg: a stream of one picture with cu_qp_delta_enabled_flag, its stages with and without the map."""
    w, h, qp = a.width, a.height, a.qp
    head = "QP per CU, %dx%d 8-bit QP %d, AdaptiveQP 1 MaxCuDQPDepth 2, 1 picture: " % (w, h, qp)
    if a.cu_qp_stream:
        stream = open(a.cu_qp_stream, "rb").read()
    elif os.path.exists(ref_tools.REF_ENC):
        yuv = ref_tools.synth_yuv(w, h, 1, seed=78)
        stream = ref_tools.run_reference(yuv, w, h, qp, ref_tools.make_labels(w, h, 1, "rand", seed=78), extra_args=["--AdaptiveQP=1", "--MaxQPAdaptationRange=6", "--MaxCuDQPDepth=2"])[2]
    else:
        return [head + "not measured (no stream given and no reference encoder to make one)"]
    t_parse, p = best(lambda: hevcdl_amd.parse_stream(stream, cu_qp=True))
    t_parse_dev, pd = best(lambda: hevcdl_amd.parse_stream(stream, cu_qp=True, engine="device"))
    assert pd.records.tobytes() == p.records.tobytes() and pd.qp_map.tobytes() == p.qp_map.tobytes() and p.qp_info.cu_qp_delta_enabled
    t_rec_map, recon = best(lambda: hevcdl_amd.reconstruct_frames(p.cfg, p.records, slices=p.slices, qp_map=p.qp_map, qp_info=p.qp_info, device=0))
    t_rec, _ = best(lambda: hevcdl_amd.reconstruct_frames(p.cfg, p.records, slices=p.slices, qps=p.qps, device=0))
    with hevcdl_amd.StreamDecoder(stream, batch=1) as dec:
        t_dbk_map, _ = best(lambda: dec.deblock_map(recon, p))
    e = hevcdl_amd.Encoder(w, h, p.qps[0], max_frames=1)
    t_dbk, _ = best(lambda: e.deblock_frames(recon, p.records))
    e.close()
    t_all, out = best(lambda: hevcdl_amd.decode_stream(stream, batch=1, cu_qp=True))
    t_dp, out_dp = best(lambda: hevcdl_amd.decode_stream(stream, batch=1, cu_qp=True, device_parse=True))
    assert all(v is True for v in out[3]) and all(v is True for v in out_dp[3]) and np.array_equal(out[0], out_dp[0])
    return [head + "measured",
            "  stream %8d bytes  QpY %d .. %d  parse with map %8.1f  parse (device) with map %8.1f" % (len(stream), p.qp_map[p.qp_map != 0].min(), p.qp_map.max(), t_parse, t_parse_dev),
            "  reconstruct with map %8.1f  without %8.1f   deblock with map %8.1f  without %8.1f   decode_stream %8.1f  with device parse %8.1f" % (t_rec_map, t_rec, t_dbk_map, t_dbk, t_all, t_dp)]


def scaling_list_leg(hevcdl_amd, stream, n):
    """The lines of the scaling-list leg: `stream` (n pictures, constant QP, this pipeline's) as it is and with scaling lists in its SPS."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import scaling_list_cover as slc
    lists = np.load(os.path.join(ROOT, "tests", "golden", "sclist_file_rand.npz"))
    sl_stream = slc.with_scaling_lists(stream, lists)
    lib = hevcdl_amd.load_library()
    p = hevcdl_amd.parse_stream(sl_stream, scaling_lists=True)
    assert p.scaling.enabled == 1 and p.records.tobytes() == hevcdl_amd.parse_stream(stream).records.tobytes()
    t_rec_sl, _ = best(lambda: hevcdl_amd.reconstruct_frames(p.cfg, p.records, slices=p.slices, qp_map=p.qp_map, qp_info=p.qp_info, scaling=p.scaling, device=0))
    t_rec_qp, _ = best(lambda: hevcdl_amd.reconstruct_frames(p.cfg, p.records, slices=p.slices, qp_map=p.qp_map, qp_info=p.qp_info, device=0))
    t_rec, _ = best(lambda: hevcdl_amd.reconstruct_frames(p.cfg, p.records, slices=p.slices, qps=p.qps, device=0))
    flat, with_lists = [], []
    for _ in range(5):
        c0 = lib.hevcdl_recon_sl_launches()
        flat.append(best(lambda: hevcdl_amd.decode_stream(stream, batch=n, scaling_lists=True), runs=1)[0])
        assert lib.hevcdl_recon_sl_launches() == c0
        with_lists.append(best(lambda: hevcdl_amd.decode_stream(sl_stream, batch=n, scaling_lists=True), runs=1)[0])
        assert lib.hevcdl_recon_sl_launches() == c0 + 1
    return ["scaling lists, the %d-picture stream above with the lists of sclist_file_rand in its SPS (rewritten on the spot; the same records): measured" % n,
            "  reconstruct with factors %8.1f  with the QP map alone %8.1f  constant QP %8.1f" % (t_rec_sl, t_rec_qp, t_rec),
            "  decode_stream, 5 calls each in alternation: constant-QP stream " + " ".join("%.1f" % t for t in flat) + "   (spread %.1f .. %.1f)" % (min(flat), max(flat)),
            "                                              with scaling lists " + " ".join("%.1f" % t for t in with_lists) + "   (spread %.1f .. %.1f)" % (min(with_lists), max(with_lists))]


def main():
    import hevcdl_amd
    from hevcdl_amd import pipeline
    import ref_tools
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--qp", type=int, default=32)
    ap.add_argument("--cu-qp-stream", default=None)
    ap.add_argument("--keep-lines", type=int, default=0)
    a = ap.parse_args()
    w, h, qp = a.width, a.height, a.qp
    lines = ["decoder times, %dx%d 8-bit QP %d, ms (best of 3; wall clock around synchronous calls)" % (w, h, qp)]
    with tempfile.TemporaryDirectory() as d:
        for n in (1, a.batch):
            note("%d picture(s): encode, then the stages" % n)
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
        note("scaling-list leg")
        sl_lines = scaling_list_leg(hevcdl_amd, stream, a.batch)
        note("QP-per-CU leg")
        lines += cu_qp_leg(hevcdl_amd, ref_tools, a, d)
        lines += sl_lines
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    lines.append("(tools/time_decode.py on one MI355X.  decode_stream is the Python entry hevcdl_amd.decode_stream: it creates and destroys a context per call, which is in its time; the\n"
                 "stage columns include their host <-> device copies.  One 2160p picture is a chain of 34 CTU rows two CTUs apart, so a single picture is bound by that chain's latency and a\n"
                 "batch amortises it.  A record, not a bound.)")
    path = os.path.join(ROOT, "profiles", "decode_time.txt")
    kept = open(path).read().splitlines()[-a.keep_lines:] if a.keep_lines > 0 and os.path.exists(path) else []
    with open(path, "w") as f:
        f.write("\n".join(lines + kept) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
