"""hevcdl_slice_decode_kernel on the MI355X (csrc/slice_decode_kernel.hip): hevcdl_parse_stream_dev against the parser byte for byte, batches against single launches,
whole decodes with hevcdl_enable_device_parse against the host-parse decode and the reference's pictures, and the error word on three damaged streams the shared source
has already survived on the CPU (tests/test_parse_core.py).  Every picture is a few CTUs."""
import ctypes
import glob
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLD
from test_decode import _join, _nals, streams_of
from test_parse_core import _parse, assert_same_parse, compare, ctu_named, damaged_three
from test_recon_gpu import STREAM_DECODES

pytestmark = pytest.mark.gpu

TIME_LIMIT = 60                                                           # seconds a test; each takes a second or two


@pytest.fixture(autouse=True)
def own_time_limit():
    """Every test here runs under its own time limit (test_recon_gpu.py): the watchdog ends the whole pytest process when a launch does not return -- nothing more is
    started on a device that a kernel has just hung."""
    import faulthandler
    faulthandler.dump_traceback_later(TIME_LIMIT, exit=True)
    yield
    faulthandler.cancel_dump_traceback_later()


def launches():
    import hevcdl_amd
    return hevcdl_amd.load_library().hevcdl_slice_decode_launches()


# partial CTUs, one row, one column; escape-coded levels, 10 bits; no transform-skip flags, no sign hiding; wavefront one CTU wide (every row initialises), two wide (the saved
# contexts come from a row's last CTU), 10 bits; tiles, uniform and not; row slices, one CTU wide, tile slices; wavefront and tile segments; a QP per picture; the filter off
PARSE_CASES = ["rd_e8x8_q32", "rd_e64x8_q20", "rd_e8x72_q40", "rd_e136_q0", "rd_e200_q51_b10", "rd_k200_q27_all0", "rd_w64_q32_r", "rd_w128_q22_r", "rd_w200_q30_b10", "rd_t512_q32_2x2",
               "rd_n832_q32_544x12", "slices_r128_a2", "slices_c64x192_a1", "slices_t512_a3", "segments_w64x192_a1", "segments_w264x136_a5", "segments_t512x128_s2_a1", "fqp_d192_q32",
               "dqr_c128_q32_n1", "lfoff_c192_q32"]


@pytest.mark.parametrize("name", PARSE_CASES)
def test_device_parse_equals_the_parser(name):
    """hevcdl_parse_stream_dev == hevcdl_parse_stream byte for byte on every stream of the fixture, and the launch counter moved."""
    f = np.load(os.path.join(GOLD, name + ".npz"))
    keys = [k for k, _ in streams_of(f)]
    assert keys
    for key in keys:
        before = launches()
        assert compare(f[key].tobytes(), (name, key), engine="device") == 0
        assert launches() > before


def access_units(stream):
    """-> (the NAL units in front of the first slice, [the NAL units of every picture: its slices and the suffix SEI behind them])"""
    head, aus = [], []
    for sc, n in _nals(stream):
        t = (n[0] >> 1) & 63
        if t < 32 and n[2] & 0x80:
            aus.append([])
        if not aus:
            head.append((sc, n))
        elif t < 32 or t == 40:
            aus[-1].append((sc, n))
    return head, aus


def forty(names):
    """Forty pictures out of the access units of the named streams, taken in turn so that neighbours differ in QP, behind the parameter sets of the first stream.
    -> (the stream of forty, forty streams of one picture)"""
    import hevcdl_amd
    heads, aus = zip(*(access_units(np.load(os.path.join(GOLD, n + ".npz"))["bitstream"].tobytes()) for n in names))
    pics = []
    for i in range(40):
        src = aus[i % len(aus)]
        pics.append(src[(i // len(aus)) % len(src)])
    whole = _join(list(heads[0]) + [n for p in pics for n in p])
    assert len(set(hevcdl_amd.parse_stream(whole, headers_only=True).qps)) > 1
    return whole, [_join(list(heads[0]) + p) for p in pics]


def one_size_family(pattern):
    """The streams of a family that can stand in one stream with the first of them: the same configuration but for the QP."""
    import hevcdl_amd

    def key(name):
        f = np.load(os.path.join(GOLD, name + ".npz"))
        if "bitstream" not in f.files:
            return None
        p = hevcdl_amd.parse_stream(f["bitstream"].tobytes(), headers_only=True)
        p.cfg.qp = p.cfg.rewrite_param_sets = 0
        return bytes(p.cfg), [(l.mode, l.argument) if l else None for l in (p.slices, p.segments)], [bytes(q.dbk) for q in p.pictures][:1]
    names = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLD, pattern)))
    return [n for n in names if key(n) is not None and key(n) == key(names[0])]


@pytest.mark.parametrize("which", ["fqp_*192_*.npz", "rd_c128_*.npz", "fqp_t512_q32.npz"], ids=["fqp192", "c128", "tiled"])
def test_forty_pictures_in_one_launch_equal_forty_single_launches(which):
    """Forty pictures whose neighbours differ in QP (the contexts are initialised per picture) -- the access units of the fqp_* streams of 192x128, of the rd_c128_* streams,
    of the 2x2-tiled fqp_t512_q32, where four units make a picture -- in one launch == the same pictures in forty launches == the parser."""
    import hevcdl_amd
    names = one_size_family(which)
    assert len(names) >= (1 if "t512" in which else 4), names
    whole, singles = forty(names)
    before = launches()
    batch = hevcdl_amd.parse_stream(whole, engine="device")
    assert launches() == before + 1 and len(batch.pictures) == 40
    assert_same_parse(hevcdl_amd.parse_stream(whole), batch, which)
    for i, s in enumerate(singles):
        one = hevcdl_amd.parse_stream(s, engine="device")
        assert one.records[0].tobytes() == batch.records[i].tobytes() and one.sao[0].tobytes() == batch.sao[i].tobytes() and one.qps == [batch.qps[i]], i
    assert launches() == before + 41


@pytest.mark.parametrize("name,key,pic_key", STREAM_DECODES, ids=["%s:%s" % (n, k) for n, k, _ in STREAM_DECODES])
def test_decode_with_device_parse_equals_the_host_parse_decode_and_the_reference(name, key, pic_key):
    """hevcdl_decode_stream with hevcdl_enable_device_parse on the nineteen streams test_recon_gpu.py decodes: pictures and verdicts are the host-parse decode's and the
    reference's picture file; the kernel ran; a changed SEI digest turns exactly its picture's verdict."""
    import hevcdl_amd
    f = np.load(os.path.join(GOLD, name + ".npz"))
    stream = f[key].tobytes()
    before = launches()
    pictures, cfg, info, verdicts = hevcdl_amd.decode_stream(stream, batch=2, device_parse=True)
    assert launches() >= before + (len(info) + 1) // 2
    host = hevcdl_amd.decode_stream(stream, batch=2)
    assert np.array_equal(pictures, host[0]) and verdicts == host[3] and [bytes(p) for p in info] == [bytes(p) for p in host[2]]
    assert all(v is True for v in verdicts if v is not None) and (pic_key is not None or all(v is True for v in verdicts))
    if pic_key is not None:
        assert np.array_equal(pictures, np.frombuffer(f[pic_key].tobytes(), pictures.dtype).reshape(len(info), -1))
    if verdicts[-1] is True:
        bad = bytearray(stream)
        bad[-3] ^= 0x55                                                   # inside the last picture's digest
        p2, _, _, v2 = hevcdl_amd.decode_stream(bytes(bad), batch=2, device_parse=True)
        assert v2 == verdicts[:-1] + [False] and np.array_equal(p2, pictures)


@pytest.mark.parametrize("name", ["rd_w200_q27_r2", "rd_x576_q30_2x3"], ids=["8bit", "10bit_tiles"])
def test_cli_device_parse_writes_the_reference_decoders_file(tmp_path, name):
    import hevcdl_amd
    f = np.load(os.path.join(GOLD, name + ".npz"))
    (tmp_path / "s.bin").write_bytes(f["bitstream"].tobytes())
    out = []
    for dp in ("1", "0"):
        r = subprocess.run([hevcdl_amd.build_decoder_app(), "-b", "s.bin", "-o", "rec%s.yuv" % dp, "--DeviceParse", dp], cwd=tmp_path, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stdout.count("(OK)") == f["records"].shape[0] and "ERROR" not in r.stdout, (r.stdout[-600:], r.stderr[-600:])
        out.append(r.stdout)
    assert out[0] == out[1]
    assert (tmp_path / "rec1.yuv").read_bytes() == f["recon_filtered"].tobytes() == (tmp_path / "rec0.yuv").read_bytes()


class Context:
    """A decoding context for a stream (hevcdl_config_from_stream), kept over several hevcdl_decode_stream calls."""

    def __init__(self, stream, batch):
        import hevcdl_amd
        self.lib = lib = hevcdl_amd.load_library()
        head = hevcdl_amd.parse_stream(stream, headers_only=True)
        self.head, cfg = head, hevcdl_amd.Config()
        assert lib.hevcdl_config_from_stream(ctypes.byref(head.cfg), hevcdl_amd._layout_ptr(head.slices), batch, 0, ctypes.byref(cfg)) == 0
        self.w = np.zeros(hevcdl_amd.WEIGHT_FLOATS, np.float32)
        self.h = ctypes.c_void_p()
        assert lib.hevcdl_create(ctypes.byref(cfg), self.w.ctypes.data, self.w.size, ctypes.byref(self.h)) == 0

    def decode(self, stream, n):
        """-> (status, sentence, pictures, verdicts)"""
        c = self.head.cfg
        buf = np.frombuffer(bytes(stream), np.uint8)
        pictures = np.zeros((n, c.width * c.height * 3 // 2), np.uint8 if c.bit_depth == 8 else np.dtype("<u2"))
        ok, count = np.zeros(n, np.int32), ctypes.c_int(0)
        st = self.lib.hevcdl_decode_stream(self.h, buf.ctypes.data, buf.size, pictures.ctypes.data, n, ctypes.byref(count), None, ok.ctypes.data)
        return st, (self.lib.hevcdl_last_error(self.h) or b"").decode(), pictures, list(ok)

    def close(self):
        self.lib.hevcdl_destroy(self.h)


def test_device_parse_turned_on_and_off_between_calls():
    """One context, rd_w200_q27_r2 (two pictures, batches of one): off, on, on, off, on -- the same pictures and verdicts every time, the kernel launched only while on, and
    a second on / off is no error."""
    stream = np.load(os.path.join(GOLD, "rd_w200_q27_r2.npz"))["bitstream"].tobytes()
    c = Context(stream, 1)
    try:
        first = None
        for on in (0, 1, 1, 0, 1):
            assert c.lib.hevcdl_enable_device_parse(c.h, on) == 0 and c.lib.hevcdl_enable_device_parse(c.h, on) == 0
            before = launches()
            st, why, pictures, verdicts = c.decode(stream, 2)
            assert st == 0 and verdicts == [1, 1], (on, st, why)
            assert launches() == before + (2 if on else 0)
            first = pictures if first is None else first
            assert np.array_equal(pictures, first)
    finally:
        c.close()


def test_the_kernel_reports_the_parsers_status_and_ctu_and_nothing_is_reconstructed():
    """Three damaged streams, no more: a sub-stream cut short, a flipped bit inside slice data, an entry point moved by one -- each through the sanitizer harness on the CPU
    already, each refused by the parser with HEVCDL_ERR_INVALID_ARG inside slice data.  hevcdl_parse_stream_dev and hevcdl_decode_stream with device parse answer the same
    status and CTU; hevcdl_recon_launches does not move; the next, undamaged call on the same context decodes correctly."""
    import hevcdl_amd
    lib = hevcdl_amd.load_library()
    sources = {"a sub-stream cut short": "slices_r128_a2", "a flipped bit inside slice data": "dbksel_inpps0_72x72_q32_dis", "an entry point moved by one": "rd_t512_q32_2x2"}
    cases = damaged_three()
    assert len(cases) == 3
    for what, damaged, ctu in cases:
        st, _, why = _parse(damaged, "device")
        assert st == 1 and ctu_named(why) == ctu, (what, why)
        good = np.load(os.path.join(GOLD, sources[what] + ".npz"))["bitstream"].tobytes()
        n = len(hevcdl_amd.parse_stream(good, headers_only=True).pictures)
        c = Context(good, n)
        try:
            assert lib.hevcdl_enable_device_parse(c.h, 1) == 0
            st, why, want, verdicts = c.decode(good, n)
            assert st == 0 and all(v == 1 for v in verdicts), (what, why)
            recon, parse = lib.hevcdl_recon_launches(), launches()
            st, why, _, _ = c.decode(damaged, n)
            assert st == 1 and ctu_named(why) == ctu and "picture 0" in why, (what, why)
            assert lib.hevcdl_recon_launches() == recon and launches() == parse + 1
            st, why, again, verdicts = c.decode(good, n)
            assert st == 0 and all(v == 1 for v in verdicts) and np.array_equal(again, want), (what, why)
        finally:
            c.close()
