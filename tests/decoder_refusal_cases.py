"""What the decoder's host code answers, group by group, as lines of `case,status,sentence` and a sha256 over them: the behaviour tests/golden/decoder_refusals.json pins.
tools/record_decoder_refusals.py writes that file with the library of another tree (the parent commit's); tests/test_decoder_refusals.py recomputes the groups with the
tree under test.  Everything here runs on the host: no case reaches a device call.  `hv` is the hevcdl_amd module whose library answers."""
import ctypes
import hashlib
import os

import numpy as np

import entropy_cases as ec
from conftest import GOLD
from test_decode import FLIP_STREAMS, REFUSALS, _flip, _join, _nals, _pps_positions, _sps_positions
from test_parse_core import TRUNCATED

ENGINES = ("host", "core")
ACCEPT_FIXTURES = (("cuqp_aq_d2", "stream_nolf"), ("sclist_file_rand", "stream_nolf"))
FORMS = ("", "_qp", "_sl")


def digest(lines):
    return {"count": len(lines), "sha256": hashlib.sha256("\n".join(lines).encode()).hexdigest()}


def load(name, key):
    return np.load(os.path.join(GOLD, name + ".npz"))[key].tobytes()


def answer(hv, stream, engine, **kw):
    """-> "status,sentence" of parse_stream (the sentence with the entry point's name in front, as HevcdlError carries it)"""
    try:
        hv.parse_stream(stream, engine=engine, **kw)
        return "0,"
    except hv.HevcdlError as e:
        return "%d,%s" % (e.status, e)


def flips(hv, name, key, engine):
    data, lines = bytearray(load(name, key)), []
    for bit in range(len(data) * 8):
        data[bit >> 3] ^= 0x80 >> (bit & 7)
        lines.append("%d,%s" % (bit, answer(hv, bytes(data), engine)))
        data[bit >> 3] ^= 0x80 >> (bit & 7)
    return lines


def truncated(hv, name, key, engine):
    """test_parse_core.py's cuts: in front of every NAL unit, and every slice NAL unit one byte short and in its middle"""
    nals, lines = _nals(load(name, key)), []
    for k in range(1, len(nals)):
        lines.append("nal %d,%s" % (k, answer(hv, _join(nals[:k]), engine)))
        if (nals[k][1][0] >> 1) & 63 < 32:
            for cut in (len(nals[k][1]) - 1, len(nals[k][1]) // 2):
                lines.append("nal %d cut %d,%s" % (k, cut, answer(hv, _join(nals[:k]) + b"\0\0\1" + nals[k][1][:cut], engine)))
    return lines


def refused_features(hv, engine):
    """test_decode.py's REFUSALS: one bit of a parameter set or of the first slice header of rd_e64x8_q20 turned"""
    stream, lines = load("rd_e64x8_q20", "bitstream"), []
    for field, nal_type, bit, _ in REFUSALS:
        nals = _nals(stream)
        k = next(i for i, (_, n) in enumerate(nals) if (n[0] >> 1) & 63 == nal_type)
        at = 0 if nal_type == 19 else (_sps_positions if nal_type == 33 else _pps_positions)(nals[k][1])[field]
        nals[k] = (nals[k][0], _flip(nals[k][1], at + bit))
        lines.append("%s,%s" % (field, answer(hv, _join(nals), engine)))
    return lines


def raw_parse(hv, stream, form, engine, accept, shape=None):
    """One call of hevcdl_parse_stream<_core><form> with room for everything the stream holds -> "status,sentence,sha256 of what it gave" (the last only behind status 0).
    The plain form has no `accept`; the forms are called as include/hevcdl.h declares them, not through parse_stream, so that every form meets every `accept`.
    shape: (pictures, width, height) of a stream whose headers do not parse to the end."""
    lib = hv.load_library()
    if shape is None:
        head = hv.parse_stream(stream, headers_only=True, cu_qp=True, scaling_lists=True)
        shape = len(head.pictures), head.cfg.width, head.cfg.height
    n, ctus = shape[0], ((shape[1] + 63) // 64) * ((shape[2] + 63) // 64)
    buf = np.frombuffer(stream, np.uint8)
    cfg = hv.StreamConfig()
    cfg.struct_size = ctypes.sizeof(hv.StreamConfig)
    sl, sg, count, info, sc = hv.SliceLayout(), hv.SegmentLayout(), ctypes.c_int(0), hv.QpInfo(), hv.ScalingInfo()
    pics, recs, sao, qp_map = (hv.ParsedPicture * n)(), np.zeros((n, ctus), hv.REC_DTYPE), np.zeros((n, ctus, 3), hv.SAO_DTYPE), np.zeros((n, ctus, 256), np.int8)
    tail = {"": (), "_qp": (ctypes.byref(info), qp_map.ctypes.data), "_sl": (ctypes.byref(info), qp_map.ctypes.data, ctypes.byref(sc))}[form]
    fn = getattr(lib, "hevcdl_parse_stream" + ("_core" if engine == "core" else "") + form)
    st = fn(buf.ctypes.data, buf.size, *(() if form == "" else (accept,)), ctypes.byref(cfg), ctypes.byref(sl), ctypes.byref(sg), pics, n, ctypes.byref(count),
            recs.ctypes.data, sao.ctypes.data, n * ctus, *tail)
    if st != 0:
        return "%d,%s," % (st, lib.hevcdl_parse_error().decode())
    h = hashlib.sha256()
    for part in (bytes(cfg), bytes(sl), bytes(sg), bytes(pics), recs.tobytes(), sao.tobytes(), bytes(info), qp_map.tobytes(), bytes(sc) if form == "_sl" else b""):
        h.update(part)
    return "0,,%d pictures %s" % (count.value, h.hexdigest())


def accepted(hv, name, key, engine):
    stream = load(name, key)
    return ["%s accept %d,%s" % (form or "plain", accept, raw_parse(hv, stream, form, engine, accept)) for form in FORMS for accept in ((0,) if form == "" else (0, 1, 3))]


def order_streams(hv):
    """Two pictures of stream_c192_q32: picture 0 with a bit of its slice data turned (the first bit, from the middle of the NAL unit on, that the parser answers with a
    CTU), picture 1 with slice_type turned.  -> (both, the second damage alone)"""
    nals = _nals(load("stream_c192_q32", "bitstream_ps0"))
    slices = [i for i, (_, n) in enumerate(nals) if (n[0] >> 1) & 63 < 32]
    a, b = slices[0], slices[1]
    header = nals[:b] + [(nals[b][0], _flip(nals[b][1], 3))] + nals[b + 1:]
    for bit in range(4 * (len(nals[a][1]) - 2), 8 * (len(nals[a][1]) - 2)):
        both = header[:a] + [(nals[a][0], _flip(nals[a][1], bit))] + header[a + 1:]
        if "CTU" in answer(hv, _join(both[:b]), "host"):
            return _join(both), _join(header)
    raise AssertionError("no bit of the slice data gave an error with a CTU")


def refusal_order(hv, engine):
    """The entry points themselves, with room for the slice data: parse_stream asks for the headers alone first and would never get to picture 0's slice data."""
    both, header = order_streams(hv)
    return ["%s %s,%s" % (what, form or "plain", raw_parse(hv, stream, form, engine, 3, shape=(3, 192, 128))) for form in FORMS
            for what, stream in (("header of picture 1", header), ("slice data of picture 0 and header of picture 1", both))]


def recon_calls(hv):
    """Calls of the reconstruction's entry points that are refused before any device call -> lines.  The *_dev forms ask for the device right behind their first check, so only
    that check is here for them; the host forms and the host-buffer forms share everything up to hevcdl_validate_records."""
    lib = hv.load_library()
    cfg = hv.stream_config(128, 128, 30)
    recs = np.stack([ec.synth_records(np.random.default_rng(11), 128, 128) for _ in range(2)])
    out = np.zeros((2, 128 * 128 * 3 // 2), np.uint16)
    qmap = np.full((2, 4, 256), 30, np.int8)
    info, sc = hv.QpInfo(1, 0, 2, -2), hv.scaling_info(np.full(hv.SCALING_FACTOR_BYTES, 16))
    qps = np.array([30, 31], np.int32)
    zero = np.full(hv.SCALING_FACTOR_BYTES, 16)
    zero[1000] = 0
    lines = []

    def call(what, form, kind, c=cfg, n=2, q=qps.ctypes.data, i=info, m=qmap.ctypes.data, s=sc, slices=None):
        ref = lambda x: None if x is None else ctypes.byref(x)
        quant = {"": (q,), "_qp": (ref(i), m), "_sl": (ref(i), m, ref(s))}[form]
        sl = None if slices is None else ctypes.byref(slices)
        if kind == "host":
            st = getattr(lib, "hevcdl_reconstruct_frames%s_host" % form)(ref(c), sl, *quant, recs.ctypes.data, n, out.ctypes.data)
        elif kind == "buffers":
            st = getattr(lib, "hevcdl_reconstruct_frames" + form)(0, ref(c), sl, *quant, recs.ctypes.data, n, out.ctypes.data)
        else:      # the device form: the pointers are never read by a call that is refused at its first check
            st = getattr(lib, "hevcdl_reconstruct_frames%s_dev" % form)(0, ref(c), sl, *quant, None, n, None, None)
        lines.append("%s %s%s,%d,%s" % (what, kind, form, st, lib.hevcdl_parse_error().decode() if st else ""))

    def changed(**kw):
        c = hv.stream_config(128, 128, 30)
        for k, v in kw.items():
            setattr(c, k, v)
        return c
    for form in FORMS:
        call("null cfg", form, "dev", c=None)
        call("n_frames -1", form, "dev", n=-1)
        call("n_frames 0", form, "dev", n=0)
        for kind in ("host", "buffers"):
            call("null cfg", form, kind, c=None)
            call("struct_size", form, kind, c=changed(struct_size=8))
            call("width 12", form, kind, c=changed(width=12))
            call("bit depth 9", form, kind, c=changed(bit_depth=9))
            call("SliceMode 2", form, kind, slices=hv.SliceLayout(2, 1, 1))
            call("n_frames -1", form, kind, n=-1)
    for kind in ("host", "buffers"):
        call("QP 52 of picture 1", "", kind, q=np.array([30, 52], np.int32).ctypes.data)
        for form in ("_qp", "_sl"):
            call("null map", form, kind, m=None)
            call("null qp_info", form, kind, i=None)
            call("chroma offset 13", form, kind, i=hv.QpInfo(1, 0, 13, 0))
        call("scaling factor 0", "_sl", kind, s=hv.scaling_info(zero))
        call("null scaling", "_sl", kind, s=None)
    call("scaling factor 0", "_sl", "dev", s=hv.scaling_info(zero))
    call("null scaling", "_sl", "dev", s=None)
    return lines


def no_such_device(hv):
    """Device 99 through the three stand-alone device forms and the three host-buffer forms: refused where they ask for the device, in front of every allocation.  (Kept out of
    groups(): it is the one case here that calls the HIP runtime.)"""
    lib = hv.load_library()
    cfg, info, sc = hv.stream_config(128, 128, 30), hv.QpInfo(1, 0, 2, -2), hv.scaling_info(np.full(hv.SCALING_FACTOR_BYTES, 16))
    recs = np.stack([ec.synth_records(np.random.default_rng(11), 128, 128) for _ in range(2)])
    out, qmap, qps = np.zeros((2, 128 * 128 * 3 // 2), np.uint8), np.full((2, 4, 256), 30, np.int8), np.array([30, 31], np.int32)
    lines = []
    for form, quant in (("", (qps.ctypes.data,)), ("_qp", (ctypes.byref(info), qmap.ctypes.data)), ("_sl", (ctypes.byref(info), qmap.ctypes.data, ctypes.byref(sc)))):
        st = getattr(lib, "hevcdl_reconstruct_frames%s_dev" % form)(99, ctypes.byref(cfg), None, *quant, None, 2, None, None)
        lines.append("dev%s,%d,%s" % (form, st, lib.hevcdl_parse_error().decode()))
        st = getattr(lib, "hevcdl_reconstruct_frames" + form)(99, ctypes.byref(cfg), None, *quant, recs.ctypes.data, 2, out.ctypes.data)
        lines.append("buffers%s,%d,%s" % (form, st, lib.hevcdl_parse_error().decode()))
    return lines


def groups(hv, only=None):
    """-> {group name: the lines}; `only`: a predicate over the names (the flips take a minute)"""
    todo = {}
    for engine in ENGINES:
        for name, key in FLIP_STREAMS:
            todo["flips %s %s" % (name, engine)] = lambda n=name, k=key, e=engine: flips(hv, n, k, e)
        for name, key in TRUNCATED:
            todo["truncated %s %s" % (name, engine)] = lambda n=name, k=key, e=engine: truncated(hv, n, k, e)
        todo["refused features %s" % engine] = lambda e=engine: refused_features(hv, e)
        for name, key in ACCEPT_FIXTURES:
            todo["accept %s %s" % (name, engine)] = lambda n=name, k=key, e=engine: accepted(hv, n, k, e)
        todo["refusal order %s" % engine] = lambda e=engine: refusal_order(hv, e)
    todo["reconstruction calls"] = lambda: recon_calls(hv)
    return {name: fn() for name, fn in todo.items() if only is None or only(name)}
