"""The C ABI's argument contract (include/hevcdl.h, csrc/hevcdl_api.hip): the status every entry that takes a context or a device returns for a null context, a null
required pointer, frame counts outside 0 .. max_frames, a bad method, a range outside the last batch, a switch that was not called, an output inside its input and a
misaligned pointer -- and the message hevcdl_last_error holds afterwards (None: still empty).  Every row runs on a context of its own (64x64, max_frames 2).
Then the four switches of the picture pipeline through on -> off -> on -> off."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

OK, INVALID, UNSUPPORTED, NO_DEVICE = 0, 1, 2, 3
W, H, MAXF = 64, 64, 2
FB = W * H * 3 // 2
RANGE = "n_frames out of range (cfg.max_frames)"
NULLDEV, NULLPTR = "null device pointer", "null pointer"
METHOD = "method must be 0 (none), 1 (MD5), 2 (CRC) or 3 (checksum)"
SRC_OFF = "hevcdl_set_source_format was not called"
SRC_PTR = "source format: null or misaligned device pointer"


class Env:
    """What a row's arguments are made of: the context h, device memory D(i) (slots of 64 KB in one allocation), host memory Hm(i), a stream configuration."""

    def __init__(self, lib, h, dev_base, host):
        self.lib, self.h, self.dev_base, self.host = lib, h, dev_base, host

    def D(self, i, plus=0):
        return self.dev_base + 65536 * i + plus

    def Hm(self, i):
        return self.host.ctypes.data + 65536 * i


@pytest.fixture(scope="module")
def world():
    import torch
    import hevcdl_amd
    lib = ctypes.CDLL(hevcdl_amd.LIB_PATH)      # a handle of this module's own: its calls pass raw integers, whatever argtypes the package has set on its handle
    for name in hevcdl_amd.EXPORTS:
        getattr(lib, name).restype = ctypes.c_int
        getattr(lib, name).argtypes = None
    lib.hevcdl_last_error.restype = ctypes.c_char_p
    lib.hevcdl_last_rd_launch.restype = ctypes.c_char_p
    lib.hevcdl_destroy.restype = None
    dev = torch.zeros(16 * 65536, dtype=torch.uint8, device="cuda:0")
    host = np.zeros(16 * 65536, np.uint8)
    return lib, hevcdl_amd, dev, host, hevcdl_amd.load_weights()


def make_ctx(world, width=W, height=H, tiles=(1, 1)):
    lib, hevcdl_amd, dev, host, weights = world
    cfg = hevcdl_amd.default_config(width, height, 32, max_frames=MAXF, tiles=tiles)
    h = ctypes.c_void_p()
    assert lib.hevcdl_create(ctypes.byref(cfg), ctypes.c_void_p(weights.ctypes.data), ctypes.c_size_t(weights.size), ctypes.byref(h)) == OK
    return Env(lib, h, dev.data_ptr(), host)


def P(v):
    return ctypes.c_void_p(v)


# ---- set-ups a row may ask for -------------------------------------------------------------------------------------------------------------------------------
def quality_on(e, m):
    assert e.lib.hevcdl_enable_quality(e.h, 1) == OK


def report_on(e, m):
    assert e.lib.hevcdl_enable_picture_report(e.h, 1, 1) == OK


def entropy_on(e, m):
    assert e.lib.hevcdl_enable_device_entropy(e.h, 1) == OK


def source_on(e, m):      # 10-bit source of the context's size: the source's samples are two bytes, the coded picture's one
    fmt = m.source_format(W, H, 10, 8)
    assert e.lib.hevcdl_set_source_format(e.h, ctypes.byref(fmt)) == OK


def frame_entries(name, ptrs, tail=(), null_msg=NULLDEV, first=()):
    """The rows every entry of the shape (ctx, pointers..., n_frames somewhere, ...) shares.  ptrs: the pointer arguments as ("D" | "H", required) in order, with "N" for
    where n_frames goes; tail: constant trailing arguments."""
    def args(e, n, null_at=None, ctx=True):
        a, slot = [e.h if ctx else P(None)] + list(first), 0
        for i, p in enumerate(ptrs):
            if p == "N":
                a.append(n)
                continue
            kind, _req = p
            a.append(P(None) if i == null_at else P(e.D(slot) if kind == "D" else e.Hm(slot)))
            slot += 1
        return a + list(tail)
    rows = [(name + "/null-ctx", name, lambda e: args(e, 1, ctx=False), INVALID, "no-ctx"),
            (name + "/n=-1", name, lambda e: args(e, -1), INVALID, RANGE),
            (name + "/n=max+1", name, lambda e: args(e, MAXF + 1), INVALID, RANGE),
            (name + "/n=0", name, lambda e: args(e, 0), OK, None)]
    for i, p in enumerate(ptrs):
        if p != "N" and p[1]:
            rows.append(("%s/null-arg%d" % (name, i), name, lambda e, i=i: args(e, 1, null_at=i), INVALID, null_msg))
    return rows


D, Dopt, Hp, Hopt, N = ("D", True), ("D", False), ("H", True), ("H", False), "N"
ROWS = []
ROWS += frame_entries("hevcdl_clamp_labels_dev", [D, N], tail=(P(None),))
ROWS += frame_entries("hevcdl_predict_depth_dev", [D, N, D, Dopt], tail=(P(None),))
ROWS += frame_entries("hevcdl_compress_frames_dev", [D, N, D, D, D, Dopt], tail=(P(None),))
ROWS += frame_entries("hevcdl_compress_tiles_dev", [D, N, D, D, D, Dopt], tail=(0, 1, P(None)))
ROWS += frame_entries("hevcdl_encode_frames_dev", [D, N, D, D, D, Dopt], tail=(P(None),))
ROWS += frame_entries("hevcdl_predict_depth", [Hp, N, Hp, Hopt], null_msg=NULLPTR)
ROWS += frame_entries("hevcdl_compress_frames", [Hp, N, Hopt, Hp, Hopt, Hopt], null_msg=NULLPTR)
ROWS += frame_entries("hevcdl_deblock_frames_dev", [D, N, D, D], tail=(P(None),))
ROWS += frame_entries("hevcdl_deblock_frames", [Hp, N, Hp, Hp], null_msg=NULLPTR)
ROWS += frame_entries("hevcdl_sao_frames_dev", [D, D, N, D, D], tail=(P(None),))
ROWS += frame_entries("hevcdl_sao_frames", [Hp, Hp, N, Hp, Hp], null_msg=NULLPTR)
ROWS += frame_entries("hevcdl_picture_quality_dev", [D, D, N, D], tail=(P(None),))
ROWS += frame_entries("hevcdl_picture_quality", [Hp, Hp, N, Hp], null_msg=NULLPTR)
ROWS += frame_entries("hevcdl_picture_report", [Hopt, Hp, N], tail=(1, P(0)), null_msg=NULLPTR)[:3]      # (its out pointer follows the method: rows below)
ROWS += frame_entries("hevcdl_encode_pictures", [Hp, N, Hopt], tail=(1, P(0), P(0), P(None), P(None)), null_msg=NULLPTR)[:3]
ROWS += frame_entries("hevcdl_begin_frames", [Hp, N, Hopt, Hopt])[:3]
ROWS += [
    # ---- entries without a frame count, or with rules of their own ----
    ("last_error/null-ctx", "hevcdl_last_error", lambda e: [P(None)], b"null ctx", "no-ctx"),
    ("last_rd_launch/null-ctx", "hevcdl_last_rd_launch", lambda e: [P(None)], b"", "no-ctx"),
    ("last_rd_launch/fresh", "hevcdl_last_rd_launch", lambda e: [e.h], b"", None),
    ("reserve_workspace/null-ctx", "hevcdl_reserve_workspace", lambda e: [P(None)], INVALID, "no-ctx"),
    ("device_memory/null", "hevcdl_device_memory", lambda e: [0, P(None), P(e.Hm(0))], INVALID, "no-ctx"),
    ("device_memory/device=-1", "hevcdl_device_memory", lambda e: [-1, P(e.Hm(14)), P(e.Hm(15))], NO_DEVICE, "no-ctx"),
    ("device_memory/device=4096", "hevcdl_device_memory", lambda e: [4096, P(e.Hm(14)), P(e.Hm(15))], NO_DEVICE, "no-ctx"),
    ("device_memory/ok", "hevcdl_device_memory", lambda e: [0, P(e.Hm(14)), P(e.Hm(15))], OK, "no-ctx"),
    ("compress_tiles_dev/range", "hevcdl_compress_tiles_dev", lambda e: [e.h, P(e.D(0)), 1, P(e.D(1)), P(e.D(2)), P(e.D(3)), P(None), 0, 2, P(None)], INVALID, "tile range outside the tile grid"),
    ("compress_tiles_dev/begin=-1", "hevcdl_compress_tiles_dev", lambda e: [e.h, P(e.D(0)), 1, P(e.D(1)), P(e.D(2)), P(e.D(3)), P(None), -1, 1, P(None)], INVALID, "tile range outside the tile grid"),
    ("compress_tiles_dev/count=0", "hevcdl_compress_tiles_dev", lambda e: [e.h, P(None), 1, P(None), P(None), P(None), P(None), 0, 0, P(None)], OK, None),
    ("predict_depth_planes/null-ctx", "hevcdl_predict_depth_planes", lambda e: [P(None), P(e.Hm(0)), 1, P(e.Hm(1)), P(None)], INVALID, "no-ctx"),
    ("predict_depth_planes/n=-1", "hevcdl_predict_depth_planes", lambda e: [e.h, P(e.Hm(0)), -1, P(e.Hm(1)), P(None)], INVALID, RANGE),
    ("predict_depth_planes/n=0", "hevcdl_predict_depth_planes", lambda e: [e.h, P(None), 0, P(None), P(None)], OK, None),
    ("predict_depth_planes/null-labels", "hevcdl_predict_depth_planes", lambda e: [e.h, P(e.Hm(0)), 1, P(None), P(None)], INVALID, NULLPTR),
    ("predict_depth_planes/null-planes", "hevcdl_predict_depth_planes", lambda e: [e.h, P(None), 1, P(e.Hm(1)), P(None)], INVALID, "null plane pointer"),
    ("compress_frames_planes/null-ctx", "hevcdl_compress_frames_planes", lambda e: [P(None), P(e.Hm(0)), 1, P(None), P(e.Hm(1)), P(None), P(None)], INVALID, "no-ctx"),
    ("compress_frames_planes/n=max+1", "hevcdl_compress_frames_planes", lambda e: [e.h, P(e.Hm(0)), MAXF + 1, P(None), P(e.Hm(1)), P(None), P(None)], INVALID, RANGE),
    ("compress_frames_planes/null-records", "hevcdl_compress_frames_planes", lambda e: [e.h, P(e.Hm(0)), 1, P(None), P(None), P(None), P(None)], INVALID, NULLPTR),
    ("compress_frames_planes/null-planes", "hevcdl_compress_frames_planes", lambda e: [e.h, P(e.Hm(13)), 1, P(None), P(e.Hm(1)), P(None), P(None)], INVALID, "null plane pointer"),      # (host slot 13 is never written: three null planes)
    ("predict_depth_rgb/null-ctx", "hevcdl_predict_depth_rgb", lambda e: [P(None), P(e.Hm(0)), 1, P(e.Hm(1)), P(None)], INVALID, "no-ctx"),
    ("predict_depth_rgb/n=-1", "hevcdl_predict_depth_rgb", lambda e: [e.h, P(e.Hm(0)), -1, P(e.Hm(1)), P(None)], INVALID, "n_ctus < 0"),
    ("predict_depth_rgb/n=0", "hevcdl_predict_depth_rgb", lambda e: [e.h, P(None), 0, P(None), P(None)], OK, None),
    ("predict_depth_rgb/null-rgb", "hevcdl_predict_depth_rgb", lambda e: [e.h, P(None), 1, P(e.Hm(1)), P(None)], INVALID, NULLPTR),
    ("predict_depth_rgb/null-labels", "hevcdl_predict_depth_rgb", lambda e: [e.h, P(e.Hm(0)), 1, P(None), P(None)], INVALID, NULLPTR),
    ("predict_depth_rgb/ok", "hevcdl_predict_depth_rgb", lambda e: [e.h, P(e.Hm(0)), 2, P(e.Hm(1)), P(e.Hm(2))], OK, None),
    ("labels_from_logits/null-ctx", "hevcdl_labels_from_logits", lambda e: [P(None), P(e.Hm(0)), 1, 0, P(e.Hm(1))], INVALID, "no-ctx"),
    ("labels_from_logits/n=-1", "hevcdl_labels_from_logits", lambda e: [e.h, P(e.Hm(0)), -1, 0, P(e.Hm(1))], INVALID, "n_ctus < 0"),
    ("labels_from_logits/n=0", "hevcdl_labels_from_logits", lambda e: [e.h, P(None), 0, 0, P(None)], OK, None),
    ("labels_from_logits/null-logits", "hevcdl_labels_from_logits", lambda e: [e.h, P(None), 1, 0, P(e.Hm(1))], INVALID, NULLPTR),
    ("labels_from_logits/null-labels", "hevcdl_labels_from_logits", lambda e: [e.h, P(e.Hm(0)), 1, 0, P(None)], INVALID, NULLPTR),
    ("labels_from_logits/ok", "hevcdl_labels_from_logits", lambda e: [e.h, P(e.Hm(0)), 2, 1, P(e.Hm(1))], OK, None),
    # picture quality
    ("picture_quality_dev/out-in-org", "hevcdl_picture_quality_dev", lambda e: [e.h, P(e.D(0)), P(e.D(1)), 1, P(e.D(0, FB - 8)), P(None)], INVALID, "picture quality: the output overlaps an input"),
    ("picture_quality_dev/out-in-pic", "hevcdl_picture_quality_dev", lambda e: [e.h, P(e.D(0)), P(e.D(1)), 2, P(e.D(1, 2 * FB - 8)), P(None)], INVALID, "picture quality: the output overlaps an input"),
    ("picture_quality_dev/out-behind-org", "hevcdl_picture_quality_dev", lambda e: [e.h, P(e.D(0)), P(e.D(1)), 1, P(e.D(0, FB)), P(None)], OK, None),
    ("plane_quality/null", "hevcdl_plane_quality", lambda e: [0, P(None), P(e.Hm(1)), 48, 32, 8, P(e.Hm(2)), P(e.Hm(3))], INVALID, "no-ctx"),
    ("plane_quality/width=0", "hevcdl_plane_quality", lambda e: [0, P(e.Hm(0)), P(e.Hm(1)), 0, 32, 8, P(e.Hm(2)), P(e.Hm(3))], INVALID, "no-ctx"),
    ("plane_quality/depth=7", "hevcdl_plane_quality", lambda e: [0, P(e.Hm(0)), P(e.Hm(1)), 48, 32, 7, P(e.Hm(2)), P(e.Hm(3))], UNSUPPORTED, "no-ctx"),
    ("plane_quality/device=-1", "hevcdl_plane_quality", lambda e: [-1, P(e.Hm(0)), P(e.Hm(1)), 48, 32, 8, P(e.Hm(2)), P(e.Hm(3))], NO_DEVICE, "no-ctx"),
    ("plane_quality/device=4096", "hevcdl_plane_quality", lambda e: [4096, P(e.Hm(0)), P(e.Hm(1)), 48, 32, 8, P(e.Hm(2)), P(e.Hm(3))], NO_DEVICE, "no-ctx"),
    ("plane_quality/ok", "hevcdl_plane_quality", lambda e: [0, P(e.Hm(0)), P(e.Hm(1)), 48, 32, 8, P(e.Hm(2)), P(e.Hm(3))], OK, "no-ctx"),
    ("enable_quality/null-ctx", "hevcdl_enable_quality", lambda e: [P(None), 1], INVALID, "no-ctx"),
    ("enable_quality/off-when-off", "hevcdl_enable_quality", lambda e: [e.h, 0], OK, None),
    ("get_quality/null-ctx", "hevcdl_get_quality", lambda e: [P(None), 0, 0, P(e.Hm(0))], INVALID, "no-ctx"),
    ("get_quality/null-out", "hevcdl_get_quality", lambda e: [e.h, 0, 0, P(None)], INVALID, "hevcdl_get_quality: bad range", quality_on),
    ("get_quality/first=-1", "hevcdl_get_quality", lambda e: [e.h, -1, 1, P(e.Hm(0))], INVALID, "hevcdl_get_quality: bad range", quality_on),
    ("get_quality/count=-1", "hevcdl_get_quality", lambda e: [e.h, 0, -1, P(e.Hm(0))], INVALID, "hevcdl_get_quality: bad range", quality_on),
    ("get_quality/switch-off", "hevcdl_get_quality", lambda e: [e.h, 0, 0, P(e.Hm(0))], INVALID, "hevcdl_get_quality: hevcdl_enable_quality was not called"),
    ("get_quality/outside-batch", "hevcdl_get_quality", lambda e: [e.h, 0, 1, P(e.Hm(0))], INVALID, "hevcdl_get_quality: pictures outside the last batch", quality_on),
    ("get_quality/empty-range", "hevcdl_get_quality", lambda e: [e.h, 0, 0, P(e.Hm(0))], OK, None, quality_on),
    # picture report
    ("picture_report/n=0", "hevcdl_picture_report", lambda e: [e.h, P(None), P(None), 0, 1, P(None)], OK, None),
    ("picture_report/method=4", "hevcdl_picture_report", lambda e: [e.h, P(None), P(e.Hm(0)), 0, 4, P(e.Hm(1))], INVALID, "picture report: " + METHOD),
    ("picture_report/method=-1", "hevcdl_picture_report", lambda e: [e.h, P(None), P(e.Hm(0)), 1, -1, P(e.Hm(1))], INVALID, "picture report: " + METHOD),
    ("picture_report/null-pic", "hevcdl_picture_report", lambda e: [e.h, P(None), P(None), 1, 1, P(e.Hm(1))], INVALID, NULLPTR),
    ("picture_report/null-out", "hevcdl_picture_report", lambda e: [e.h, P(None), P(e.Hm(0)), 1, 1, P(None)], INVALID, NULLPTR),
    ("picture_report_dev/null-ctx", "hevcdl_picture_report_dev", lambda e: [P(None), P(None), P(e.D(1)), 1, 1, P(e.D(2)), P(None)], INVALID, "no-ctx"),
    ("picture_report_dev/n=-1", "hevcdl_picture_report_dev", lambda e: [e.h, P(None), P(e.D(1)), -1, 1, P(e.D(2)), P(None)], INVALID, RANGE),
    ("picture_report_dev/n=max+1", "hevcdl_picture_report_dev", lambda e: [e.h, P(None), P(e.D(1)), MAXF + 1, 1, P(e.D(2)), P(None)], INVALID, RANGE),
    ("picture_report_dev/n=0", "hevcdl_picture_report_dev", lambda e: [e.h, P(None), P(None), 0, 1, P(None), P(None)], OK, None),
    ("picture_report_dev/method=4", "hevcdl_picture_report_dev", lambda e: [e.h, P(None), P(e.D(1)), 1, 4, P(e.D(2)), P(None)], INVALID, "picture report: " + METHOD),
    ("picture_report_dev/null-pic", "hevcdl_picture_report_dev", lambda e: [e.h, P(None), P(None), 1, 1, P(e.D(2)), P(None)], INVALID, "picture report: null or misaligned device pointer"),
    ("picture_report_dev/null-out", "hevcdl_picture_report_dev", lambda e: [e.h, P(None), P(e.D(1)), 1, 1, P(None), P(None)], INVALID, "picture report: null or misaligned device pointer"),
    ("picture_report_dev/misaligned-out", "hevcdl_picture_report_dev", lambda e: [e.h, P(None), P(e.D(1)), 1, 1, P(e.D(2, 4)), P(None)], INVALID, "picture report: null or misaligned device pointer"),
    ("picture_report_dev/out-in-pic", "hevcdl_picture_report_dev", lambda e: [e.h, P(None), P(e.D(1)), 1, 1, P(e.D(1, FB - 8)), P(None)], INVALID, "picture report: the output overlaps an input"),
    ("picture_report_dev/out-in-org", "hevcdl_picture_report_dev", lambda e: [e.h, P(e.D(0)), P(e.D(1)), 1, 1, P(e.D(0, 8)), P(None)], INVALID, "picture report: the output overlaps an input"),
    ("picture_report_dev/out-behind-pic", "hevcdl_picture_report_dev", lambda e: [e.h, P(None), P(e.D(1)), 1, 1, P(e.D(1, FB)), P(None)], OK, None),
    ("plane_hash/null", "hevcdl_plane_hash", lambda e: [0, P(None), 48, 32, 8, 1, P(e.Hm(1))], INVALID, "no-ctx"),
    ("plane_hash/method=0", "hevcdl_plane_hash", lambda e: [0, P(e.Hm(0)), 48, 32, 8, 0, P(e.Hm(1))], INVALID, "no-ctx"),
    ("plane_hash/method=4", "hevcdl_plane_hash", lambda e: [0, P(e.Hm(0)), 48, 32, 8, 4, P(e.Hm(1))], INVALID, "no-ctx"),
    ("plane_hash/depth=17", "hevcdl_plane_hash", lambda e: [0, P(e.Hm(0)), 48, 32, 17, 1, P(e.Hm(1))], UNSUPPORTED, "no-ctx"),
    ("plane_hash/device=-1", "hevcdl_plane_hash", lambda e: [-1, P(e.Hm(0)), 48, 32, 8, 1, P(e.Hm(1))], NO_DEVICE, "no-ctx"),
    ("plane_hash/ok", "hevcdl_plane_hash", lambda e: [0, P(e.Hm(0)), 48, 32, 8, 1, P(e.Hm(1))], OK, "no-ctx"),
    ("enable_picture_report/null-ctx", "hevcdl_enable_picture_report", lambda e: [P(None), 1, 1], INVALID, "no-ctx"),
    ("enable_picture_report/method=4", "hevcdl_enable_picture_report", lambda e: [e.h, 1, 4], INVALID, "hevcdl_enable_picture_report: " + METHOD),
    ("enable_picture_report/off-ignores-method", "hevcdl_enable_picture_report", lambda e: [e.h, 0, 9], OK, None),
    ("get_picture_report/null-ctx", "hevcdl_get_picture_report", lambda e: [P(None), 0, 0, P(e.Hm(0))], INVALID, "no-ctx"),
    ("get_picture_report/null-out", "hevcdl_get_picture_report", lambda e: [e.h, 0, 0, P(None)], INVALID, "hevcdl_get_picture_report: bad range", report_on),
    ("get_picture_report/first=-1", "hevcdl_get_picture_report", lambda e: [e.h, -1, 0, P(e.Hm(0))], INVALID, "hevcdl_get_picture_report: bad range", report_on),
    ("get_picture_report/switch-off", "hevcdl_get_picture_report", lambda e: [e.h, 0, 0, P(e.Hm(0))], INVALID, "hevcdl_get_picture_report: hevcdl_enable_picture_report was not called"),
    ("get_picture_report/outside-batch", "hevcdl_get_picture_report", lambda e: [e.h, 1, 1, P(e.Hm(0))], INVALID, "hevcdl_get_picture_report: pictures outside the last batch", report_on),
    ("get_report_info/null-ctx", "hevcdl_get_report_info", lambda e: [P(None), P(e.Hm(0))], INVALID, "no-ctx"),
    ("get_report_info/null-out", "hevcdl_get_report_info", lambda e: [e.h, P(None)], INVALID, None),
    ("get_report_info/ok", "hevcdl_get_report_info", lambda e: [e.h, P(e.Hm(0))], OK, None),
    # source format
    ("set_source_format/null-ctx", "hevcdl_set_source_format", lambda e: [P(None), P(None)], INVALID, "no-ctx"),
    ("set_source_format/bad-format", "hevcdl_set_source_format", lambda e: [e.h, P(e.Hm(13))], INVALID, "source format: even source size of at least 2 x 2 and at most the context's, even padding, bit depths 8 .. 16"),
    ("set_source_format/off-when-off", "hevcdl_set_source_format", lambda e: [e.h, P(None)], OK, None),
    ("load_source_dev/null-ctx", "hevcdl_load_source_dev", lambda e: [P(None), P(e.D(0)), 1, P(e.D(1)), P(None)], INVALID, "no-ctx"),
    ("load_source_dev/n=-1", "hevcdl_load_source_dev", lambda e: [e.h, P(e.D(0)), -1, P(e.D(1)), P(None)], INVALID, RANGE),
    ("load_source_dev/no-format", "hevcdl_load_source_dev", lambda e: [e.h, P(e.D(0)), 1, P(e.D(1)), P(None)], INVALID, SRC_OFF),
    ("load_source_dev/no-format-n=0", "hevcdl_load_source_dev", lambda e: [e.h, P(e.D(0)), 0, P(e.D(1)), P(None)], INVALID, SRC_OFF),
    ("load_source_dev/n=0", "hevcdl_load_source_dev", lambda e: [e.h, P(None), 0, P(None), P(None)], OK, None, source_on),
    ("load_source_dev/null-src", "hevcdl_load_source_dev", lambda e: [e.h, P(None), 1, P(e.D(1)), P(None)], INVALID, SRC_PTR, source_on),
    ("load_source_dev/null-coded", "hevcdl_load_source_dev", lambda e: [e.h, P(e.D(0)), 1, P(None), P(None)], INVALID, SRC_PTR, source_on),
    ("load_source_dev/misaligned-src", "hevcdl_load_source_dev", lambda e: [e.h, P(e.D(0, 1)), 1, P(e.D(1)), P(None)], INVALID, SRC_PTR, source_on),
    ("store_output_dev/null-ctx", "hevcdl_store_output_dev", lambda e: [P(None), P(e.D(0)), 1, P(e.D(1)), P(None)], INVALID, "no-ctx"),
    ("store_output_dev/no-format", "hevcdl_store_output_dev", lambda e: [e.h, P(e.D(0)), 1, P(e.D(1)), P(None)], INVALID, SRC_OFF),
    ("store_output_dev/n=max+1", "hevcdl_store_output_dev", lambda e: [e.h, P(e.D(0)), MAXF + 1, P(e.D(1)), P(None)], INVALID, RANGE, source_on),
    ("store_output_dev/null-out", "hevcdl_store_output_dev", lambda e: [e.h, P(e.D(0)), 1, P(None), P(None)], INVALID, SRC_PTR, source_on),
    ("load_source/null-ctx", "hevcdl_load_source", lambda e: [P(None), P(e.Hm(0)), 1, P(e.Hm(1))], INVALID, "no-ctx"),
    ("load_source/no-format", "hevcdl_load_source", lambda e: [e.h, P(e.Hm(0)), 1, P(e.Hm(1))], INVALID, SRC_OFF),
    ("load_source/null-src", "hevcdl_load_source", lambda e: [e.h, P(None), 1, P(e.Hm(1))], INVALID, SRC_PTR, source_on),
    ("load_source/n=0", "hevcdl_load_source", lambda e: [e.h, P(None), 0, P(None)], OK, None, source_on),
    ("store_output/no-format", "hevcdl_store_output", lambda e: [e.h, P(e.Hm(0)), 1, P(e.Hm(1))], INVALID, SRC_OFF),
    ("store_output/null-out", "hevcdl_store_output", lambda e: [e.h, P(e.Hm(0)), 1, P(None)], INVALID, SRC_PTR, source_on),
    ("store_output/n=-1", "hevcdl_store_output", lambda e: [e.h, P(e.Hm(0)), -1, P(e.Hm(1))], INVALID, RANGE, source_on),
    ("get_output_frames/null-ctx", "hevcdl_get_output_frames", lambda e: [P(None), 0, 1, P(e.Hm(0))], INVALID, "no-ctx"),
    ("get_output_frames/no-format", "hevcdl_get_output_frames", lambda e: [e.h, 0, 1, P(e.Hm(0))], INVALID, "hevcdl_get_output_frames: hevcdl_set_source_format was not called"),
    ("get_output_frames/outside-batch", "hevcdl_get_output_frames", lambda e: [e.h, 0, 1, P(e.Hm(0))], INVALID, "hevcdl_get_output_frames: pictures outside the last batch", source_on),
    ("get_output_frames/null-out", "hevcdl_get_output_frames", lambda e: [e.h, 0, 0, P(None)], INVALID, "hevcdl_get_output_frames: pictures outside the last batch", source_on),
    # picture pipeline
    ("encode_pictures/n=0", "hevcdl_encode_pictures", lambda e: [e.h, P(None), 0, P(None), 1, P(None), P(None), P(None), P(None)], OK, None),
    ("encode_pictures/null-yuv", "hevcdl_encode_pictures", lambda e: [e.h, P(None), 1, P(None), 1, P(e.Hm(1)), P(e.Hm(2)), P(None), P(None)], INVALID, NULLPTR),
    ("encode_pictures/null-records", "hevcdl_encode_pictures", lambda e: [e.h, P(e.Hm(0)), 1, P(None), 1, P(None), P(e.Hm(2)), P(None), P(None)], INVALID, NULLPTR),
    ("encode_pictures/null-picture", "hevcdl_encode_pictures", lambda e: [e.h, P(e.Hm(0)), 1, P(None), 1, P(e.Hm(1)), P(None), P(None), P(None)], INVALID, NULLPTR),
    ("encode_pictures_chunked/null-ctx", "hevcdl_encode_pictures_chunked", lambda e: [P(None), P(e.Hm(0)), 1, P(None), 1, 1, 0, P(None), P(None)], INVALID, "no-ctx"),
    ("encode_pictures_chunked/n=-1", "hevcdl_encode_pictures_chunked", lambda e: [e.h, P(e.Hm(0)), -1, P(None), 1, 1, 0, P(None), P(None)], INVALID, RANGE),
    ("encode_pictures_chunked/n=0", "hevcdl_encode_pictures_chunked", lambda e: [e.h, P(None), 0, P(None), 1, 1, 0, P(None), P(None)], OK, None),
    ("encode_pictures_chunked/null-fn", "hevcdl_encode_pictures_chunked", lambda e: [e.h, P(e.Hm(0)), 1, P(None), 1, 1, 0, P(None), P(None)], INVALID, NULLPTR),
    ("encode_pictures_stream/null-ctx", "hevcdl_encode_pictures_stream", lambda e: [P(None), P(e.Hm(0)), 1, P(None), 1, 1, 0, 0, 0, P(None), P(None)], INVALID, "no-ctx"),
    ("encode_pictures_stream/n=max+1", "hevcdl_encode_pictures_stream", lambda e: [e.h, P(e.Hm(0)), MAXF + 1, P(None), 1, 1, 0, 0, 0, P(None), P(None)], INVALID, RANGE),
    ("encode_pictures_stream/switch-off", "hevcdl_encode_pictures_stream", lambda e: [e.h, P(e.Hm(0)), 0, P(None), 1, 1, 0, 0, 0, P(None), P(None)], INVALID, "hevcdl_encode_pictures_stream: hevcdl_enable_device_entropy was not called"),
    ("encode_pictures_stream/n=0", "hevcdl_encode_pictures_stream", lambda e: [e.h, P(None), 0, P(None), 1, 1, 0, 0, 0, P(None), P(None)], OK, None, entropy_on),
    ("encode_pictures_stream/null-fn", "hevcdl_encode_pictures_stream", lambda e: [e.h, P(e.Hm(0)), 1, P(None), 1, 1, 0, 0, 0, P(None), P(None)], INVALID, NULLPTR, entropy_on),
    # device entropy
    ("code_slice_data/null-cfg", "hevcdl_code_slice_data", lambda e: [0, P(None), P(e.Hm(1)), P(None), 1, 4096, P(e.Hm(4)), ctypes.c_size_t(8 * 65536), P(e.Hm(2)), P(e.Hm(3))], INVALID, "no-ctx"),
    ("code_slice_data/n=-1", "hevcdl_code_slice_data", lambda e: [0, "stream", P(e.Hm(1)), P(None), -1, 4096, P(e.Hm(4)), ctypes.c_size_t(8 * 65536), P(e.Hm(2)), P(e.Hm(3))], INVALID, "no-ctx"),
    ("code_slice_data/small-out", "hevcdl_code_slice_data", lambda e: [0, "stream", P(e.Hm(1)), P(None), 1, 4096, P(e.Hm(4)), ctypes.c_size_t(64), P(e.Hm(2)), P(e.Hm(3))], INVALID, "no-ctx"),
    ("code_slice_data/n=0", "hevcdl_code_slice_data", lambda e: [0, "stream", P(e.Hm(1)), P(None), 0, 4096, P(e.Hm(4)), ctypes.c_size_t(8 * 65536), P(e.Hm(2)), P(e.Hm(3))], OK, "no-ctx"),
    ("code_slice_data/device=-1", "hevcdl_code_slice_data", lambda e: [-1, "stream", P(e.Hm(1)), P(None), 1, 4096, P(e.Hm(4)), ctypes.c_size_t(8 * 65536), P(e.Hm(2)), P(e.Hm(3))], NO_DEVICE, "no-ctx"),
    ("enable_device_entropy/null-ctx", "hevcdl_enable_device_entropy", lambda e: [P(None), 1], INVALID, "no-ctx"),
    ("enable_device_entropy/off-when-off", "hevcdl_enable_device_entropy", lambda e: [e.h, 0], OK, None),
    ("set_entropy_capacity/null-ctx", "hevcdl_set_entropy_capacity", lambda e: [P(None), 64], INVALID, "no-ctx"),
    ("set_entropy_capacity/not-a-multiple", "hevcdl_set_entropy_capacity", lambda e: [e.h, 6], INVALID, "hevcdl_set_entropy_capacity: not a multiple of 4"),
    ("set_entropy_capacity/switch-on", "hevcdl_set_entropy_capacity", lambda e: [e.h, 64], INVALID, "hevcdl_set_entropy_capacity: the switch is on", entropy_on),
    ("set_entropy_capacity/ok", "hevcdl_set_entropy_capacity", lambda e: [e.h, 64], OK, None),
    ("get_entropy_info/null-ctx", "hevcdl_get_entropy_info", lambda e: [P(None), P(None), P(None)], INVALID, "no-ctx"),
    ("get_entropy_info/switch-off", "hevcdl_get_entropy_info", lambda e: [e.h, P(None), P(None)], INVALID, "hevcdl_get_entropy_info: hevcdl_enable_device_entropy was not called"),
    ("get_entropy_info/ok", "hevcdl_get_entropy_info", lambda e: [e.h, P(None), P(None)], OK, None, entropy_on),
    ("get_slice_data/null-ctx", "hevcdl_get_slice_data", lambda e: [P(None), 0, 0, P(e.Hm(0)), P(e.Hm(1)), P(e.Hm(2))], INVALID, "no-ctx"),
    ("get_slice_data/null-data", "hevcdl_get_slice_data", lambda e: [e.h, 0, 0, P(None), P(e.Hm(1)), P(e.Hm(2))], INVALID, "hevcdl_get_slice_data: bad range", entropy_on),
    ("get_slice_data/count=-1", "hevcdl_get_slice_data", lambda e: [e.h, 0, -1, P(e.Hm(0)), P(e.Hm(1)), P(e.Hm(2))], INVALID, "hevcdl_get_slice_data: bad range", entropy_on),
    ("get_slice_data/switch-off", "hevcdl_get_slice_data", lambda e: [e.h, 0, 0, P(e.Hm(0)), P(e.Hm(1)), P(e.Hm(2))], INVALID, "hevcdl_get_slice_data: hevcdl_enable_device_entropy was not called"),
    ("get_slice_data/outside-batch", "hevcdl_get_slice_data", lambda e: [e.h, 0, 0, P(e.Hm(0)), P(e.Hm(1)), P(e.Hm(2))], INVALID, "hevcdl_get_slice_data: pictures outside the last batch", entropy_on),
    # per-CTU session
    ("begin_frames/n=0", "hevcdl_begin_frames", lambda e: [e.h, P(e.Hm(0)), 0, P(None), P(None)], INVALID, "begin_frames: no frames"),
    ("begin_frames/null-yuv", "hevcdl_begin_frames", lambda e: [e.h, P(None), 1, P(None), P(None)], INVALID, "begin_frames: no frames"),
    ("compress_ctu/null-ctx", "hevcdl_compress_ctu", lambda e: [P(None), 0, 0, P(None), P(e.Hm(0)), P(None)], INVALID, "no-ctx"),
    ("compress_ctu/no-session", "hevcdl_compress_ctu", lambda e: [e.h, 0, 0, P(None), P(e.Hm(0)), P(None)], INVALID, "compress_ctu: frame outside the session (hevcdl_begin_frames)"),
    ("compress_ctu/frame=-1", "hevcdl_compress_ctu", lambda e: [e.h, -1, 0, P(None), P(e.Hm(0)), P(None)], INVALID, "compress_ctu: frame outside the session (hevcdl_begin_frames)"),
    ("get_recon/null-ctx", "hevcdl_get_recon", lambda e: [P(None), 0, P(e.Hm(0))], INVALID, "no-ctx"),
    ("get_recon/no-session", "hevcdl_get_recon", lambda e: [e.h, 0, P(e.Hm(0))], INVALID, "get_recon: frame outside the session / null pointer"),
    # profile
    ("profile_enable/null-ctx", "hevcdl_profile_enable", lambda e: [P(None), 1], INVALID, "no-ctx"),
    ("profile_enable/ok", "hevcdl_profile_enable", lambda e: [e.h, 1], OK, None),
    ("profile_get/null-ctx", "hevcdl_profile_get", lambda e: [P(None), P(e.Hm(0))], INVALID, "no-ctx"),
    ("profile_get/null-out", "hevcdl_profile_get", lambda e: [e.h, P(None)], INVALID, None),
    ("profile_get/ok", "hevcdl_profile_get", lambda e: [e.h, P(e.Hm(0))], OK, None),
]
assert len({r[0] for r in ROWS}) == len(ROWS)


@pytest.mark.parametrize("row", ROWS, ids=[r[0] for r in ROWS])
def test_entry_contract(world, row):
    """One row: the call's status, and hevcdl_last_error of its context afterwards -- the row's message, or still empty (None)."""
    lib, m = world[0], world[1]
    name, entry, make_args, status, message = row[:5]
    e = make_ctx(world)
    try:
        if len(row) > 5:
            row[5](e, m)
            assert lib.hevcdl_last_error(e.h) == b""
        stream = m.stream_config(W, H, 32)
        args = [ctypes.byref(stream) if isinstance(a, str) else a for a in make_args(e)]
        got = getattr(lib, entry)(*args)
        assert got == status, "%s returned %r, expected %r (%r)" % (name, got, status, lib.hevcdl_last_error(e.h))
        if message != "no-ctx":      # ("no-ctx": the call had no context to leave a message in)
            assert lib.hevcdl_last_error(e.h) == (message or "").encode(), name
        else:
            assert lib.hevcdl_last_error(e.h) == b"", name
    finally:
        lib.hevcdl_destroy(e.h)
    lib.hevcdl_destroy(P(None))


def test_tiled_context_has_no_per_ctu_session(world):
    lib = world[0]
    e = make_ctx(world, 256, 128, tiles=(1, 2))
    try:
        assert lib.hevcdl_compress_ctu(e.h, 0, 0, P(None), P(e.Hm(0)), P(None)) == UNSUPPORTED
        assert lib.hevcdl_last_error(e.h) == b"compress_ctu: the per-CTU session walks the untiled raster scan; with tiles use hevcdl_compress_frames"
    finally:
        lib.hevcdl_destroy(e.h)


# ---- the switches ---------------------------------------------------------------------------------------------------------------------------------------------
def _same(a, b):
    return all((x is None and y is None) or (np.asarray(x).tobytes() == np.asarray(y).tobytes()) for x, y in zip(a, b))


@pytest.mark.parametrize("switch", ["quality", "report", "entropy", "source"])
def test_switch_on_off_on_off_leaves_the_pipeline_as_a_fresh_context(switch):
    """A switch turned on, off, on and off again around hevcdl_encode_pictures of one 72x40 picture in a 128x64 context: with the switch off the records, pictures, SAO
    parameters and statistics are byte for byte a fresh context's that never touched a switch, and what the switch adds is the same the second time it is on."""
    import hevcdl_amd as m
    cw, ch, sw, sh = 128, 64, 72, 40
    rng = np.random.default_rng(72)
    src = rng.integers(0, 256, (1, sw * sh * 3 // 2)).astype(np.uint8)
    fmt = m.source_format(sw, sh, 8, 8)
    coded = m.load_source_host(fmt, cw, ch, 8, src)      # the 72x40 picture padded to the context's size: what a context without a source format is given
    fresh = m.Encoder(cw, ch, 32, max_frames=1)
    want = fresh.encode_pictures(coded)
    fresh.close()
    enc = m.Encoder(cw, ch, 32, max_frames=1)

    def on():
        if switch == "quality":
            enc.enable_quality(True)
            return enc.encode_pictures(coded) + (enc.get_quality(0, 1),)
        if switch == "report":
            enc.enable_picture_report(True, 1)
            return enc.encode_pictures(coded) + (enc.get_picture_report(0, 1),)
        if switch == "entropy":
            enc.enable_device_entropy(True)
            out = enc.encode_pictures(coded)
            data, sizes = enc.get_slice_data(0, 1)
            return out + (np.frombuffer(data[0], np.uint8), sizes)
        enc.set_source_format(fmt)
        return enc.encode_pictures(src) + (enc.get_output_frames(0, 1),)

    def off():
        if switch == "quality":
            enc.enable_quality(False)
        elif switch == "report":
            enc.enable_picture_report(False)
        elif switch == "entropy":
            enc.enable_device_entropy(False)
        else:
            enc.set_source_format(None)
        return enc.encode_pictures(coded)
    try:
        first = on()
        assert _same(off(), want), "after the first off"
        second = on()
        assert _same(first, second), "the second on"
        assert _same(off(), want), "after the second off"
        if switch != "source":      # (a padded source format takes the statistics' SSE over the window: the others add results and change none)
            assert _same(first[:4], want), "records, pictures, SAO parameters and statistics with the switch on"
    finally:
        enc.close()
