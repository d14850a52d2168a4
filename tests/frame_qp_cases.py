"""The fixtures tests/golden/fqp_*.npz (tools/gen_frame_qp_fixtures.py: runs of the reference encoder with dQPFile, QPIncrementFrame, IntraQPOffset, LambdaModifierI and
LambdaModifier0) and what the two test files share: loading, and the restatement of the reference's rule in Python."""
import glob
import os

import numpy as np

from conftest import GOLD

CASES = sorted(glob.glob(os.path.join(GOLD, "fqp_*.npz")))
# the set of the issue, by what each is there for: 1 the permuted path; 2 the increment with FrameSkip, no copy; 3 file over increment, a short file; 4 IntraQPOffset with
# LambdaModifierI, LambdaModifier0 alone; 5 wavefront, tiles; 6 ten bits, the clip at 51; 7 slices
EXPECTED = {"d192_q32", "i192_q32_s1", "di192_q32", "o192_q32_lmi", "o192_q32_lm0", "w192_q32", "t512_q32", "d192_q32_b10", "c192_q50", "s192_q32"}


def case_id(path):
    return os.path.basename(path)[len("fqp_"):-4]


def path_of(name):
    return os.path.join(GOLD, "fqp_%s.npz" % name)


def switching_poc(value, frame_skip, ratio):
    """TAppEncCfg.cpp:1667-1676"""
    return (value - frame_skip) // ratio if value > frame_skip else 0


def offsets(n, qpif=None, frame_skip=0, ratio=1, file_values=()):
    """TAppEncCfg.cpp:1663-1681, then :1735-1753: the file is read afterwards and overwrites, for at most n POCs."""
    d = [0] * n
    if qpif is not None:
        for i in range(switching_poc(qpif, frame_skip, ratio), n):
            d[i] = 1
    for i, v in enumerate(list(file_values)[:n]):
        d[i] = int(v)
    return d


def picture_qp(base, dqp, intra_qp_offset, bd):
    """TEncTop.cpp:1409-1423, 1449 for an I slice"""
    return max(-6 * (bd - 8), min(51, base + dqp + intra_qp_offset))


def contiguous(qps):
    """Every QP is one contiguous run of the list: nothing needs copying."""
    starts = [q for i, q in enumerate(qps) if i == 0 or q != qps[i - 1]]
    return len(starts) == len(set(starts))


class Case:
    """One fixture: the keys of the reference run and its results."""

    def __init__(self, path):
        f = np.load(path)
        self.f, self.name = f, case_id(path)
        self.w, self.h, self.qp, self.bd = int(f["width"]), int(f["height"]), int(f["qp"]), int(f["bit_depth"])
        self.tiles, self.wpp, self.skip = tuple(int(v) for v in f["tiles"]), bool(int(f["wavefront"])), int(f["frame_skip"])
        self.slices = tuple(int(v) for v in f["slices"]) if int(f["slices"][0]) else None
        self.qpif = None if int(f["qp_increment_frame"]) < 0 else int(f["qp_increment_frame"])
        self.intra_qp_offset, self.dqp_text = int(f["intra_qp_offset"]), str(f["dqp_text"])
        lmi, lm0 = float(f["lambda_modifier_i"]), float(f["lambda_modifier_0"])
        self.lmi, self.lm0 = (None if lmi < 0 else lmi), (None if lm0 < 0 else lm0)
        self.modifier = self.lmi if self.lmi is not None else (self.lm0 if self.lm0 is not None else 1.0)      # TEncSlice.cpp:512-520
        self.nf, self.nctu = f["records"].shape[0], f["records"].shape[1]
        self.dt = np.uint8 if self.bd == 8 else np.dtype("<u2")
        self.fs = self.w * self.h * 3 // 2
        self.file_yuv = f["yuv"].reshape(self.nf + self.skip, self.fs)      # the input file, FrameSkip frames in front included
        self.yuv, self.labels = self.file_yuv[self.skip:], f["labels"]
        self.qps, self.dqp = [int(v) for v in f["qps"]], [int(v) for v in f["dqp"]]
        self.stream, self.stream_nosao = f["bitstream"].tobytes(), f["bitstream_nosao"].tobytes()
        self.final = np.frombuffer(f["recon_file"].tobytes(), self.dt).reshape(self.nf, self.fs)          # the reconstruction file: behind deblocking and SAO
        self.deblocked = np.frombuffer(f["deblocked_file"].tobytes(), self.dt).reshape(self.nf, self.fs)  # ... of the run with --SAO=0: behind deblocking
        self.prefilter = f["prefilter"].reshape(self.nf, self.fs)
        self.keys = [str(k) for k in f["keys"]]

    def records(self, dtype):
        return np.frombuffer(self.f["records"].tobytes(), dtype=dtype).reshape(self.nf, self.nctu)

    def encoder(self, **kw):
        import hevcdl_amd
        kw.setdefault("max_frames", self.nf)
        return hevcdl_amd.Encoder(self.w, self.h, self.qp, tiles=self.tiles, bit_depth=self.bd, wavefront=self.wpp, slices=self.slices, **kw)

    def writer_kw(self):
        return dict(tiles=self.tiles, bit_depth=self.bd, wavefront=self.wpp, slices=self.slices)


def strip_sei(stream):
    import hevc_parse
    return b"".join((b"\x00" if sc == 4 else b"") + b"\x00\x00\x01" + n for sc, n in hevc_parse.split_annexb(stream) if ((n[0] >> 1) & 63) != 40)
