"""The segment fixtures tests/golden/segments_*.npz (tools/gen_segment_fixtures.py: runs of the reference encoder with SliceSegmentMode 1 over wavefront rows and
SliceSegmentMode 3 over tiles) and what the segment tests share: loading, the reference's pictures as frames, the NAL units of a stream."""
import glob
import os
import sys

import numpy as np

from conftest import GOLD, ROOT

CASES = sorted(glob.glob(os.path.join(GOLD, "segments_*.npz")))
# the set of the issue, by what each is there for
EXPECTED = {"w264x136_a5", "w264x264_a10", "w64x192_a1", "t512x128_a1", "t512x128_a3", "t512x128_s2_a1"}


def case_id(path):
    return os.path.basename(path)[len("segments_"):-4]


def path_of(name):
    return os.path.join(GOLD, "segments_%s.npz" % name)


class Case:
    """One fixture: the keys of the reference run and its results.  All fixtures are 8-bit runs with the reference's tool set, both in-loop filters on and the
    across-tiles / across-slices flags 1."""

    def __init__(self, path):
        f = np.load(path)
        self.f, self.name = f, case_id(path)
        self.w, self.h, self.qp, self.bd = int(f["width"]), int(f["height"]), int(f["qp"]), int(f["bit_depth"])
        self.segments = (int(f["segment_mode"]), int(f["segment_argument"]))
        self.wavefront = bool(int(f["wavefront"]))
        self.tiles = tuple(int(v) for v in f["tiles"])
        self.slices = tuple(int(v) for v in f["slices"]) if int(f["slices"][0]) else None
        self.tools = int(f["tools"])
        self.dependent = [int(v) for v in f["dependent"]]      # dependent_slice_segment_flag of the slice NAL units of one picture
        self.nf, self.nctu = f["records"].shape[0], f["records"].shape[1]
        self.cx, self.cy = (self.w + 63) // 64, (self.h + 63) // 64
        self.fs = self.w * self.h * 3 // 2
        self.yuv, self.labels = f["yuv"].reshape(self.nf, self.fs), f["labels"]
        self.stream, self.stream_nosao = f["bitstream"].tobytes(), f["bitstream_nosao"].tobytes()
        self._pics = None

    def kw(self):
        """The keyword arguments default_config / Encoder / write_access_unit share for this case's context."""
        d = dict(tiles=self.tiles, wavefront=self.wavefront, tools=self.tools, segments=self.segments)
        if self.slices:
            d["slices"] = self.slices
        return d

    def substreams_ending_a_dependent_border(self):
        """The sub-streams (CTU rows, tiles) whose last CTU ends a segment in mid-slice: the ones the segment keys change (end_of_slice_segment_flag 1 where the stream
        without the keys has flag 0 and end_of_subset_one_bit)."""
        units = self.cy if self.wavefront else self.tiles[0] * self.tiles[1]
        seg = self.segments[1] // self.cx if self.segments[0] == 1 else self.segments[1]
        per = self.slices[1] if self.slices else units
        out = []
        for k0 in range(0, units, per):
            k1 = min(k0 + per, units)
            out += [s0 - 1 for s0 in range(k0 + seg, k1, seg)]
        return out

    def records(self, dtype):
        return np.frombuffer(self.f["records"].tobytes(), dtype=dtype).reshape(self.nf, self.nctu)

    def _pictures(self):
        if self._pics is None:
            f, w, h = self.f, self.w, self.h
            unf = np.zeros((self.nf, self.fs), np.uint8)
            for fr in range(self.nf):
                Y = np.zeros((h + 64, w + 64), np.uint8); U = np.zeros((h // 2 + 32, w // 2 + 32), np.uint8); V = U.copy()
                for a in range(self.nctu):
                    x0, y0 = (a % self.cx) * 64, (a // self.cx) * 64
                    Y[y0:y0 + 64, x0:x0 + 64] = f["rec_y"][fr, a].reshape(64, 64)
                    U[y0 // 2:y0 // 2 + 32, x0 // 2:x0 // 2 + 32] = f["rec_cb"][fr, a].reshape(32, 32)
                    V[y0 // 2:y0 // 2 + 32, x0 // 2:x0 // 2 + 32] = f["rec_cr"][fr, a].reshape(32, 32)
                unf[fr] = np.concatenate([Y[:h, :w].ravel(), U[:h // 2, :w // 2].ravel(), V[:h // 2, :w // 2].ravel()])
            dbk = unf.astype(np.int16) + f["deblocked_delta"].reshape(self.nf, self.fs)
            fin = dbk + f["final_delta"].reshape(self.nf, self.fs)
            assert dbk.min() >= 0 and dbk.max() <= 255 and fin.min() >= 0 and fin.max() <= 255
            self._pics = (unf, dbk.astype(np.uint8), fin.astype(np.uint8))
        return self._pics

    def prefilter(self):
        """The reference's reconstruction before the in-loop filters as frames, from the per-CTU blocks behind every compressCtu."""
        return self._pictures()[0]

    @property
    def deblocked(self):
        """The reconstruction file of the run with --SAO=0."""
        return self._pictures()[1]

    @property
    def final(self):
        """The reconstruction file: behind deblocking and SAO."""
        return self._pictures()[2]


def split_annexb(stream):
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import hevc_parse
    return hevc_parse.split_annexb(stream)


def slice_nals(stream):
    """Per access unit (one starts at a VPS: ReWriteParamSetsFlag 1): [(NAL unit type, first_slice_segment_in_pic_flag, dependent_slice_segment_flag)] of its slice NAL
    units, read by oracle/hevc_parse.py's slice_segment_header(): the flag exists under the PPS's dependent_slice_segments_enabled_flag in every header but the
    picture's first; elsewhere it is reported as 0."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import hevc_parse
    out, sps, pps = [], None, None
    for _, n in split_annexb(stream):
        t = (n[0] >> 1) & 63
        if t == 32:
            out.append([])
        elif t == 33:
            sps = hevc_parse.parse_sps(n)
        elif t == 34:
            pps = hevc_parse.parse_pps(n)
        elif t <= 21:
            hdr, _ = hevc_parse.parse_slice_header(n, sps, pps)
            out[-1].append((t, hdr["first_slice"], hdr["dependent"]))
    return out


def access_units(stream):
    """The access units of a stream as byte strings, hash SEI included."""
    out = []
    for sc, n in split_annexb(stream):
        if ((n[0] >> 1) & 63) == 32:
            out.append(b"")
        out[-1] += (b"\x00" if sc == 4 else b"") + b"\x00\x00\x01" + n
    return out


def strip_sei(stream):
    return b"".join((b"\x00" if sc == 4 else b"") + b"\x00\x00\x01" + n for sc, n in split_annexb(stream) if ((n[0] >> 1) & 63) != 40)
