"""The slice fixtures tests/golden/slices_*.npz (tools/gen_slice_fixtures.py: runs of the reference encoder with SliceMode 1 / 3) and what the slice tests share:
loading, the tile grid that computes what a fixture's slices compute, the reference's pictures as frames."""
import glob
import os
import sys

import numpy as np

from conftest import GOLD, ROOT

CASES = sorted(glob.glob(os.path.join(GOLD, "slices_*.npz")))
# the suggested set of the issue, by what each is there for
EXPECTED = {"r128_a2", "r192x200_a6", "r192x200_a6_lf0", "c64x192_a1", "r128_a2_b10", "r128_a2_off", "r128_a2_k", "r128_a2_inpps0", "r264x136_a5_lf0", "t512_a1", "t512_a3",
            "t512_a1_lf0"}


def case_id(path):
    return os.path.basename(path)[len("slices_"):-4]


def path_of(name):
    return os.path.join(GOLD, "slices_%s.npz" % name)


class Case:
    """One fixture: the keys of the reference run and its results."""

    def __init__(self, path):
        f = np.load(path)
        self.f, self.name = f, case_id(path)
        self.w, self.h, self.qp, self.bd = int(f["width"]), int(f["height"]), int(f["qp"]), int(f["bit_depth"])
        self.mode, self.arg, self.lf_slices = int(f["slice_mode"]), int(f["slice_argument"]), bool(int(f["lf_across_slices"]))
        self.tiles, self.lf_tiles = tuple(int(v) for v in f["tiles"]), bool(int(f["lf_across_tiles"]))
        self.tools, self.sao, self.lf_disable = int(f["tools"]), bool(int(f["sao"])), bool(int(f["lf_disable"]))
        self.in_pps, self.offsets = bool(int(f["lf_offset_in_pps"])), tuple(int(v) for v in f["lf_offsets"])
        self.nf, self.nctu = f["records"].shape[0], f["records"].shape[1]
        self.cx, self.cy = (self.w + 63) // 64, (self.h + 63) // 64
        self.dt = np.uint8 if self.bd == 8 else np.dtype("<u2")
        self.fs = self.w * self.h * 3 // 2
        self.yuv, self.labels = f["yuv"].reshape(self.nf, self.fs), f["labels"]
        self.stream = f["bitstream"].tobytes()
        self.final = np.frombuffer(f["recon_file"].tobytes(), self.dt).reshape(self.nf, self.fs)      # the reconstruction file: behind deblocking and SAO
        self.n_slices = int(f["n_slices"])

    @property
    def slices(self):
        return (self.mode, self.arg)

    def grid(self):
        """(tiles, lf_across_tiles) of the tile context that computes what this case's slice context computes: a column of row slices, or the cfg's tiles with the
        two flags combined."""
        if self.mode == 3:
            return self.tiles, self.lf_tiles and self.lf_slices
        rows = self.arg // self.cx
        return ([self.cx], [min(rows, self.cy - r) for r in range(0, self.cy, rows)]), self.lf_slices

    def records(self, dtype):
        return np.frombuffer(self.f["records"].tobytes(), dtype=dtype).reshape(self.nf, self.nctu)

    def prefilter(self):
        """The reference's reconstruction before the in-loop filters as frames, from the per-CTU blocks behind every compressCtu."""
        f, w, h = self.f, self.w, self.h
        frames = np.zeros((self.nf, self.fs), self.dt)
        for fr in range(self.nf):
            Y = np.zeros((h + 64, w + 64), self.dt); U = np.zeros((h // 2 + 32, w // 2 + 32), self.dt); V = U.copy()
            for a in range(self.nctu):
                x0, y0 = (a % self.cx) * 64, (a // self.cx) * 64
                Y[y0:y0 + 64, x0:x0 + 64] = f["rec_y"][fr, a].reshape(64, 64)
                U[y0 // 2:y0 // 2 + 32, x0 // 2:x0 // 2 + 32] = f["rec_cb"][fr, a].reshape(32, 32)
                V[y0 // 2:y0 // 2 + 32, x0 // 2:x0 // 2 + 32] = f["rec_cr"][fr, a].reshape(32, 32)
            frames[fr] = np.concatenate([Y[:h, :w].ravel(), U[:h // 2, :w // 2].ravel(), V[:h // 2, :w // 2].ravel()])
        return frames

    def choice(self):
        """What every slice header says about deblocking (hevcdl_dbk_choice): with LoopFilterOffsetInPPS 0 the cfg's values behind an override flag, otherwise nothing."""
        if self.in_pps:
            return None
        return (1, 1, int(self.lf_disable), 0 if self.lf_disable else self.offsets[0], 0 if self.lf_disable else self.offsets[1])


def split_annexb(stream):
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import hevc_parse
    return hevc_parse.split_annexb(stream)


def slice_nals(stream):
    """Slice NAL units per access unit (an access unit starts at a VPS: ReWriteParamSetsFlag 1)."""
    counts = []
    for _, n in split_annexb(stream):
        t = (n[0] >> 1) & 63
        if t == 32:
            counts.append(0)
        elif t <= 21:
            counts[-1] += 1
    return counts


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
