"""The DeltaQpRD fixtures tests/golden/dqr_*.npz (tools/gen_deltaqprd_fixtures.py: runs of the reference encoder with --DeltaQpRD=N) and what the two test files share:
loading, the reference's pictures as frames, and the restatement of the reference's rules in Python."""
import glob
import os

import numpy as np

from conftest import GOLD

CASES = sorted(glob.glob(os.path.join(GOLD, "dqr_*.npz")))
# the set of the issue, by what each is there for
EXPECTED = {"c128_q32_n1", "c192x136_q27_n2", "e64_q51_n1", "e64_q0_n1", "w192x128_q32_n1", "t512x128_q32_n1", "c128_q30_n1_b10", "k128_q27_n1"}


def case_id(path):
    return os.path.basename(path)[len("dqr_"):-4]


def path_of(name):
    return os.path.join(GOLD, "dqr_%s.npz" % name)


def offset_of(idx):
    """TEncSlice.cpp:294: 0, -1, +1, -2, +2, ..."""
    return ((idx + 1) >> 1) * (-1 if idx & 1 else 1)


def coded_qp(qp, idx, bd):
    """TEncSlice.cpp:523"""
    return max(-6 * (bd - 8), min(51, qp + offset_of(idx)))


def frame_lambda(qp):
    """TEncSlice.cpp:615-623, GOP size 1"""
    return 0.68 * 2.0 ** ((qp - 12) / 3.0)


def pick(bits, dist, lam):
    """TEncSlice.cpp:604-653 with TComRdCost::calcRdCost(bits, dist, DF_SSE_FRAME) (TComRdCost.cpp:62-107): Python floats are IEEE doubles and every operation rounds once,
    so the multiply and the add are the reference's two operations."""
    best, best_idx = 1.7e+308, 0
    for i, (b, d) in enumerate(zip(bits, dist)):
        cost = float(int(d)) + float(int(b)) * lam
        if cost < best:
            best, best_idx = cost, i
    return best_idx


class Case:
    """One fixture: the keys of the reference run and its results."""

    def __init__(self, path):
        f = np.load(path)
        self.f, self.name = f, case_id(path)
        self.w, self.h, self.qp, self.bd, self.n = int(f["width"]), int(f["height"]), int(f["qp"]), int(f["bit_depth"]), int(f["delta_qp_rd"])
        self.tiles, self.wpp, self.tools = tuple(int(v) for v in f["tiles"]), bool(int(f["wavefront"])), int(f["tools"])
        self.nf, self.nctu = f["records"].shape[0], f["records"].shape[1]
        self.cx, self.cy = (self.w + 63) // 64, (self.h + 63) // 64
        self.dt = np.uint8 if self.bd == 8 else np.dtype("<u2")
        self.fs = self.w * self.h * 3 // 2
        self.yuv, self.labels = f["yuv"].reshape(self.nf, self.fs), f["labels"]
        self.stream = f["bitstream"].tobytes()
        self.final = np.frombuffer(f["recon_file"].tobytes(), self.dt).reshape(self.nf, self.fs)          # the reconstruction file: behind deblocking and SAO
        self.deblocked = np.frombuffer(f["deblocked_file"].tobytes(), self.dt).reshape(self.nf, self.fs)  # ... of the run with --SAO=0: behind deblocking
        self.chosen_idx, self.chosen_qp = f["chosen_idx"].astype(np.int32), f["chosen_qp"].astype(np.int32)
        # picture sums of every candidate, [picture][candidate]
        self.bits = f["cand_bits"].astype(np.uint64).sum(axis=2)
        self.dist = f["cand_dist"].astype(np.uint64).sum(axis=2)

    def records(self, dtype):
        return np.frombuffer(self.f["records"].tobytes(), dtype=dtype).reshape(self.nf, self.nctu)

    def prefilter(self):
        """The reference's reconstruction before the in-loop filters as frames, from the per-CTU blocks behind every compressCtu of the final pass."""
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


def strip_sei(stream):
    import hevc_parse
    return b"".join((b"\x00" if sc == 4 else b"") + b"\x00\x00\x01" + n for sc, n in hevc_parse.split_annexb(stream) if ((n[0] >> 1) & 63) != 40)
