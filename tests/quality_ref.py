"""Test helper (not a conftest): TEncGOP::xCalculateMSSSIM (HM_dl/source/Lib/TLibEncoder/TEncGOP.cpp:2559-2727) restated in f64 in the reference's own
order of operations, the bound on what a different order of the block sum may change, and readers for the quality fixtures (tests/golden/quality_*.npz).

Order: numpy's elementwise multiply and add are separate IEEE operations (nothing is fused), so evaluating one window tap at a time for ALL blocks of a scale
at once -- taps in the reference's y-then-x order, each term (a * b) * w added to the running sum -- gives every block exactly the reference's value.  The mean
over the blocks is the reference's serial raster-order sum (np.cumsum accumulates left to right)."""
import math
import os
import re

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EXPONENTS = [[1.0, 0, 0, 0, 0], [0.1356, 0.8644, 0, 0, 0], [0.0711, 0.4530, 0.4760, 0, 0], [0.0517, 0.3295, 0.3462, 0.2726, 0], [0.0448, 0.2856, 0.3001, 0.2363, 0.1333]]      # :2614-2618
CASES = ["c416_q32", "r200_q27_f2", "b192_q30_b10", "s64_q32", "k64_q32_const", "t16_q32"]


def n_scales(width, height):
    """:2567-2587"""
    for s, cut in enumerate((22, 44, 88, 176)):
        if width < cut or height < cut:
            return s + 1
    return 5


def window():
    """:2591-2611, libm's exp, the reference's loop order."""
    w = [[math.exp(-((y - 5) * (y - 5) + (x - 5) * (x - 5)) / (5 - 0.5)) for x in range(11)] for y in range(11)]
    total = 0.0
    for y in range(11):
        for x in range(11):
            total += w[y][x]
    return [[w[y][x] / total for x in range(11)] for y in range(11)]


def pyramid(plane, scales):
    """:2620-2661.  Level s is read from level s - 1 as a FLAT array with row pitch 2 * (width >> s), as the reference does."""
    h, w = plane.shape
    levels = [plane.astype(np.float64)]
    for s in range(1, scales):
        hs, ws = h >> s, w >> s
        prev = levels[-1].ravel()
        y, x = np.mgrid[0:hs, 0:ws]
        a, b = 2 * y * (2 * ws) + 2 * x, (2 * y + 1) * (2 * ws) + 2 * x
        levels.append((prev[a] + prev[a + 1] + prev[b] + prev[b + 1]) / 4.0)
    return levels


def msssim(org, rec, bit_depth, details=False):
    """One plane ([rows][cols] integer samples).  details: also [(blocks, max |block value|, mean)] per scale, for msssim_tolerance."""
    h, w = org.shape
    scales = n_scales(w, h)
    wt = window()
    po, pr = pyramid(np.asarray(org), scales), pyramid(np.asarray(rec), scales)
    max_value = (1 << bit_depth) - 1
    c1, c2 = (0.01 * max_value) * (0.01 * max_value), (0.03 * max_value) * (0.03 * max_value)
    final, info = 1.0, []
    for s in range(scales):
        o, r = po[s], pr[s]
        hs, ws = o.shape
        bw, bh = ws - 11 + 1, hs - 11 + 1
        total = bw * bh
        mean_sum, bmax = 0.0, 0.0
        if bw > 0 and bh > 0:
            oo, rr, orr = o * o, r * r, o * r
            m_o, m_r, m_oo, m_rr, m_or = (np.zeros((bh, bw)) for _ in range(5))
            for y in range(11):
                for x in range(11):
                    g = wt[y][x]
                    m_o += o[y:y + bh, x:x + bw] * g
                    m_r += r[y:y + bh, x:x + bw] * g
                    m_oo += oo[y:y + bh, x:x + bw] * g
                    m_rr += rr[y:y + bh, x:x + bw] * g
                    m_or += orr[y:y + bh, x:x + bw] * g
            var_o, var_r, cov = m_oo - (m_o * m_o), m_rr - (m_r * m_r), m_or - (m_o * m_r)
            blk = (2.0 * cov + c2) / (var_o + var_r + c2)
            if s == scales - 1:
                blk = blk * ((2.0 * m_o * m_r + c1) / (m_o * m_o + m_r * m_r + c1))
            mean_sum = float(np.cumsum(blk.ravel())[-1])
            bmax = float(np.abs(blk).max())
        with np.errstate(all="ignore"):
            mean = float(np.float64(mean_sum) / np.float64(total))          # 0 / totalBlocks where the loops are empty (:2721)
        info.append((max(total, 0) if bw > 0 and bh > 0 else 0, bmax, mean))
        try:
            final *= math.pow(mean, EXPONENTS[scales - 1][s])
        except ValueError:
            final = float("nan")
    return (final, info) if details else final


U = 2.0 ** -53
POW_ULPS = 4      # "a few ulp" for pow itself (the device's and the host's libm each round pow to within a couple of units of the last place)


def msssim_tolerance(final, info):
    """Bound on |kernel - restatement| for one plane, derived, not measured.
    Every block value is bit-identical by construction; only the ORDER in which a scale's N blocks are added differs (fixed tree on the device, serial raster
    order here and in the reference).  Per scale  |d mean| <= N * 2^-53 * max |block|: this is the first-order worst case of ONE order of summation against
    the exact sum (N - 1 additions, each rounding a partial sum of at most N max |block|, divided by N).  The distance between two orders is at most the
    sum of both orders' errors; the device's order is a tree about 520 additions deep at most (4 per lane, 8 tree levels, up to ~500 tile sums per lane of
    the last pass, 4 levels), so its own share is about 520 / N of that figure for a picture-sized plane and the serial order's share is what counts.  The
    bound is kept at the one-sided figure, as this feature was specified, which is the STRICTER choice for the kernel; a rounding error that is a random
    walk stays near sqrt(N) * 2^-53, far inside either.  The result is the product over the scales of mean^e, so to first order
    |d final| / |final| <= sum_s e_s * |d mean_s| / |mean_s|; on top of it every pow may be POW_ULPS units of the last place off on either side and every
    multiplication of the product rounds once: (POW_ULPS + 1) * 2^-52 per scale.
    A scale with no block (plane smaller than the window) or a mean that is not positive has no freedom: 0 / totalBlocks and pow of it must agree exactly."""
    if not math.isfinite(final) or final == 0.0:
        return 0.0
    scales = len(info)
    rel = 0.0
    for s, (n, bmax, mean) in enumerate(info):
        if n == 0 or not mean > 0.0:
            return 0.0
        rel += EXPONENTS[scales - 1][s] * (n * U * bmax) / abs(mean) + (POW_ULPS + 1) * 2.0 * U
    return abs(final) * rel


def planes(frame, width, height):
    """One packed planar 4:2:0 picture -> [Y, U, V] as 2-D arrays."""
    n, c = width * height, (width // 2) * (height // 2)
    return [frame[:n].reshape(height, width), frame[n:n + c].reshape(height // 2, width // 2), frame[n + c:n + 2 * c].reshape(height // 2, width // 2)]


def sse(org, rec):
    d = org.astype(np.int64) - rec.astype(np.int64)
    return int((d * d).sum())


class Fixture:
    """tests/golden/quality_<case>.npz: input frames, labels, the reference's final pictures and its stdout lines (run with the three Print keys)."""

    def __init__(self, case):
        f = np.load(os.path.join(GOLD, "quality_%s.npz" % case))
        self.case = case
        self.width, self.height, self.qp, self.bit_depth = int(f["width"]), int(f["height"]), int(f["qp"]), int(f["bit_depth"])
        self.yuv, self.labels, self.recon = f["yuv"], f["labels"], f["recon_filtered"]
        self.n = self.yuv.shape[0]
        self.lines = [str(l) for l in f["stdout"]]
        self.poc_lines = [l for l in self.lines if l.startswith("POC")]
        i = next(k for k, l in enumerate(self.lines) if l.startswith("SUMMARY"))
        self.summary = self.lines[i + 1:i + 3]               # header and the averaged row

    def printed_msssim(self):
        """[(Y, U, V) text] per picture"""
        return [re.search(r"\[MS-SSIM Y (\S+) +U (\S+) +V (\S+)\]", l).groups() for l in self.poc_lines]

    def printed_psnr_mse(self):
        return [(re.search(r"\[Y (\S+) dB +U (\S+) dB +V (\S+) dB\]", l).groups(), re.search(r"\[Y MSE (\S+) +U MSE (\S+) +V MSE (\S+)\]", l).groups()) for l in self.poc_lines]

    def bits(self):
        return [int(re.search(r"\) +(\d+) bits", l).group(1)) for l in self.poc_lines]


def strip_et(line):
    """A picture line without its [ET ...] group and without what follows it (reference list groups, hash text)."""
    return line.split(" [ET", 1)[0]
