"""The reconstruction from records on the CPU (csrc/recon_core.h through hevcdl_reconstruct_frames_host: the source the device kernel compiles, one sample at a time):
the reference encoder's streams, parsed, give the reference's unfiltered reconstruction byte for byte.  No GPU (the kernel: tests/test_recon_gpu.py)."""
import glob
import os
import sys

import numpy as np
import pytest

from conftest import GOLD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

RD = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLD, "rd_*.npz")))
LAYOUTS = sorted(os.path.basename(p)[:-4] for fam in ("slices", "segments", "dqr") for p in glob.glob(os.path.join(GOLD, fam + "_*.npz")))


def parsed_and_expected(name):
    """-> (ParsedStream of the fixture's stream, the fixture) -- the records are the parser's, so the whole path stream -> records -> samples is under test."""
    import hevcdl_amd
    f = np.load(os.path.join(GOLD, name + ".npz"))
    return hevcdl_amd.parse_stream(f["bitstream"].tobytes()), f


def assert_unfiltered(recon, f, name):
    """recon [pictures, samples] against the fixture's rec_y / rec_cb / rec_cr: the reference's reconstruction of every CTU before the in-loop filters."""
    import ref_tools
    w, h = int(f["width"]), int(f["height"])
    assert recon.shape[0] == f["rec_y"].shape[0]
    for fr in range(recon.shape[0]):
        for a in range(f["rec_y"].shape[1]):
            y, u, v = ref_tools.ctu_recon_from_frame(recon[fr], w, h, a)
            for got, key in ((y, "rec_y"), (u, "rec_cb"), (v, "rec_cr")):
                assert np.array_equal(got, f[key][fr, a]), (name, fr, a, key, np.argwhere(np.asarray(got) != f[key][fr, a])[:4].tolist())


@pytest.mark.parametrize("name", RD)
def test_host_reconstruction_of_every_rd_fixture(name):
    """All 56 reference runs: every size and edge, QP 0 and 51, 10 bits, each tool switch (transform skip, strong smoothing off), tiles, wavefront."""
    import hevcdl_amd
    p, f = parsed_and_expected(name)
    assert_unfiltered(hevcdl_amd.reconstruct_frames(p.cfg, p.records, slices=p.slices, qps=p.qps), f, name)


@pytest.mark.parametrize("name", LAYOUTS)
def test_host_reconstruction_under_slices_segments_and_picture_qps(name):
    """Row and tile slices (a neighbour in another slice is not available), dependent segments (they change nothing), a QP per picture (dqr_*)."""
    import hevcdl_amd
    p, f = parsed_and_expected(name)
    assert_unfiltered(hevcdl_amd.reconstruct_frames(p.cfg, p.records, slices=p.slices, qps=p.qps), f, name)


def test_reconstruction_refuses_records_that_do_not_validate():
    import entropy_cases as ec
    import hevcdl_amd
    cfg = hevcdl_amd.stream_config(72, 72, 30)
    with pytest.raises(hevcdl_amd.HevcdlError) as e:
        hevcdl_amd.reconstruct_frames(cfg, ec.garbage_records(3, 4)[None])
    assert e.value.status == 1
    cfg.bit_depth = 12
    with pytest.raises(hevcdl_amd.HevcdlError) as e:
        hevcdl_amd.reconstruct_frames(cfg, ec.synth_records(np.random.default_rng(5), 72, 72)[None])
    assert e.value.status == 2
