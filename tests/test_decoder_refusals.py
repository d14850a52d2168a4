"""The decoder's host code answers what the commit before its stream walk and its launch path became one answered: tests/golden/decoder_refusals.json holds a sha256 per
group of tests/decoder_refusal_cases.py, recorded from that commit by tools/record_decoder_refusals.py -- every single-bit flip and every cut of the streams that
test_decode.py and test_parse_core.py damage, the refused features, every `accept` through every form of hevcdl_parse_stream (with what an accepted stream parses to),
slice data of one picture against the header of the next, and the reconstruction's entry points called badly.  On a device: the three stand-alone device forms of the
reconstruction against their CPU forms, the three launch counters, and the refusals that need a device to be reached."""
import ctypes
import json
import os

import numpy as np
import pytest

import decoder_refusal_cases as cases
import entropy_cases as ec
from conftest import GOLD

RECORDED = json.load(open(os.path.join(GOLD, "decoder_refusals.json")))
GROUPS = sorted(RECORDED["groups"])


def test_the_recorded_groups_are_the_groups_of_the_cases():
    import hevcdl_amd
    names = []
    cases.groups(hevcdl_amd, only=lambda name: names.append(name))
    assert sorted(names) == GROUPS and len(GROUPS) == 23


@pytest.mark.parametrize("group", GROUPS)
def test_the_answers_are_the_recorded_ones(group):
    import hevcdl_amd
    lines = cases.groups(hevcdl_amd, only=lambda name: name == group)[group]
    got = cases.digest(lines)
    print("%s: %d lines, %s" % (group, got["count"], got["sha256"]))
    assert got == RECORDED["groups"][group], "\n".join(lines[:40])
    if group.startswith("refusal order"):      # an error in the slice data of picture 0 is reported, not the refused header of picture 1 behind it
        assert all("CTU 3: the slice data ends inside the CTU" in l for l in lines[1::2]) and all(",2,slice_type 0" in l for l in lines[0::2])


@pytest.mark.gpu
def test_device_forms_equal_their_host_forms_and_count_their_launches():
    """A pair of 128 x 128 pictures (two CTU rows: the row wait; two pictures: the stepping of records, pictures and map), synthetic records with levels up to +-32767, a QP
    per picture, a QP per 4x4 partition with chroma offsets, factors of 1 .. 255: at 8 and 10 bits hevcdl_reconstruct_frames_dev, _qp_dev and _sl_dev on device memory give
    the bytes of their *_host forms; hevcdl_recon_launches counts each launch, hevcdl_recon_qp_launches and hevcdl_recon_sl_launches only their own.  Then the refusals
    that only a machine with a device can reach, each in front of any launch: device 99 (the recorded lines), and a picture count of 65537, which the launch path refuses
    behind its configuration check (that sentence cannot be recorded without a device; it is the source's)."""
    import torch
    import hevcdl_amd as hv
    lib = hv.load_library()
    rng = np.random.default_rng(20250211)
    recs = np.stack([ec.synth_records(rng, 128, 128) for _ in range(2)])
    qps = np.array([22, 37], np.int32)
    info = hv.QpInfo(1, 0, 3, -5)
    i = np.arange(hv.SCALING_FACTOR_BYTES)
    sc = hv.scaling_info(1 + (i * 37) % 255)
    counters = lambda: (lib.hevcdl_recon_launches(), lib.hevcdl_recon_qp_launches(), lib.hevcdl_recon_sl_launches())
    d_recs = torch.from_numpy(recs.view(np.uint8).reshape(-1)).cuda()
    for bd in (8, 10):
        cfg = hv.stream_config(128, 128, 30, bit_depth=bd)
        assert hv.validate_records(cfg, recs) is None
        qmap = rng.integers(-6 * (bd - 8), 52, (2, 4, 256)).astype(np.int8)
        d_map = torch.from_numpy(qmap.reshape(-1)).cuda()
        forms = (("", (qps.ctypes.data,), dict(qps=qps), (1, 0, 0)),
                 ("_qp", (ctypes.byref(info), d_map.data_ptr()), dict(qp_map=qmap, qp_info=info), (1, 1, 0)),
                 ("_sl", (ctypes.byref(info), d_map.data_ptr(), ctypes.byref(sc)), dict(qp_map=qmap, qp_info=info, scaling=sc), (1, 0, 1)))
        for form, quant, host_args, moves in forms:
            host = hv.reconstruct_frames(cfg, recs, **host_args)
            d_out = torch.zeros(host.size * host.itemsize, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            c0 = counters()
            st = getattr(lib, "hevcdl_reconstruct_frames%s_dev" % form)(0, ctypes.byref(cfg), None, *quant, d_recs.data_ptr(), 2, d_out.data_ptr(), None)
            assert st == 0, lib.hevcdl_parse_error().decode()
            assert tuple(b - a for a, b in zip(c0, counters())) == moves, form
            assert d_out.cpu().numpy().tobytes() == host.tobytes(), (bd, form)
            assert len(np.unique(host)) > 16
            c0 = counters()
            st = getattr(lib, "hevcdl_reconstruct_frames%s_dev" % form)(0, ctypes.byref(cfg), None, *quant, d_recs.data_ptr(), 65537, d_out.data_ptr(), None)
            assert (st, lib.hevcdl_parse_error().decode()) == (1, "null device pointer, or a picture count outside 1 .. 65536") and counters() == c0
    c0 = counters()
    assert cases.digest(cases.no_such_device(hv)) == RECORDED["device_side"]["no such device"] and counters() == c0
