"""The deblocking and SAO kernels on the adversarial corpus (oracle/filter_cases.py) against the C oracle -- and so, by tests/test_filters_adversarial.py,
against the restatement of H.265 8.7.2 / 8.7.3.  Every case is a legal call on legal buffers.  For the SAO decision chain the oracle is the only
yardstick on inputs no encode reaches; the statistics stay internal, an error in them shows in the decided parameters (`packed-max`, `rounding`)."""
import numpy as np
import pytest

import filter_cases as fc
import filter_spec as fs
from test_filters_adversarial import deblock_corpus, sao_corpus, oracle_deblocked, oracle_sao, spec_deblock, first_difference

pytestmark = pytest.mark.gpu

DEBLOCK_IDS = [c["name"] for c in deblock_corpus()]
SAO_IDS = [c["name"] for c in sao_corpus()]
IN_PLACE = [i for i, c in enumerate(deblock_corpus()) if c["n_frames"] == 3]          # the batches: another content and TU grid per frame


def encoder_for(c):
    import hevcdl_amd
    return hevcdl_amd.Encoder(c["w"], c["h"], c["qp"], max_frames=c["n_frames"], bit_depth=c["bit_depth"], tiles=c["tiles"], lf_across_tiles=c["lf_across_tiles"],
                              lf_offsets=c.get("lf_offsets", (0, 0)))


def check_deblocked(c, out, ref, how):
    for f in range(c["n_frames"]):
        if not np.array_equal(out[f], ref[f]):
            p, y, x = first_difference(out[f], ref[f], c["w"], c["h"])
            _, tally = spec_deblock(c, f)
            pytest.fail("%s (%s): plane %d differs first at (frame %d, y %d, x %d): kernel %d, oracle %d, input %d; %s" % (
                c["name"], how, p, f, y, x, fs.split_planes(out[f], c["w"], c["h"])[p][y, x], fs.split_planes(ref[f], c["w"], c["h"])[p][y, x],
                fs.split_planes(c["planes"][f], c["w"], c["h"])[p][y, x], fs.describe_sample(tally, p, y, x)))


@pytest.mark.parametrize("i", range(len(DEBLOCK_IDS)), ids=DEBLOCK_IDS)
def test_gpu_deblock_matches_oracle_on_adversarial_case(oracle_built, i):
    c = deblock_corpus()[i]
    ref = oracle_deblocked(i)
    e = encoder_for(c)
    try:
        out = e.deblock_frames(c["planes"], c["records"])
    finally:
        e.close()
    check_deblocked(c, out, ref, "deblock_frames")


@pytest.mark.parametrize("i", IN_PLACE, ids=[DEBLOCK_IDS[i] for i in IN_PLACE])
def test_gpu_deblock_in_place_matches_oracle(oracle_built, i):
    """in == out through the device-pointer entry point: a workgroup reads and writes its own rectangle only."""
    import torch
    c = deblock_corpus()[i]
    ref = oracle_deblocked(i)
    dev = torch.device("cuda", 0)
    e = encoder_for(c)
    try:
        d_pic = torch.from_numpy(np.ascontiguousarray(c["planes"]).view(np.uint8).reshape(-1).copy()).to(dev)
        d_rec = torch.from_numpy(np.ascontiguousarray(c["records"]).view(np.uint8).reshape(-1).copy()).to(dev)
        e.deblock_frames_dev(d_pic.data_ptr(), c["n_frames"], d_rec.data_ptr(), d_pic.data_ptr())
        torch.cuda.synchronize()
        out = d_pic.cpu().numpy().view(c["planes"].dtype).reshape(c["planes"].shape)
    finally:
        e.close()
    check_deblocked(c, out, ref, "deblock_frames_dev, in == out")


@pytest.mark.parametrize("i", range(len(SAO_IDS)), ids=SAO_IDS)
def test_gpu_sao_matches_oracle_on_adversarial_case(oracle_built, i):
    c = sao_corpus()[i]
    o_params, o_out = oracle_sao(i)
    e = encoder_for(c)
    try:
        params, out = e.sao_frames(c["org"], c["dbk"])
    finally:
        e.close()
    if params.tobytes() != o_params.tobytes():
        for f in range(c["n_frames"]):
            for a in range(params.shape[1]):
                for comp in range(3):
                    for field in ("mode", "type", "aux", "offset"):
                        if not np.array_equal(params[f, a, comp][field], o_params[f, a, comp][field]):
                            pytest.fail("%s: frame %d ctu %d component %d field %s: kernel %s, oracle %s" % (
                                c["name"], f, a, comp, field, params[f, a, comp][field].tolist(), o_params[f, a, comp][field].tolist()))
    for f in range(c["n_frames"]):
        if not np.array_equal(out[f], o_out[f]):
            p, y, x = first_difference(out[f], o_out[f], c["w"], c["h"])
            s = 1 if p == 0 else 2
            a = (y * s // 64) * ((c["w"] + 63) // 64) + x * s // 64
            pytest.fail("%s: parameters equal, picture differs first at frame %d ctu %d component %d (y %d, x %d): kernel %d, oracle %d, parameters %s" % (
                c["name"], f, a, p, y, x, fs.split_planes(out[f], c["w"], c["h"])[p][y, x], fs.split_planes(o_out[f], c["w"], c["h"])[p][y, x], o_params[f, a, p]))
