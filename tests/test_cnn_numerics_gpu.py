"""GPU: the label CNN (csrc/cnn_kernel.hip, csrc/fc_kernel.hip) against the f64 restatement of its graph (oracle/cnn_torch.py), on the adversarial corpus of
oracle/cnn_cases.py, on degenerate pictures through the planar path, and with synthetic weight blobs that reach what the shipped checkpoint never does (negative and
zero gamma: the min-pool epilogues; both ends and the cap of the per-layer weight scale; an outlier weight; zero and large biases on a flat input).

The bound.  It comes from the reference, never from the kernel: E_ref = max |f32 graph - f64 graph| over the corpus and the CTUs of tests/golden/cnn_f1.npz (torch on the CPU, the
weights of the test), and the kernel must stay within 16 * E_ref of the f64 graph:
    x4  split operands carry 22 significant bits against f32's 24,
    x2  both operands of every product are split,
    x2  accumulation order of the MFMA tree against a serial f32 sum.
With the shipped weights E_ref is 1.8e-5 (training-mode BatchNorm) / 2.2e-5 (eval), i.e. a bound of 3.0e-4 / 3.5e-4 -- against the 1e-3 of tests/test_cnn_gpu.py, which stays.
Labels must equal labels_from_logits(f64 logits) for every CTU whose 16 argmax decisions all have a top-2 gap above 2 * 16 * E_ref in the f64 logits.
profiles/cnn_numerics.txt records what the kernel measured per group (tools/cnn_err.py); it is a record, not the source of any bound here.
Measured on an MI355X when this was written: every group within 2.5 x E_ref except a flat black CTU (every map flat: variance 0, gain 316), 1.1e-4 = 6.2 x E_ref; the synthetic
blobs between 1.1 and 11.4 x their own E_ref (the largest where the flat black CTU of the mix meets a rescaled layer); no label wrong anywhere.
"""
import json
import os

import numpy as np
import pytest

from conftest import GOLD

pytestmark = pytest.mark.gpu
FACTOR = 16


@pytest.fixture(scope="module")
def shipped():
    import cnn_oracle
    import hevcdl_amd
    return cnn_oracle.load_weights(hevcdl_amd.WEIGHTS_PATH)


@pytest.fixture(scope="module")
def f1_ctus():
    return np.load(os.path.join(GOLD, "cnn_f1.npz"))["ctu_rgb"]


@pytest.fixture(scope="module")
def yardstick(shipped, f1_ctus):
    """{bn_eval: (f64 logits of corpus ++ cnn_f1, E_ref over all of them)} with the shipped weights."""
    import torch
    import cnn_cases
    import cnn_torch
    ctus = np.concatenate([cnn_cases.stacked()[0], f1_ctus])
    return {ev: cnn_torch.reference_pair(torch, shipped, ctus, ev) for ev in (False, True)}


def _compare(what, labels, logits, l64, e_ref):
    """The bound and the label rule; prints the figures before it asserts."""
    import cnn_oracle
    import cnn_torch
    err = float(np.abs(logits.astype(np.float64) - l64).max())
    safe = cnn_torch.decided(l64, 2 * FACTOR * e_ref)
    want = cnn_oracle.labels_from_logits(l64)
    wrong = int((labels[safe] != want[safe]).any(axis=1).sum())
    print("%-28s E_ref %.3e  bound %.3e  kernel error %.3e  ratio %5.2f  CTUs %d  decided %d  labels wrong %d" % (what, e_ref, FACTOR * e_ref, err, err / e_ref, len(l64), int(safe.sum()), wrong))
    assert np.isfinite(logits).all(), what
    assert err <= FACTOR * e_ref, (what, err, e_ref)
    assert wrong == 0, what
    return safe


@pytest.mark.parametrize("bn_mode", [0, 1])
def test_every_corpus_group_stays_within_the_bound_of_the_f64_graph(yardstick, f1_ctus, bn_mode):
    """Shipped weights, training-mode BatchNorm (what the reference runs) and bn_mode=1 against the f64 eval graph: each group of the corpus, then the CTUs of cnn_f1."""
    import cnn_cases
    import hevcdl_amd
    ctus, spans = cnn_cases.stacked()
    l64, e_ref = yardstick[bool(bn_mode)]
    e = hevcdl_amd.Encoder(128, 128, 32, max_frames=1, bn_mode=bn_mode)
    try:
        results = {g: e.predict_depth_rgb(ctus[sl]) for g, sl in spans.items()}
        results["cnn_f1"] = e.predict_depth_rgb(f1_ctus)
        whole = e.predict_depth_rgb(ctus)
    finally:
        e.close()
    spans = dict(spans, cnn_f1=slice(len(ctus), len(ctus) + len(f1_ctus)))
    failed = []
    for g, (labels, logits) in results.items():
        try:
            safe = _compare("%s bn_mode=%d" % (g, bn_mode), labels, logits, l64[spans[g]], e_ref)
            assert safe.any(), g                       # (tests/test_cnn_numerics.py caps what the band may skip)
        except AssertionError as a:
            failed.append(str(a))
    assert not failed, failed
    assert np.array_equal(whole[1], np.concatenate([results[g][1] for g in cnn_cases.GROUPS]))      # a group alone or inside the corpus: the same bits


FLAT_PICTURES = (("video black", 16, 128, 128), ("video white", 235, 128, 128), ("below range", 0, 0, 0), ("above range", 255, 255, 255),
                 ("chroma 0", 128, 0, 0), ("chroma 255", 128, 255, 255))


@pytest.mark.parametrize("width,height", [(200, 136), (1928, 1080)])
@pytest.mark.parametrize("mode,cnn_input", [("rgb601", 0), ("luma", 1)])
def test_degenerate_pictures_through_the_planar_path(yardstick, shipped, mode, cnn_input, width, height):
    """Flat 8-bit 4:2:0 pictures -- video black / white, samples outside the nominal range (the BT.601 clip is active), saturated chroma -- at sizes whose last CTU column and row lie
    mostly outside the picture (8 samples inside), so that quadrants are partly and wholly zero fill: flat maps, BatchNorm variance 0.  The frame path against
    cnn_oracle.yuv_to_rgb_ctus + the f64 graph; the input transform is integer, so the frame path's logits are also bit-equal to the RGB-CTU path's on the oracle's samples."""
    import torch
    import cnn_oracle
    import cnn_torch
    import hevcdl_amd
    e_ref = yardstick[False][1]
    yuv = np.stack([np.concatenate([np.full(width * height, y, np.uint8), np.full(width * height // 4, u, np.uint8), np.full(width * height // 4, v, np.uint8)]) for _, y, u, v in FLAT_PICTURES])
    e = hevcdl_amd.Encoder(width, height, 32, max_frames=len(yuv), cnn_input=cnn_input)
    try:
        labels, logits = e.predict_depth(yuv, want_logits=True)
        rgb = [cnn_oracle.yuv_to_rgb_ctus(fr, width, height, mode=mode) for fr in yuv]
        by_ctu = [e.predict_depth_rgb(c)[1] for c in rgb]
    finally:
        e.close()
    failed = []
    for f, (name, y, u, v) in enumerate(FLAT_PICTURES):
        assert np.array_equal(logits[f], by_ctu[f]), name
        uniq, inv = np.unique(rgb[f].reshape(len(rgb[f]), -1), axis=0, return_inverse=True)          # a flat picture has at most four different CTUs
        assert len(uniq) <= 4
        l64 = cnn_torch.logits_np(torch, shipped, uniq.reshape(-1, 64, 64, 3), "f64")[inv.reshape(-1)]
        try:
            what = "%s %dx%d %s" % (name, width, height, mode)
            err = float(np.abs(logits[f].astype(np.float64) - l64).max())
            safe = cnn_torch.decided(l64, 2 * FACTOR * e_ref)
            want = cnn_oracle.clamp_labels(cnn_oracle.labels_from_logits(l64)[None], width, height)[0]
            wrong = int((labels[f][safe] != want[safe]).any(axis=1).sum())
            print("%-40s E_ref %.3e  kernel error %.3e  ratio %5.2f  different CTUs %d  decided %d of %d  labels wrong %d" % (what, e_ref, err, err / e_ref, len(uniq), int(safe.sum()), len(l64), wrong))
            assert err <= FACTOR * e_ref, (what, err)
            assert wrong == 0 and safe.any(), what
        except AssertionError as a:
            failed.append(str(a))
    assert not failed, failed


# ---- synthetic weights: the shipped blob, changed through the manifest --------------------------------------------------------------------------------------------------
CONVS = ("conv1", "conv64", "conv2", "conv3")


def _views(blob):
    import hevcdl_amd
    man = json.load(open(os.path.splitext(hevcdl_amd.WEIGHTS_PATH)[0] + ".json"))
    assert man["floats"] == blob.size
    return {t["name"]: blob[t["offset"]:t["offset"] + int(np.prod(t["shape"]))].reshape(t["shape"]) for t in man["tensors"]}


def _neg_gamma(v, layers):
    for name in layers:
        v[name + ".1.weight"][1::2] *= -1


def _zero_gamma(v):
    for name in CONVS:
        v[name + ".1.weight"][[0, 5, 11]] = 0


def _scale(v, name, s):
    """The layer's weights times s (a power of two).  Training-mode BatchNorm undoes it up to eps; for eval mode the running statistics follow: conv(x) * s + b has the
    mean (m - b) * s + b and the variance var * s^2."""
    v[name + ".0.weight"] *= np.float32(s)
    if name in CONVS:
        b = v[name + ".0.bias"]
        v[name + ".1.running_mean"][:] = (v[name + ".1.running_mean"] - b) * np.float32(s) + b
        v[name + ".1.running_var"] *= np.float32(s * s)


def _outlier(v, name):
    """One weight of magnitude 100, every other one at most 1e-4: the scale is set by the outlier, the rest falls to the split pair's absolute floor."""
    w = v[name + ".0.weight"]
    w *= np.float32(1e-4) / np.abs(w).max()
    w.reshape(-1)[w.size // 3] = 100.0


def _bias(v, value):
    for name in CONVS + ("fc1", "fc2"):
        b = v[name + ".0.bias"]
        if value == 0 or name in ("conv1", "conv64"):
            new = np.zeros_like(b) if value == 0 else np.where(np.arange(b.size) % 2, -value, value).astype(np.float32)
            if name in CONVS:
                v[name + ".1.running_mean"] += new - b
            b[:] = new
    if value == 0:
        v["fc3.bias"][:] = 0


VARIANTS = {}
for _l in CONVS:
    VARIANTS["neg_gamma_" + _l] = (lambda v, _l=_l: _neg_gamma(v, (_l,)), (0, 1))
VARIANTS["neg_gamma_all"] = (lambda v: _neg_gamma(v, CONVS), (0, 1))
VARIANTS["zero_gamma"] = (_zero_gamma, (0, 1))
for _l in CONVS + ("fc1",):
    VARIANTS["scale_%s_2^-12" % _l] = (lambda v, _l=_l: _scale(v, _l, 2.0 ** -12), (0, 1))
    VARIANTS["scale_%s_2^+10" % _l] = (lambda v, _l=_l: _scale(v, _l, 2.0 ** 10), (0, 1))
for _l in ("conv1", "conv2", "conv3", "fc1"):
    VARIANTS["outlier_" + _l] = (lambda v, _l=_l: _outlier(v, _l), (0,))          # (the running statistics of a layer rebuilt like this mean nothing: training mode only)
VARIANTS["bias_0"] = (lambda v: _bias(v, 0), (0, 1))
VARIANTS["bias_4_flat_input"] = (lambda v: _bias(v, 4.0), (0, 1))
CASES = [(name, m) for name, (_, modes) in VARIANTS.items() for m in modes]


@pytest.mark.parametrize("variant,bn_mode", CASES, ids=["%s-bn%d" % c for c in CASES])
def test_synthetic_weights_stay_within_the_bound_of_the_f64_graph_with_the_same_weights(f1_ctus, variant, bn_mode):
    """Encoder(..., weights=...) accepts any blob, so these are product inputs.  32 CTUs (corpus and cnn_f1 mixed; the large bias also on the whole flat group: variance 0 and a large
    mean, the worst case of the folded form x * alpha + beta'), E_ref recomputed for the weights of the variant, the same 16 * E_ref and the same label rule.
    Measured on an MI355X (E_ref, kernel error, ratio): see the table of profiles/cnn_numerics.txt."""
    import torch
    import cnn_cases
    import cnn_torch
    import hevcdl_amd
    blob = hevcdl_amd.load_weights().copy()
    v = _views(blob)
    VARIANTS[variant][0](v)
    assert blob.size == hevcdl_amd.WEIGHT_FLOATS and blob.dtype == np.dtype("<f4") and np.isfinite(blob).all()          # checked on the host: the ABI does not look at the values
    assert not np.array_equal(blob, hevcdl_amd.load_weights())
    ctus = cnn_cases.mix(f1_ctus)
    if variant.startswith("bias_4"):
        ctus = np.concatenate([cnn_cases.corpus()["flat"], ctus])
    l64, e_ref = cnn_torch.reference_pair(torch, v, ctus, bool(bn_mode))
    assert np.isfinite(l64).all() and e_ref > 0
    e = hevcdl_amd.Encoder(128, 128, 32, max_frames=1, bn_mode=bn_mode, weights=blob)
    try:
        labels, logits = e.predict_depth_rgb(ctus)
    finally:
        e.close()
    _compare("%s bn_mode=%d" % (variant, bn_mode), labels, logits, l64, e_ref)


def test_negated_gamma_changes_the_labels(shipped, f1_ctus):
    """The synthetic blobs are different networks, not relabelled copies: with gamma negated on every second channel the f64 logits move by more than any bound above."""
    import torch
    import cnn_cases
    import cnn_torch
    import hevcdl_amd
    ctus = cnn_cases.mix(f1_ctus)
    base = cnn_torch.logits_np(torch, shipped, ctus)
    for layers in [(name,) for name in CONVS]:
        blob = hevcdl_amd.load_weights().copy()
        v = _views(blob)
        _neg_gamma(v, layers)
        assert np.abs(cnn_torch.logits_np(torch, v, ctus) - base).max() > 0.1, layers


def test_logits_do_not_depend_on_the_batch(f1_ctus):
    """BatchNorm statistics are per CTU = per workgroup and the fully connected head works on rows: the same CTU alone, first, in the middle and last of a 600-CTU call (where the
    second workgroup of every CU starts late, HEVCDL_CNN_SKEW) gives the same bits; so do calls of 1 and of an odd 257 CTUs."""
    import cnn_cases
    import hevcdl_amd
    corpus = cnn_cases.stacked()[0]
    probes = (f1_ctus[1], corpus[0], corpus[-1], cnn_cases.corpus()["noise"][0])
    fill = np.concatenate([f1_ctus, corpus, f1_ctus, corpus])[:600].copy()
    e = hevcdl_amd.Encoder(128, 128, 32, max_frames=1)
    try:
        base_labels, base_logits = e.predict_depth_rgb(fill)
        for probe in probes:
            alone_labels, alone = e.predict_depth_rgb(probe[None])
            assert alone.shape == (1, 4, 16) and np.isfinite(alone).all()
            for at in (0, 300, 599):
                batch = fill.copy()
                batch[at] = probe
                labels, logits = e.predict_depth_rgb(batch)
                assert np.array_equal(logits[at], alone[0]) and np.array_equal(labels[at], alone_labels[0]), at
                keep = np.arange(600) != at
                assert np.array_equal(logits[keep], base_logits[keep]) and np.array_equal(labels[keep], base_labels[keep])
        odd_labels, odd = e.predict_depth_rgb(fill[:257])
        assert np.array_equal(odd, base_logits[:257]) and np.array_equal(odd_labels, base_labels[:257])
    finally:
        e.close()
