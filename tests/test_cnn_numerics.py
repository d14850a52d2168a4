"""CPU: the yardsticks of tests/test_cnn_numerics_gpu.py.  The f64 restatement of the label CNN (oracle/cnn_torch.py) is pinned to the reference model's own logits on every
CNN fixture, the adversarial corpus (oracle/cnn_cases.py) is deterministic and decides its labels outside the tie band, and the C ABI turns a blob of the wrong length away."""
import ctypes
import os

import numpy as np
import pytest

from conftest import GOLD

# max |f64 graph - reference model's logits (f32 torch)| measured on an x86-64 host with torch's CPU convolutions.  The f64 graph hardly rounds, so the figure is the
# f32 reference's own rounding; each test asserts 2 x the pinned figure AND the absolute cap below, so that a wrong graph cannot hide behind a "measured" bound.
PINNED = {"cnn_f1": 1.62e-5, "cnn_f1_eval": 2.44e-5, "cnn_f3": 1.65e-5, "cnn_f4": 1.98e-5, "cnn_f4_eval": 2.77e-5}
ABS_CAP = 1e-4


@pytest.fixture(scope="module")
def weights():
    import cnn_oracle
    import hevcdl_amd
    return cnn_oracle.load_weights(hevcdl_amd.WEIGHTS_PATH)


def _f64(weights, ctus, bn_eval=False, dtype="f64"):
    import torch
    import cnn_torch
    return cnn_torch.logits_np(torch, weights, ctus, dtype, bn_eval=bn_eval)


def _check(name, err):
    print("%s: max |f64 graph - reference model| %.3e (pinned %.3e)" % (name, err, PINNED[name]))
    assert err < 2 * PINNED[name], (name, err)
    assert err < ABS_CAP, (name, err)


def test_f64_graph_matches_the_reference_models_logits_on_cnn_f1(weights):
    f = np.load(os.path.join(GOLD, "cnn_f1.npz"))
    lg = _f64(weights, f["ctu_rgb"])
    assert lg.dtype == np.float64
    _check("cnn_f1", np.abs(lg - f["logits"]).max())
    import cnn_oracle
    srt = np.sort(lg.reshape(-1, 4, 4, 4), axis=-1)
    safe = ((srt[..., -1] - srt[..., -2]) > 2 * ABS_CAP).all(axis=(1, 2))
    assert safe.sum() > 200 and np.array_equal(cnn_oracle.labels_from_logits(lg)[safe], f["labels"][safe])


def test_f64_eval_graph_matches_the_reference_model_in_eval_mode(weights):
    f, g = np.load(os.path.join(GOLD, "cnn_f1.npz")), np.load(os.path.join(GOLD, "cnn_f1_eval.npz"))
    lg = _f64(weights, f["ctu_rgb"], bn_eval=True)
    _check("cnn_f1_eval", np.abs(lg - g["logits"]).max())
    assert np.abs(lg - f["logits"]).max() > 0.1          # the two BatchNorm modes are different networks: a mix-up cannot pass


def test_f64_graph_matches_the_reference_loop_on_whole_pictures(weights):
    import cnn_oracle
    f = np.load(os.path.join(GOLD, "cnn_f3.npz"))
    err = max(np.abs(_f64(weights, cnn_oracle.rgb_picture_to_ctus(f["rgb%d" % n])) - f["logits%d" % n]).max() for n in range(int(f["n_pictures"])))
    _check("cnn_f3", err)


def test_both_oracles_match_the_reference_model_on_the_adversarial_corpus(weights):
    """tests/golden/cnn_f4.npz: the reference model itself (training-mode and eval-mode BatchNorm) on the corpus of oracle/cnn_cases.py, regenerated here from its seed.  The f64
    graph within the pinned bound, the numpy f32 oracle of every other CNN test within the same cap, the labels of the reference's own lines exactly."""
    import cnn_cases
    import cnn_oracle
    f = np.load(os.path.join(GOLD, "cnn_f4.npz"))
    assert int(f["seed"]) == cnn_cases.SEED and int(f["version"]) == cnn_cases.VERSION, "the corpus changed: regenerate the fixture (oracle/gen_fixtures.py cnncases)"
    assert [str(g) for g in f["groups"]] == list(cnn_cases.GROUPS) and [int(n) for n in f["sizes"]] == [cnn_cases.SIZES[g] for g in cnn_cases.GROUPS]
    ctus, spans = cnn_cases.stacked()
    lg, lg_eval = _f64(weights, ctus), _f64(weights, ctus, bn_eval=True)
    _check("cnn_f4", np.abs(lg - f["logits"]).max())
    _check("cnn_f4_eval", np.abs(lg_eval - f["logits_eval"]).max())
    assert np.array_equal(cnn_oracle.labels_from_logits(lg), f["labels"]) and np.array_equal(cnn_oracle.labels_from_logits(lg_eval), f["labels_eval"])
    # the numpy oracle (0.3 s a CTU): the flat, impulse and colour CTUs that no other fixture has, a few of each
    pick = np.r_[0, 3, 6, 9, 12, 25, 33, 48, 54, 55, 64, 65]
    assert np.abs(cnn_oracle.ctu_logits(weights, ctus[pick]) - f["logits"][pick]).max() < ABS_CAP
    assert np.abs(cnn_oracle.ctu_logits(weights, ctus[pick[:4]], bn_eval=True) - f["logits_eval"][pick[:4]]).max() < ABS_CAP


def test_taps_and_dtypes_of_the_torch_graph(weights):
    """taps=True returns the four pooled maps and the two hidden fully connected activations, per quadrant, without changing the logits; the f32 form is what it was (the
    checker of bench.py's label leg) and lies within 1e-4 of the f64 form tap by tap."""
    import torch
    import cnn_torch
    ctus = np.load(os.path.join(GOLD, "cnn_f1.npz"))["ctu_rgb"][:6]
    out = {}
    for name, dt in (("f32", torch.float32), ("f64", torch.float64)):
        w = cnn_torch.weights_to(torch, weights, "cpu", dt)
        lg, taps = cnn_torch.ctu_logits(torch, w, ctus, taps=True)
        assert lg.dtype == dt and torch.equal(lg, cnn_torch.ctu_logits(torch, w, ctus))
        assert {k: tuple(v.shape[1:]) for k, v in taps.items()} == {"cat": (4, 32, 16, 16), "conv2": (4, 64, 8, 8), "conv3": (4, 128, 4, 4), "fc1": (4, 256), "fc2": (4, 64)}
        assert all(v.dtype == dt and bool((v >= 0).all()) for v in taps.values())
        assert torch.equal(taps["cat"][:, 0, 16:], taps["cat"][:, 3, 16:])          # the conv64 half of the cat is the same for the four quadrants
        out[name] = (lg, taps)
    assert torch.equal(out["f32"][0], cnn_torch.ctu_logits(torch, cnn_torch.weights_to(torch, weights, "cpu"), ctus))
    for k in out["f32"][1]:
        assert (out["f32"][1][k].double() - out["f64"][1][k]).abs().max() < 1e-4, k


def test_corpus_is_deterministic_and_complete():
    import cnn_cases
    a, b = cnn_cases.corpus(), cnn_cases.corpus()
    assert list(a) == list(cnn_cases.GROUPS)
    assert {g: len(v) for g, v in a.items()} == {"flat": 12, "impulse": 36, "pattern": 7, "noise": 9, "colour": 4}
    for g in a:
        assert a[g].dtype == np.uint8 and a[g].shape[1:] == (64, 64, 3) and np.array_equal(a[g], b[g])
        assert len(np.unique(a[g].reshape(len(a[g]), -1), axis=0)) == len(a[g]), "two equal CTUs in group " + g
    assert not np.array_equal(cnn_cases.corpus(seed=1)["noise"], a["noise"])
    # what the groups are for
    assert [int(v) for v in a["flat"][:7, 0, 0, 0]] == [0, 1, 2, 16, 128, 254, 255] and all(len(np.unique(c)) <= 2 for c in a["flat"])
    imp = a["impulse"]
    assert all(int((c != c[5, 5]).any(axis=-1).sum()) == 1 for c in imp)                      # exactly one pixel differs from the background
    assert {tuple(int(v) for v in np.argwhere((c != c[5, 5]).any(axis=-1))[0]) for c in imp} == set(cnn_cases.IMPULSE_POS)
    assert int(sum(int((c != c[5, 5]).sum()) == 1 for c in imp)) == 18                        # half of them in one colour plane only
    assert all((c[..., 0] != c[..., 2]).mean() > 0.9 for c in a["colour"])
    assert not a["noise"][7][56:].any() and not a["noise"][8][:, 32:].any() and a["noise"][0].min() == 0 and a["noise"][0].max() == 255
    m = cnn_cases.mix(np.load(os.path.join(GOLD, "cnn_f1.npz"))["ctu_rgb"])
    assert m.shape == (32, 64, 64, 3) and np.array_equal(m[0], a["flat"][0])


def test_corpus_decisions_lie_outside_the_label_band(weights):
    """The label rule of the GPU tests skips a CTU with an argmax decision whose two largest f64 logits are closer than 2 * 16 * E_ref.  Caps on what it may skip: at most 5 % of the
    corpus' decisions, and no group wholly -- otherwise the label half of those tests would be vacuous."""
    import cnn_cases
    ctus, spans = cnn_cases.stacked()
    f1 = np.load(os.path.join(GOLD, "cnn_f1.npz"))["ctu_rgb"]
    for bn_eval in (False, True):
        lg, lg1 = _f64(weights, ctus, bn_eval), _f64(weights, f1, bn_eval)
        e_ref = max(np.abs(_f64(weights, ctus, bn_eval, "f32") - lg).max(), np.abs(_f64(weights, f1, bn_eval, "f32") - lg1).max())
        assert 1e-6 < e_ref < 5e-5, e_ref          # the f32 graph's own error: 1.8e-5 (train) / 2.2e-5 (eval) where this was written
        band = 2 * 16 * e_ref
        srt = np.sort(lg.reshape(-1, 4, 4, 4), axis=-1)
        near = ((srt[..., -1] - srt[..., -2]) < band).reshape(len(lg), 16)
        print("bn_eval %d: E_ref %.3e band %.3e decisions inside %d of %d, smallest gap %.3e" % (bn_eval, e_ref, band, near.sum(), near.size, (srt[..., -1] - srt[..., -2]).min()))
        assert near.mean() <= 0.05
        for g, sl in spans.items():
            assert not near[sl].all(), g


def test_create_rejects_a_blob_of_the_wrong_length():
    """hevcdl_create checks the blob's length before it touches a device (HEVCDL_ERR_INVALID_ARG = 1).  It does not look at the values: a NaN / Inf weight is accepted by the
    ABI as it stands, so the synthetic blobs of tests/test_cnn_numerics_gpu.py are checked for finiteness and length on the host before they are handed over."""
    import hevcdl_amd
    lib = hevcdl_amd.load_library()
    cfg = hevcdl_amd.default_config(64, 64, 32)
    for n in (0, hevcdl_amd.WEIGHT_FLOATS - 1, hevcdl_amd.WEIGHT_FLOATS + 1):
        w = np.zeros(max(n, 1), "<f4")
        h = ctypes.c_void_p()
        assert lib.hevcdl_create(ctypes.byref(cfg), w.ctypes.data, n, ctypes.byref(h)) == 1 and not h.value
        with pytest.raises(hevcdl_amd.HevcdlError):
            hevcdl_amd.Encoder(64, 64, 32, weights=w[:n])
