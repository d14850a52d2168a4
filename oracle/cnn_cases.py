"""oracle/cnn_cases.py -- TEST INFRASTRUCTURE, not product code.

Adversarial input corpus of the label CNN: deterministic, seeded, named groups of [N,64,64,3] uint8 RGB CTUs that put the only signal where an im2col slot, a halo
offset, a quadrant seam, a colour-plane order or a degenerate BatchNorm (flat map: variance 0, gain 1 / sqrt(eps) = 316) decides the result.  The smooth, near-grey
pictures of ref_tools.synth_yuv and tests/golden/cnn_f1.npz average such mistakes away.  tests/golden/cnn_f4.npz holds the reference model's logits on this corpus
(oracle/gen_fixtures.py gen_cnn_cases; the CTUs are regenerated from SEED, the fixture stores VERSION to notice a corpus that moved under it).
"""
import numpy as np

SEED = 20250117
VERSION = 1          # bump whenever a CTU of the corpus changes (tests/golden/cnn_f4.npz is then regenerated)

# the quadrant seams (31 | 32), the 2-pixel halo of the 5x5 layers (0, 2, 61, 63), conv64's half-CTU seam (rows 31 / 32) and one interior point: (y, x)
IMPULSE_POS = ((0, 0), (63, 63), (0, 63), (31, 31), (32, 32), (31, 32), (2, 2), (61, 61), (16, 47))
GROUPS = ("flat", "impulse", "pattern", "noise", "colour")
SIZES = {"flat": 12, "impulse": 36, "pattern": 7, "noise": 9, "colour": 4}


def _flat(rng):
    out = [np.full((64, 64, 3), v, np.uint8) for v in (0, 1, 2, 16, 128, 254, 255)]
    for c in range(3):                                                  # pure R, G, B
        a = np.zeros((64, 64, 3), np.uint8)
        a[..., c] = 255
        out.append(a)
    out.append(rng.integers(1, 3, (64, 64, 3)).astype(np.uint8))        # dark mix {1, 2} per sample
    out.append(rng.integers(254, 256, (64, 64, 3)).astype(np.uint8))    # bright mix {254, 255}
    return np.stack(out)


def _impulse(rng):
    out = []
    for bg, fg in ((0, 255), (255, 0)):                                 # one white pixel in black, one black pixel in white
        for y, x in IMPULSE_POS:
            a = np.full((64, 64, 3), bg, np.uint8)
            a[y, x] = fg
            out.append(a)
    for bg, fg in ((0, 255), (255, 0)):                                 # the same in ONE colour plane (the plane walks with the position)
        for k, (y, x) in enumerate(IMPULSE_POS):
            a = np.full((64, 64, 3), bg, np.uint8)
            a[y, x, k % 3] = fg
            out.append(a)
    return np.stack(out)


def _pattern(rng):
    yy, xx = np.mgrid[0:64, 0:64]
    grey = lambda g: np.repeat(np.asarray(g, np.uint8)[..., None], 3, axis=2)
    out = [grey(((xx + yy) & 1) * 255),                                 # checkerboard, period 1
           grey((((xx >> 3) + (yy >> 3)) & 1) * 255),                   # period 8
           grey((yy & 1) * 255),                                        # horizontal 1-pixel stripes
           grey((xx & 1) * 255),                                        # vertical
           grey(4 * xx),                                                # horizontal ramp
           grey(4 * yy),                                                # vertical ramp
           np.stack([4 * xx, 4 * yy, np.full_like(xx, 90)], axis=-1).astype(np.uint8)]      # R along x, G along y, B constant
    return np.stack(out)


def _noise(rng):
    out = [rng.integers(0, 256, (64, 64, 3)).astype(np.uint8),
           rng.integers(0, 256, (64, 64, 3)).astype(np.uint8),
           (rng.integers(0, 2, (64, 64, 3)) * 255).astype(np.uint8)]    # binary {0, 255}
    for q in range(4):                                                  # noise in one quadrant, the rest black
        a = np.zeros((64, 64, 3), np.uint8)
        oy, ox = (q >> 1) * 32, (q & 1) * 32
        a[oy:oy + 32, ox:ox + 32] = rng.integers(0, 256, (32, 32, 3))
        out.append(a)
    a = rng.integers(0, 256, (64, 64, 3)).astype(np.uint8)
    a[56:] = 0                                                          # bottom CTU row of a 1080-line picture
    out.append(a)
    a = rng.integers(0, 256, (64, 64, 3)).astype(np.uint8)
    a[:, 32:] = 0                                                       # right half past the picture edge
    out.append(a)
    return np.stack(out)


def _colour(rng):
    yy, xx = np.mgrid[0:64, 0:64].astype(np.float64)
    r = 200 + 50 * np.sin(xx / 7.0) * np.cos(yy / 11.0)
    g = 60 + 40 * np.cos((xx + 2 * yy) / 9.0)
    b = 120 + 100 * np.sin(yy / 5.0 + 1.0)
    base = np.stack([r, g, b], axis=-1)
    out = []
    for perm in ((0, 1, 2), (2, 1, 0), (1, 2, 0), (0, 2, 1)):           # the same picture with its planes exchanged: only the channel order differs
        out.append(np.clip(base[..., perm] + rng.normal(0, 1.5, (64, 64, 3)), 0, 255).astype(np.uint8))
    return np.stack(out)


def corpus(seed=SEED):
    """-> {group name: [N,64,64,3] uint8}, the groups in the order of GROUPS; every group draws from its own generator, so a group can change alone."""
    makers = {"flat": _flat, "impulse": _impulse, "pattern": _pattern, "noise": _noise, "colour": _colour}
    out = {}
    for k, name in enumerate(GROUPS):
        out[name] = np.ascontiguousarray(makers[name](np.random.default_rng([seed, k])))
        assert out[name].shape == (SIZES[name], 64, 64, 3) and out[name].dtype == np.uint8
    return out


def stacked(seed=SEED):
    """-> (ctus [N,64,64,3], {group: slice into them})"""
    groups = corpus(seed)
    spans, at = {}, 0
    for name in GROUPS:
        spans[name] = slice(at, at + len(groups[name]))
        at += len(groups[name])
    return np.concatenate([groups[n] for n in GROUPS]), spans


def mix(extra_ctus, n=32, seed=SEED):
    """The n-CTU mix the synthetic-weight tests run on: every third CTU of the corpus, walking through all groups (flat black and the per-channel ramps among
    them), the two grey ramps (the group on which the f32 graph itself is least accurate), filled up with CTUs of `extra_ctus` (tests/golden/cnn_f1.npz: ordinary content)."""
    ctus, spans = stacked(seed)
    ramps = ctus[spans["pattern"]][4:6]
    pick = np.concatenate([ctus[::3], ramps])
    assert len(pick) < n
    step = max(1, len(extra_ctus) // (n - len(pick)))
    return np.ascontiguousarray(np.concatenate([pick, np.asarray(extra_ctus)[::step][:n - len(pick)]]))
