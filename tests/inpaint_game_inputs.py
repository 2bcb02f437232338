"""Inputs of the inpainting-game fixture (tests/golden/golden_inpaint_game.npz), shared by its generator and the tests that replay it: everything
here is a seeded function of the case, so the fixture stores results only.

A case: an original in network format (synth.synth_smooth_images of subject A), its inpainted twin (the original with a rectangle taken from
subject B), the rectangle as ground truth, and saliency maps: smooth non-negative bumps, the lowest 30 % of which are cut to exact zeros."""
import numpy as np

from xfr_amd import synth
from xfr_amd.models.resnet import MEAN_RGB

STANDARD = np.arange(0, 101)                                                 # run_inpainting_game_eval.py: 101 percentiles
COARSE = np.concatenate([np.arange(0, 91, 3), [100]])                        # 32 levels: 0, 3, ..., 90, 100
THRESHOLDS = np.array([1e-4, 4e-5, 2e-5, 1e-5, 0.0])                         # explicit s / sum(s) thresholds, falling

# name -> (arch, levels kind, levels, include_zero_elements, maps in the call)
CASES = {
    'mini/zero_on': ('stresnet_mini', 'percent-density', STANDARD, True, 1),
    'mini/zero_off': ('stresnet_mini', 'percent-density', STANDARD, False, 1),
    'mini/thresholds': ('stresnet_mini', 'thresholds', THRESHOLDS, True, 1),
    'mini/two_maps': ('stresnet_mini', 'percent-density', STANDARD, True, 2),
    'lcnn/zero_on': ('lightcnn29v2', 'percent-density', STANDARD, True, 1),
    'r101/coarse': ('stresnet101', 'percent-density', COARSE, True, 1),
}
NUM_CLASSES = {'stresnet_mini': 5, 'lightcnn29v2': 10, 'stresnet101': 65359}


def in_shape(arch):
    return (1, 128, 128) if arch == 'lightcnn29v2' else (3, 224, 224)


def subject(arch, seed):
    """One image in network format, float32 C x H x W."""
    if arch == 'lightcnn29v2':
        return synth.synth_smooth_images(1, in_shape(arch), seed=seed, scale255=False)[0].numpy()
    return synth.synth_smooth_images(1, in_shape(arch), seed=seed, mean=MEAN_RGB)[0].numpy()


def rectangle(arch):
    _, h, w = in_shape(arch)
    return int(0.30 * h), int(0.70 * h), int(0.25 * w), int(0.65 * w)


def twin_of(arch, a, b):
    y0, y1, x0, x1 = rectangle(arch)
    t = a.copy()
    t[:, y0:y1, x0:x1] = b[:, y0:y1, x0:x1]
    return t


def ground_truth(arch):
    _, h, w = in_shape(arch)
    y0, y1, x0, x1 = rectangle(arch)
    gt = np.zeros((h, w), dtype=bool)
    gt[y0:y1, x0:x1] = True
    return gt


def probe_pair(arch):
    """(original, inpainted twin) of the probe: subject A (seed 11) and the rectangle of subject B (seed 12)."""
    a, b = subject(arch, 11), subject(arch, 12)
    return a, twin_of(arch, a, b)


def gallery_pairs(arch):
    """Three more (original, twin) pairs of the same two subjects: each a tenth of another image mixed in."""
    a, b = subject(arch, 11), subject(arch, 12)
    out = []
    for k in range(3):
        d = np.float32(0.1) * (subject(arch, 21 + k) - subject(arch, 31 + k))
        out.append((a + d, twin_of(arch, a + d, b + d)))
    return out


def bump_map(shape, seed):
    """Float64 H x W: five Gaussian bumps, shifted down by their 30th percentile and clipped at zero."""
    h, w = shape
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    m = np.zeros((h, w))
    for _ in range(5):
        cy, cx = rng.uniform(0.2, 0.8) * h, rng.uniform(0.2, 0.8) * w
        s = rng.uniform(0.06, 0.2) * min(h, w)
        m += rng.uniform(0.3, 1.0) * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * s * s))
    return np.maximum(m - np.percentile(m, 30), 0.0)


def maps_of(name, seed):
    arch, _, _, _, n_maps = CASES[name]
    return np.stack([bump_map(in_shape(arch)[1:], seed + 1000 * k) for k in range(n_maps)])
