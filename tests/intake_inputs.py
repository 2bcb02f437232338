"""Cases and seeded images of the image-intake tests (tests/test_intake_inputs.py on the host, tests/test_gpu_intake.py on the device).  No test
lives here.  The truth is the host chain itself: Whitebox.convert_from_numpy's arithmetic, saliency_io.resize_linear + the truncation to bytes.

The shapes are the smallest at which each branch of the law can go wrong."""
import numpy as np

from xfr_amd import intake
from xfr_amd.saliency_io import resize_linear

# (h, w) -> (H, W), and what the shape exercises
SMALL_CASES = [
    ((1, 1), (4, 5)),            # lines of one value
    ((2, 3), (5, 4)),            # both edge folds
    ((7, 5), (16, 12)),          # a non-square enlargement
    ((6, 7), (6, 14)),           # one axis the identity
    ((10, 4), (5, 8)),           # one axis shrinks, the other enlarges: one sigma skipped
    ((9, 11), (4, 5)),           # radii 3 and 2
    ((8, 3), (1, 2)),            # radius 14 on a line of 8: several mirror periods
    ((40, 5), (4, 4)),           # radius 18
]
NET_CASES = [((224, 224), (224, 224)), ((223, 225), (224, 224)), ((160, 160), (224, 224)), ((112, 112), (224, 224)), ((300, 300), (224, 224)),
             ((421, 333), (224, 224))]
CASES = SMALL_CASES + NET_CASES
CHANNELS = (1, 3, 4)
HEADS = (intake.HEAD_F64, intake.HEAD_F32)


def case_id(case):
    return '%dx%d-%dx%d' % (case[0] + case[1])


def ramp(h, w, c):
    """[(3y + 2x) % 256, (5y + 40) % 256, (7x) % 256 (, (y + x) % 256)]: smooth, where values within 1e-9 of an integer cluster before truncation."""
    y, x = np.mgrid[0:h, 0:w]
    planes = [(3 * y + 2 * x) % 256, (5 * y + 40) % 256, (7 * x) % 256, (y + x) % 256]
    return np.stack(planes[:c], axis=2).astype(np.uint8)


def random_image(h, w, c, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(h, w, c), dtype=np.uint8)


def all_values(h, w, c):
    """Every byte value in every channel, for the same-size case: uint8(float32(u) / 255 * 255) is not u everywhere."""
    return (np.arange(h * w * c).reshape(h, w, c) % 256).astype(np.uint8)


def images_of(case, c):
    """The images a case is run on: random and the ramp; the same-size case on every byte value too."""
    (h, w), out = case
    imgs = [random_image(h, w, c, seed=1000 * h + w + c), ramp(h, w, c)]
    if (h, w) == tuple(out):
        imgs.append(all_values(h, w, c))
    return imgs


def parent_bytes(u8, out_hw, head):
    """The parent's chain on a uint8 h x w x C crop, up to the bytes PIL receives: whitebox.py:787-806 with the / 255 of the caller that owns the
    head (files and DataFrame rows divide in float64 before convert_from_numpy sees them, uint8 arrays are divided in float32 inside it)."""
    u8 = np.asarray(u8)
    img = u8.astype(np.float32) / 255 if head == intake.HEAD_F32 else u8.astype(float) / 255
    img = resize_linear(img, out_hw)
    b = (img * 255).astype(np.uint8)
    if b.ndim == 2 or b.shape[2] == 1:
        return np.repeat(b.reshape(b.shape[0], b.shape[1], 1), 3, axis=2)
    return np.ascontiguousarray(b[:, :, :3])


_TRUTH = {}


def truth(case, c, head):
    """[(image, parent_bytes), ...] of a case, computed once and shared; the arrays are read-only."""
    key = (case, c, head)
    if key not in _TRUTH:
        rows = []
        for u in images_of(case, c):
            b = parent_bytes(u, case[1], head)
            u.setflags(write=False)
            b.setflags(write=False)
            rows.append((u, b))
        _TRUTH[key] = rows
    return _TRUTH[key]
