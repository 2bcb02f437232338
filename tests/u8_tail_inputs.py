"""What the host and the GPU tests of the uint8 saliency tail share (test_u8_tail_inputs, test_gpu_u8_tail): seeded maps and the truth.

Truth.  _mwp_to_saliency of ebp_version != 6 (whitebox.py:451-454) is
    img = np.uint8(255*((img-np.min(img))/(self.eps+(np.max(img)-np.min(img)))))        stage A
    img = np.array(PIL.Image.fromarray(img).filter(PIL.ImageFilter.GaussianBlur(radius=2)))
    img = np.uint8(255*((img-np.min(img))/(self.eps+(np.max(img)-np.min(img)))))        stage B
Restated here with every dtype explicit, so that it does not depend on the promotion rules of the installed NumPy, and with the blur as integer
arithmetic instead of Pillow: stretch_f32 (a float32 map under NumPy 2: the Python floats are weak, everything stays float32), stretch_u8 (a uint8
map: NumPy evaluates the same expression in float64) and pil_gaussian_blur_2 (Pillow's three extended box passes per axis, box radius 1).
tests/test_u8_tail_inputs.py holds all of it to the installed NumPy and Pillow, to the byte, without a device.
"""
import functools

import numpy as np

WW, FW = 4473924, 1677722           # Pillow's BoxBlur.c for GaussianBlur(2): 2^24 / 3.75 and (2^24 - 3 ww) / 2
EPS = (1e-16, 1e-12)                # Whitebox's default, and what the docstrings of versions 7-12 prescribe
# the smallest shapes at which each clamp branch (lines of 1, 2, 3 pixels: the window is wider than the line), a partial last wave, more than one
# turn of a workgroup's loop and the LDS limit (256 x 256 = 65536 pixels) are exercised, and the two sizes the networks produce
SHAPES = ((1, 1), (1, 7), (2, 3), (3, 2), (7, 7), (5, 112), (113, 97), (112, 112), (128, 128), (256, 256))
F32_FAMILIES = ('binades', 'spikes', 'constant', 'below_eps', 'steps', 'negative')
U8_FAMILIES = ('bytes', 'constant_bytes', 'd1', 'ramp')


def stretch_f32(img, eps):
    """Stage A of a float32 map: every operation one rounded float32 operation, truncation to uint8."""
    img = np.ascontiguousarray(img, dtype=np.float32)
    mn, mx = np.float32(img.min()), np.float32(img.max())
    den = np.float32(np.float32(eps) + np.float32(mx - mn))
    q = np.divide(np.subtract(img, mn, dtype=np.float32), den, dtype=np.float32)
    return np.multiply(np.float32(255.0), q, dtype=np.float32).astype(np.uint8)


def stretch_u8(img, eps):
    """Stage A of a uint8 map, and stage B: float64, literally -- not floor(255 v / d)."""
    assert img.dtype == np.uint8
    v = img.astype(np.int64)
    mn, mx = int(v.min()), int(v.max())
    den = np.float64(eps) + np.float64(mx - mn)
    q = np.divide((v - mn).astype(np.float64), den, dtype=np.float64)
    return np.multiply(np.float64(255.0), q, dtype=np.float64).astype(np.uint8)


def _box_pass(a, axis):
    n = a.shape[axis]
    idx = np.arange(n)
    v = a.astype(np.int64)
    t = lambda k: np.take(v, np.clip(idx + k, 0, n - 1), axis=axis)          # noqa: E731  (replicated edges)
    acc = WW * (t(-1) + t(0) + t(1)) + FW * (t(-2) + t(2)) + (1 << 23)
    assert acc.max() < 1 << 32
    return (acc >> 24).astype(np.uint8)


def pil_gaussian_blur_2(img):
    """PIL.ImageFilter.GaussianBlur(radius=2) of an 'L' image: three box passes along the rows, then three along the columns, bytes in between."""
    assert img.dtype == np.uint8 and img.ndim == 2
    for axis in (1, 1, 1, 0, 0, 0):
        img = _box_pass(img, axis)
    return img


def truth(img, eps):
    """The uint8 saliency map of one float32 or uint8 map."""
    a = stretch_u8(img, eps) if img.dtype == np.uint8 else stretch_f32(img, eps)
    return stretch_u8(pil_gaussian_blur_2(a), eps)


@functools.lru_cache(maxsize=None)
def case(family, shape):
    """One seeded map, float32 (F32_FAMILIES) or uint8 (U8_FAMILIES); read-only."""
    h, w = shape
    rng = np.random.RandomState(7000 + 131 * (F32_FAMILIES + U8_FAMILIES).index(family) + 17 * h + w)
    if family == 'binades':              # values over 20 binades
        m = (rng.rand(h, w) * 2.0 ** rng.randint(-10, 10, size=shape)).astype(np.float32)
    elif family == 'spikes':             # 2 % spikes on zero
        m = np.where(rng.rand(h, w) < 0.02, rng.rand(h, w) + 0.1, 0.0).astype(np.float32)
        m.flat[rng.randint(m.size)] = 1.5
    elif family == 'constant':           # max == min
        m = np.full(shape, 0.37, dtype=np.float32)
    elif family == 'below_eps':          # the range lies below eps: den is all eps
        m = ((1.0 + rng.rand(h, w)) * 1e-20).astype(np.float32)
    elif family == 'steps':              # mn + k * step, a third of them one ulp up or down: 255 q lands on and next to integers
        k = rng.randint(0, 256, size=shape)
        k.flat[0], k.flat[-1] = 0, 255
        m = (np.float32(0.125) + k.astype(np.float32) * np.float32(1.0 / 255.0)).astype(np.float32)
        nudge = rng.randint(0, 6, size=shape)
        inner = (k > 0) & (k < 255)
        m = np.where(inner & (nudge == 0), np.nextafter(m, np.float32(9), dtype=np.float32), m)
        m = np.where(inner & (nudge == 1), np.nextafter(m, np.float32(-9), dtype=np.float32), m).astype(np.float32)
    elif family == 'negative':
        m = rng.randn(h, w).astype(np.float32)
    elif family == 'bytes':
        m = rng.randint(0, 256, size=shape).astype(np.uint8)
    elif family == 'constant_bytes':
        m = np.full(shape, 93, dtype=np.uint8)
    elif family == 'd1':                 # max - min = 1
        m = (200 + rng.randint(0, 2, size=shape)).astype(np.uint8)
        if m.size > 1:
            m.flat[0], m.flat[-1] = 200, 201
    elif family == 'ramp':               # 0, 1, 2, ...: the identity 0..255 once there are 256 pixels
        m = (np.arange(h * w) % 256).astype(np.uint8).reshape(shape)
    else:
        raise KeyError(family)
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def case_truth(family, shape, eps):
    t = truth(case(family, shape), eps)
    t.setflags(write=False)
    return t


IDENTITY = np.arange(256, dtype=np.uint8).reshape(16, 16)
